// Squeeze-and-excitation on a bottleneck's last BatchNorm, and the 2x2 average pool of the avg-pool shortcut, for the
// ResNet-RS / ResNet-D backbones (gfx950), NHWC.
//
// Replaces timm's SEModule inside Bottleneck (timm/models/resnet.py: x = bn3(conv3(x)); x = se(x); x += shortcut; relu)
// and nn.AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False) of downsample_avg, with their autograd backward.
//
//   z = gamma (y - mean) rstd + beta         the block's last BatchNorm over the raw conv3 output y [B][HW][C]
//   pooled[b][c] = mean_hw z = gamma (mean_hw y - mean) rstd + beta      (the BatchNorm is affine per channel, so the
//                                                                        squeeze reads y, never z)
//   hidden = relu(w1 pooled + b1),  gate = sigmoid(w2 hidden + b2)       (f32, per image)
//   out = relu(z * gate[b][c] + shortcut)
//
// The passes over the activation read 8 consecutive channels per thread (16 B in bf16, 2 x 16 B in f32).  Every sum
// has one fixed order (no atomics), an image's gate depends on that image's rows alone, and nothing synchronises with
// the host.  Summation orders (the tests derive their bounds from them):
//   * per-image channel sums (squeeze, bwd_stats): image rows are cut into P = sv_se_nparts parts of rpp =
//     ceil(HW / P) rows; in a part, thread (rsub, channel group) adds rows r0 + rsub, + rp, ... ascending (rp = 256 /
//     (C / 8) rows in flight), the rp threads of a channel group are added in rsub order, and the consumer adds the P
//     parts in part order;
//   * the matvec rows (fc1, fc2), the transposed matvec columns (the gate backward) and the outer products over the
//     batch (the gate's weight gradients): se_core.h;
//   * the BatchNorm sums over the batch: b ascending, fmaf.
#include <math.h>

#include "chanvec.h"
#include "common.h"
#include "se_core.h"

namespace sv {
namespace se {

constexpr int kThreads = 256;
constexpr int kMaxC = 2048;
constexpr int kMaxParts = 32;

// C a power of two in 16..2048: C / 8 threads cover a row and divide the block
static bool c_ok(int C) { return C >= 16 && C <= kMaxC && (C & (C - 1)) == 0; }

static int nparts_for(int HW, int C) {
  const int rp = kThreads / (C / 8);
  int p = HW / (8 * rp);  // >= 8 rows per thread
  if (p > kMaxParts) p = kMaxParts;
  if (p < 1) p = 1;
  return p;
}

// ---- per-image channel sums ---------------------------------------------------------------------------------------
// grid (P, B).  NS = 1: part [B][P][C] = sum_rows y;  NS = 2 (backward): part [B][P][2][C] = (sum g, sum g xhat) with
// g = dout * (act > 0) written back over dout.
template <int NS>
__global__ void __launch_bounds__(kThreads) sums_kernel(const void* __restrict__ y, int ydt, void* dout, int ddt,
                                                        const void* __restrict__ act, int adt,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        float* __restrict__ part, int HW, int C, int P, int rpp) {
  __shared__ float red[NS][8][kThreads];
  const int tpr = C / 8, rp = kThreads / tpr;
  const int t = threadIdx.x, cg = t % tpr, rsub = t / tpr, c = cg * 8;
  const int p = blockIdx.x, b = blockIdx.y;
  const int r0 = p * rpp, r1 = min(HW, r0 + rpp);
  const size_t base = (size_t)b * HW * C + c;
  float s1[8], s2[8], mu[8], rs[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s1[k] = s2[k] = 0.f;
  if constexpr (NS == 2) {
    ldp(mean, c, mu);
    ldp(rstd, c, rs);
  }
  for (int r = r0 + rsub; r < r1; r += rp) {
    const size_t e = base + (size_t)r * C;
    float v[8];
    ldv(y, ydt, e, v);
    if constexpr (NS == 1) {
#pragma unroll
      for (int k = 0; k < 8; ++k) s1[k] += v[k];
    } else {
      float g[8], a[8];
      ldv(dout, ddt, e, g);
      ldv(act, adt, e, a);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        g[k] = a[k] > 0.f ? g[k] : 0.f;
        s1[k] += g[k];
        s2[k] = fmaf(g[k], (v[k] - mu[k]) * rs[k], s2[k]);
      }
      stv(dout, ddt, e, g);
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    red[0][k][t] = s1[k];
    if constexpr (NS == 2) red[1][k][t] = s2[k];
  }
  __syncthreads();
  if (rsub == 0) {
    for (int j = 1; j < rp; ++j) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        s1[k] += red[0][k][j * tpr + cg];
        if constexpr (NS == 2) s2[k] += red[1][k][j * tpr + cg];
      }
    }
    float* o = part + ((size_t)b * P + p) * NS * C + c;
    *reinterpret_cast<float4*>(o) = make_float4(s1[0], s1[1], s1[2], s1[3]);
    *reinterpret_cast<float4*>(o + 4) = make_float4(s1[4], s1[5], s1[6], s1[7]);
    if constexpr (NS == 2) {
      *reinterpret_cast<float4*>(o + C) = make_float4(s2[0], s2[1], s2[2], s2[3]);
      *reinterpret_cast<float4*>(o + C + 4) = make_float4(s2[4], s2[5], s2[6], s2[7]);
    }
  }
}

// ---- excite: out[b][n] = f(W[n][:] . x[b][:] + bias[n]) ---------------------------------------------------------
// grid (ceil(N / 32), B), 4 waves x 8 rows.  FC = 1: x = the BatchNorm of the folded squeeze partials (workgroup
// x = 0 also stores ymean and pooled), f = ReLU;  FC = 2: x = hidden, f = sigmoid.
constexpr int kFcRows = 32;
struct FcArgs {
  const float *part, *mean, *rstd, *gamma, *beta;  // FC 1
  float *ymean, *pooled;                           // FC 1
  const float* x;                                  // FC 2
  const float *W, *bias;
  float* out;
  int P, N, K;
  float inv_hw;
};
template <int FC>
__global__ void __launch_bounds__(kThreads) fc_kernel(FcArgs a) {
  __shared__ float xs[kMaxC];
  const int t = threadIdx.x, b = blockIdx.y, K = a.K;
  if constexpr (FC == 1) {
    for (int c = t; c < K; c += kThreads) {
      float s = 0.f;
      for (int p = 0; p < a.P; ++p) s += a.part[((size_t)b * a.P + p) * K + c];
      const float m = s * a.inv_hw;
      const float z = fmaf(a.gamma[c] * a.rstd[c], m - a.mean[c], a.beta[c]);
      xs[c] = z;
      if (blockIdx.x == 0) {
        a.ymean[(size_t)b * K + c] = m;
        a.pooled[(size_t)b * K + c] = z;
      }
    }
  } else {
    for (int k = t; k < K; k += kThreads) xs[k] = a.x[(size_t)b * K + k];
  }
  __syncthreads();
  matvec_rows<kFcRows>(xs, a.W, a.bias, a.N, K, [&](int n, float v) {
    a.out[(size_t)b * a.N + n] = FC == 1 ? fmaxf(v, 0.f) : 1.0f / (1.0f + expf(-v));
  });
}

// ---- join: out = relu(z * gate + shortcut) --------------------------------------------------------------------------
struct JoinArgs {
  const void *y, *res;
  const float *mean, *rstd, *gamma, *beta, *gate, *rmean, *rrstd, *rgamma, *rbeta;
  void* out;
  int ydt, rdt, odt, HW, C;
};
__global__ void __launch_bounds__(kThreads) join_kernel(JoinArgs a) {
  const int b = blockIdx.y, C = a.C, tpr = C / 8;
  const int64_t n8 = (int64_t)a.HW * tpr;
  const size_t img = (size_t)b * a.HW * C;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n8; i += (int64_t)gridDim.x * kThreads) {
    const int c = (int)(i % tpr) * 8;
    const size_t e = img + (size_t)i * 8;
    float v[8], r[8], mu[8], rs[8], ga[8], be[8], g[8], o[8];
    ldv(a.y, a.ydt, e, v);
    ldv(a.res, a.rdt, e, r);
    ldp(a.mean, c, mu);
    ldp(a.rstd, c, rs);
    ldp(a.gamma, c, ga);
    ldp(a.beta, c, be);
    ldp(a.gate + (size_t)b * C, c, g);
    if (a.rmean) {
      float m2[8], r2[8], g2[8], b2[8];
      ldp(a.rmean, c, m2);
      ldp(a.rrstd, c, r2);
      ldp(a.rgamma, c, g2);
      ldp(a.rbeta, c, b2);
#pragma unroll
      for (int k = 0; k < 8; ++k) r[k] = fmaf(g2[k] * r2[k], r[k] - m2[k], b2[k]);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float z = fmaf(ga[k] * rs[k], v[k] - mu[k], be[k]);
      o[k] = fmaxf(fmaf(z, g[k], r[k]), 0.f);
    }
    stv(a.out, a.odt, e, o);
  }
}

// ---- gate backward ------------------------------------------------------------------------------------------------
// out[b][n] = sum_k v[b][k] W[k][n]; grid (ceil(N / 64), B); thread (q = t / 16, 4 columns at (t % 16) * 4).
// TM = 1: v = dsig[b][c] = dgate * gate (1 - gate), dgate = gamma sum g xhat + beta sum g from the folded bwd_stats
//         partials (workgroup x = 0 also stores dsig and the two folded sums), W = w2 [C][rd], out = dhidden masked by
//         hidden > 0;
// TM = 2: v = dhidden, W = w1 [rd][C], out = dpool.
struct TmArgs {
  const float *part, *gamma, *beta, *gate, *hidden;  // TM 1
  float *dsig, *sg, *sgx;                            // TM 1
  const float* v;                                    // TM 2
  const float* W;
  float* out;
  int P, N, K;
};
template <int TM>
__global__ void __launch_bounds__(kThreads) tmatvec_kernel(TmArgs a) {
  __shared__ float vs[kMaxC];
  __shared__ float red[16][64];
  const int t = threadIdx.x, b = blockIdx.y, K = a.K, N = a.N;
  if constexpr (TM == 1) {
    for (int c = t; c < K; c += kThreads) {
      float s1 = 0.f, s2 = 0.f;
      for (int p = 0; p < a.P; ++p) {
        const float* q = a.part + ((size_t)b * a.P + p) * 2 * K;
        s1 += q[c];
        s2 += q[K + c];
      }
      const float g = a.gate[(size_t)b * K + c];
      const float dgate = fmaf(a.gamma[c], s2, a.beta[c] * s1);
      const float ds = dgate * (g * (1.0f - g));
      vs[c] = ds;
      if (blockIdx.x == 0) {
        a.dsig[(size_t)b * K + c] = ds;
        a.sg[(size_t)b * K + c] = s1;
        a.sgx[(size_t)b * K + c] = s2;
      }
    }
  } else {
    for (int k = t; k < K; k += kThreads) vs[k] = a.v[(size_t)b * K + k];
  }
  __syncthreads();
  tmatvec_cols(vs, red, a.W, N, K, [&](int n, float s) {
    if constexpr (TM == 1) s = a.hidden[(size_t)b * N + n] > 0.f ? s : 0.f;
    a.out[(size_t)b * N + n] = s;
  });
}

// the BatchNorm's sums of dz = g * gate + dpool / HW over (b, hw):  sums[0][c] = sum dz,  sums[1][c] = sum dz xhat
// (sum_hw xhat = HW (ymean - mean) rstd);  dbeta += sums[0], dgamma += sums[1];  eval mode stores zero sums
__global__ void __launch_bounds__(kThreads) bn_sums_kernel(const float* __restrict__ sg, const float* __restrict__ sgx,
                                                           const float* __restrict__ gate, const float* __restrict__ dpool,
                                                           const float* __restrict__ ymean, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, float* __restrict__ sums,
                                                           float* dgamma, float* dbeta, int batch_stats, int B, int C) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= C) return;
  const float mu = mean[c], rs = rstd[c];
  float s0 = 0.f, s1 = 0.f;
  for (int b = 0; b < B; ++b) {
    const size_t i = (size_t)b * C + c;
    const float g = gate[i], dp = dpool[i];
    s0 += fmaf(g, sg[i], dp);
    s1 += fmaf(g, sgx[i], dp * ((ymean[i] - mu) * rs));
  }
  if (dbeta) dbeta[c] += s0;
  if (dgamma) dgamma[c] += s1;
  sums[c] = batch_stats ? s0 : 0.f;
  sums[C + c] = batch_stats ? s1 : 0.f;
}

// dy = gamma rstd (g gate + dpool / HW - sums0 / n - xhat sums1 / n),  n = B HW
struct ApplyArgs {
  const void *g, *y;
  const float *mean, *rstd, *gamma, *gate, *dpool, *sums;
  void* dx;
  int gdt, ydt, xdt, HW, C;
  float inv_hw, inv_n;
};
__global__ void __launch_bounds__(kThreads) apply_kernel(ApplyArgs a) {
  const int b = blockIdx.y, C = a.C, tpr = C / 8;
  const int64_t n8 = (int64_t)a.HW * tpr;
  const size_t img = (size_t)b * a.HW * C;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n8; i += (int64_t)gridDim.x * kThreads) {
    const int c = (int)(i % tpr) * 8;
    const size_t e = img + (size_t)i * 8;
    float g[8], v[8], mu[8], rs[8], ga[8], gt[8], dp[8], s0[8], s1[8], o[8];
    ldv(a.g, a.gdt, e, g);
    ldv(a.y, a.ydt, e, v);
    ldp(a.mean, c, mu);
    ldp(a.rstd, c, rs);
    ldp(a.gamma, c, ga);
    ldp(a.gate + (size_t)b * C, c, gt);
    ldp(a.dpool + (size_t)b * C, c, dp);
    ldp(a.sums, c, s0);
    ldp(a.sums + C, c, s1);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float dz = fmaf(g[k], gt[k], dp[k] * a.inv_hw);
      const float a1 = fmaf(-s0[k], a.inv_n, dz);
      const float xs = ((v[k] - mu[k]) * rs[k]) * s1[k];
      o[k] = (ga[k] * rs[k]) * fmaf(-xs, a.inv_n, a1);
    }
    stv(a.dx, a.xdt, e, o);
  }
}

// ---- AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False) ---------------------------------------------------------
// grid (x over OW * C / 8, OH, B) forward; (x over W * C / 8, H, B) backward
__global__ void __launch_bounds__(kThreads) pool2_fwd_kernel(const void* __restrict__ x, int dt, void* __restrict__ y,
                                                             int H, int W, int C) {
  const int OH = (H + 1) / 2, OW = (W + 1) / 2, c8 = C / 8;
  const int oy = blockIdx.y, b = blockIdx.z;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < OW * c8; i += gridDim.x * kThreads) {
    const int ox = i / c8, c = (i % c8) * 8;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
    for (int ky = 0; ky < 2; ++ky) {
      const int iy = 2 * oy + ky;
      if (iy >= H) continue;
      for (int kx = 0; kx < 2; ++kx) {
        const int ix = 2 * ox + kx;
        if (ix >= W) continue;
        float v[8];
        ldv(x, dt, (((size_t)b * H + iy) * W + ix) * C + c, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] += v[k];
        ++cnt;
      }
    }
    const float inv = cnt == 4 ? 0.25f : cnt == 2 ? 0.5f : 1.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] *= inv;
    stv(y, dt, (((size_t)b * OH + oy) * OW + ox) * C + c, s);
  }
}
__global__ void __launch_bounds__(kThreads) pool2_bwd_kernel(const void* __restrict__ dout, int ddt, void* __restrict__ dx,
                                                             int xdt, int H, int W, int C) {
  const int OH = (H + 1) / 2, OW = (W + 1) / 2, c8 = C / 8;
  const int iy = blockIdx.y, b = blockIdx.z;
  const int ny = (iy | 1) < H ? 2 : 1;  // valid rows of this pixel's window
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < W * c8; i += gridDim.x * kThreads) {
    const int ix = i / c8, c = (i % c8) * 8;
    const int cnt = ny * ((ix | 1) < W ? 2 : 1);
    const float inv = cnt == 4 ? 0.25f : cnt == 2 ? 0.5f : 1.0f;
    float g[8];
    ldv(dout, ddt, (((size_t)b * OH + iy / 2) * OW + ix / 2) * C + c, g);
#pragma unroll
    for (int k = 0; k < 8; ++k) g[k] *= inv;
    stv(dx, xdt, (((size_t)b * H + iy) * W + ix) * C + c, g);
  }
}

static int row_grid(int64_t groups) {
  int64_t g = (groups + kThreads - 1) / kThreads;
  return (int)(g < 1 ? 1 : g > 1024 ? 1024 : g);
}

}  // namespace se
}  // namespace sv

using namespace sv;
using namespace sv::se;

extern "C" int sv_se_nparts(int32_t HW, int32_t C) { return (c_ok(C) && HW > 0) ? nparts_for(HW, C) : 0; }

extern "C" int sv_se_squeeze(const void* y, int32_t y_dtype, float* part, int32_t B, int32_t HW, int32_t C,
                             sv_stream_t stream) {
  SV_REQUIRE(y && part && B > 0 && B <= 65535 && HW > 0 && c_ok(C) && dt_ok(y_dtype), "sv_se_squeeze: bad arguments");
  const int P = nparts_for(HW, C), rpp = (HW + P - 1) / P;
  sums_kernel<1><<<dim3(P, B), kThreads, 0, (hipStream_t)stream>>>(y, y_dtype, nullptr, 0, nullptr, 0, nullptr, nullptr,
                                                                   part, HW, C, P, rpp);
  return check_launch("sv_se_squeeze");
}

extern "C" int sv_se_excite(const float* part, int32_t nparts, const float* mean, const float* rstd, const float* gamma,
                            const float* beta, const float* w1, const float* b1, const float* w2, const float* b2,
                            float* ymean, float* pooled, float* hidden, float* gate, int32_t B, int32_t HW, int32_t C,
                            int32_t rd, sv_stream_t stream) {
  SV_REQUIRE(part && mean && rstd && gamma && beta && w1 && b1 && w2 && b2 && ymean && pooled && hidden && gate,
             "sv_se_excite: null argument");
  SV_REQUIRE(B > 0 && B <= 65535 && HW > 0 && c_ok(C) && rd >= 4 && rd % 4 == 0 && rd <= kMaxC && nparts >= 1 &&
                 nparts <= kMaxParts, "sv_se_excite: unsupported shape B=%d HW=%d C=%d rd=%d nparts=%d", B, HW, C, rd, nparts);
  FcArgs a{};
  a.part = part; a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta;
  a.ymean = ymean; a.pooled = pooled;
  a.W = w1; a.bias = b1; a.out = hidden;
  a.P = nparts; a.N = rd; a.K = C;
  a.inv_hw = 1.0f / (float)HW;
  fc_kernel<1><<<dim3((rd + kFcRows - 1) / kFcRows, B), kThreads, 0, (hipStream_t)stream>>>(a);
  if (int rc = check_launch("sv_se_excite: fc1")) return rc;
  FcArgs f{};
  f.x = hidden; f.W = w2; f.bias = b2; f.out = gate;
  f.N = C; f.K = rd;
  fc_kernel<2><<<dim3((C + kFcRows - 1) / kFcRows, B), kThreads, 0, (hipStream_t)stream>>>(f);
  return check_launch("sv_se_excite: fc2");
}

extern "C" int sv_se_join_fwd(const void* y, int32_t y_dtype, const float* mean, const float* rstd, const float* gamma,
                              const float* beta, const float* gate, const void* res, int32_t res_dtype,
                              const float* res_mean, const float* res_rstd, const float* res_gamma,
                              const float* res_beta, void* out, int32_t out_dtype, int32_t B, int32_t HW, int32_t C,
                              sv_stream_t stream) {
  SV_REQUIRE(y && mean && rstd && gamma && beta && gate && res && out && B > 0 && B <= 65535 && HW > 0 && c_ok(C) &&
                 dt_ok(y_dtype) && dt_ok(res_dtype) && dt_ok(out_dtype), "sv_se_join_fwd: bad arguments");
  SV_REQUIRE(!res_mean || (res_rstd && res_gamma && res_beta), "sv_se_join_fwd: incomplete shortcut BatchNorm");
  JoinArgs a{};
  a.y = y; a.res = res; a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta; a.gate = gate;
  a.rmean = res_mean; a.rrstd = res_rstd; a.rgamma = res_gamma; a.rbeta = res_beta;
  a.out = out; a.ydt = y_dtype; a.rdt = res_dtype; a.odt = out_dtype; a.HW = HW; a.C = C;
  join_kernel<<<dim3(row_grid((int64_t)HW * C / 8), B), kThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch("sv_se_join_fwd");
}

extern "C" int sv_se_bwd_stats(void* dout, int32_t dout_dtype, const void* act, int32_t act_dtype, const void* y,
                               int32_t y_dtype, const float* mean, const float* rstd, float* part, int32_t B,
                               int32_t HW, int32_t C, sv_stream_t stream) {
  SV_REQUIRE(dout && act && y && mean && rstd && part && B > 0 && B <= 65535 && HW > 0 && c_ok(C) && dt_ok(dout_dtype) &&
                 dt_ok(act_dtype) && dt_ok(y_dtype), "sv_se_bwd_stats: bad arguments");
  const int P = nparts_for(HW, C), rpp = (HW + P - 1) / P;
  sums_kernel<2><<<dim3(P, B), kThreads, 0, (hipStream_t)stream>>>(y, y_dtype, dout, dout_dtype, act, act_dtype, mean,
                                                                   rstd, part, HW, C, P, rpp);
  return check_launch("sv_se_bwd_stats");
}

extern "C" int sv_se_bwd_gate(const float* part, int32_t nparts, const float* ymean, const float* pooled,
                              const float* hidden, const float* gate, const float* mean, const float* rstd,
                              const float* gamma, const float* beta, const float* w1, const float* w2, float* work,
                              float* dpool, float* sums, float* dgamma, float* dbeta, float* dw1, float* db1,
                              float* dw2, float* db2, int32_t batch_stats, int32_t B, int32_t HW, int32_t C, int32_t rd,
                              sv_stream_t stream) {
  SV_REQUIRE(part && ymean && pooled && hidden && gate && mean && rstd && gamma && beta && w1 && w2 && work && dpool &&
                 sums && dw1 && db1 && dw2 && db2, "sv_se_bwd_gate: null argument");
  SV_REQUIRE(B > 0 && B <= 65535 && HW > 0 && c_ok(C) && rd >= 4 && rd % 4 == 0 && rd <= kMaxC && nparts >= 1 &&
                 nparts <= kMaxParts, "sv_se_bwd_gate: unsupported shape B=%d HW=%d C=%d rd=%d nparts=%d", B, HW, C, rd,
             nparts);
  hipStream_t s = (hipStream_t)stream;
  // work: dsig [B][C], sum g [B][C], sum g xhat [B][C], dhidden [B][rd]
  float *dsig = work, *sg = work + (size_t)B * C, *sgx = work + (size_t)2 * B * C, *dh = work + (size_t)3 * B * C;
  TmArgs a{};
  a.part = part; a.gamma = gamma; a.beta = beta; a.gate = gate; a.hidden = hidden;
  a.dsig = dsig; a.sg = sg; a.sgx = sgx;
  a.W = w2; a.out = dh; a.P = nparts; a.N = rd; a.K = C;
  tmatvec_kernel<1><<<dim3((rd + 63) / 64, B), kThreads, 0, s>>>(a);
  if (int rc = check_launch("sv_se_bwd_gate: fc2^T")) return rc;
  TmArgs p{};
  p.v = dh; p.W = w1; p.out = dpool; p.N = C; p.K = rd;
  tmatvec_kernel<2><<<dim3((C + 63) / 64, B), kThreads, 0, s>>>(p);
  if (int rc = check_launch("sv_se_bwd_gate: fc1^T")) return rc;
  launch_outer(dsig, hidden, dw2, db2, B, C, rd, s);
  if (int rc = check_launch("sv_se_bwd_gate: dw2")) return rc;
  launch_outer(dh, pooled, dw1, db1, B, rd, C, s);
  if (int rc = check_launch("sv_se_bwd_gate: dw1")) return rc;
  bn_sums_kernel<<<(C + kThreads - 1) / kThreads, kThreads, 0, s>>>(sg, sgx, gate, dpool, ymean, mean, rstd, sums, dgamma,
                                                                  dbeta, batch_stats, B, C);
  return check_launch("sv_se_bwd_gate: BatchNorm sums");
}

extern "C" int sv_se_bwd_apply(const void* g, int32_t g_dtype, const void* y, int32_t y_dtype, const float* mean,
                               const float* rstd, const float* gamma, const float* gate, const float* dpool,
                               const float* sums, void* dx, int32_t dx_dtype, int32_t B, int32_t HW, int32_t C,
                               sv_stream_t stream) {
  SV_REQUIRE(g && y && mean && rstd && gamma && gate && dpool && sums && dx && B > 0 && B <= 65535 && HW > 0 && c_ok(C) &&
                 dt_ok(g_dtype) && dt_ok(y_dtype) && dt_ok(dx_dtype), "sv_se_bwd_apply: bad arguments");
  ApplyArgs a{};
  a.g = g; a.y = y; a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.gate = gate; a.dpool = dpool; a.sums = sums;
  a.dx = dx; a.gdt = g_dtype; a.ydt = y_dtype; a.xdt = dx_dtype; a.HW = HW; a.C = C;
  a.inv_hw = 1.0f / (float)HW;
  a.inv_n = 1.0f / ((float)B * (float)HW);
  apply_kernel<<<dim3(row_grid((int64_t)HW * C / 8), B), kThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch("sv_se_bwd_apply");
}

extern "C" int sv_avgpool2x2_fwd(const void* x, int32_t dtype, void* y, int32_t B, int32_t H, int32_t W, int32_t C,
                                 sv_stream_t stream) {
  SV_REQUIRE(x && y && B > 0 && B <= 65535 && H > 0 && H <= 65535 && W > 0 && C > 0 && C % 8 == 0 && dt_ok(dtype) &&
                 (int64_t)W * C < (1ll << 31), "sv_avgpool2x2_fwd: bad arguments");
  const int OH = (H + 1) / 2, OW = (W + 1) / 2;
  pool2_fwd_kernel<<<dim3(row_grid((int64_t)OW * C / 8), OH, B), kThreads, 0, (hipStream_t)stream>>>(x, dtype, y, H, W, C);
  return check_launch("sv_avgpool2x2_fwd");
}

extern "C" int sv_avgpool2x2_bwd(const void* dout, int32_t dout_dtype, void* dx, int32_t dx_dtype, int32_t B, int32_t H,
                                 int32_t W, int32_t C, sv_stream_t stream) {
  SV_REQUIRE(dout && dx && B > 0 && B <= 65535 && H > 0 && H <= 65535 && W > 0 && C > 0 && C % 8 == 0 &&
                 dt_ok(dout_dtype) && dt_ok(dx_dtype) && (int64_t)W * C < (1ll << 31), "sv_avgpool2x2_bwd: bad arguments");
  pool2_bwd_kernel<<<dim3(row_grid((int64_t)W * C / 8), H, B), kThreads, 0, (hipStream_t)stream>>>(dout, dout_dtype, dx,
                                                                                                dx_dtype, H, W, C);
  return check_launch("sv_avgpool2x2_bwd");
}
