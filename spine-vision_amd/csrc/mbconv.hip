// MBConv pieces of the EfficientNetV2 backbones (gfx950), NHWC: depthwise 3x3 convolution, BatchNorm + SiLU, and the
// squeeze-and-excitation that gates the expanded activation in front of the project convolution.
//
// Replaces, with their autograd backward, timm's InvertedResidual between its 1x1 convolutions
// (timm/models/_efficientnet_blocks.py: x = bn1(conv_pw(x)); x = bn2(conv_dw(x)); x = se(x); x = bn3(conv_pwl(x))), the
// BatchNormAct2d(act=SiLU) of every block type, and SqueezeExcite(act=SiLU, gate=sigmoid).
//
//   pre = gamma (y - mean) rstd + beta = fmaf(gamma * rstd, y - mean, beta)      (f32, the same expression everywhere)
//   sig(x) = 1 / (1 + expf(-x)),  silu(x) = x sig(x),  silu'(x) = sig(x) (1 + x (1 - sig(x)))
//   s = silu(pre)                      the activated depthwise output; never stored, every pass recomputes it from y
//   pooled[b][c] = (1 / HW) sum_hw s,  hidden = silu(w1 pooled + b1),  gate = sigmoid(w2 hidden + b2)   (f32, per image)
//   a = s * gate[b][c]                 the project GEMM's operand (stored)
//
// Every pass reads 8 consecutive channels per thread (16 B in bf16, 2 x 16 B in f32), computes in f32 and rounds once, at
// the store.  No atomics: every sum has one fixed order, an image's gate depends on that image's rows alone, nothing
// synchronises with the host.  Summation orders and rounding points (the tests derive their bounds from them):
//   * depthwise taps: one accumulator per element, fmaf over (ky, kx) ascending, taps in the padding skipped;
//   * channel sums over rows (forward statistics, bn_silu_bwd_stats, the per-image squeeze / backward sums, the
//     depthwise weight gradient): a workgroup owns 32 channels and one part of the rows (P = sv_mbconv_nparts parts of
//     rpp = ceil(rows / P) rows); thread (lane q = t / 4, channel group t % 4) adds rows r0 + q, + 64, ... ascending into
//     one accumulator per channel (fmaf where a product is summed); the 64 lanes are added in two levels (lane q < 8
//     adds lanes q + 8, q + 16, ... ascending, then lane 0 adds lanes 1 .. 7 ascending); the consumer adds the P parts in
//     part order;
//   * sv_mbse_bwd_apply rounds dpre to the output dtype first and sums the ROUNDED value (the BatchNorm apply pass reads
//     the stored tensor);
//   * the matvec rows (fc1, fc2), the transposed matvec columns (the gate backward) and the outer products over the
//     batch (the gate's weight gradients): se_core.h.
#include <math.h>

#include "chanvec.h"
#include "common.h"
#include "se_core.h"

namespace sv {
namespace mb {

constexpr int kThreads = 256;
constexpr int kMaxC = 3840;
constexpr int kMaxParts = 64;
constexpr int kSlab = 32;  // channels per reduction workgroup

// the value a store in dtype dt leaves in memory
__device__ __forceinline__ float rnd(float v, int dt) { return dt == SV_F32 ? v : bf2f(f2bf(v)); }

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float silu_f(float x) { return x * sigmoid_f(x); }
__device__ __forceinline__ float silu_grad_f(float x) {
  const float s = sigmoid_f(x);
  return s * fmaf(x, 1.0f - s, 1.0f);
}

// the BatchNorm of 8 channels: pre = fmaf(gamma * rstd, y - mean, beta), xhat = (y - mean) * rstd
struct Bn8 {
  float mu[8], rs[8], ga[8], be[8];
  __device__ __forceinline__ void load(const float* mean, const float* rstd, const float* gamma, const float* beta, int c) {
    ldp(mean, c, mu);
    ldp(rstd, c, rs);
    ldp(gamma, c, ga);
    ldp(beta, c, be);
  }
  __device__ __forceinline__ float pre(float y, int k) const { return fmaf(ga[k] * rs[k], y - mu[k], be[k]); }
  __device__ __forceinline__ float xhat(float y, int k) const { return (y - mu[k]) * rs[k]; }
};

static bool c_ok(int C) { return C >= kSlab && C <= kMaxC && C % kSlab == 0; }

static int nparts_for(int64_t rows) {
  int64_t p = rows / (64 * 8);  // >= 8 rows per thread
  if (p > kMaxParts) p = kMaxParts;
  if (p < 1) p = 1;
  return (int)p;
}
static int flat_grid(int64_t groups) {
  int64_t g = (groups + kThreads - 1) / kThreads;
  return (int)(g < 1 ? 1 : g > 2048 ? 2048 : g);
}

// the 64 row-lanes of each of the workgroup's 4 channel groups, added in two levels; the sum lands in lane 0 (t < 4)
__device__ __forceinline__ void lanes_sum(float (&v)[8], float (*red)[kThreads]) {
  const int t = threadIdx.x, q = t >> 2, cg = t & 3;
#pragma unroll
  for (int k = 0; k < 8; ++k) red[k][t] = v[k];
  __syncthreads();
  if (q < 8) {
    for (int j = 1; j < 8; ++j) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] += red[k][((q + 8 * j) << 2) | cg];
    }
  }
  __syncthreads();
  if (q < 8) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red[k][t] = v[k];
  }
  __syncthreads();
  if (q == 0) {
    for (int j = 1; j < 8; ++j) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] += red[k][(j << 2) | cg];
    }
  }
  __syncthreads();
}

// ---- channel sums over rows ---------------------------------------------------------------------------------------
// grid (P, C / 32, B): image b's rows [p rpp, (p + 1) rpp) of the workgroup's 32 channels; B = 1 for sums over all rows.
//   STATS     part[p][2][C]        = (sum y, sum y^2)                            forward BatchNorm statistics
//   SILU_BWD  part[p][2][C]        = (sum g, sum g xhat), g = d silu'(pre)
//   SQUEEZE   part[b][p][C]        = sum silu(pre)
//   GATE_BWD  part[b][p][C]        = sum d silu(pre)
//   APPLY     part[b P + p][2][C]  = (sum r, sum r xhat), r = the stored rnd((d gate + dpool / HW) silu'(pre))
enum { STATS = 0, SILU_BWD = 1, SQUEEZE = 2, GATE_BWD = 3, APPLY = 4 };
struct SumArgs {
  const void *y, *d;
  const float *mean, *rstd, *gamma, *beta, *gate, *dpool;
  void* out;
  float* part;
  int ydt, ddt, odt, C, P;
  int64_t HW, rpp;
  float inv_hw;
};
template <int MODE>
__global__ void __launch_bounds__(kThreads) sums_kernel(SumArgs a) {
  constexpr int NS = (MODE == SQUEEZE || MODE == GATE_BWD) ? 1 : 2;
  __shared__ float red[8][kThreads];
  const int t = threadIdx.x, q = t >> 2, cg = t & 3;
  const int p = blockIdx.x, b = blockIdx.z, C = a.C, c = blockIdx.y * kSlab + cg * 8;
  const int64_t r0 = p * a.rpp, r1 = r0 + a.rpp < a.HW ? r0 + a.rpp : a.HW;
  const size_t base = (size_t)b * a.HW * C + c;
  float s1[8], s2[8], gt[8], dp[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s1[k] = s2[k] = 0.f;
  Bn8 bn;
  if constexpr (MODE != STATS) bn.load(a.mean, a.rstd, a.gamma, a.beta, c);
  if constexpr (MODE == APPLY) {
    ldp(a.gate + (size_t)b * C, c, gt);
    ldp(a.dpool + (size_t)b * C, c, dp);
  }
  for (int64_t r = r0 + q; r < r1; r += 64) {
    const size_t e = base + (size_t)r * C;
    float v[8], d[8], o[8];
    ldv(a.y, a.ydt, e, v);
    if constexpr (MODE == SILU_BWD || MODE == GATE_BWD || MODE == APPLY) ldv(a.d, a.ddt, e, d);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if constexpr (MODE == STATS) {
        s1[k] += v[k];
        s2[k] = fmaf(v[k], v[k], s2[k]);
      } else if constexpr (MODE == SILU_BWD) {
        const float g = d[k] * silu_grad_f(bn.pre(v[k], k));
        s1[k] += g;
        s2[k] = fmaf(g, bn.xhat(v[k], k), s2[k]);
      } else if constexpr (MODE == SQUEEZE) {
        s1[k] += silu_f(bn.pre(v[k], k));
      } else if constexpr (MODE == GATE_BWD) {
        s1[k] = fmaf(d[k], silu_f(bn.pre(v[k], k)), s1[k]);
      } else {
        o[k] = rnd(fmaf(d[k], gt[k], dp[k] * a.inv_hw) * silu_grad_f(bn.pre(v[k], k)), a.odt);
        s1[k] += o[k];
        s2[k] = fmaf(o[k], bn.xhat(v[k], k), s2[k]);
      }
    }
    if constexpr (MODE == APPLY) stv(a.out, a.odt, e, o);
  }
  lanes_sum(s1, red);
  if constexpr (NS == 2) lanes_sum(s2, red);
  if (q == 0) {
    float* o = a.part + ((size_t)b * a.P + p) * NS * C + c;
    stp(o, s1);
    if constexpr (NS == 2) stp(o + C, s2);
  }
}

// ---- BatchNorm + SiLU ---------------------------------------------------------------------------------------------
struct ActArgs {
  const void *y, *d, *res;
  const float *mean, *rstd, *gamma, *beta, *gate, *sums;
  void* out;
  int ydt, ddt, rdt, odt, C;
  int64_t HW;  // rows of one image (grid y = B), or all rows (grid y = 1)
  float inv_n;
};
// FWD: out = silu(pre) (+ res);  SCALE: out = silu(pre) * gate[b][c];
// BWD: out = gamma rstd (g - sums[0] / n - xhat sums[1] / n), g = d silu'(pre)
enum { FWD = 0, SCALE = 1, BWD = 2 };
template <int MODE>
__global__ void __launch_bounds__(kThreads) act_kernel(ActArgs a) {
  const int b = blockIdx.y, C = a.C, tpr = C / 8;
  const int64_t n8 = a.HW * tpr;
  const size_t img = (size_t)b * a.HW * C;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n8; i += (int64_t)gridDim.x * kThreads) {
    const int c = (int)(i % tpr) * 8;
    const size_t e = img + (size_t)i * 8;
    float v[8], o[8];
    Bn8 bn;
    ldv(a.y, a.ydt, e, v);
    bn.load(a.mean, a.rstd, a.gamma, a.beta, c);
    if constexpr (MODE == FWD) {
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = silu_f(bn.pre(v[k], k));
      if (a.res) {
        float r[8];
        ldv(a.res, a.rdt, e, r);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] += r[k];
      }
    } else if constexpr (MODE == SCALE) {
      float g[8];
      ldp(a.gate + (size_t)b * C, c, g);
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = silu_f(bn.pre(v[k], k)) * g[k];
    } else {
      float d[8], s0[8], s1[8];
      ldv(a.d, a.ddt, e, d);
      ldp(a.sums, c, s0);
      ldp(a.sums + C, c, s1);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float g = d[k] * silu_grad_f(bn.pre(v[k], k));
        const float a1 = fmaf(-s0[k], a.inv_n, g);
        const float xs = bn.xhat(v[k], k) * s1[k];
        o[k] = (bn.ga[k] * bn.rs[k]) * fmaf(-xs, a.inv_n, a1);
      }
    }
    stv(a.out, a.odt, e, o);
  }
}

// dst += src (the identity shortcut's gradient joining the block-input gradient); the sum in f32, rounded once
__global__ void __launch_bounds__(kThreads) add_kernel(void* dst, int ddt, const void* src, int sdt, int64_t n8) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n8; i += (int64_t)gridDim.x * kThreads) {
    float x[8], y[8];
    ldv(dst, ddt, (size_t)i * 8, x);
    ldv(src, sdt, (size_t)i * 8, y);
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] += y[k];
    stv(dst, ddt, (size_t)i * 8, x);
  }
}

// ---- depthwise 3x3, pad 1, stride 1 | 2 ---------------------------------------------------------------------------
// w is the torch weight [C][1][3][3] f32: the 8 channels of a thread are 72 consecutive floats
struct DwArgs {
  const void *x, *dy;
  const float* w;
  void* out;
  float* part;
  int xdt, ddt, odt, B, H, W, OH, OW, C, stride, P;
  int64_t rpp;
};
__device__ __forceinline__ void ldw(const float* w, int c, float (&o)[72]) {
  const float4* p = reinterpret_cast<const float4*>(w + (size_t)c * 9);
#pragma unroll
  for (int j = 0; j < 18; ++j) {
    const float4 v = p[j];
    o[4 * j] = v.x; o[4 * j + 1] = v.y; o[4 * j + 2] = v.z; o[4 * j + 3] = v.w;
  }
}
// y[b][oy][ox][c] = sum_{ky,kx} x[b][oy s + ky - 1][ox s + kx - 1][c] w[c][ky][kx]
__global__ void __launch_bounds__(kThreads) dw_fwd_kernel(DwArgs a) {
  const int tpr = a.C / 8, s = a.stride;
  const int64_t n8 = (int64_t)a.B * a.OH * a.OW * tpr;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n8; i += (int64_t)gridDim.x * kThreads) {
    const int c = (int)(i % tpr) * 8;
    const int64_t pix = i / tpr;
    const int ox = (int)(pix % a.OW), oy = (int)((pix / a.OW) % a.OH), b = (int)(pix / ((int64_t)a.OW * a.OH));
    float wl[72], acc[8];
    ldw(a.w, c, wl);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * s + ky - 1;
      if (iy < 0 || iy >= a.H) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox * s + kx - 1;
        if (ix < 0 || ix >= a.W) continue;
        float v[8];
        ldv(a.x, a.xdt, (((size_t)b * a.H + iy) * a.W + ix) * a.C + c, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = fmaf(v[k], wl[k * 9 + ky * 3 + kx], acc[k]);
      }
    }
    stv(a.out, a.odt, (size_t)i * 8, acc);
  }
}
// dx[b][iy][ix][c] = sum_{ky,kx : (iy + 1 - ky) % s == 0, (ix + 1 - kx) % s == 0} dy[b][(iy + 1 - ky) / s][(ix + 1 - kx) / s][c] w[c][ky][kx]
__global__ void __launch_bounds__(kThreads) dw_bwd_data_kernel(DwArgs a) {
  const int tpr = a.C / 8, s = a.stride;
  const int64_t n8 = (int64_t)a.B * a.H * a.W * tpr;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n8; i += (int64_t)gridDim.x * kThreads) {
    const int c = (int)(i % tpr) * 8;
    const int64_t pix = i / tpr;
    const int ix = (int)(pix % a.W), iy = (int)((pix / a.W) % a.H), b = (int)(pix / ((int64_t)a.W * a.H));
    float wl[72], acc[8];
    ldw(a.w, c, wl);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int ty = iy + 1 - ky;
      if (ty < 0 || ty % s) continue;
      const int oy = ty / s;
      if (oy >= a.OH) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int tx = ix + 1 - kx;
        if (tx < 0 || tx % s) continue;
        const int ox = tx / s;
        if (ox >= a.OW) continue;
        float v[8];
        ldv(a.dy, a.ddt, (((size_t)b * a.OH + oy) * a.OW + ox) * a.C + c, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = fmaf(v[k], wl[k * 9 + ky * 3 + kx], acc[k]);
      }
    }
    stv(a.out, a.odt, (size_t)i * 8, acc);
  }
}
// part[p][tap][C] = sum over the part's output pixels of dy[pixel][c] x[pixel's tap][c]; grid (P, C / 32)
__global__ void __launch_bounds__(kThreads) dw_bwd_weight_kernel(DwArgs a) {
  __shared__ float red[8][kThreads];
  const int t = threadIdx.x, q = t >> 2, cg = t & 3, s = a.stride;
  const int p = blockIdx.x, c = blockIdx.y * kSlab + cg * 8;
  const int64_t rows = (int64_t)a.B * a.OH * a.OW;
  const int64_t r0 = p * a.rpp, r1 = r0 + a.rpp < rows ? r0 + a.rpp : rows;
  float acc[9][8];
#pragma unroll
  for (int j = 0; j < 9; ++j)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[j][k] = 0.f;
  for (int64_t r = r0 + q; r < r1; r += 64) {
    const int ox = (int)(r % a.OW), oy = (int)((r / a.OW) % a.OH), b = (int)(r / ((int64_t)a.OW * a.OH));
    float g[8];
    ldv(a.dy, a.ddt, (size_t)r * a.C + c, g);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * s + ky - 1;
      if (iy < 0 || iy >= a.H) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox * s + kx - 1;
        if (ix < 0 || ix >= a.W) continue;
        float v[8];
        ldv(a.x, a.xdt, (((size_t)b * a.H + iy) * a.W + ix) * a.C + c, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[ky * 3 + kx][k] = fmaf(g[k], v[k], acc[ky * 3 + kx][k]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    lanes_sum(acc[j], red);
    if (q == 0) stp(a.part + ((size_t)p * 9 + j) * a.C + c, acc[j]);
  }
}
// dw[c][tap] (+)= sum_p part[p][tap][c], p ascending
__global__ void __launch_bounds__(kThreads) dw_fold_kernel(const float* __restrict__ part, int P, int C, float* dw,
                                                           int accumulate) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= C * 9) return;
  const int c = i / 9, j = i % 9;
  float s = 0.f;
  for (int p = 0; p < P; ++p) s += part[((size_t)p * 9 + j) * C + c];
  dw[i] = accumulate ? dw[i] + s : s;
}

// ---- excite: out[b][n] = f(W[n][:] . x[b][:] + bias[n]) ---------------------------------------------------------
// grid (ceil(N / 32), B), 4 waves x 8 rows.  FC = 1: x = pooled = the folded squeeze partials / HW (workgroup x = 0 also
// stores pooled), out = hpre and hidden = silu(hpre);  FC = 2: x = hidden, out = gate = sigmoid.
constexpr int kFcRows = 32;
struct FcArgs {
  const float* part;  // FC 1
  float *pooled, *hidden;
  const float* x;  // FC 2
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
      xs[c] = m;
      if (blockIdx.x == 0) a.pooled[(size_t)b * K + c] = m;
    }
  } else {
    for (int k = t; k < K; k += kThreads) xs[k] = a.x[(size_t)b * K + k];
  }
  __syncthreads();
  matvec_rows<kFcRows>(xs, a.W, a.bias, a.N, K, [&](int n, float v) {
    if constexpr (FC == 1) {
      const size_t o = (size_t)b * a.N + n;  // spelled once: two spellings keep two row pointers live (2 VGPRs more)
      a.out[o] = v;
      a.hidden[o] = silu_f(v);
    } else {
      a.out[(size_t)b * a.N + n] = sigmoid_f(v);
    }
  });
}

// ---- gate backward ------------------------------------------------------------------------------------------------
// out[b][n] = sum_k v[b][k] W[k][n]; grid (ceil(N / 64), B); thread (q = t / 16, 4 columns at (t % 16) * 4).
// TM = 1: v = dsig[b][c] = dgate gate (1 - gate), dgate = the folded GATE_BWD partials (workgroup x = 0 also stores dsig),
//         W = w2 [C][rd], out = dhpre = (.) silu'(hpre);   TM = 2: v = dhpre, W = w1 [rd][C], out = dpool.
struct TmArgs {
  const float *part, *gate, *hpre;  // TM 1
  float* dsig;                      // TM 1
  const float* v;                   // TM 2
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
      float s = 0.f;
      for (int p = 0; p < a.P; ++p) s += a.part[((size_t)b * a.P + p) * K + c];
      const float g = a.gate[(size_t)b * K + c];
      const float ds = s * (g * (1.0f - g));
      vs[c] = ds;
      if (blockIdx.x == 0) a.dsig[(size_t)b * K + c] = ds;
    }
  } else {
    for (int k = t; k < K; k += kThreads) vs[k] = a.v[(size_t)b * K + k];
  }
  __syncthreads();
  tmatvec_cols(vs, red, a.W, N, K, [&](int n, float s) {
    if constexpr (TM == 1) s *= silu_grad_f(a.hpre[(size_t)b * N + n]);
    a.out[(size_t)b * N + n] = s;
  });
}

static bool bn_ok(const float* mean, const float* rstd, const float* gamma, const float* beta) {
  return mean && rstd && gamma && beta && al16(mean) && al16(rstd) && al16(gamma) && al16(beta);
}
static bool dw_ok(int B, int H, int W, int C, int stride) {
  return B > 0 && H > 0 && W > 0 && c_ok(C) && (stride == 1 || stride == 2);
}
static DwArgs dw_args(int B, int H, int W, int C, int stride) {
  DwArgs a{};
  a.B = B; a.H = H; a.W = W; a.C = C; a.stride = stride;
  a.OH = (H - 1) / stride + 1;
  a.OW = (W - 1) / stride + 1;
  return a;
}

}  // namespace mb
}  // namespace sv

using namespace sv;
using namespace sv::mb;

#define MB_UNSUPPORTED(cond, ...)                                          \
  do {                                                                     \
    if (!(cond)) return ::sv::set_error(SV_ERR_UNSUPPORTED, __VA_ARGS__);  \
  } while (0)

extern "C" int sv_mbconv_nparts(int64_t rows, int32_t C) { return (c_ok(C) && rows > 0) ? nparts_for(rows) : 0; }

extern "C" int sv_mbconv_bn_stats(const void* y, int32_t y_dtype, int64_t rows, int32_t C, float* part,
                                  sv_stream_t stream) {
  SV_REQUIRE(y && part && rows > 0 && dt_ok(y_dtype) && al16(y) && al16(part), "sv_mbconv_bn_stats: bad arguments");
  MB_UNSUPPORTED(c_ok(C), "sv_mbconv_bn_stats: C=%d must be a multiple of 32 up to 3840", (int)C);
  SumArgs a{};
  a.y = y; a.ydt = y_dtype; a.part = part; a.C = C; a.HW = rows;
  a.P = nparts_for(rows);
  a.rpp = (rows + a.P - 1) / a.P;
  sums_kernel<STATS><<<dim3(a.P, C / kSlab, 1), kThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch("sv_mbconv_bn_stats");
}

extern "C" int sv_bn_silu_fwd(const void* y, int32_t y_dtype, const float* mean, const float* rstd, const float* gamma,
                              const float* beta, const void* res, int32_t res_dtype, void* out, int32_t out_dtype,
                              int64_t rows, int32_t C, sv_stream_t stream) {
  SV_REQUIRE(y && out && rows > 0 && dt_ok(y_dtype) && dt_ok(out_dtype) && (!res || dt_ok(res_dtype)) && al16(y) &&
                 al16(out) && al16(res) && bn_ok(mean, rstd, gamma, beta), "sv_bn_silu_fwd: bad arguments");
  MB_UNSUPPORTED(c_ok(C), "sv_bn_silu_fwd: C=%d must be a multiple of 32 up to 3840", (int)C);
  ActArgs a{};
  a.y = y; a.ydt = y_dtype; a.res = res; a.rdt = res_dtype; a.out = out; a.odt = out_dtype;
  a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta; a.C = C; a.HW = rows;
  act_kernel<FWD><<<dim3(flat_grid(rows * (C / 8)), 1), kThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch("sv_bn_silu_fwd");
}

extern "C" int sv_bn_silu_bwd_stats(const void* dout, int32_t dout_dtype, const void* y, int32_t y_dtype,
                                    const float* mean, const float* rstd, const float* gamma, const float* beta,
                                    int64_t rows, int32_t C, float* part, sv_stream_t stream) {
  SV_REQUIRE(dout && y && part && rows > 0 && dt_ok(dout_dtype) && dt_ok(y_dtype) && al16(dout) && al16(y) &&
                 al16(part) && bn_ok(mean, rstd, gamma, beta), "sv_bn_silu_bwd_stats: bad arguments");
  MB_UNSUPPORTED(c_ok(C), "sv_bn_silu_bwd_stats: C=%d must be a multiple of 32 up to 3840", (int)C);
  SumArgs a{};
  a.y = y; a.ydt = y_dtype; a.d = dout; a.ddt = dout_dtype; a.part = part; a.C = C; a.HW = rows;
  a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta;
  a.P = nparts_for(rows);
  a.rpp = (rows + a.P - 1) / a.P;
  sums_kernel<SILU_BWD><<<dim3(a.P, C / kSlab, 1), kThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch("sv_bn_silu_bwd_stats");
}

extern "C" int sv_bn_silu_bwd_apply(const void* dout, int32_t dout_dtype, const void* y, int32_t y_dtype,
                                    const float* mean, const float* rstd, const float* gamma, const float* beta,
                                    const float* sums, void* dx, int32_t dx_dtype, int64_t rows, int32_t C,
                                    sv_stream_t stream) {
  SV_REQUIRE(dout && y && sums && dx && rows > 0 && dt_ok(dout_dtype) && dt_ok(y_dtype) && dt_ok(dx_dtype) &&
                 al16(dout) && al16(y) && al16(sums) && al16(dx) && bn_ok(mean, rstd, gamma, beta),
             "sv_bn_silu_bwd_apply: bad arguments");
  MB_UNSUPPORTED(c_ok(C), "sv_bn_silu_bwd_apply: C=%d must be a multiple of 32 up to 3840", (int)C);
  ActArgs a{};
  a.y = y; a.ydt = y_dtype; a.d = dout; a.ddt = dout_dtype; a.out = dx; a.odt = dx_dtype; a.sums = sums;
  a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta; a.C = C; a.HW = rows;
  a.inv_n = 1.0f / (float)rows;
  act_kernel<BWD><<<dim3(flat_grid(rows * (C / 8)), 1), kThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch("sv_bn_silu_bwd_apply");
}

extern "C" int sv_mbconv_add(void* dst, int32_t dst_dtype, const void* src, int32_t src_dtype, int64_t n,
                             sv_stream_t stream) {
  SV_REQUIRE(dst && src && n > 0 && n % 8 == 0 && dt_ok(dst_dtype) && dt_ok(src_dtype) && al16(dst) && al16(src),
             "sv_mbconv_add: bad arguments");
  add_kernel<<<flat_grid(n / 8), kThreads, 0, (hipStream_t)stream>>>(dst, dst_dtype, src, src_dtype, n / 8);
  return check_launch("sv_mbconv_add");
}

extern "C" int sv_dwconv3_fwd(const void* x, int32_t x_dtype, const float* w, void* y, int32_t y_dtype, int32_t B,
                              int32_t H, int32_t W, int32_t C, int32_t stride, sv_stream_t stream) {
  SV_REQUIRE(x && w && y && dt_ok(x_dtype) && dt_ok(y_dtype) && al16(x) && al16(w) && al16(y),
             "sv_dwconv3_fwd: bad arguments");
  MB_UNSUPPORTED(dw_ok(B, H, W, C, stride), "sv_dwconv3_fwd: unsupported shape B=%d H=%d W=%d C=%d stride=%d", (int)B,
                 (int)H, (int)W, (int)C, (int)stride);
  DwArgs a = dw_args(B, H, W, C, stride);
  a.x = x; a.xdt = x_dtype; a.w = w; a.out = y; a.odt = y_dtype;
  dw_fwd_kernel<<<flat_grid((int64_t)B * a.OH * a.OW * (C / 8)), kThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch("sv_dwconv3_fwd");
}

extern "C" int sv_dwconv3_bwd_data(const void* dy, int32_t dy_dtype, const float* w, void* dx, int32_t dx_dtype,
                                   int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride, sv_stream_t stream) {
  SV_REQUIRE(dy && w && dx && dt_ok(dy_dtype) && dt_ok(dx_dtype) && al16(dy) && al16(w) && al16(dx),
             "sv_dwconv3_bwd_data: bad arguments");
  MB_UNSUPPORTED(dw_ok(B, H, W, C, stride), "sv_dwconv3_bwd_data: unsupported shape B=%d H=%d W=%d C=%d stride=%d",
                 (int)B, (int)H, (int)W, (int)C, (int)stride);
  DwArgs a = dw_args(B, H, W, C, stride);
  a.dy = dy; a.ddt = dy_dtype; a.w = w; a.out = dx; a.odt = dx_dtype;
  dw_bwd_data_kernel<<<flat_grid((int64_t)B * H * W * (C / 8)), kThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch("sv_dwconv3_bwd_data");
}

extern "C" int sv_dwconv3_bwd_weight_nparts(int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride) {
  if (!dw_ok(B, H, W, C, stride)) return 0;
  return nparts_for((int64_t)B * ((H - 1) / stride + 1) * ((W - 1) / stride + 1));
}

extern "C" int sv_dwconv3_bwd_weight(const void* dy, int32_t dy_dtype, const void* x, int32_t x_dtype, float* part,
                                     float* dw, int32_t accumulate, int32_t B, int32_t H, int32_t W, int32_t C,
                                     int32_t stride, sv_stream_t stream) {
  SV_REQUIRE(dy && x && part && dw && dt_ok(dy_dtype) && dt_ok(x_dtype) && al16(dy) && al16(x) && al16(part),
             "sv_dwconv3_bwd_weight: bad arguments");
  MB_UNSUPPORTED(dw_ok(B, H, W, C, stride), "sv_dwconv3_bwd_weight: unsupported shape B=%d H=%d W=%d C=%d stride=%d",
                 (int)B, (int)H, (int)W, (int)C, (int)stride);
  DwArgs a = dw_args(B, H, W, C, stride);
  a.dy = dy; a.ddt = dy_dtype; a.x = x; a.xdt = x_dtype; a.part = part;
  const int64_t rows = (int64_t)B * a.OH * a.OW;
  a.P = nparts_for(rows);
  a.rpp = (rows + a.P - 1) / a.P;
  dw_bwd_weight_kernel<<<dim3(a.P, C / kSlab), kThreads, 0, (hipStream_t)stream>>>(a);
  if (int rc = check_launch("sv_dwconv3_bwd_weight")) return rc;
  dw_fold_kernel<<<(C * 9 + kThreads - 1) / kThreads, kThreads, 0, (hipStream_t)stream>>>(part, a.P, C, dw, accumulate);
  return check_launch("sv_dwconv3_bwd_weight: fold");
}

static int se_shape_ok(const char* who, int B, int64_t HW, int C, int rd) {
  if (B > 0 && B <= 65535 && HW > 0 && c_ok(C) && rd >= 4 && rd % 4 == 0 && rd <= kMaxC) return SV_OK;
  return ::sv::set_error(SV_ERR_UNSUPPORTED, "%s: unsupported shape B=%d HW=%lld C=%d rd=%d", who, B, (long long)HW, C, rd);
}

static SumArgs se_sum_args(const void* y, int ydt, const float* mean, const float* rstd, const float* gamma,
                           const float* beta, float* part, int64_t HW, int C) {
  SumArgs a{};
  a.y = y; a.ydt = ydt; a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta; a.part = part; a.C = C; a.HW = HW;
  a.P = nparts_for(HW);
  a.rpp = (HW + a.P - 1) / a.P;
  a.inv_hw = 1.0f / (float)HW;
  return a;
}

extern "C" int sv_mbse_squeeze(const void* y, int32_t y_dtype, const float* mean, const float* rstd, const float* gamma,
                               const float* beta, float* part, int32_t B, int32_t HW, int32_t C, sv_stream_t stream) {
  SV_REQUIRE(y && part && dt_ok(y_dtype) && al16(y) && al16(part) && bn_ok(mean, rstd, gamma, beta),
             "sv_mbse_squeeze: bad arguments");
  if (int rc = se_shape_ok("sv_mbse_squeeze", B, HW, C, 4)) return rc;
  SumArgs a = se_sum_args(y, y_dtype, mean, rstd, gamma, beta, part, HW, C);
  sums_kernel<SQUEEZE><<<dim3(a.P, C / kSlab, B), kThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch("sv_mbse_squeeze");
}

extern "C" int sv_mbse_excite(const float* part, int32_t nparts, const float* w1, const float* b1, const float* w2,
                              const float* b2, float* pooled, float* hpre, float* hidden, float* gate, int32_t B,
                              int32_t HW, int32_t C, int32_t rd, sv_stream_t stream) {
  SV_REQUIRE(part && w1 && b1 && w2 && b2 && pooled && hpre && hidden && gate && al16(w1) && al16(w2) && nparts >= 1 &&
                 nparts <= kMaxParts, "sv_mbse_excite: bad arguments");
  if (int rc = se_shape_ok("sv_mbse_excite", B, HW, C, rd)) return rc;
  FcArgs a{};
  a.part = part; a.pooled = pooled; a.hidden = hidden;
  a.W = w1; a.bias = b1; a.out = hpre;
  a.P = nparts; a.N = rd; a.K = C;
  a.inv_hw = 1.0f / (float)HW;
  fc_kernel<1><<<dim3((rd + kFcRows - 1) / kFcRows, B), kThreads, 0, (hipStream_t)stream>>>(a);
  if (int rc = check_launch("sv_mbse_excite: fc1")) return rc;
  FcArgs f{};
  f.x = hidden; f.W = w2; f.bias = b2; f.out = gate;
  f.N = C; f.K = rd;
  fc_kernel<2><<<dim3((C + kFcRows - 1) / kFcRows, B), kThreads, 0, (hipStream_t)stream>>>(f);
  return check_launch("sv_mbse_excite: fc2");
}

extern "C" int sv_mbse_scale(const void* y, int32_t y_dtype, const float* mean, const float* rstd, const float* gamma,
                             const float* beta, const float* gate, void* out, int32_t out_dtype, int32_t B, int32_t HW,
                             int32_t C, sv_stream_t stream) {
  SV_REQUIRE(y && gate && out && dt_ok(y_dtype) && dt_ok(out_dtype) && al16(y) && al16(gate) && al16(out) &&
                 bn_ok(mean, rstd, gamma, beta), "sv_mbse_scale: bad arguments");
  if (int rc = se_shape_ok("sv_mbse_scale", B, HW, C, 4)) return rc;
  ActArgs a{};
  a.y = y; a.ydt = y_dtype; a.out = out; a.odt = out_dtype; a.gate = gate;
  a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta; a.C = C; a.HW = HW;
  int gx = flat_grid((int64_t)HW * (C / 8));
  act_kernel<SCALE><<<dim3(gx, B), kThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch("sv_mbse_scale");
}

extern "C" int sv_mbse_bwd_stats(const void* da, int32_t da_dtype, const void* y, int32_t y_dtype, const float* mean,
                                 const float* rstd, const float* gamma, const float* beta, float* part, int32_t B,
                                 int32_t HW, int32_t C, sv_stream_t stream) {
  SV_REQUIRE(da && y && part && dt_ok(da_dtype) && dt_ok(y_dtype) && al16(da) && al16(y) && al16(part) &&
                 bn_ok(mean, rstd, gamma, beta), "sv_mbse_bwd_stats: bad arguments");
  if (int rc = se_shape_ok("sv_mbse_bwd_stats", B, HW, C, 4)) return rc;
  SumArgs a = se_sum_args(y, y_dtype, mean, rstd, gamma, beta, part, HW, C);
  a.d = da; a.ddt = da_dtype;
  sums_kernel<GATE_BWD><<<dim3(a.P, C / kSlab, B), kThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch("sv_mbse_bwd_stats");
}

extern "C" int sv_mbse_bwd_gate(const float* part, int32_t nparts, const float* pooled, const float* hpre,
                                const float* hidden, const float* gate, const float* w1, const float* w2, float* work,
                                float* dpool, float* dw1, float* db1, float* dw2, float* db2, int32_t B, int32_t C,
                                int32_t rd, sv_stream_t stream) {
  SV_REQUIRE(part && pooled && hpre && hidden && gate && w1 && w2 && work && dpool && dw1 && db1 && dw2 && db2 &&
                 al16(w1) && al16(w2) && al16(dw1) && al16(dw2) && al16(work) && al16(pooled) && al16(hidden) &&
                 nparts >= 1 && nparts <= kMaxParts, "sv_mbse_bwd_gate: bad arguments");
  if (int rc = se_shape_ok("sv_mbse_bwd_gate", B, 1, C, rd)) return rc;
  hipStream_t s = (hipStream_t)stream;
  // work: dsig [B][C], dhpre [B][rd]
  float *dsig = work, *dh = work + (size_t)B * C;
  TmArgs a{};
  a.part = part; a.gate = gate; a.hpre = hpre; a.dsig = dsig;
  a.W = w2; a.out = dh; a.P = nparts; a.N = rd; a.K = C;
  tmatvec_kernel<1><<<dim3((rd + 63) / 64, B), kThreads, 0, s>>>(a);
  if (int rc = check_launch("sv_mbse_bwd_gate: fc2^T")) return rc;
  TmArgs p{};
  p.v = dh; p.W = w1; p.out = dpool; p.N = C; p.K = rd;
  tmatvec_kernel<2><<<dim3((C + 63) / 64, B), kThreads, 0, s>>>(p);
  if (int rc = check_launch("sv_mbse_bwd_gate: fc1^T")) return rc;
  launch_outer(dsig, hidden, dw2, db2, B, C, rd, s);
  if (int rc = check_launch("sv_mbse_bwd_gate: dw2")) return rc;
  launch_outer(dh, pooled, dw1, db1, B, rd, C, s);
  return check_launch("sv_mbse_bwd_gate: dw1");
}

extern "C" int sv_mbse_bwd_apply(const void* da, int32_t da_dtype, const void* y, int32_t y_dtype, const float* mean,
                                 const float* rstd, const float* gamma, const float* beta, const float* gate,
                                 const float* dpool, void* dpre, int32_t dpre_dtype, float* part, int32_t B, int32_t HW,
                                 int32_t C, sv_stream_t stream) {
  SV_REQUIRE(da && y && gate && dpool && dpre && part && dt_ok(da_dtype) && dt_ok(y_dtype) && dt_ok(dpre_dtype) &&
                 al16(da) && al16(y) && al16(gate) && al16(dpool) && al16(dpre) && al16(part) &&
                 bn_ok(mean, rstd, gamma, beta), "sv_mbse_bwd_apply: bad arguments");
  if (int rc = se_shape_ok("sv_mbse_bwd_apply", B, HW, C, 4)) return rc;
  SumArgs a = se_sum_args(y, y_dtype, mean, rstd, gamma, beta, part, HW, C);
  a.d = da; a.ddt = da_dtype; a.gate = gate; a.dpool = dpool; a.out = dpre; a.odt = dpre_dtype;
  sums_kernel<APPLY><<<dim3(a.P, C / kSlab, B), kThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch("sv_mbse_bwd_apply");
}
