// Global Response Normalization (ConvNeXt V2; timm 1.0.22 GlobalResponseNorm, channels-last, eps 1e-6) over the
// 4C-wide hidden activation a = GELU(h) of a block, a [B*HW][n] matrix:
//
//   G[b,c] = sqrt(sum_p a[b,p,c]^2)    D[b] = mean_c G[b,c] + eps    N[b,c] = G[b,c] / D[b]
//   u      = a * (1 + gamma[c] N[b,c]) + beta[c]
//
// and its backward from du = dL/du:
//
//   S[b,c] = sum_p du a    dbeta[c] = sum_{b,p} du    dgamma[c] = sum_b S N    dN = gamma S
//   dG     = dN / D - (sum_c dN G) / (n D^2)          k = dG / G  (0 where G == 0)
//   dh     = (du (1 + gamma N) + a k) GELU'(h)
//
// Six HBM-bound passes.  The three that walk the activation (stats, apply and their backward twins) share one
// geometry: a workgroup of 4 waves owns one chunk of chunk_rows (or fewer) pixels of ONE image and 64 column groups of 8
// consecutive channels, a lane one column group (one 16-byte bf16 access per row, two for f32), the waves stride the
// chunk's rows with kUnroll loads in flight each.  Chunks never cross an image, so HW may be anything.  The
// per-workgroup partial sums go to [B][P][n] (P = sv_grn_nparts) and the finish passes fold them in chunk order:
// no float atomics, run-to-run bitwise results.  All arithmetic is f32 on the stored operand values.
#include "common.h"

namespace sv {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kUnroll = 4;
// the per-image finish passes are latency-bound folds of [P][n] partials by ONE workgroup per image (the channel mean
// spans the image's channels): the largest workgroup, so the most loads in flight
constexpr int kFinThreads = 1024;

// rows of one image per workgroup: 64 where the image has many pixels (S1 / S2 at training resolutions: the partials
// stay ~3 % of the activation's bytes), 32 below, so the late stages still spread over the chip
__host__ __device__ inline int chunk_rows(int64_t HW) { return HW > 512 ? 64 : 32; }

__device__ __forceinline__ void ld8(const uint16_t* p, size_t i, float* v) {
  const uint4 u = *reinterpret_cast<const uint4*>(p + i);
  v[0] = __uint_as_float(u.x << 16), v[1] = __uint_as_float(u.x & 0xffff0000u);
  v[2] = __uint_as_float(u.y << 16), v[3] = __uint_as_float(u.y & 0xffff0000u);
  v[4] = __uint_as_float(u.z << 16), v[5] = __uint_as_float(u.z & 0xffff0000u);
  v[6] = __uint_as_float(u.w << 16), v[7] = __uint_as_float(u.w & 0xffff0000u);
}
__device__ __forceinline__ void ld8(const float* p, size_t i, float* v) {
  const float4 a = *reinterpret_cast<const float4*>(p + i), b = *reinterpret_cast<const float4*>(p + i + 4);
  v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}
__device__ __forceinline__ void st8(uint16_t* p, size_t i, const float* v) {
  *reinterpret_cast<uint4*>(p + i) =
      make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
}
__device__ __forceinline__ void st8(float* p, size_t i, const float* v) {
  *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + i + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// the workgroup's piece of the activation: image blockIdx.z, rows [r0, r1) of it, channels [c0, c0 + 8) of this lane
struct Piece {
  int b, r0, r1, c0;
  bool active;   // the lane's column group exists (n / 8 need not be a multiple of 64)
  size_t base;   // element index of (image b, row 0, channel c0)
};
__device__ __forceinline__ Piece piece(int64_t HW, int n) {
  Piece q;
  const int R = chunk_rows(HW);
  q.b = blockIdx.z;
  q.r0 = blockIdx.y * R;
  q.r1 = (int)(q.r0 + R < HW ? q.r0 + R : HW);
  q.c0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 8;
  q.active = q.c0 < n;
  q.base = (size_t)q.b * (size_t)HW * (size_t)n + (size_t)q.c0;
  return q;
}

// sum acc[NACC][8] over the workgroup's waves in wave order and store it to part_k[(b * P + chunk) * n + c0 ..]
template <int NACC>
__device__ __forceinline__ void fold_waves(float (&acc)[NACC][8], const Piece& q, int n, float* const (&part)[NACC]) {
  __shared__ float red[kWaves][NACC][8][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NACC; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) red[w][k][j][lane] = acc[k][j];
  __syncthreads();
  if (w != 0 || !q.active) return;
  const size_t o = ((size_t)q.b * gridDim.y + blockIdx.y) * (size_t)n + (size_t)q.c0;
#pragma unroll
  for (int k = 0; k < NACC; ++k) {
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s[j] = red[0][k][j][lane];
#pragma unroll
      for (int i = 1; i < kWaves; ++i) s[j] += red[i][k][j][lane];
    }
    st8(part[k], o, s);
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kThreads) grn_stats_kernel(const T* __restrict__ a, float* __restrict__ part,
                                                              int64_t HW, int n) {
  const Piece q = piece(HW, n);
  const int w = threadIdx.x >> 6;
  float acc[1][8] = {};
  if (q.active) {
    for (int r = q.r0 + w; r < q.r1; r += kWaves * kUnroll) {
      float v[kUnroll][8];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int rr = r + u * kWaves;
        if (rr < q.r1) ld8(a, q.base + (size_t)rr * n, v[u]);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (r + u * kWaves < q.r1) {
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[0][j] = fmaf(v[u][j], v[u][j], acc[0][j]);
        }
      }
    }
  }
  float* const out[1] = {part};
  fold_waves<1>(acc, q, n, out);
}

// one workgroup per image: fold the P partials per channel, G = sqrt, the channel mean of G, then N and 1 + gamma N
__global__ void __launch_bounds__(kFinThreads) grn_finish_kernel(const float* __restrict__ part, int P,
                                                               const float* __restrict__ gamma, float* __restrict__ G,
                                                               float* __restrict__ N, float* __restrict__ scale,
                                                               float* __restrict__ D, int n, float eps) {
  __shared__ float red[kFinThreads / 64];
  const int b = blockIdx.x;
  const float* pb = part + (size_t)b * P * n;
  float* Gb = G + (size_t)b * n;
  float sum = 0.f;
  for (int c = threadIdx.x; c < n; c += kFinThreads) {
    float s = 0.f;
#pragma unroll 4
    for (int p = 0; p < P; ++p) s += pb[(size_t)p * n + c];
    const float g = sqrtf(s);
    Gb[c] = g;
    sum += g;
  }
  const float d = block_sum(sum, red) / (float)n + eps;
  if (threadIdx.x == 0) D[b] = d;
  for (int c = threadIdx.x; c < n; c += kFinThreads) {
    const float nn = Gb[c] / d;  // this thread's own store above
    N[(size_t)b * n + c] = nn;
    scale[(size_t)b * n + c] = fmaf(gamma[c], nn, 1.0f);
  }
}

// u = a * scale[b, c] + beta[c]; u may be a (every element is read and then written by the same lane)
template <typename T>
__global__ void __launch_bounds__(kThreads) grn_apply_kernel(const T* a, const float* __restrict__ scale,
                                                              const float* __restrict__ beta, T* u, int64_t HW,
                                                              int n) {
  const Piece q = piece(HW, n);
  if (!q.active) return;
  const int w = threadIdx.x >> 6;
  float sc[8], be[8];
  ld8(scale, (size_t)q.b * n + q.c0, sc);
  ld8(beta, (size_t)q.c0, be);
  for (int r = q.r0 + w; r < q.r1; r += kWaves * kUnroll) {
    float v[kUnroll][8];
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      const int rr = r + k * kWaves;
      if (rr < q.r1) ld8(a, q.base + (size_t)rr * n, v[k]);
    }
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      const int rr = r + k * kWaves;
      if (rr < q.r1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[k][j] = fmaf(v[k][j], sc[j], be[j]);
        st8(u, q.base + (size_t)rr * n, v[k]);
      }
    }
  }
}

// ---- backward --------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kThreads) grn_bwd_stats_kernel(const T* __restrict__ du, const T* __restrict__ a,
                                                                  float* __restrict__ s_part,
                                                                  float* __restrict__ d_part, int64_t HW, int n) {
  const Piece q = piece(HW, n);
  const int w = threadIdx.x >> 6;
  float acc[2][8] = {};
  if (q.active) {
    for (int r = q.r0 + w; r < q.r1; r += kWaves * kUnroll) {
      float g[kUnroll][8], v[kUnroll][8];
#pragma unroll
      for (int k = 0; k < kUnroll; ++k) {
        const int rr = r + k * kWaves;
        if (rr < q.r1) {
          ld8(du, q.base + (size_t)rr * n, g[k]);
          ld8(a, q.base + (size_t)rr * n, v[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < kUnroll; ++k) {
        if (r + k * kWaves < q.r1) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            acc[0][j] = fmaf(g[k][j], v[k][j], acc[0][j]);
            acc[1][j] += g[k][j];
          }
        }
      }
    }
  }
  float* const out[2] = {s_part, d_part};
  fold_waves<2>(acc, q, n, out);
}

// one workgroup per image: fold the partials of S and sum du per channel (the totals are left in chunk 0 of the
// partial buffers, each written by the thread that read the channel's partials), then k
__global__ void __launch_bounds__(kFinThreads) grn_bwd_image_kernel(float* __restrict__ s_part,
                                                                  float* __restrict__ d_part, int P,
                                                                  const float* __restrict__ gamma,
                                                                  const float* __restrict__ G,
                                                                  const float* __restrict__ D, float* __restrict__ kout,
                                                                  int n) {
  __shared__ float red[kFinThreads / 64];
  const int b = blockIdx.x;
  float* sb = s_part + (size_t)b * P * n;
  float* db = d_part + (size_t)b * P * n;
  const float* Gb = G + (size_t)b * n;
  float dot = 0.f;
  for (int c = threadIdx.x; c < n; c += kFinThreads) {
    float s = 0.f, t = 0.f;
#pragma unroll 4
    for (int p = 0; p < P; ++p) {
      s += sb[(size_t)p * n + c];
      t += db[(size_t)p * n + c];
    }
    sb[c] = s;
    db[c] = t;
    dot = fmaf(gamma[c] * s, Gb[c], dot);
  }
  dot = block_sum(dot, red);
  const float d = D[b];
  const float tail = dot / ((float)n * d * d);
  for (int c = threadIdx.x; c < n; c += kFinThreads) {
    const float g = Gb[c];
    const float dg = gamma[c] * sb[c] / d - tail;
    kout[(size_t)b * n + c] = g > 0.f ? dg / g : 0.f;
  }
}

// dgamma[c] (+)= sum_b S[b,c] N[b,c], dbeta[c] (+)= sum_b (sum du)[b,c], images in order
__global__ void __launch_bounds__(kThreads) grn_bwd_param_kernel(const float* __restrict__ s_part,
                                                                  const float* __restrict__ d_part, int P, int B,
                                                                  const float* __restrict__ N,
                                                                  float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                  int accumulate, int n) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= n) return;
  float dg = 0.f, dbt = 0.f;
  for (int b = 0; b < B; ++b) {
    dg = fmaf(s_part[(size_t)b * P * n + c], N[(size_t)b * n + c], dg);
    dbt += d_part[(size_t)b * P * n + c];
  }
  dgamma[c] = accumulate ? dgamma[c] + dg : dg;
  dbeta[c] = accumulate ? dbeta[c] + dbt : dbt;
}

// dh = (du * scale[b, c] + a * k[b, c]) * gh; dh may be du
template <typename T>
__global__ void __launch_bounds__(kThreads) grn_bwd_apply_kernel(const T* du, const T* __restrict__ a,
                                                                  const T* __restrict__ gh,
                                                                  const float* __restrict__ scale,
                                                                  const float* __restrict__ kk, T* dh, int64_t HW,
                                                                  int n) {
  const Piece q = piece(HW, n);
  if (!q.active) return;
  const int w = threadIdx.x >> 6;
  float sc[8], kc[8];
  ld8(scale, (size_t)q.b * n + q.c0, sc);
  ld8(kk, (size_t)q.b * n + q.c0, kc);
  constexpr int U = 2;  // three streams per row: 6 loads in flight
  for (int r = q.r0 + w; r < q.r1; r += kWaves * U) {
    float g[U][8], v[U][8], e[U][8];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int rr = r + k * kWaves;
      if (rr < q.r1) {
        ld8(du, q.base + (size_t)rr * n, g[k]);
        ld8(a, q.base + (size_t)rr * n, v[k]);
        ld8(gh, q.base + (size_t)rr * n, e[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int rr = r + k * kWaves;
      if (rr < q.r1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) g[k][j] = fmaf(g[k][j], sc[j], v[k][j] * kc[j]) * e[k][j];
        st8(dh, q.base + (size_t)rr * n, g[k]);
      }
    }
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// shape checks shared by the passes that walk the activation; the grid, or 0 with the error set
int walk_grid(const char* who, int32_t B, int64_t HW, int32_t n, dim3* grid) {
  if (B <= 0 || HW <= 0 || n <= 0) return set_error(SV_ERR_INVALID_ARG, "%s: B, HW and n must be positive", who);
  if (n % 8 != 0) return set_error(SV_ERR_INVALID_ARG, "%s: n=%d must be a multiple of 8", who, n);
  const int64_t P = (HW + chunk_rows(HW) - 1) / chunk_rows(HW);
  if (B > 65535 || P > 65535 || HW > INT32_MAX)
    return set_error(SV_ERR_UNSUPPORTED, "%s: B=%d / HW=%lld exceed the grid", who, B, (long long)HW);
  *grid = dim3((unsigned)((n / 8 + 63) / 64), (unsigned)P, (unsigned)B);
  return SV_OK;
}

}  // namespace
}  // namespace sv

using namespace sv;

extern "C" {

int sv_grn_nparts(int64_t HW, int32_t n) {
  (void)n;
  if (HW <= 0) return 0;
  const int64_t P = (HW + chunk_rows(HW) - 1) / chunk_rows(HW);
  return P > INT32_MAX ? 0 : (int)P;
}

int sv_grn_stats(const void* a, int32_t dtype, float* part, int32_t B, int64_t HW, int32_t n, sv_stream_t stream) {
  SV_REQUIRE(a && part, "sv_grn_stats: null pointer");
  dim3 grid;
  if (const int rc = walk_grid("sv_grn_stats", B, HW, n, &grid)) return rc;
  SV_REQUIRE(al16(a) && al16(part), "sv_grn_stats: pointers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SV_BF16) grn_stats_kernel<uint16_t><<<grid, kThreads, 0, s>>>((const uint16_t*)a, part, HW, n);
  else if (dtype == SV_F32) grn_stats_kernel<float><<<grid, kThreads, 0, s>>>((const float*)a, part, HW, n);
  else return set_error(SV_ERR_INVALID_ARG, "sv_grn_stats: bad dtype");
  return check_launch("sv_grn_stats");
}

int sv_grn_finish(const float* part, int32_t nparts, const float* gamma, float* G, float* N, float* scale, float* D,
                  int32_t B, int32_t n, float eps, sv_stream_t stream) {
  SV_REQUIRE(part && gamma && G && N && scale && D, "sv_grn_finish: null pointer");
  SV_REQUIRE(B > 0 && n > 0 && nparts > 0, "sv_grn_finish: B, n and nparts must be positive");
  grn_finish_kernel<<<B, kFinThreads, 0, (hipStream_t)stream>>>(part, nparts, gamma, G, N, scale, D, n, eps);
  return check_launch("sv_grn_finish");
}

int sv_grn_apply(const void* a, int32_t dtype, const float* scale, const float* beta, void* u, int32_t B, int64_t HW,
                 int32_t n, sv_stream_t stream) {
  SV_REQUIRE(a && scale && beta && u, "sv_grn_apply: null pointer");
  dim3 grid;
  if (const int rc = walk_grid("sv_grn_apply", B, HW, n, &grid)) return rc;
  SV_REQUIRE(al16(a) && al16(u) && al16(scale) && al16(beta), "sv_grn_apply: pointers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SV_BF16)
    grn_apply_kernel<uint16_t><<<grid, kThreads, 0, s>>>((const uint16_t*)a, scale, beta, (uint16_t*)u, HW, n);
  else if (dtype == SV_F32)
    grn_apply_kernel<float><<<grid, kThreads, 0, s>>>((const float*)a, scale, beta, (float*)u, HW, n);
  else return set_error(SV_ERR_INVALID_ARG, "sv_grn_apply: bad dtype");
  return check_launch("sv_grn_apply");
}

int sv_grn_bwd_stats(const void* du, const void* a, int32_t dtype, float* s_part, float* d_part, int32_t B,
                     int64_t HW, int32_t n, sv_stream_t stream) {
  SV_REQUIRE(du && a && s_part && d_part, "sv_grn_bwd_stats: null pointer");
  dim3 grid;
  if (const int rc = walk_grid("sv_grn_bwd_stats", B, HW, n, &grid)) return rc;
  SV_REQUIRE(al16(du) && al16(a) && al16(s_part) && al16(d_part),
             "sv_grn_bwd_stats: pointers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SV_BF16)
    grn_bwd_stats_kernel<uint16_t><<<grid, kThreads, 0, s>>>((const uint16_t*)du, (const uint16_t*)a, s_part, d_part,
                                                             HW, n);
  else if (dtype == SV_F32)
    grn_bwd_stats_kernel<float><<<grid, kThreads, 0, s>>>((const float*)du, (const float*)a, s_part, d_part, HW, n);
  else return set_error(SV_ERR_INVALID_ARG, "sv_grn_bwd_stats: bad dtype");
  return check_launch("sv_grn_bwd_stats");
}

int sv_grn_bwd_finish(float* s_part, float* d_part, int32_t nparts, const float* gamma, const float* G,
                      const float* N, const float* D, float* k, float* dgamma, float* dbeta, int32_t accumulate,
                      int32_t B, int32_t n, sv_stream_t stream) {
  SV_REQUIRE(s_part && d_part && gamma && G && N && D && k && dgamma && dbeta, "sv_grn_bwd_finish: null pointer");
  SV_REQUIRE(B > 0 && n > 0 && nparts > 0, "sv_grn_bwd_finish: B, n and nparts must be positive");
  hipStream_t s = (hipStream_t)stream;
  grn_bwd_image_kernel<<<B, kFinThreads, 0, s>>>(s_part, d_part, nparts, gamma, G, D, k, n);
  grn_bwd_param_kernel<<<(n + kThreads - 1) / kThreads, kThreads, 0, s>>>(s_part, d_part, nparts, B, N, dgamma,
                                                                           dbeta, accumulate, n);
  return check_launch("sv_grn_bwd_finish");
}

int sv_grn_bwd_apply(const void* du, const void* a, const void* gh, int32_t dtype, const float* scale, const float* k,
                     void* dh, int32_t B, int64_t HW, int32_t n, sv_stream_t stream) {
  SV_REQUIRE(du && a && gh && scale && k && dh, "sv_grn_bwd_apply: null pointer");
  dim3 grid;
  if (const int rc = walk_grid("sv_grn_bwd_apply", B, HW, n, &grid)) return rc;
  SV_REQUIRE(al16(du) && al16(a) && al16(gh) && al16(dh) && al16(scale) && al16(k),
             "sv_grn_bwd_apply: pointers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SV_BF16)
    grn_bwd_apply_kernel<uint16_t><<<grid, kThreads, 0, s>>>((const uint16_t*)du, (const uint16_t*)a,
                                                             (const uint16_t*)gh, scale, k, (uint16_t*)dh, HW, n);
  else if (dtype == SV_F32)
    grn_bwd_apply_kernel<float><<<grid, kThreads, 0, s>>>((const float*)du, (const float*)a, (const float*)gh, scale,
                                                          k, (float*)dh, HW, n);
  else return set_error(SV_ERR_INVALID_ARG, "sv_grn_bwd_apply: bad dtype");
  return check_launch("sv_grn_bwd_apply");
}

}  // extern "C"
