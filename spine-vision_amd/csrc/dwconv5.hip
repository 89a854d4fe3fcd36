// Depthwise 5x5 convolution of the EfficientNet-B0..B4 backbones (gfx950), NHWC, pad 2, stride 1 | 2: forward, data
// gradient and weight gradient.  The 3x3 family of csrc/mbconv.hip keeps a thread's taps (72 floats) and its weight
// gradient (9 x 8 accumulators) in registers; 25 taps would be 200 of either, so both passes are cut differently here.
//
// Replaces, with its autograd backward, the depthwise Conv2d(k = 5) of timm's InvertedResidual (efficientnet_b0..b4).
//
//   y[b][oy][ox][c]  = sum_{ky,kx} x[b][oy s + ky - 2][ox s + kx - 2][c] w[c][ky][kx]
//   dx[b][iy][ix][c] = sum_{ky,kx : s | iy + 2 - ky, s | ix + 2 - kx} dy[b][(iy + 2 - ky) / s][(ix + 2 - kx) / s][c] w[c][ky][kx]
//   dw[c][ky][kx]    = sum_{b,oy,ox} dy[b][oy][ox][c] x[b][oy s + ky - 2][ox s + kx - 2][c]
//
// A thread owns 8 consecutive channels (16 B in bf16, 2 x 16 B in f32) and a STRIP of 4 consecutive pixels of one row;
// arithmetic is f32, rounded once at the store.  No atomics, nothing synchronises with the host.
//   * weights (forward, data gradient): a workgroup owns 64 channels (the last slab of a C % 64 == 32 tensor is half
//     idle); it reads their 64 x 25 floats once (16-B loads) into LDS as [tap][channel], and a thread fetches the 5 x 8
//     weights of ONE tap row at a time (10 ds_read_b128): 40 weight registers instead of 200;
//   * input reuse: per tap row a thread loads the 8 (stride 1) or 11 (stride 2) input pixels under its strip once and
//     feeds each to every output of the strip that reads it -- 40 | 55 loads per 4 outputs where the per-output form of
//     the 3x3 kernel would issue 100; the data gradient loads 8 | 4 gradient pixels per tap row the same way;
//   * weight gradient: a workgroup owns 32 channels and one part of the strips (P = sv_dwconv5_bwd_weight_nparts parts of
//     spp = ceil(strips / P) strips, strips = B OH ceil(OW / 4) in (b, oy, strip) order); its 320 threads are (strip lane
//     q = t / 20, tap row ky = (t / 4) % 5, channel group t % 4): a thread keeps the 5 x 8 accumulators of ITS tap row
//     only.  The 5 threads of a strip read the same dy addresses in the same wave instruction, so dy leaves HBM once.
//
// Summation orders and rounding points (the tests derive their bounds from them):
//   * taps (forward, data gradient): one accumulator per output element, one fmaf chain over (ky, kx) ascending; a tap
//     row in the padding is skipped, a tap column in the padding enters as an exact zero (fmaf(0, w, acc) == acc), so the
//     chain has at most 25 links;
//   * weight gradient: thread (q, ky) takes strips r0 + q, + 16, ... ascending and inside a strip the pixels ascending,
//     one fmaf per pixel into acc[kx] (a pixel or a tap outside the tensor enters as an exact zero): at most
//     4 ceil(spp / 16) links; lane 0 then adds lanes 1 .. 15 ascending (15 links); part[p][ky 5 + kx][c] holds the
//     result; the fold adds the P parts in part order into dw[c][ky][kx] (accumulate: dw + sum).
#include "chanvec.h"
#include "common.h"

namespace sv {
namespace dw5 {

constexpr int kThreads = 256;
constexpr int kMaxC = 3840;
constexpr int kMaxParts = 64;
constexpr int kSlab = 64;     // channels per forward / data-gradient workgroup
constexpr int kLanes = 32;    // strips per such workgroup
constexpr int kTW = 4;        // pixels per strip
constexpr int kWThreads = 320;
constexpr int kWLanes = 16;   // strip lanes of a weight-gradient workgroup
constexpr int kWSlab = 32;    // its channels

struct Args {
  const void *x, *dy;
  const float* w;
  void* out;
  float* part;
  int xdt, ddt, odt, B, H, W, OH, OW, C, P;
  int64_t spp;
};

// 8 channels at element i, or zeros for a pixel outside the tensor
__device__ __forceinline__ void ldz(const void* p, int dt, bool inside, size_t i, float (&v)[8]) {
  if (inside) {
    ldv(p, dt, i, v);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = 0.f;
  }
}

// the torch weight [C][25] of channels [c0, c0 + nch) -> LDS [tap][channel]
__device__ __forceinline__ void stage_w(const float* w, int c0, int nch, float (*wl)[kSlab]) {
  const float4* src = reinterpret_cast<const float4*>(w + (size_t)c0 * 25);
  for (int i4 = threadIdx.x; i4 < nch * 25 / 4; i4 += kThreads) {
    const float4 v = src[i4];
    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = 4 * i4 + j;
      wl[i % 25][i / 25] = e[j];
    }
  }
}
// the 5 x 8 weights of tap row ky
__device__ __forceinline__ void row_w(const float (*wl)[kSlab], int ky, int cl, float (&wr)[5][8]) {
#pragma unroll
  for (int kx = 0; kx < 5; ++kx) ldp(wl[ky * 5 + kx], cl, wr[kx]);
}

// grid (strip groups, ceil(C / 64)); thread (strip lane t / 8, channel group t % 8)
template <int S>
__global__ void __launch_bounds__(kThreads) fwd_kernel(Args a) {
  constexpr int NJ = S * (kTW - 1) + 5;  // input pixels under a strip
  __shared__ __attribute__((aligned(16))) float wl[25][kSlab];
  const int t = threadIdx.x, cl = (t & 7) * 8, q = t >> 3;
  const int c0 = blockIdx.y * kSlab, c = c0 + cl, C = a.C;
  stage_w(a.w, c0, C - c0 < kSlab ? C - c0 : kSlab, wl);
  __syncthreads();
  if (c >= C) return;
  const int nsx = (a.OW + kTW - 1) / kTW;
  const int64_t strips = (int64_t)a.B * a.OH * nsx;
  for (int64_t r = (int64_t)blockIdx.x * kLanes + q; r < strips; r += (int64_t)gridDim.x * kLanes) {
    const int ox0 = (int)(r % nsx) * kTW, oy = (int)((r / nsx) % a.OH), b = (int)(r / ((int64_t)nsx * a.OH));
    const int ix0 = ox0 * S - 2;
    float acc[kTW][8];
#pragma unroll
    for (int o = 0; o < kTW; ++o)
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[o][k] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 5; ++ky) {
      const int iy = oy * S + ky - 2;
      if (iy < 0 || iy >= a.H) continue;
      float wr[5][8];
      row_w(wl, ky, cl, wr);
      const size_t row = ((size_t)b * a.H + iy) * a.W;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int ix = ix0 + j;
        float v[8];
        ldz(a.x, a.xdt, ix >= 0 && ix < a.W, (row + ix) * C + c, v);
#pragma unroll
        for (int kx = 0; kx < 5; ++kx) {
          if (j >= kx && (j - kx) % S == 0 && (j - kx) / S < kTW) {
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[(j - kx) / S][k] = fmaf(v[k], wr[kx][k], acc[(j - kx) / S][k]);
          }
        }
      }
    }
    const size_t orow = ((size_t)b * a.OH + oy) * a.OW;
#pragma unroll
    for (int o = 0; o < kTW; ++o)
      if (ox0 + o < a.OW) stv(a.out, a.odt, (orow + ox0 + o) * C + c, acc[o]);
  }
}

// a strip of dx; gradient column ox = oxb + jj reaches output o of the strip through tap kx = o + 4 - S jj, so jj runs
// downwards for kx to ascend
template <int S>
__global__ void __launch_bounds__(kThreads) bwd_data_kernel(Args a) {
  constexpr int NJ = S == 1 ? kTW + 4 : kTW / 2 + 2;  // gradient pixels over a strip
  __shared__ __attribute__((aligned(16))) float wl[25][kSlab];
  const int t = threadIdx.x, cl = (t & 7) * 8, q = t >> 3;
  const int c0 = blockIdx.y * kSlab, c = c0 + cl, C = a.C;
  stage_w(a.w, c0, C - c0 < kSlab ? C - c0 : kSlab, wl);
  __syncthreads();
  if (c >= C) return;
  const int nsx = (a.W + kTW - 1) / kTW;
  const int64_t strips = (int64_t)a.B * a.H * nsx;
  for (int64_t r = (int64_t)blockIdx.x * kLanes + q; r < strips; r += (int64_t)gridDim.x * kLanes) {
    const int ix0 = (int)(r % nsx) * kTW, iy = (int)((r / nsx) % a.H), b = (int)(r / ((int64_t)nsx * a.H));
    const int oxb = S == 1 ? ix0 - 2 : ix0 / 2 - 1;
    float acc[kTW][8];
#pragma unroll
    for (int o = 0; o < kTW; ++o)
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[o][k] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 5; ++ky) {
      const int ty = iy + 2 - ky;
      if (ty < 0 || ty % S) continue;
      const int oy = ty / S;
      if (oy >= a.OH) continue;
      float wr[5][8];
      row_w(wl, ky, cl, wr);
      const size_t row = ((size_t)b * a.OH + oy) * a.OW;
#pragma unroll
      for (int jj = NJ - 1; jj >= 0; --jj) {
        const int ox = oxb + jj;
        float v[8];
        ldz(a.dy, a.ddt, ox >= 0 && ox < a.OW, (row + ox) * C + c, v);
#pragma unroll
        for (int o = 0; o < kTW; ++o) {
          const int kx = o + 4 - S * jj;
          if (kx >= 0 && kx < 5) {
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[o][k] = fmaf(v[k], wr[kx][k], acc[o][k]);
          }
        }
      }
    }
    const size_t orow = ((size_t)b * a.H + iy) * a.W;
#pragma unroll
    for (int o = 0; o < kTW; ++o)
      if (ix0 + o < a.W) stv(a.out, a.odt, (orow + ix0 + o) * C + c, acc[o]);
  }
}

// part[p][ky 5 + kx][C]; grid (P, C / 32); thread (strip lane t / 20, tap row (t / 4) % 5, channel group t % 4)
template <int S>
__global__ void __launch_bounds__(kWThreads) bwd_weight_kernel(Args a) {
  constexpr int NJ = S * (kTW - 1) + 5;
  __shared__ float red[8][kWThreads];
  const int t = threadIdx.x, cg = t & 3, ky = (t >> 2) % 5, q = t / 20;
  const int p = blockIdx.x, C = a.C, c = blockIdx.y * kWSlab + cg * 8;
  const int nsx = (a.OW + kTW - 1) / kTW;
  const int64_t strips = (int64_t)a.B * a.OH * nsx;
  const int64_t r0 = p * a.spp, r1 = r0 + a.spp < strips ? r0 + a.spp : strips;
  float acc[5][8];
#pragma unroll
  for (int kx = 0; kx < 5; ++kx)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[kx][k] = 0.f;
  for (int64_t r = r0 + q; r < r1; r += kWLanes) {
    const int ox0 = (int)(r % nsx) * kTW, oy = (int)((r / nsx) % a.OH), b = (int)(r / ((int64_t)nsx * a.OH));
    const int iy = oy * S + ky - 2, ix0 = ox0 * S - 2;
    if (iy < 0 || iy >= a.H) continue;
    float g[kTW][8];
    const size_t orow = ((size_t)b * a.OH + oy) * a.OW, row = ((size_t)b * a.H + iy) * a.W;
#pragma unroll
    for (int o = 0; o < kTW; ++o) ldz(a.dy, a.ddt, ox0 + o < a.OW, (orow + ox0 + o) * C + c, g[o]);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int ix = ix0 + j;
      float v[8];
      ldz(a.x, a.xdt, ix >= 0 && ix < a.W, (row + ix) * C + c, v);
#pragma unroll
      for (int kx = 0; kx < 5; ++kx) {
        if (j >= kx && (j - kx) % S == 0 && (j - kx) / S < kTW) {
#pragma unroll
          for (int k = 0; k < 8; ++k) acc[kx][k] = fmaf(g[(j - kx) / S][k], v[k], acc[kx][k]);
        }
      }
    }
  }
#pragma unroll
  for (int kx = 0; kx < 5; ++kx) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red[k][t] = acc[kx][k];
    __syncthreads();
    if (q == 0) {
      for (int j = 1; j < kWLanes; ++j) {
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[kx][k] += red[k][t + 20 * j];
      }
      stp(a.part + ((size_t)p * 25 + ky * 5 + kx) * C + c, acc[kx]);
    }
    __syncthreads();
  }
}

// dw[c][tap] (+)= sum_p part[p][tap][c], p ascending
__global__ void __launch_bounds__(kThreads) fold_kernel(const float* __restrict__ part, int P, int C, float* dw,
                                                        int accumulate) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= C * 25) return;
  const int c = i / 25, j = i % 25;
  float s = 0.f;
  for (int p = 0; p < P; ++p) s += part[((size_t)p * 25 + j) * C + c];
  dw[i] = accumulate ? dw[i] + s : s;
}

static bool shape_ok(int B, int H, int W, int C, int stride) {
  return B > 0 && H > 0 && W > 0 && C >= 32 && C <= kMaxC && C % 32 == 0 && (stride == 1 || stride == 2);
}
static Args make_args(int B, int H, int W, int C, int stride) {
  Args a{};
  a.B = B; a.H = H; a.W = W; a.C = C;
  a.OH = (H - 1) / stride + 1;
  a.OW = (W - 1) / stride + 1;
  return a;
}
static int64_t strips_of(int B, int rows, int cols) { return (int64_t)B * rows * ((cols + kTW - 1) / kTW); }
static int nparts_for(int64_t strips) {
  int64_t p = strips / (kWLanes * 4);  // >= 4 strips per thread
  return (int)(p > kMaxParts ? kMaxParts : p < 1 ? 1 : p);
}
// one strip per thread while that keeps the launch under 2048 workgroups, grid-stride beyond
static dim3 strip_grid(int64_t strips, int C) {
  const int gy = (C + kSlab - 1) / kSlab;
  int64_t gx = (strips + kLanes - 1) / kLanes;
  const int64_t cap = 2048 / gy > 1 ? 2048 / gy : 1;
  return dim3((unsigned)(gx > cap ? cap : gx), gy);
}

}  // namespace dw5
}  // namespace sv

using namespace sv;
using namespace sv::dw5;

#define DW5_UNSUPPORTED(who)                                                                                        \
  do {                                                                                                              \
    if (!shape_ok(B, H, W, C, stride))                                                                              \
      return ::sv::set_error(SV_ERR_UNSUPPORTED, who ": unsupported shape B=%d H=%d W=%d C=%d stride=%d", (int)B,  \
                             (int)H, (int)W, (int)C, (int)stride);                                                  \
  } while (0)

extern "C" int sv_dwconv5_fwd(const void* x, int32_t x_dtype, const float* w, void* y, int32_t y_dtype, int32_t B,
                              int32_t H, int32_t W, int32_t C, int32_t stride, sv_stream_t stream) {
  SV_REQUIRE(x && w && y && dt_ok(x_dtype) && dt_ok(y_dtype) && al16(x) && al16(w) && al16(y),
             "sv_dwconv5_fwd: bad arguments");
  DW5_UNSUPPORTED("sv_dwconv5_fwd");
  Args a = make_args(B, H, W, C, stride);
  a.x = x; a.xdt = x_dtype; a.w = w; a.out = y; a.odt = y_dtype;
  const dim3 grid = strip_grid(strips_of(B, a.OH, a.OW), C);
  if (stride == 1) fwd_kernel<1><<<grid, kThreads, 0, (hipStream_t)stream>>>(a);
  else fwd_kernel<2><<<grid, kThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch("sv_dwconv5_fwd");
}

extern "C" int sv_dwconv5_bwd_data(const void* dy, int32_t dy_dtype, const float* w, void* dx, int32_t dx_dtype,
                                   int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride, sv_stream_t stream) {
  SV_REQUIRE(dy && w && dx && dt_ok(dy_dtype) && dt_ok(dx_dtype) && al16(dy) && al16(w) && al16(dx),
             "sv_dwconv5_bwd_data: bad arguments");
  DW5_UNSUPPORTED("sv_dwconv5_bwd_data");
  Args a = make_args(B, H, W, C, stride);
  a.dy = dy; a.ddt = dy_dtype; a.w = w; a.out = dx; a.odt = dx_dtype;
  const dim3 grid = strip_grid(strips_of(B, H, W), C);
  if (stride == 1) bwd_data_kernel<1><<<grid, kThreads, 0, (hipStream_t)stream>>>(a);
  else bwd_data_kernel<2><<<grid, kThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch("sv_dwconv5_bwd_data");
}

extern "C" int sv_dwconv5_bwd_weight_nparts(int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride) {
  if (!shape_ok(B, H, W, C, stride)) return 0;
  return nparts_for(strips_of(B, (H - 1) / stride + 1, (W - 1) / stride + 1));
}

extern "C" int sv_dwconv5_bwd_weight(const void* dy, int32_t dy_dtype, const void* x, int32_t x_dtype, float* part,
                                     float* dw, int32_t accumulate, int32_t B, int32_t H, int32_t W, int32_t C,
                                     int32_t stride, sv_stream_t stream) {
  SV_REQUIRE(dy && x && part && dw && dt_ok(dy_dtype) && dt_ok(x_dtype) && al16(dy) && al16(x) && al16(part),
             "sv_dwconv5_bwd_weight: bad arguments");
  DW5_UNSUPPORTED("sv_dwconv5_bwd_weight");
  Args a = make_args(B, H, W, C, stride);
  a.dy = dy; a.ddt = dy_dtype; a.x = x; a.xdt = x_dtype; a.part = part;
  const int64_t strips = strips_of(B, a.OH, a.OW);
  a.P = nparts_for(strips);
  a.spp = (strips + a.P - 1) / a.P;
  const dim3 grid(a.P, C / kWSlab);
  if (stride == 1) bwd_weight_kernel<1><<<grid, kWThreads, 0, (hipStream_t)stream>>>(a);
  else bwd_weight_kernel<2><<<grid, kWThreads, 0, (hipStream_t)stream>>>(a);
  if (int rc = check_launch("sv_dwconv5_bwd_weight")) return rc;
  fold_kernel<<<(C * 25 + kThreads - 1) / kThreads, kThreads, 0, (hipStream_t)stream>>>(part, a.P, C, dw, accumulate);
  return check_launch("sv_dwconv5_bwd_weight: fold");
}
