// Fragment helpers shared by the attention kernels (attn.hip: one pass, N <= 256; attn_stream.hip: streamed tiles):
// the 32x32x16 bf16 MFMA, its accumulator layout, 64-wide row fragments and the stores of a transposed result.
#pragma once

#include "common.h"

namespace sv {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ f32x16 mfma(uint4 a, uint4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}
// row of accumulator register i in lane half h of a 32x32 tile
__device__ __forceinline__ int arow(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// the four k-step fragments (d = 16 s + 8 h .. + 7) of one 64-wide row; `row` = nullptr: zeros
__device__ __forceinline__ void load_row(const uint16_t* row, int h, uint4 (&f)[4]) {
#pragma unroll
  for (int s = 0; s < 4; ++s)
    f[s] = row ? *reinterpret_cast<const uint4*>(row + 16 * s + 8 * h) : make_uint4(0u, 0u, 0u, 0u);
}
// registers 8 s .. 8 s + 7 of an accumulator tile as the bf16 fragment of k-step s of the next MFMA (element j is
// tile row 16 s + 8 (j >> 2) + 4 h + (j & 3))
__device__ __forceinline__ uint4 acc_frag(const f32x16& x, int s) {
  return make_uint4(pack2bf(x[8 * s], x[8 * s + 1]), pack2bf(x[8 * s + 2], x[8 * s + 3]),
                    pack2bf(x[8 * s + 4], x[8 * s + 5]), pack2bf(x[8 * s + 6], x[8 * s + 7]));
}
// the matching fragment of the OTHER operand from a transposed image with rows of `ldt` elements: row `r` of the
// image, tokens t0 + 16 s + 4 h + {0..3} and t0 + 16 s + 8 + 4 h + {0..3}
__device__ __forceinline__ uint4 tr_frag(const uint16_t* img, int ldt, int r, int t0, int s, int h) {
  const uint16_t* p = img + r * ldt + t0 + 16 * s + 4 * h;
  const uint2 lo = *reinterpret_cast<const uint2*>(p);
  const uint2 hi = *reinterpret_cast<const uint2*>(p + 8);
  return make_uint4(lo.x, lo.y, hi.x, hi.y);
}
// 64 columns of rows [n, rows) of a [rows][ld] bf16 matrix := 0
__device__ __forceinline__ void zero_pad_rows(uint16_t* dst, int64_t ld, int n, int rows, int tid, int nthreads) {
  for (int idx = tid; idx < (rows - n) * 8; idx += nthreads)
    *reinterpret_cast<uint4*>(dst + (int64_t)(n + (idx >> 3)) * ld + (idx & 7) * 8) = make_uint4(0u, 0u, 0u, 0u);
}
// a 64 (d) x 32 (token on the lane) pair of accumulator tiles -> rows of a [token][ld] bf16 matrix
__device__ __forceinline__ void store_t(uint16_t* row, const f32x16 (&acc)[2], float mul, int h) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<uint2*>(row + dt * 32 + 8 * g + 4 * h) =
          make_uint2(pack2bf(acc[dt][4 * g] * mul, acc[dt][4 * g + 1] * mul),
                     pack2bf(acc[dt][4 * g + 2] * mul, acc[dt][4 * g + 3] * mul));
}
// rowsum(dO . O) of one 64-wide bf16 row pair, in f32, in element order
__device__ __forceinline__ float row_dot64(const uint16_t* o_row, const uint16_t* g_row) {
  float dsum = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const uint4 o = *reinterpret_cast<const uint4*>(o_row + c * 8);
    const uint4 g = *reinterpret_cast<const uint4*>(g_row + c * 8);
    const uint32_t ow[4] = {o.x, o.y, o.z, o.w}, gw[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dsum = fmaf(__uint_as_float(ow[j] << 16), __uint_as_float(gw[j] << 16), dsum);
      dsum = fmaf(__uint_as_float(ow[j] & 0xffff0000u), __uint_as_float(gw[j] & 0xffff0000u), dsum);
    }
  }
  return dsum;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

constexpr int kD = 64;  // head dimension
constexpr float kLog2e = 1.4426950408889634f;

}  // namespace
}  // namespace sv
