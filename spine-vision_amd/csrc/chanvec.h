// Channel-vector I/O of the streaming NHWC passes (bn.hip, se.hip, mbconv.hip, grn.hip, norm.hip): a thread's run of
// consecutive channels as float[V], in memory as f32 or as bf16 bit patterns, and the argument checks that go with it.
#pragma once

#include "common.h"

namespace sv {

// ---- 4 channels of a tensor whose dtype (SV_F32 | SV_BF16) is a run-time argument -----------------------------------
template <typename T>
__device__ __forceinline__ float4 ld4t(const void* p, size_t i) {
  return ld4(reinterpret_cast<const T*>(p), i);
}
__device__ __forceinline__ float4 ld4d(const void* p, int dt, size_t i) {
  return dt == SV_F32 ? ld4t<float>(p, i) : ld4t<uint16_t>(p, i);
}
__device__ __forceinline__ void st4d(void* p, int dt, size_t i, float4 v) {
  if (dt == SV_F32) st4(reinterpret_cast<float*>(p), i, v);
  else st4(reinterpret_cast<uint16_t*>(p), i, v);
}

// ---- V = 8 | 4 channels at element i of such a tensor (V deduces from the array): for V = 8 one 16-B bf16 access or
// two 16-B f32 accesses, 16-B aligned -----------------------------------------------------------------------------
template <int V>
__device__ __forceinline__ void ldv(const void* p, int dt, size_t i, float (&o)[V]) {
  if constexpr (V == 8) {
    if (dt == SV_F32) {
      const float* f = reinterpret_cast<const float*>(p) + i;
      const float4 a = *reinterpret_cast<const float4*>(f), b = *reinterpret_cast<const float4*>(f + 4);
      o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
    } else {
      const uint4 u = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(p) + i);
      const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        o[2 * k] = __uint_as_float(w[k] << 16);
        o[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
      }
    }
  } else {
    const float4 a = ld4d(p, dt, i);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
  }
}
template <int V>
__device__ __forceinline__ void stv(void* p, int dt, size_t i, const float (&v)[V]) {
  if constexpr (V == 8) {
    if (dt == SV_F32) {
      float* f = reinterpret_cast<float*>(p) + i;
      *reinterpret_cast<float4*>(f) = make_float4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<float4*>(f + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
      *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(p) + i) =
          make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
    }
  } else {
    st4d(p, dt, i, make_float4(v[0], v[1], v[2], v[3]));
  }
}

// ---- 8 channels at a typed pointer: the dtype is the pointer's type, so the branch above folds away -----------------
__device__ __forceinline__ void ld8(const float* p, float (&o)[8]) { ldv(p, SV_F32, 0, o); }
__device__ __forceinline__ void ld8(const uint16_t* p, float (&o)[8]) { ldv(p, SV_BF16, 0, o); }
__device__ __forceinline__ void st8(float* p, const float (&v)[8]) { stv(p, SV_F32, 0, v); }
__device__ __forceinline__ void st8(uint16_t* p, const float (&v)[8]) { stv(p, SV_BF16, 0, v); }

// ---- per-channel f32 parameters and partial sums, read and written as float4s ---------------------------------------
template <int V>
__device__ __forceinline__ void ldp(const float* p, int c, float (&o)[V]) {
#pragma unroll
  for (int k = 0; k < V; k += 4) {
    const float4 a = *reinterpret_cast<const float4*>(p + c + k);
    o[k] = a.x; o[k + 1] = a.y; o[k + 2] = a.z; o[k + 3] = a.w;
  }
}
__device__ __forceinline__ void stp(float* p, const float (&v)[8]) { st8(p, v); }

// ---- host-side argument checks ------------------------------------------------------------------------------------
inline bool dt_ok(int dt) { return dt == SV_F32 || dt == SV_BF16; }
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace sv
