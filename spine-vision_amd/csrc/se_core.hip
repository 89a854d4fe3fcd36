// The squeeze-and-excitation gate's weight gradients (se_core.h): one kernel for se.hip and mbconv.hip.
#include "se_core.h"

namespace sv {

constexpr int kOuterThreads = 256;

// dW[m][n] += sum_b u[b][m] v[b][n],  db[m] += sum_b u[b][m]   (one thread per 4 columns of one row)
__global__ void __launch_bounds__(kOuterThreads) outer_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                              float* __restrict__ dW, float* __restrict__ db, int B,
                                                              int M, int N) {
  const int n4 = N / 4;
  const int64_t i = (int64_t)blockIdx.x * kOuterThreads + threadIdx.x;
  if (i >= (int64_t)M * n4) return;
  const int m = (int)(i / n4), n = (int)(i % n4) * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float sb = 0.f;
  for (int b = 0; b < B; ++b) {
    const float x = u[(size_t)b * M + m];
    const float4 w = *reinterpret_cast<const float4*>(v + (size_t)b * N + n);
    acc.x = fmaf(x, w.x, acc.x);
    acc.y = fmaf(x, w.y, acc.y);
    acc.z = fmaf(x, w.z, acc.z);
    acc.w = fmaf(x, w.w, acc.w);
    sb += x;
  }
  float4* o = reinterpret_cast<float4*>(dW + (size_t)m * N + n);
  float4 d = *o;
  d.x += acc.x; d.y += acc.y; d.z += acc.z; d.w += acc.w;
  *o = d;
  if (n == 0) db[m] += sb;
}

void launch_outer(const float* u, const float* v, float* dW, float* db, int B, int M, int N, hipStream_t s) {
  const int grid = (int)(((int64_t)M * (N / 4) + kOuterThreads - 1) / kOuterThreads);
  outer_kernel<<<grid, kOuterThreads, 0, s>>>(u, v, dW, db, B, M, N);
}

}  // namespace sv
