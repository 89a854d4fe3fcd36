// The squeeze-and-excitation gate's three reductions, shared by se.hip (ResNet-RS) and mbconv.hip (EfficientNetV2).
// Each file stages its own vector into LDS and passes its epilogue as `put`; the sums, and so their orders, are here.
// Summation orders (the tests derive their bounds from them), for workgroups of 256 threads:
//   * a matvec row (fc1, fc2): lane l multiplies-adds (fmaf) elements 4 l + 256 j + (0..3) ascending into one
//     accumulator, then the 64 lanes are added by the xor butterfly wave_sum, then the bias is added;
//   * a transposed matvec column (the gate backward): 16 k-groups, group q fmaf-accumulating k = q, q + 16, ...
//     ascending, then the groups added in q order;
//   * an outer product summed over the batch (the gate's weight gradients): b ascending, fmaf; the bias gradient the
//     plain sum in the same order; each then added to the value in memory.
#pragma once

#include "common.h"

namespace sv {

// put(n, W[n][:] . xs + bias[n]) from lane 0 of the wave that owns row n: workgroup x of 4 waves owns rows
// [ROWS x, ROWS (x + 1)), a wave ROWS / 4 consecutive ones.  xs [K] in LDS, W [N][K] 16-B aligned rows (K % 4 == 0).
template <int ROWS, typename Put>
__device__ __forceinline__ void matvec_rows(const float* xs, const float* W, const float* bias, int N, int K, Put put) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int i = 0; i < ROWS / 4; ++i) {
    const int n = blockIdx.x * ROWS + w * (ROWS / 4) + i;  // wave-uniform
    if (n >= N) break;
    const float* wr = W + (size_t)n * K;
    float acc = 0.f;
    for (int k = lane * 4; k < K; k += 256) {
      const float4 wv = *reinterpret_cast<const float4*>(wr + k);
      acc = fmaf(wv.x, xs[k], acc);
      acc = fmaf(wv.y, xs[k + 1], acc);
      acc = fmaf(wv.z, xs[k + 2], acc);
      acc = fmaf(wv.w, xs[k + 3], acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) put(n, acc + bias[n]);
  }
}

// put(n, sum_k vs[k] W[k][n]) from thread n - 64 x of workgroup x, which owns columns [64 x, 64 (x + 1)): thread
// (q = t / 16, 4 columns at (t % 16) * 4).  vs [K] in LDS, staged and synchronised by the caller; red is the
// workgroup's LDS scratch; W [K][N] with N % 4 == 0.
template <typename Put>
__device__ __forceinline__ void tmatvec_cols(const float* vs, float (*red)[64], const float* W, int N, int K, Put put) {
  const int t = threadIdx.x, q = t >> 4, col = (t & 15) * 4, n0 = blockIdx.x * 64 + col;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (n0 < N) {
    for (int k = q; k < K; k += 16) {
      const float4 wv = *reinterpret_cast<const float4*>(W + (size_t)k * N + n0);
      const float x = vs[k];
      acc.x = fmaf(x, wv.x, acc.x);
      acc.y = fmaf(x, wv.y, acc.y);
      acc.z = fmaf(x, wv.z, acc.z);
      acc.w = fmaf(x, wv.w, acc.w);
    }
  }
  red[q][col] = acc.x;
  red[q][col + 1] = acc.y;
  red[q][col + 2] = acc.z;
  red[q][col + 3] = acc.w;
  __syncthreads();
  const int n = blockIdx.x * 64 + t;
  if (t < 64 && n < N) {
    float s = red[0][t];
    for (int j = 1; j < 16; ++j) s += red[j][t];
    put(n, s);
  }
}

// dW[m][n] += sum_b u[b][m] v[b][n],  db[m] += sum_b u[b][m];  u [B][M], v [B][N], N % 4 == 0 (se_core.hip).
// Enqueues one launch on s; the caller reports it through check_launch.
void launch_outer(const float* u, const float* v, float* dW, float* db, int B, int M, int N, hipStream_t s);

}  // namespace sv
