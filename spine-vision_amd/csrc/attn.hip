// Fused multi-head self-attention for the ViT / DeiT-III blocks (timm Attention, head dimension 64), forward and
// backward, bf16 operands on the 32x32x16 bf16 MFMA with f32 accumulation and an f32 softmax.
//
// Layouts (exactly what the neighbouring GEMMs store and read; nothing is permuted or copied):
//   qkv / dqkv  bf16 [B][img_rows][3 * heads * 64]   columns ordered (q|k|v, head, d): the qkv Linear's output
//   out / dout  bf16 [B][img_rows][heads * 64]       heads concatenated on the channel axis: the proj Linear's operand
//   lse         f32  [B][heads][N]                   row log-sum-exp of the scaled scores, kept for the backward
// An image owns img_rows >= N rows of each matrix, of which the first N are tokens.  Rows N .. img_rows - 1 are
// padding: never read, and written as zeros in `out` and `dqkv` (so the GEMMs that follow see zero rows there).
//
// N <= 256 and d = 64, so an (image, head)'s whole K or V is 32 KiB: every key of a head is visited in ONE pass --
// no online-softmax rescaling.  The N x N probabilities never reach HBM.
//
// Forward, a workgroup = 4 waves = 128 queries of one (image, head), a wave = 32 queries:
//   S^T = K Q^T  (A = a 32-key tile of K, B = the wave's Q rows, both 16-byte row reads from global memory; the K
//   tiles are shared by the 4 waves through L1/L2).  The 32x32 accumulator has the QUERY on the lane and the keys in
//   the 16 registers, for up to 8 key tiles = 128 registers: row max and row sum are register loops plus one
//   exchange between the two lane halves; P is rounded to bf16 once and IS the B operand of O^T = V^T P^T (an
//   accumulator tile as the next MFMA's operand: no LDS, no lane movement); the A operand V^T comes from a transposed
//   LDS image of V [d][key], written once per workgroup.  O^T again has the query on the lane, so 1 / rowsum is a
//   lane constant.  Keys >= N are excluded from max and sum (p = 0); query rows >= N are neither loaded nor stored.
//
// Backward, ONE workgroup (8 waves) per (image, head), so dK and dV have one owner and dQ is summed inside it in a
// fixed order: no atomics, bitwise reproducible.  P is recomputed from lse, D = rowsum(dO . O).
//   phase A (key on the lane; wave w owns keys 32w..32w+31, loops over query tiles):
//     S = Q K^T, dP = dO V^T, P = exp(scale S - lse), dS = P (dP - D) scale;
//     dV^T += dO^T P, dK^T += Q^T dS   (P / dS accumulators as B operands; dO^T, Q^T from transposed LDS images)
//   phase B (query on the lane; wave w owns queries 32w..32w+31, loops over key tiles):
//     S^T = K Q^T, dP^T = V dO^T, dS^T as above; dQ^T += K^T dS^T   (K^T from a transposed LDS image)
//   Phase B recomputes S and dP (7 MFMA products instead of 5) so that no accumulator tile crosses LDS.
//
// Bounds: every global row access is guarded by row < N (zero fragment otherwise); LDS images are zero-filled up to
// the 32-row tile boundary and only read below it.
#include "attn_common.h"

namespace sv {
namespace {

constexpr int kMaxN = 256;        // tokens per image
constexpr int kLdT = kMaxN + 8;   // row length (elements) of a transposed [d][token] LDS image: 528 B, 8-B aligned
constexpr int kFwdThreads = 256, kBwdThreads = 512;
constexpr int kImgElems = kD * kLdT;
constexpr int kBwdLds = 3 * kImgElems * 2 + 2 * kMaxN * 4;

// rows [0, np) of a [rows][ld] bf16 matrix (64 columns from `src`) into a transposed image; rows >= n are zeros
__device__ __forceinline__ void fill_transposed(uint16_t* img, const uint16_t* src, int64_t ld, int n, int np,
                                                int tid, int nthreads) {
  for (int idx = tid; idx < np * 8; idx += nthreads) {
    const int t = idx >> 3, c = idx & 7;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (t < n) v = *reinterpret_cast<const uint4*>(src + (int64_t)t * ld + c * 8);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      img[(c * 8 + 2 * j) * kLdT + t] = (uint16_t)(w[j] & 0xffffu);
      img[(c * 8 + 2 * j + 1) * kLdT + t] = (uint16_t)(w[j] >> 16);
    }
  }
}

__global__ void __launch_bounds__(kFwdThreads) attn_fwd_kernel(const uint16_t* __restrict__ qkv,
                                                                uint16_t* __restrict__ out, float* __restrict__ lse,
                                                                int N, int64_t img_rows, int heads, float scale) {
  __shared__ __attribute__((aligned(16))) uint16_t Vt[kImgElems];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int b = blockIdx.z, hd = blockIdx.y, q0 = blockIdx.x * 128 + w * 32;
  const int C = heads * kD;
  const int64_t ld = 3 * (int64_t)C;
  const uint16_t* qb = qkv + (int64_t)b * img_rows * ld + hd * kD;
  const uint16_t* kb = qb + C;
  uint16_t* ob = out + (int64_t)b * img_rows * C + hd * kD;
  const int nt = (N + 31) >> 5;
  fill_transposed(Vt, qb + 2 * C, ld, N, nt * 32, tid, kFwdThreads);
  if (blockIdx.x == 0) zero_pad_rows(ob, C, N, (int)img_rows, tid, kFwdThreads);
  __syncthreads();
  if (q0 >= N) return;  // wave-uniform; no barrier below
  const int q = q0 + r;
  const bool qv = q < N;
  uint4 qf[4];
  load_row(qv ? qb + (int64_t)q * ld : nullptr, h, qf);
  f32x16 S[8];
#pragma unroll
  for (int kt = 0; kt < 8; ++kt) {
    if (kt < nt) {
      const int key = kt * 32 + r;
      uint4 kf[4];
      load_row(key < N ? kb + (int64_t)key * ld : nullptr, h, kf);
      S[kt] = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s) S[kt] = mfma(kf[s], qf[s], S[kt]);
    }
  }
  // softmax over the keys of this lane's query: the registers of both lane halves
  float m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < 8; ++kt)
    if (kt < nt)
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (kt * 32 + arow(i, h) < N) m = fmaxf(m, S[kt][i]);
  m = fmaxf(m, xlane_xor<32>(m));
  const float sl2 = scale * kLog2e;
  float l = 0.f;
#pragma unroll
  for (int kt = 0; kt < 8; ++kt)
    if (kt < nt)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = kt * 32 + arow(i, h) < N ? __builtin_amdgcn_exp2f((S[kt][i] - m) * sl2) : 0.f;
        S[kt][i] = p;
        l += p;
      }
  l += xlane_xor<32>(l);
  if (qv && h == 0) lse[((int64_t)b * heads + hd) * N + q] = m * scale + __logf(l);
  // O^T = V^T P^T
  f32x16 O[2] = {zero16(), zero16()};
#pragma unroll
  for (int kt = 0; kt < 8; ++kt)
    if (kt < nt)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const uint4 pf = acc_frag(S[kt], s);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) O[dt] = mfma(tr_frag(Vt, kLdT, dt * 32 + r, kt * 32, s, h), pf, O[dt]);
      }
  if (qv) store_t(ob + (int64_t)q * C, O, 1.0f / l, h);
}

__global__ void __launch_bounds__(kBwdThreads) attn_bwd_kernel(const uint16_t* __restrict__ qkv,
                                                                const uint16_t* __restrict__ out,
                                                                const float* __restrict__ lse,
                                                                const uint16_t* __restrict__ dout,
                                                                uint16_t* __restrict__ dqkv, int N, int64_t img_rows,
                                                                int heads, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t* Qt = reinterpret_cast<uint16_t*>(smem);
  uint16_t* dOt = Qt + kImgElems;
  uint16_t* Kt = dOt + kImgElems;
  float* L2 = reinterpret_cast<float*>(Kt + kImgElems);  // lse * log2(e); rows >= N: huge (p = 0)
  float* Dl = L2 + kMaxN;                                // rowsum(dO . O)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int hd = blockIdx.x, b = blockIdx.y;
  const int C = heads * kD;
  const int64_t ld = 3 * (int64_t)C;
  const uint16_t* qb = qkv + (int64_t)b * img_rows * ld + hd * kD;
  const uint16_t* kb = qb + C;
  const uint16_t* vb = qb + 2 * C;
  const uint16_t* ob = out + (int64_t)b * img_rows * C + hd * kD;
  const uint16_t* dob = dout + (int64_t)b * img_rows * C + hd * kD;
  uint16_t* dqb = dqkv + (int64_t)b * img_rows * ld + hd * kD;
  const int nt = (N + 31) >> 5;
  fill_transposed(Qt, qb, ld, N, nt * 32, tid, kBwdThreads);
  fill_transposed(dOt, dob, C, N, nt * 32, tid, kBwdThreads);
  fill_transposed(Kt, kb, ld, N, nt * 32, tid, kBwdThreads);
  if (tid < kMaxN) {
    float l2 = 3.0e38f, dsum = 0.f;
    if (tid < N) {
      l2 = lse[((int64_t)b * heads + hd) * N + tid] * kLog2e;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint4 o = *reinterpret_cast<const uint4*>(ob + (int64_t)tid * C + c * 8);
        const uint4 g = *reinterpret_cast<const uint4*>(dob + (int64_t)tid * C + c * 8);
        const uint32_t ow[4] = {o.x, o.y, o.z, o.w}, gw[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          dsum = fmaf(__uint_as_float(ow[j] << 16), __uint_as_float(gw[j] << 16), dsum);
          dsum = fmaf(__uint_as_float(ow[j] & 0xffff0000u), __uint_as_float(gw[j] & 0xffff0000u), dsum);
        }
      }
    }
    L2[tid] = l2;
    Dl[tid] = dsum;
  }
#pragma unroll
  for (int part = 0; part < 3; ++part) zero_pad_rows(dqb + part * C, ld, N, (int)img_rows, tid, kBwdThreads);
  __syncthreads();  // the LDS images are read-only from here on: no further barrier
  if (w >= nt) return;
  const float sl2 = scale * kLog2e;
  const int own = w * 32 + r;  // this lane's key (phase A) / query (phase B)
  const bool ownv = own < N;
  {  // ---- phase A: dK, dV of keys 32 w .. 32 w + 31
    uint4 kf[4], vf[4];
    load_row(ownv ? kb + (int64_t)own * ld : nullptr, h, kf);
    load_row(ownv ? vb + (int64_t)own * ld : nullptr, h, vf);
    f32x16 dVt[2] = {zero16(), zero16()}, dKt[2] = {zero16(), zero16()};
    for (int qt = 0; qt < nt; ++qt) {
      const int q = qt * 32 + r;
      uint4 qa[4], da[4];
      load_row(q < N ? qb + (int64_t)q * ld : nullptr, h, qa);
      load_row(q < N ? dob + (int64_t)q * C : nullptr, h, da);
      f32x16 S = zero16(), dP = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s) S = mfma(qa[s], kf[s], S);
#pragma unroll
      for (int s = 0; s < 4; ++s) dP = mfma(da[s], vf[s], dP);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 l4 = *reinterpret_cast<const float4*>(L2 + qt * 32 + 8 * g + 4 * h);
        const float4 d4 = *reinterpret_cast<const float4*>(Dl + qt * 32 + 8 * g + 4 * h);
        const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, dq[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float p = ownv ? __builtin_amdgcn_exp2f(fmaf(S[4 * g + j], sl2, -lq[j])) : 0.f;
          S[4 * g + j] = p;
          dP[4 * g + j] = p * (dP[4 * g + j] - dq[j]) * scale;
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const uint4 pf = acc_frag(S, s), dsf = acc_frag(dP, s);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dVt[dt] = mfma(tr_frag(dOt, kLdT, dt * 32 + r, qt * 32, s, h), pf, dVt[dt]);
          dKt[dt] = mfma(tr_frag(Qt, kLdT, dt * 32 + r, qt * 32, s, h), dsf, dKt[dt]);
        }
      }
    }
    if (ownv) {
      store_t(dqb + (int64_t)own * ld + C, dKt, 1.0f, h);
      store_t(dqb + (int64_t)own * ld + 2 * C, dVt, 1.0f, h);
    }
  }
  {  // ---- phase B: dQ of queries 32 w .. 32 w + 31
    uint4 qf[4], df[4];
    load_row(ownv ? qb + (int64_t)own * ld : nullptr, h, qf);
    load_row(ownv ? dob + (int64_t)own * C : nullptr, h, df);
    const float lq = L2[own], dq = Dl[own];
    f32x16 dQt[2] = {zero16(), zero16()};
    for (int kt = 0; kt < nt; ++kt) {
      const int key = kt * 32 + r;
      uint4 ka[4], va[4];
      load_row(key < N ? kb + (int64_t)key * ld : nullptr, h, ka);
      load_row(key < N ? vb + (int64_t)key * ld : nullptr, h, va);
      f32x16 S = zero16(), dP = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s) S = mfma(ka[s], qf[s], S);
#pragma unroll
      for (int s = 0; s < 4; ++s) dP = mfma(va[s], df[s], dP);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = kt * 32 + arow(i, h) < N ? __builtin_amdgcn_exp2f(fmaf(S[i], sl2, -lq)) : 0.f;
        dP[i] = p * (dP[i] - dq) * scale;
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const uint4 dsf = acc_frag(dP, s);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) dQt[dt] = mfma(tr_frag(Kt, kLdT, dt * 32 + r, kt * 32, s, h), dsf, dQt[dt]);
      }
    }
    if (ownv) store_t(dqb + (int64_t)own * ld, dQt, 1.0f, h);
  }
}

// argument checks shared by the two passes; SV_OK, or the status already reported through set_error
static int check_args(const char* who, int B, int N, int64_t img_rows, int heads, int head_dim, float scale) {
  if (B <= 0 || N <= 0 || heads <= 0 || img_rows < N)
    return set_error(SV_ERR_INVALID_ARG, "%s: need B, N, heads > 0 and img_rows >= N (B %d, N %d, heads %d, img_rows %lld)",
                     who, B, N, heads, (long long)img_rows);
  if (!(scale > 0.f) || !(scale < 1e30f)) return set_error(SV_ERR_INVALID_ARG, "%s: scale must be positive and finite", who);
  if (head_dim != kD) return set_error(SV_ERR_UNSUPPORTED, "%s: head dimension %d (only 64 is built)", who, head_dim);
  if (N > kMaxN) return set_error(SV_ERR_UNSUPPORTED, "%s: N = %d tokens (at most %d)", who, N, kMaxN);
  if (B > 65535 || heads > 65535) return set_error(SV_ERR_UNSUPPORTED, "%s: B and heads at most 65535", who);
  return SV_OK;
}

}  // namespace
}  // namespace sv

using namespace sv;

extern "C" {

int sv_attn_fwd(const uint16_t* qkv, uint16_t* out, float* lse, int32_t B, int32_t N, int64_t img_rows, int32_t heads,
                int32_t head_dim, float scale, sv_stream_t stream) {
  SV_REQUIRE(qkv && out && lse, "sv_attn_fwd: null pointer");
  if (img_rows == 0) img_rows = N;
  if (const int rc = check_args("sv_attn_fwd", B, N, img_rows, heads, head_dim, scale)) return rc;
  SV_REQUIRE(al16(qkv) && al16(out) && ((uintptr_t)lse & 3) == 0, "sv_attn_fwd: qkv / out must be 16-byte aligned");
  attn_fwd_kernel<<<dim3((N + 127) / 128, heads, B), kFwdThreads, 0, (hipStream_t)stream>>>(qkv, out, lse, N, img_rows,
                                                                                          heads, scale);
  return check_launch("sv_attn_fwd");
}

int sv_attn_bwd(const uint16_t* qkv, const uint16_t* out, const float* lse, const uint16_t* dout, uint16_t* dqkv,
                int32_t B, int32_t N, int64_t img_rows, int32_t heads, int32_t head_dim, float scale,
                sv_stream_t stream) {
  SV_REQUIRE(qkv && out && lse && dout && dqkv, "sv_attn_bwd: null pointer");
  if (img_rows == 0) img_rows = N;
  if (const int rc = check_args("sv_attn_bwd", B, N, img_rows, heads, head_dim, scale)) return rc;
  SV_REQUIRE(al16(qkv) && al16(out) && al16(dout) && al16(dqkv) && ((uintptr_t)lse & 3) == 0,
             "sv_attn_bwd: qkv / out / dout / dqkv must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (const int rc = ensure_lds_attr(reinterpret_cast<const void*>(&attn_bwd_kernel), kBwdLds, s)) return rc;
  attn_bwd_kernel<<<dim3(heads, B), kBwdThreads, kBwdLds, s>>>(qkv, out, lse, dout, dqkv, N, img_rows, heads, scale);
  return check_launch("sv_attn_bwd");
}

}  // extern "C"
