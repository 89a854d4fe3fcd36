// Streaming (flash-style) multi-head self-attention for ViT / DeiT-III above 256 tokens, forward and backward: the
// maths, layouts and number formats of attn.hip (head dimension 64, bf16 operands on the 32x32x16 bf16 MFMA, f32
// accumulation and softmax, P and dS rounded to bf16 once where they become MFMA operands), for 1 <= N <= 2048.
//
// Layouts (see attn.hip): qkv / dqkv bf16 [B][img_rows][3 * heads * 64], out / dout bf16 [B][img_rows][heads * 64],
// lse f32 [B][heads][N]; rows N .. img_rows - 1 of an image are padding, never read, written as zeros in out / dqkv.
// dws f32 [B][heads][N] is the backward's workspace (D = rowsum(dO . O)), allocated by the caller.
//
// The opposite side of the N x N matrix is streamed in tiles of kT = 64 tokens through LDS, shared by the
// workgroup's 4 waves; a workgroup owns kBlk = 128 tokens of one (image, head), a wave 32 of them, one per lane
// (both lane halves).  A tile is staged row-major [token][d] (16-byte row reads = the A operand of a product over d)
// and / or transposed [d][token] (the A operand of a product over tokens, as attn.hip's images; written as packed
// token pairs, conflict-free; where a kernel needs both forms of a matrix they come from the same loads), rows of
// kLd = 72 elements.  One buffer per tile and two barriers per step, nothing prefetched: the other resident
// workgroups cover the tile load, so the register budgets (__launch_bounds__) are set for 4 / 2 / 3 waves per SIMD
// in the forward / dK dV / dQ kernels, without spills (DESIGN.md "ViT / DeiT-III at 256-512 px").
//
// Forward (workgroup per 128 queries, loop over key tiles): S^T = K Q^T with the query on the lane, so the running
// max m and the running sum l are lane values; per key tile one exchange between the lane halves (the max; the two
// halves keep partial sums, added once at the end), then alpha = exp2((m_old - m_new) scale log2e) rescales l and
// O^T; the bf16 P tile is the B operand of O^T += V^T P^T as it stands; 1 / l is a lane constant at the store.
// Backward, three launches on one stream, every element with ONE owning wave that sums in a fixed order (no atomics):
//   D pre-pass   D[b][h][q] = rowsum(dO . O), one thread per row;
//   dK / dV      workgroup per 128 keys (key on the lane), loop over query tiles: attn.hip's phase A with the Q, dO
//                tiles (row-major and transposed), lse and D staged per query tile;
//   dQ           workgroup per 128 queries (query on the lane), loop over key tiles: attn.hip's phase B with K, V
//                (row-major) and K^T staged per key tile.  Block x = 0 also zeroes the pad rows of dqkv.
//
// Hazards, closed by construction:
//  * -inf: m starts at -inf.  A key tile kt exists only if its first key kt * 64 < N, so every tile holds a valid
//    key and m_new is finite after the first tile: (m_old - m_new) is -inf (alpha = exp2(-inf) = 0, and l = 0,
//    O = 0 are rescaled to 0) or finite, never (-inf) - (-inf).  Keys >= N inside the last tile are excluded from the
//    max and contribute p = 0.  The backward has no running max: p = exp2(S scale log2e - lse log2e), with lse of
//    rows >= N replaced by 3e38 (p = 0) and keys >= N forced to p = 0.
//  * EXEC: no ds_read_b64_tr_b16 and no DPP row operation depends on inactive lanes here; the transposed operands are
//    written transposed.  Waves whose 32 tokens are all >= N skip the maths under a wave-uniform flag but run every
//    barrier of the tile loop (no early return before the last barrier).
//  * Bounds: every global row access is guarded by row < N; LDS tiles are zero-filled up to the tile edge, so a
//    masked score is a finite number times zero operands.  kLd * 2 = 144 bytes keeps every 16-byte row fragment and
//    every 8-byte transposed fragment aligned.
//  * LDS: 18 KiB (forward), 36.5 KiB (dK / dV) and 27 KiB (dQ) of static LDS: under 64 KiB, so no attribute call.
//  * Determinism: a workgroup reads only its own (image, head); every sum has one owner and a fixed order, so the
//    results are bitwise equal run to run and an image alone gives the bits of its rows inside a batch.
#include "attn_common.h"

namespace sv {
namespace {

constexpr int kStreamMaxN = 2048;
constexpr int kT = 64;          // tokens of a streamed tile
constexpr int kBlk = 128;       // tokens a workgroup owns (4 waves x 32)
constexpr int kLd = kD + 8;     // row length (elements) of an LDS tile, row-major or transposed (kT == kD)
constexpr int kThreads = 256;
constexpr int kTile = kT * kLd;
static_assert(kT == kD, "one row length serves both tile forms");

// rows t0 .. t0 + kT - 1 of a [rows][ld] bf16 matrix (64 columns from `src`) into a row-major tile; rows >= n: zeros
__device__ __forceinline__ void fill_rows(uint16_t* tile, const uint16_t* src, int64_t ld, int t0, int n, int tid) {
  for (int idx = tid; idx < kT * 8; idx += kThreads) {
    const int t = idx >> 3, c = idx & 7;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (t0 + t < n) v = *reinterpret_cast<const uint4*>(src + (int64_t)(t0 + t) * ld + c * 8);
    *reinterpret_cast<uint4*>(tile + t * kLd + c * 8) = v;
  }
}
// the same rows into a transposed tile [d][token] `tr`: a thread loads the tokens 2 p, 2 p + 1 of 8 columns and packs
// them into 8 words (lanes 0..31: consecutive words of one row; lanes 32..63: 8 rows = 288 words further, the other
// 32 banks); with `rows` it also writes the two rows of the row-major tile from the same loads
__device__ __forceinline__ void fill_tr(uint16_t* rows, uint16_t* tr, const uint16_t* src, int64_t ld, int t0, int n,
                                        int tid) {
  for (int idx = tid; idx < (kT / 2) * 8; idx += kThreads) {
    const int p = idx & (kT / 2 - 1), c = idx / (kT / 2);
    const int t = t0 + 2 * p;
    uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
    if (t < n) a = *reinterpret_cast<const uint4*>(src + (int64_t)t * ld + c * 8);
    if (t + 1 < n) b = *reinterpret_cast<const uint4*>(src + (int64_t)(t + 1) * ld + c * 8);
    if (rows) {
      *reinterpret_cast<uint4*>(rows + (2 * p) * kLd + c * 8) = a;
      *reinterpret_cast<uint4*>(rows + (2 * p + 1) * kLd + c * 8) = b;
    }
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
    uint32_t* dst = reinterpret_cast<uint32_t*>(tr + c * 8 * kLd + 2 * p);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dst[(2 * j) * (kLd / 2)] = (aw[j] & 0xffffu) | (bw[j] << 16);
      dst[(2 * j + 1) * (kLd / 2)] = (aw[j] >> 16) | (bw[j] & 0xffff0000u);
    }
  }
}
// the four k-step fragments of row `t` of a row-major tile
__device__ __forceinline__ void tile_row(const uint16_t* tile, int t, int h, uint4 (&f)[4]) {
  load_row(tile + t * kLd, h, f);
}

__global__ void __launch_bounds__(kThreads, 4) attn_stream_fwd_kernel(const uint16_t* __restrict__ qkv,
                                                                    uint16_t* __restrict__ out,
                                                                    float* __restrict__ lse, int N, int64_t img_rows,
                                                                    int heads, float scale) {
  __shared__ __attribute__((aligned(16))) uint16_t Ks[kTile];
  __shared__ __attribute__((aligned(16))) uint16_t Vt[kTile];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int b = blockIdx.z, hd = blockIdx.y, q0 = blockIdx.x * kBlk + w * 32;
  const int C = heads * kD;
  const int64_t ld = 3 * (int64_t)C;
  const uint16_t* qb = qkv + (int64_t)b * img_rows * ld + hd * kD;
  const uint16_t* kb = qb + C;
  const uint16_t* vb = qb + 2 * C;
  uint16_t* ob = out + (int64_t)b * img_rows * C + hd * kD;
  if (blockIdx.x == 0) zero_pad_rows(ob, C, N, (int)img_rows, tid, kThreads);
  const bool active = q0 < N;  // wave-uniform
  const int q = q0 + r;
  const bool qv = q < N;
  uint4 qf[4];
  load_row(qv ? qb + (int64_t)q * ld : nullptr, h, qf);
  const float sl2 = scale * kLog2e;
  float m = -INFINITY, l = 0.f;  // l: this lane half's part of the row sum
  f32x16 O[2] = {zero16(), zero16()};
  const int nkt = (N + kT - 1) / kT;
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * kT;
    __syncthreads();  // every wave is done with the previous tile
    fill_rows(Ks, kb, ld, k0, N, tid);
    fill_tr(nullptr, Vt, vb, ld, k0, N, tid);
    __syncthreads();
    if (!active) continue;
    f32x16 S[2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      uint4 kf[4];
      tile_row(Ks, sub * 32 + r, h, kf);
      S[sub] = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s) S[sub] = mfma(kf[s], qf[s], S[sub]);
    }
    float tm = -INFINITY;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (k0 + sub * 32 + arow(i, h) < N) tm = fmaxf(tm, S[sub][i]);
    tm = fmaxf(tm, xlane_xor<32>(tm));  // finite: key k0 < N is in the tile
    const float mn = fmaxf(m, tm);
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * sl2);  // first tile: exp2(-inf) = 0
    m = mn;
    float ts = 0.f;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = k0 + sub * 32 + arow(i, h) < N ? __builtin_amdgcn_exp2f((S[sub][i] - mn) * sl2) : 0.f;
        S[sub][i] = p;
        ts += p;
      }
    l = fmaf(l, alpha, ts);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) O[dt][i] *= alpha;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const uint4 pf = acc_frag(S[sub], s);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) O[dt] = mfma(tr_frag(Vt, kLd, dt * 32 + r, sub * 32, s, h), pf, O[dt]);
      }
  }
  l += xlane_xor<32>(l);
  if (!qv) return;  // after the last barrier and the last exchange
  if (h == 0) lse[((int64_t)b * heads + hd) * N + q] = m * scale + __logf(l);
  store_t(ob + (int64_t)q * C, O, 1.0f / l, h);
}

// D[b][hd][q] = rowsum(dO . O)
__global__ void __launch_bounds__(kThreads) attn_stream_dsum_kernel(const uint16_t* __restrict__ out,
                                                                     const uint16_t* __restrict__ dout,
                                                                     float* __restrict__ dws, int N, int64_t img_rows,
                                                                     int heads) {
  const int q = blockIdx.x * kThreads + threadIdx.x, hd = blockIdx.y, b = blockIdx.z;
  if (q >= N) return;
  const int C = heads * kD;
  const int64_t off = ((int64_t)b * img_rows + q) * C + hd * kD;
  dws[((int64_t)b * heads + hd) * N + q] = row_dot64(out + off, dout + off);
}

__global__ void __launch_bounds__(kThreads, 2) attn_stream_dkv_kernel(const uint16_t* __restrict__ qkv,
                                                                    const float* __restrict__ lse,
                                                                    const float* __restrict__ dws,
                                                                    const uint16_t* __restrict__ dout,
                                                                    uint16_t* __restrict__ dqkv, int N, int64_t img_rows,
                                                                    int heads, float scale) {
  __shared__ __attribute__((aligned(16))) uint16_t Qs[kTile];
  __shared__ __attribute__((aligned(16))) uint16_t dOs[kTile];
  __shared__ __attribute__((aligned(16))) uint16_t Qt[kTile];
  __shared__ __attribute__((aligned(16))) uint16_t dOt[kTile];
  __shared__ __attribute__((aligned(16))) float L2[kT];  // lse * log2(e); rows >= N: huge (p = 0)
  __shared__ __attribute__((aligned(16))) float Dl[kT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int b = blockIdx.z, hd = blockIdx.y, key0 = blockIdx.x * kBlk + w * 32;
  const int C = heads * kD;
  const int64_t ld = 3 * (int64_t)C;
  const uint16_t* qb = qkv + (int64_t)b * img_rows * ld + hd * kD;
  const uint16_t* kb = qb + C;
  const uint16_t* vb = qb + 2 * C;
  const uint16_t* dob = dout + (int64_t)b * img_rows * C + hd * kD;
  uint16_t* dqb = dqkv + (int64_t)b * img_rows * ld + hd * kD;
  const float* lb = lse + ((int64_t)b * heads + hd) * N;
  const float* db = dws + ((int64_t)b * heads + hd) * N;
  const bool active = key0 < N;  // wave-uniform
  const int own = key0 + r;
  const bool ownv = own < N;
  const float sl2 = scale * kLog2e;
  uint4 kf[4], vf[4];
  load_row(ownv ? kb + (int64_t)own * ld : nullptr, h, kf);
  load_row(ownv ? vb + (int64_t)own * ld : nullptr, h, vf);
  f32x16 dVt[2] = {zero16(), zero16()}, dKt[2] = {zero16(), zero16()};
  const int nqt = (N + kT - 1) / kT;
  for (int qt = 0; qt < nqt; ++qt) {
    const int t0 = qt * kT;
    __syncthreads();
    fill_tr(Qs, Qt, qb, ld, t0, N, tid);
    fill_tr(dOs, dOt, dob, C, t0, N, tid);
    if (tid < kT) {
      const bool v = t0 + tid < N;
      L2[tid] = v ? lb[t0 + tid] * kLog2e : 3.0e38f;
      Dl[tid] = v ? db[t0 + tid] : 0.f;
    }
    __syncthreads();
    if (!active) continue;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      uint4 qa[4], da[4];
      tile_row(Qs, sub * 32 + r, h, qa);
      tile_row(dOs, sub * 32 + r, h, da);
      f32x16 S = zero16(), dP = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s) S = mfma(qa[s], kf[s], S);
#pragma unroll
      for (int s = 0; s < 4; ++s) dP = mfma(da[s], vf[s], dP);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 l4 = *reinterpret_cast<const float4*>(L2 + sub * 32 + 8 * g + 4 * h);
        const float4 d4 = *reinterpret_cast<const float4*>(Dl + sub * 32 + 8 * g + 4 * h);
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
          dVt[dt] = mfma(tr_frag(dOt, kLd, dt * 32 + r, sub * 32, s, h), pf, dVt[dt]);
          dKt[dt] = mfma(tr_frag(Qt, kLd, dt * 32 + r, sub * 32, s, h), dsf, dKt[dt]);
        }
      }
    }
  }
  if (!ownv) return;  // after the last barrier
  store_t(dqb + (int64_t)own * ld + C, dKt, 1.0f, h);
  store_t(dqb + (int64_t)own * ld + 2 * C, dVt, 1.0f, h);
}

__global__ void __launch_bounds__(kThreads, 3) attn_stream_dq_kernel(const uint16_t* __restrict__ qkv,
                                                                   const float* __restrict__ lse,
                                                                   const float* __restrict__ dws,
                                                                   const uint16_t* __restrict__ dout,
                                                                   uint16_t* __restrict__ dqkv, int N, int64_t img_rows,
                                                                   int heads, float scale) {
  __shared__ __attribute__((aligned(16))) uint16_t Ks[kTile];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[kTile];
  __shared__ __attribute__((aligned(16))) uint16_t Kt[kTile];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int b = blockIdx.z, hd = blockIdx.y, q0 = blockIdx.x * kBlk + w * 32;
  const int C = heads * kD;
  const int64_t ld = 3 * (int64_t)C;
  const uint16_t* qb = qkv + (int64_t)b * img_rows * ld + hd * kD;
  const uint16_t* kb = qb + C;
  const uint16_t* vb = qb + 2 * C;
  const uint16_t* dob = dout + (int64_t)b * img_rows * C + hd * kD;
  uint16_t* dqb = dqkv + (int64_t)b * img_rows * ld + hd * kD;
  if (blockIdx.x == 0) {
#pragma unroll
    for (int part = 0; part < 3; ++part) zero_pad_rows(dqb + part * C, ld, N, (int)img_rows, tid, kThreads);
  }
  const bool active = q0 < N;  // wave-uniform
  const int own = q0 + r;
  const bool ownv = own < N;
  const float sl2 = scale * kLog2e;
  uint4 qf[4], df[4];
  load_row(ownv ? qb + (int64_t)own * ld : nullptr, h, qf);
  load_row(ownv ? dob + (int64_t)own * C : nullptr, h, df);
  const float lq = ownv ? lse[((int64_t)b * heads + hd) * N + own] * kLog2e : 3.0e38f;
  const float dq = ownv ? dws[((int64_t)b * heads + hd) * N + own] : 0.f;
  f32x16 dQt[2] = {zero16(), zero16()};
  const int nkt = (N + kT - 1) / kT;
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * kT;
    __syncthreads();
    fill_tr(Ks, Kt, kb, ld, k0, N, tid);
    fill_rows(Vs, vb, ld, k0, N, tid);
    __syncthreads();
    if (!active) continue;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      uint4 ka[4], va[4];
      tile_row(Ks, sub * 32 + r, h, ka);
      tile_row(Vs, sub * 32 + r, h, va);
      f32x16 S = zero16(), dP = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s) S = mfma(ka[s], qf[s], S);
#pragma unroll
      for (int s = 0; s < 4; ++s) dP = mfma(va[s], df[s], dP);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = k0 + sub * 32 + arow(i, h) < N ? __builtin_amdgcn_exp2f(fmaf(S[i], sl2, -lq)) : 0.f;
        dP[i] = p * (dP[i] - dq) * scale;
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const uint4 dsf = acc_frag(dP, s);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) dQt[dt] = mfma(tr_frag(Kt, kLd, dt * 32 + r, sub * 32, s, h), dsf, dQt[dt]);
      }
    }
  }
  if (ownv) store_t(dqb + (int64_t)own * ld, dQt, 1.0f, h);
}

// argument checks shared by the two passes; SV_OK, or the status already reported through set_error
static int check_args(const char* who, int B, int N, int64_t img_rows, int heads, int head_dim, float scale) {
  if (B <= 0 || N <= 0 || heads <= 0 || img_rows < N)
    return set_error(SV_ERR_INVALID_ARG, "%s: need B, N, heads > 0 and img_rows >= N (B %d, N %d, heads %d, img_rows %lld)",
                     who, B, N, heads, (long long)img_rows);
  if (!(scale > 0.f) || !(scale < 1e30f)) return set_error(SV_ERR_INVALID_ARG, "%s: scale must be positive and finite", who);
  if (head_dim != kD) return set_error(SV_ERR_UNSUPPORTED, "%s: head dimension %d (only 64 is built)", who, head_dim);
  if (N > kStreamMaxN) return set_error(SV_ERR_UNSUPPORTED, "%s: N = %d tokens (at most %d)", who, N, kStreamMaxN);
  if (B > 65535 || heads > 65535) return set_error(SV_ERR_UNSUPPORTED, "%s: B and heads at most 65535", who);
  if (img_rows > (int64_t)1 << 30) return set_error(SV_ERR_UNSUPPORTED, "%s: img_rows at most 2^30", who);
  return SV_OK;
}

}  // namespace
}  // namespace sv

using namespace sv;

extern "C" {

int sv_attn_stream_fwd(const uint16_t* qkv, uint16_t* out, float* lse, int32_t B, int32_t N, int64_t img_rows,
                       int32_t heads, int32_t head_dim, float scale, sv_stream_t stream) {
  SV_REQUIRE(qkv && out && lse, "sv_attn_stream_fwd: null pointer");
  if (img_rows == 0) img_rows = N;
  if (const int rc = check_args("sv_attn_stream_fwd", B, N, img_rows, heads, head_dim, scale)) return rc;
  SV_REQUIRE(al16(qkv) && al16(out) && ((uintptr_t)lse & 3) == 0, "sv_attn_stream_fwd: qkv / out must be 16-byte aligned");
  attn_stream_fwd_kernel<<<dim3((N + kBlk - 1) / kBlk, heads, B), kThreads, 0, (hipStream_t)stream>>>(
      qkv, out, lse, N, img_rows, heads, scale);
  return check_launch("sv_attn_stream_fwd");
}

int sv_attn_stream_bwd(const uint16_t* qkv, const uint16_t* out, const float* lse, const uint16_t* dout,
                       uint16_t* dqkv, float* dws, int32_t B, int32_t N, int64_t img_rows, int32_t heads,
                       int32_t head_dim, float scale, sv_stream_t stream) {
  SV_REQUIRE(qkv && out && lse && dout && dqkv && dws, "sv_attn_stream_bwd: null pointer");
  if (img_rows == 0) img_rows = N;
  if (const int rc = check_args("sv_attn_stream_bwd", B, N, img_rows, heads, head_dim, scale)) return rc;
  SV_REQUIRE(al16(qkv) && al16(out) && al16(dout) && al16(dqkv) && ((uintptr_t)lse & 3) == 0 && ((uintptr_t)dws & 3) == 0,
             "sv_attn_stream_bwd: qkv / out / dout / dqkv must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  attn_stream_dsum_kernel<<<dim3((N + kThreads - 1) / kThreads, heads, B), kThreads, 0, s>>>(out, dout, dws, N, img_rows,
                                                                                           heads);
  if (const int rc = check_launch("sv_attn_stream_bwd (D)")) return rc;
  const dim3 grid((N + kBlk - 1) / kBlk, heads, B);
  attn_stream_dkv_kernel<<<grid, kThreads, 0, s>>>(qkv, lse, dws, dout, dqkv, N, img_rows, heads, scale);
  if (const int rc = check_launch("sv_attn_stream_bwd (dK, dV)")) return rc;
  attn_stream_dq_kernel<<<grid, kThreads, 0, s>>>(qkv, lse, dws, dout, dqkv, N, img_rows, heads, scale);
  return check_launch("sv_attn_stream_bwd (dQ)");
}

}  // extern "C"
