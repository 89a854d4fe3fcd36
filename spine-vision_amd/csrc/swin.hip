// Swin Transformer kernels: shifted-window attention with a learned relative-position bias (timm WindowAttention,
// head dimension 32, windows of up to 8 x 8 tokens), forward and backward, on the 32x32x16 bf16 MFMA with f32
// accumulation and an f32 softmax; the bias table's expansion and gradient; the 2x2 patch-merging gather and its
// inverse; and the two per-sample row scalings of stochastic depth.
//
// Layouts of the attention pair (what the neighbouring GEMMs store and read; no permute, roll or window copy):
//   qkv / dqkv  bf16 [rows][3 * heads * 32]   columns (q|k|v, head, d), rows in image raster order b*H*W + y*W + x
//   out / dout  bf16 [rows][heads * 32]
//   lse         f32  [B * nW][heads][w*w]      nW = (H/w) * (W/w) windows per image, window (wy, wx) = wy * (W/w) + wx
//   bias        f32  [heads][w*w][w*w]         dense, from sv_swin_bias_expand
// Token (i, j) of window (wy, wx) is the pixel ((wy*w + i + shift) mod H, (wx*w + j + shift) mod W): the cyclic
// shift, the window partition and their inverses are this one index.  The shifted-window mask is computed from the
// region of the ROLLED coordinate (wy*w + i, wx*w + j): rows [0, H-w) | [H-w, H-shift) | [H-shift, H), columns
// likewise; a query / key pair of different regions gets -100 added to its score before the softmax.
//
// A workgroup is ONE wave, which walks the windows part, part + nparts, ... of one head.  N = w*w <= 64 tokens and
// d = 32, so a whole (window, head) is four 32x32 score tiles at two k-steps each.  The head's dense bias stays in
// LDS (a [64][65] f32 image) across the windows of the walk.
//   forward (query on the lane): S^T = K Q^T; score = scale S + bias + mask; row max / sum are register loops and
//     one exchange between the lane halves; P rounded to bf16 once IS the B operand of O^T = V^T P^T (V^T from a
//     transposed LDS image).
//   backward (key on the lane): S = Q K^T, dP = dO V^T, P = exp(score - lse), T = P (dP - D), dS = scale T;
//     dV^T += dO^T P, dK^T += Q^T dS (accumulators as B operands, Q^T / dO^T from transposed LDS images); dS goes
//     through LDS once as bf16 [query][key] and is the B operand of dQ^T = K^T dS^T.  dq, dk, dv of a (window, head)
//     have this one owner.  T is summed over the walk in 64 accumulator registers and stored once per wave as
//     dbias_part [part][head][N][N]; sv_swin_bias_grad folds the parts in part order.  No atomics anywhere.
// Bounds: a token >= N has no row (zero fragments, zero LDS columns, p = 0, nothing stored); rows >= B*H*W of `out`
// and `dqkv` are written as zeros and never read.
#include "attn_common.h"

namespace sv {
namespace {

constexpr int kHd = 32;            // head dimension
constexpr int kMaxW = 8;           // window side
constexpr int kTok = 64;           // tokens of the largest window
constexpr int kLdI = kTok + 8;     // row (elements) of a transposed [d][token] bf16 image / the dS image: 144 B
constexpr int kLdB = kTok + 1;     // row (floats) of the bias image: conflict-free by row and by column
constexpr int kImg = kHd * kLdI;
constexpr float kMasked = -100.0f;
constexpr int kWaveTarget = 1024;  // waves of a launch: one per SIMD of the device

struct WinGeom {
  int B, H, W, w, shift, heads, nwx, nwin, N;  // nwx windows per row, nwin per image, N = w * w
};

// the raster row and the mask region of token t of (global) window `win`
__device__ __forceinline__ void token_of(const WinGeom& g, int win, int t, int& row, int& label) {
  const int b = win / g.nwin, wi = win - b * g.nwin, wy = wi / g.nwx, wx = wi - wy * g.nwx;
  const int i = t / g.w, j = t - i * g.w;
  const int yr = wy * g.w + i, xr = wx * g.w + j;  // in the rolled map
  int y = yr + g.shift, x = xr + g.shift;
  if (y >= g.H) y -= g.H;
  if (x >= g.W) x -= g.W;
  row = (b * g.H + y) * g.W + x;
  const int ly = yr < g.H - g.w ? 0 : (yr < g.H - g.shift ? 1 : 2);
  const int lx = xr < g.W - g.w ? 0 : (xr < g.W - g.shift ? 1 : 2);
  label = g.shift ? ly * 3 + lx : 0;
}

// the two k-step fragments (d = 16 s + 8 h .. + 7) of one 32-wide row; row < 0: zeros
__device__ __forceinline__ void load_row32(const uint16_t* base, int64_t ld, int row, int h, uint4 (&f)[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s)
    f[s] = row >= 0 ? *reinterpret_cast<const uint4*>(base + (int64_t)row * ld + 16 * s + 8 * h) : make_uint4(0u, 0u, 0u, 0u);
}
// one token's 32-wide row (zeros when row < 0) into column t of a transposed image
__device__ __forceinline__ void put_transposed(uint16_t* img, const uint4 (&v)[4], int t) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const uint32_t w[4] = {v[c].x, v[c].y, v[c].z, v[c].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      img[(c * 8 + 2 * j) * kLdI + t] = (uint16_t)(w[j] & 0xffffu);
      img[(c * 8 + 2 * j + 1) * kLdI + t] = (uint16_t)(w[j] >> 16);
    }
  }
}
__device__ __forceinline__ void load_full32(const uint16_t* base, int64_t ld, int row, uint4 (&v)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c)
    v[c] = row >= 0 ? *reinterpret_cast<const uint4*>(base + (int64_t)row * ld + c * 8) : make_uint4(0u, 0u, 0u, 0u);
}
// a 32 (d) x 32 (token on the lane) accumulator tile -> one row of a [token][ld] bf16 matrix
__device__ __forceinline__ void store_t32(uint16_t* row, const f32x16& acc, float mul, int h) {
#pragma unroll
  for (int g = 0; g < 4; ++g)
    *reinterpret_cast<uint2*>(row + 8 * g + 4 * h) = make_uint2(pack2bf(acc[4 * g] * mul, acc[4 * g + 1] * mul),
                                                                pack2bf(acc[4 * g + 2] * mul, acc[4 * g + 3] * mul));
}
// the head's dense bias [N][N] as a [64][65] image, zero outside
__device__ __forceinline__ void fill_bias(float* Bs, const float* bias_h, int N, int lane) {
  for (int idx = lane; idx < kTok * kTok; idx += 64) {
    const int q = idx >> 6, k = idx & 63;
    Bs[q * kLdB + k] = (q < N && k < N) ? bias_h[q * N + k] : 0.f;
  }
}
// 32 columns of rows [n, rows) of a [rows][ld] bf16 matrix := 0
__device__ __forceinline__ void zero_tail32(uint16_t* dst, int64_t ld, int64_t n, int64_t rows, int lane) {
  for (int64_t idx = lane; idx < (rows - n) * 4; idx += 64)
    *reinterpret_cast<uint4*>(dst + (n + (idx >> 2)) * ld + (idx & 3) * 8) = make_uint4(0u, 0u, 0u, 0u);
}

__global__ void __launch_bounds__(64) winattn_fwd_kernel(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ out,
                                                          float* __restrict__ lse, const float* __restrict__ bias,
                                                          WinGeom g, int nparts, float scale, int64_t rows_total) {
  __shared__ float Bs[kTok * kLdB];
  __shared__ __attribute__((aligned(16))) uint16_t Vt[kImg];
  __shared__ int rowi[kTok];
  __shared__ __attribute__((aligned(4))) uint8_t lab[kTok];
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int part = blockIdx.x, hd = blockIdx.y;
  const int N = g.N, nt = (N + 31) >> 5, C = g.heads * kHd;
  const int64_t ld = 3 * (int64_t)C;
  const uint16_t* qb = qkv + hd * kHd;
  const uint16_t* kb = qb + C;
  const uint16_t* vb = qb + 2 * C;
  uint16_t* ob = out + hd * kHd;
  fill_bias(Bs, bias + (int64_t)hd * N * N, N, lane);
  if (part == 0) zero_tail32(ob, C, (int64_t)g.B * g.H * g.W, rows_total, lane);
  const int total = g.B * g.nwin;
  for (int win = part; win < total; win += nparts) {
    __syncthreads();  // the previous window's reads of Vt / rowi / lab are done
    {
      int row = -1, label = 0;
      if (lane < N) token_of(g, win, lane, row, label);
      rowi[lane] = row;
      lab[lane] = (uint8_t)label;
      uint4 v[4];
      load_full32(vb, ld, row, v);
      put_transposed(Vt, v, lane);
    }
    __syncthreads();
    uint4 qf[2][2], kf[2][2];
    int qrow[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
      if (t < nt) {
        qrow[t] = rowi[t * 32 + r];
        load_row32(qb, ld, qrow[t], h, qf[t]);
        load_row32(kb, ld, qrow[t], h, kf[t]);
      }
    f32x16 S[2][2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
        if (qt < nt && kt < nt) {
          S[qt][kt] = zero16();
#pragma unroll
          for (int s = 0; s < 2; ++s) S[qt][kt] = mfma(kf[kt][s], qf[qt][s], S[qt][kt]);
        }
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
      if (qt < nt) {
        const int q = qt * 32 + r;
        const uint32_t lq = lab[q];
        const float* brow = Bs + q * kLdB;
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
          if (kt < nt)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
              const uint32_t l4 = *reinterpret_cast<const uint32_t*>(lab + kt * 32 + 8 * gq + 4 * h);
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const int key = kt * 32 + 8 * gq + 4 * h + j;
                float v = fmaf(S[qt][kt][4 * gq + j], scale, brow[key]);
                if (((l4 >> (8 * j)) & 0xffu) != lq) v += kMasked;
                S[qt][kt][4 * gq + j] = v;
                if (key < N) m = fmaxf(m, v);
              }
            }
        m = fmaxf(m, xlane_xor<32>(m));
        float l = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
          if (kt < nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const float p = kt * 32 + arow(i, h) < N ? __builtin_amdgcn_exp2f((S[qt][kt][i] - m) * kLog2e) : 0.f;
              S[qt][kt][i] = p;
              l += p;
            }
        l += xlane_xor<32>(l);
        const bool qv = q < N;
        if (qv && h == 0) lse[((int64_t)win * g.heads + hd) * N + q] = m + __logf(l);
        f32x16 O = zero16();
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
          if (kt < nt)
#pragma unroll
            for (int s = 0; s < 2; ++s) O = mfma(tr_frag(Vt, kLdI, r, kt * 32, s, h), acc_frag(S[qt][kt], s), O);
        if (qv) store_t32(ob + (int64_t)qrow[qt] * C, O, 1.0f / l, h);
      }
  }
}

__global__ void __launch_bounds__(64) winattn_bwd_kernel(const uint16_t* __restrict__ qkv,
                                                          const uint16_t* __restrict__ out,
                                                          const float* __restrict__ lse,
                                                          const uint16_t* __restrict__ dout,
                                                          const float* __restrict__ bias, uint16_t* __restrict__ dqkv,
                                                          float* __restrict__ dbias_part, WinGeom g, int nparts,
                                                          float scale, int64_t rows_total) {
  __shared__ float Bs[kTok * kLdB];
  __shared__ __attribute__((aligned(16))) uint16_t Qt[kImg], dOt[kImg], Kt[kImg];
  __shared__ __attribute__((aligned(16))) uint16_t dSq[kTok * kLdI];  // bf16 dS [query][key]
  __shared__ __attribute__((aligned(16))) float Ls[kTok], Dl[kTok];   // lse (tokens >= N: huge, p = 0), rowsum(dO . O)
  __shared__ int rowi[kTok];
  __shared__ __attribute__((aligned(4))) uint8_t lab[kTok];
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int part = blockIdx.x, hd = blockIdx.y;
  const int N = g.N, nt = (N + 31) >> 5, C = g.heads * kHd;
  const int64_t ld = 3 * (int64_t)C;
  const uint16_t* qb = qkv + hd * kHd;
  const uint16_t* kb = qb + C;
  const uint16_t* vb = qb + 2 * C;
  const uint16_t* ob = out + hd * kHd;
  const uint16_t* dob = dout + hd * kHd;
  uint16_t* dqb = dqkv + hd * kHd;
  fill_bias(Bs, bias + (int64_t)hd * N * N, N, lane);
  if (part == 0) {
#pragma unroll
    for (int p3 = 0; p3 < 3; ++p3) zero_tail32(dqb + p3 * C, ld, (int64_t)g.B * g.H * g.W, rows_total, lane);
  }
  f32x16 dB[2][2] = {{zero16(), zero16()}, {zero16(), zero16()}};
  const int total = g.B * g.nwin;
  for (int win = part; win < total; win += nparts) {
    __syncthreads();  // the previous window's LDS reads are done
    {
      int row = -1, label = 0;
      if (lane < N) token_of(g, win, lane, row, label);
      rowi[lane] = row;
      lab[lane] = (uint8_t)label;
      uint4 a[4], o[4];
      load_full32(qb, ld, row, a);
      put_transposed(Qt, a, lane);
      load_full32(kb, ld, row, a);
      put_transposed(Kt, a, lane);
      load_full32(dob, C, row, a);
      put_transposed(dOt, a, lane);
      load_full32(ob, C, row, o);
      float dsum = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t ow[4] = {o[c].x, o[c].y, o[c].z, o[c].w}, gw[4] = {a[c].x, a[c].y, a[c].z, a[c].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          dsum = fmaf(__uint_as_float(ow[j] << 16), __uint_as_float(gw[j] << 16), dsum);
          dsum = fmaf(__uint_as_float(ow[j] & 0xffff0000u), __uint_as_float(gw[j] & 0xffff0000u), dsum);
        }
      }
      Dl[lane] = dsum;
      Ls[lane] = lane < N ? lse[((int64_t)win * g.heads + hd) * N + lane] : 1.0e30f;
    }
    __syncthreads();
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
      if (kt < nt) {  // ---- dK, dV of keys 32 kt .. 32 kt + 31 (key on the lane)
        const int key = kt * 32 + r, krow = rowi[key];
        const bool kv = key < N;
        const uint32_t lk = lab[key];
        uint4 kf[2], vf[2];
        load_row32(kb, ld, krow, h, kf);
        load_row32(vb, ld, krow, h, vf);
        f32x16 dVt = zero16(), dKt = zero16();
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
          if (qt < nt) {
            const int qrow = rowi[qt * 32 + r];
            uint4 qa[2], da[2];
            load_row32(qb, ld, qrow, h, qa);
            load_row32(dob, C, qrow, h, da);
            f32x16 S = zero16(), dP = zero16();
#pragma unroll
            for (int s = 0; s < 2; ++s) S = mfma(qa[s], kf[s], S);
#pragma unroll
            for (int s = 0; s < 2; ++s) dP = mfma(da[s], vf[s], dP);
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
              const int q0 = qt * 32 + 8 * gq + 4 * h;
              const float4 l4 = *reinterpret_cast<const float4*>(Ls + q0);
              const float4 d4 = *reinterpret_cast<const float4*>(Dl + q0);
              const uint32_t m4 = *reinterpret_cast<const uint32_t*>(lab + q0);
              const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, dq[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                float v = fmaf(S[4 * gq + j], scale, Bs[(q0 + j) * kLdB + key]);
                if (((m4 >> (8 * j)) & 0xffu) != lk) v += kMasked;
                const float p = kv ? __builtin_amdgcn_exp2f((v - lq[j]) * kLog2e) : 0.f;
                const float t = p * (dP[4 * gq + j] - dq[j]);
                dB[qt][kt][4 * gq + j] += t;
                S[4 * gq + j] = p;
                dP[4 * gq + j] = t * scale;
                dSq[(q0 + j) * kLdI + key] = f2bf(t * scale);
              }
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
              dVt = mfma(tr_frag(dOt, kLdI, r, qt * 32, s, h), acc_frag(S, s), dVt);
              dKt = mfma(tr_frag(Qt, kLdI, r, qt * 32, s, h), acc_frag(dP, s), dKt);
            }
          }
        if (kv) {
          store_t32(dqb + (int64_t)krow * ld + C, dKt, 1.0f, h);
          store_t32(dqb + (int64_t)krow * ld + 2 * C, dVt, 1.0f, h);
        }
      }
    __syncthreads();  // dSq is complete
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
      if (qt < nt) {  // ---- dQ of queries 32 qt .. 32 qt + 31 (query on the lane)
        const int q = qt * 32 + r;
        f32x16 dQt = zero16();
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
          if (kt < nt)
#pragma unroll
            for (int s = 0; s < 2; ++s)
              dQt = mfma(tr_frag(Kt, kLdI, r, kt * 32, s, h), tr_frag(dSq, kLdI, q, kt * 32, s, h), dQt);
        if (q < N) store_t32(dqb + (int64_t)rowi[q] * ld, dQt, 1.0f, h);
      }
  }
  float* dp = dbias_part + ((int64_t)part * g.heads + hd) * N * N;
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
      if (qt < nt && kt < nt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int q = qt * 32 + arow(i, h), key = kt * 32 + r;
          if (q < N && key < N) dp[q * N + key] = dB[qt][kt][i];
        }
}

__global__ void __launch_bounds__(256) bias_expand_kernel(const float* __restrict__ table, float* __restrict__ dense,
                                                           int w, int heads) {
  const int N = w * w, idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= heads * N * N) return;
  const int j = idx % N, i = (idx / N) % N, hd = idx / (N * N);
  const int e = (i / w - j / w + w - 1) * (2 * w - 1) + (i % w - j % w + w - 1);
  dense[idx] = table[e * heads + hd];
}

// one wave per (table entry, head): lane = one (i, j) pair of the entry, summed over the parts in part order; the
// pairs are then folded in lane order by lane 0
__global__ void __launch_bounds__(64) bias_grad_kernel(const float* __restrict__ part, float* __restrict__ dtable,
                                                        int nparts, int w, int heads, int accumulate) {
  __shared__ float red[64];
  const int lane = threadIdx.x, e = blockIdx.x, hd = blockIdx.y, N = w * w;
  const int dy = e / (2 * w - 1) - (w - 1), dx = e % (2 * w - 1) - (w - 1);
  const int ny = w - (dy < 0 ? -dy : dy), nx = w - (dx < 0 ? -dx : dx);
  float acc = 0.f;
  if (lane < ny * nx) {
    const int yj = (dy < 0 ? -dy : 0) + lane / nx, xj = (dx < 0 ? -dx : 0) + lane % nx;
    const int i = (yj + dy) * w + xj + dx, j = yj * w + xj;
    const float* p = part + ((int64_t)hd * N + i) * N + j;
    const int64_t stride = (int64_t)heads * N * N;
    for (int k = 0; k < nparts; ++k) acc += p[k * stride];
  }
  red[lane] = acc;
  __syncthreads();
  if (lane == 0) {
    float t = 0.f;
    for (int k = 0; k < ny * nx; ++k) t += red[k];
    dtable[e * heads + hd] = accumulate ? dtable[e * heads + hd] + t : t;
  }
}

// 16-byte chunks; cpr chunks per C-wide row.  inverse = 0: y[o][q*C + c] = x[pixel(o, q)][c]; inverse = 1: the
// reverse copy.  Rows [nreal, rows_total) of the written matrix are zeros.
__global__ void __launch_bounds__(256) patch_merge_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, int H,
                                                           int W, int cpr, int64_t nchunks, int64_t nreal_chunks,
                                                           int inverse) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nchunks) return;
  if (idx >= nreal_chunks) {
    dst[idx] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const int H2 = H >> 1, W2 = W >> 1;
  int64_t o, in;
  int c;
  if (!inverse) {  // idx runs over the merged matrix
    o = idx / (4 * cpr);
    c = (int)(idx - o * 4 * cpr);
  } else {  // idx runs over the pixel matrix
    in = idx / cpr;
    const int cc = (int)(idx - in * cpr);
    const int x = (int)(in % W), y = (int)((in / W) % H);
    const int64_t b = in / ((int64_t)W * H);
    o = (b * H2 + (y >> 1)) * W2 + (x >> 1);
    c = ((y & 1) + 2 * (x & 1)) * cpr + cc;
  }
  if (!inverse) {
    const int q = c / cpr, cc = c - q * cpr;
    const int x2 = (int)(o % W2), y2 = (int)((o / W2) % H2);
    const int64_t b = o / ((int64_t)W2 * H2);
    in = ((b * H + 2 * y2 + (q & 1)) * W + 2 * x2 + (q >> 1));
    dst[idx] = src[in * cpr + cc];
  } else {
    dst[idx] = src[o * 4 * cpr + c];
  }
}

// out = x + s[r / rows_per_img] * t (ADD) over f32 rows; rows of images >= B (the tail) and dropped samples copy x
__global__ void __launch_bounds__(256) rowscale_add_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                            const float* __restrict__ s, float* __restrict__ out,
                                                            int64_t n4, int c4, int64_t rows_per_img, int B) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n4) return;
  const int64_t img = (idx / c4) / rows_per_img;
  const float sc = img < B ? s[img] : 0.f;
  float4 v = reinterpret_cast<const float4*>(x)[idx];
  if (sc != 0.f) {
    const float4 u = reinterpret_cast<const float4*>(t)[idx];
    v = make_float4(fmaf(sc, u.x, v.x), fmaf(sc, u.y, v.y), fmaf(sc, u.z, v.z), fmaf(sc, u.w, v.w));
  }
  reinterpret_cast<float4*>(out)[idx] = v;
}

__global__ void __launch_bounds__(256) rowscale_cast_kernel(const float* __restrict__ d, const float* __restrict__ s,
                                                             uint16_t* __restrict__ out, int64_t n4, int c4,
                                                             int64_t rows_per_img, int B) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n4) return;
  const int64_t img = (idx / c4) / rows_per_img;
  const float sc = img < B ? s[img] : 0.f;
  uint2 o = make_uint2(0u, 0u);
  if (sc != 0.f) {
    const float4 v = reinterpret_cast<const float4*>(d)[idx];
    o = make_uint2(pack2bf(sc * v.x, sc * v.y), pack2bf(sc * v.z, sc * v.w));
  }
  reinterpret_cast<uint2*>(out)[idx] = o;
}

int win_nparts(int64_t windows, int heads) {
  int64_t p = kWaveTarget / (heads > 0 ? heads : 1);
  if (p < 1) p = 1;
  if (p > windows) p = windows;
  return (int)(p < 1 ? 1 : p);
}

// argument checks shared by the two passes; SV_OK, or the status already reported through set_error
int check_win(const char* who, int B, int H, int W, int w, int shift, int heads, int head_dim, float scale,
              int64_t rows_total, WinGeom* g) {
  if (B <= 0 || H <= 0 || W <= 0 || heads <= 0)
    return set_error(SV_ERR_INVALID_ARG, "%s: need B, H, W, heads > 0 (B %d, H %d, W %d, heads %d)", who, B, H, W, heads);
  if (w < 1 || shift < 0 || shift >= w)
    return set_error(SV_ERR_INVALID_ARG, "%s: need w >= 1 and 0 <= shift < w (w %d, shift %d)", who, w, shift);
  if (head_dim != kHd) return set_error(SV_ERR_UNSUPPORTED, "%s: head dimension %d (only 32 is built)", who, head_dim);
  if (w > kMaxW) return set_error(SV_ERR_UNSUPPORTED, "%s: window %d (at most %d)", who, w, kMaxW);
  if (H % w || W % w)
    return set_error(SV_ERR_INVALID_ARG, "%s: H and W must be multiples of the window (H %d, W %d, w %d)", who, H, W, w);
  if (!(scale > 0.f) || !(scale < 1e30f)) return set_error(SV_ERR_INVALID_ARG, "%s: scale must be positive and finite", who);
  const int64_t real = (int64_t)B * H * W;
  if (rows_total < real)
    return set_error(SV_ERR_INVALID_ARG, "%s: rows_total %lld < B * H * W = %lld", who, (long long)rows_total, (long long)real);
  if (rows_total >= (1ll << 31) || heads > 65535)
    return set_error(SV_ERR_UNSUPPORTED, "%s: rows_total below 2^31 and heads at most 65535", who);
  *g = WinGeom{B, H, W, w, shift, heads, W / w, (H / w) * (W / w), w * w};
  return SV_OK;
}

int check_rowscale(const char* who, int64_t rows, int64_t rows_per_img, int B, int C) {
  if (rows <= 0 || rows_per_img <= 0 || B <= 0 || C <= 0 || C % 4)
    return set_error(SV_ERR_INVALID_ARG, "%s: need rows, rows_per_img, B > 0 and C a positive multiple of 4", who);
  return SV_OK;
}

}  // namespace
}  // namespace sv

using namespace sv;

extern "C" {

int sv_winattn_bwd_nparts(int32_t B, int32_t H, int32_t W, int32_t w, int32_t heads) {
  if (B <= 0 || H <= 0 || W <= 0 || w <= 0 || heads <= 0) return 1;
  return win_nparts((int64_t)B * (H / w) * (W / w), heads);
}

int sv_winattn_fwd(const uint16_t* qkv, uint16_t* out, float* lse, const float* bias, int32_t B, int32_t H, int32_t W,
                   int32_t w, int32_t shift, int32_t heads, int32_t head_dim, float scale, int64_t rows_total,
                   sv_stream_t stream) {
  SV_REQUIRE(qkv && out && lse && bias, "sv_winattn_fwd: null pointer");
  WinGeom g;
  if (const int rc = check_win("sv_winattn_fwd", B, H, W, w, shift, heads, head_dim, scale, rows_total, &g)) return rc;
  SV_REQUIRE(al16(qkv) && al16(out) && ((uintptr_t)lse & 3) == 0 && ((uintptr_t)bias & 3) == 0,
             "sv_winattn_fwd: qkv / out must be 16-byte aligned");
  const int np = win_nparts((int64_t)B * g.nwin, heads);
  winattn_fwd_kernel<<<dim3(np, heads), 64, 0, (hipStream_t)stream>>>(qkv, out, lse, bias, g, np, scale, rows_total);
  return check_launch("sv_winattn_fwd");
}

int sv_winattn_bwd(const uint16_t* qkv, const uint16_t* out, const float* lse, const uint16_t* dout, const float* bias,
                   uint16_t* dqkv, float* dbias_part, int32_t B, int32_t H, int32_t W, int32_t w, int32_t shift,
                   int32_t heads, int32_t head_dim, float scale, int64_t rows_total, sv_stream_t stream) {
  SV_REQUIRE(qkv && out && lse && dout && bias && dqkv && dbias_part, "sv_winattn_bwd: null pointer");
  WinGeom g;
  if (const int rc = check_win("sv_winattn_bwd", B, H, W, w, shift, heads, head_dim, scale, rows_total, &g)) return rc;
  SV_REQUIRE(al16(qkv) && al16(out) && al16(dout) && al16(dqkv) && ((uintptr_t)lse & 3) == 0 &&
                 ((uintptr_t)bias & 3) == 0 && ((uintptr_t)dbias_part & 3) == 0,
             "sv_winattn_bwd: qkv / out / dout / dqkv must be 16-byte aligned");
  const int np = win_nparts((int64_t)B * g.nwin, heads);
  winattn_bwd_kernel<<<dim3(np, heads), 64, 0, (hipStream_t)stream>>>(qkv, out, lse, dout, bias, dqkv, dbias_part, g, np,
                                                                     scale, rows_total);
  return check_launch("sv_winattn_bwd");
}

int sv_swin_bias_expand(const float* table, float* dense, int32_t w, int32_t heads, sv_stream_t stream) {
  SV_REQUIRE(table && dense, "sv_swin_bias_expand: null pointer");
  SV_REQUIRE(w >= 1 && w <= kMaxW && heads > 0 && heads <= 65535, "sv_swin_bias_expand: need 1 <= w <= 8, heads > 0");
  const int n = heads * w * w * w * w;
  bias_expand_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(table, dense, w, heads);
  return check_launch("sv_swin_bias_expand");
}

int sv_swin_bias_grad(const float* dbias_part, float* dtable, int32_t nparts, int32_t w, int32_t heads,
                      int32_t accumulate, sv_stream_t stream) {
  SV_REQUIRE(dbias_part && dtable, "sv_swin_bias_grad: null pointer");
  SV_REQUIRE(w >= 1 && w <= kMaxW && heads > 0 && heads <= 65535 && nparts > 0,
             "sv_swin_bias_grad: need 1 <= w <= 8, heads > 0, nparts > 0");
  bias_grad_kernel<<<dim3((2 * w - 1) * (2 * w - 1), heads), 64, 0, (hipStream_t)stream>>>(dbias_part, dtable, nparts, w,
                                                                                        heads, accumulate);
  return check_launch("sv_swin_bias_grad");
}

static int patch_merge_launch(const char* who, const void* src, void* dst, int32_t dtype, int32_t B, int32_t H,
                              int32_t W, int32_t C, int64_t rows_total, int inverse, sv_stream_t stream) {
  SV_REQUIRE(src && dst, "%s: null pointer", who);
  SV_REQUIRE(dtype == SV_F32 || dtype == SV_BF16, "%s: dtype must be SV_F32 or SV_BF16", who);
  SV_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0, "%s: need B, C > 0 and even H, W > 0", who);
  const int es = dtype == SV_F32 ? 4 : 2;
  SV_REQUIRE(((int64_t)C * es) % 16 == 0 && al16(src) && al16(dst), "%s: rows must be 16-byte multiples, 16-byte aligned", who);
  const int cpr = C * es / 16;
  const int64_t real_rows = inverse ? (int64_t)B * H * W : (int64_t)B * (H / 2) * (W / 2);
  SV_REQUIRE(rows_total >= real_rows, "%s: rows_total %lld below the %lld rows written", who, (long long)rows_total,
             (long long)real_rows);
  const int64_t per_row = inverse ? cpr : 4 * (int64_t)cpr;
  const int64_t nchunks = rows_total * per_row, nreal = real_rows * per_row;
  SV_REQUIRE((nchunks + 255) / 256 < (1ll << 31), "%s: too large", who);
  patch_merge_kernel<<<(unsigned)((nchunks + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      static_cast<const uint4*>(src), static_cast<uint4*>(dst), H, W, cpr, nchunks, nreal, inverse);
  return check_launch(who);
}

int sv_patch_merge(const void* x, void* y, int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C,
                   int64_t rows_out_total, sv_stream_t stream) {
  return patch_merge_launch("sv_patch_merge", x, y, dtype, B, H, W, C, rows_out_total, 0, stream);
}

int sv_patch_merge_bwd(const void* dy, void* dx, int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C,
                       int64_t rows_in_total, sv_stream_t stream) {
  return patch_merge_launch("sv_patch_merge_bwd", dy, dx, dtype, B, H, W, C, rows_in_total, 1, stream);
}

int sv_rowscale_add(const float* x, const float* t, const float* s, float* out, int64_t rows, int64_t rows_per_img,
                    int32_t B, int32_t C, sv_stream_t stream) {
  SV_REQUIRE(x && t && s && out, "sv_rowscale_add: null pointer");
  if (const int rc = check_rowscale("sv_rowscale_add", rows, rows_per_img, B, C)) return rc;
  SV_REQUIRE(al16(x) && al16(t) && al16(out), "sv_rowscale_add: x / t / out must be 16-byte aligned");
  const int64_t n4 = rows * (C / 4);
  rowscale_add_kernel<<<(unsigned)((n4 + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, t, s, out, n4, C / 4,
                                                                                     rows_per_img, B);
  return check_launch("sv_rowscale_add");
}

int sv_rowscale_cast_bf16(const float* d, const float* s, uint16_t* out, int64_t rows, int64_t rows_per_img, int32_t B,
                          int32_t C, sv_stream_t stream) {
  SV_REQUIRE(d && s && out, "sv_rowscale_cast_bf16: null pointer");
  if (const int rc = check_rowscale("sv_rowscale_cast_bf16", rows, rows_per_img, B, C)) return rc;
  SV_REQUIRE(al16(d) && ((uintptr_t)out & 7) == 0, "sv_rowscale_cast_bf16: d 16-byte, out 8-byte aligned");
  const int64_t n4 = rows * (C / 4);
  rowscale_cast_kernel<<<(unsigned)((n4 + 255) / 256), 256, 0, (hipStream_t)stream>>>(d, s, out, n4, C / 4, rows_per_img,
                                                                                      B);
  return check_launch("sv_rowscale_cast_bf16");
}

}  // extern "C"
