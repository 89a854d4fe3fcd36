// Grouped 3x3 convolution (pad 1, stride 1 or 2, C_in = C_out = C, Cg = C / groups in {4, 8, 16, 32}) over NHWC bf16
// activations with f32 accumulation on v_mfma_f32_16x16x32_bf16: the conv2 of a ResNeXt bottleneck (timm resnet.py
// Bottleneck with cardinality 32), forward, backward-data and backward-weight.
//
// The operator is HBM-bound (1.2 GFLOP against 8 .. 67 MB per ResNeXt-50 stage at 256 px, batch 32), so every kernel
// here is shaped by its bytes: all global accesses are one 16-byte NHWC access per lane (8 consecutive channels of
// one pixel), nothing is transposed in memory and nothing goes through LDS except the weight gradient's in-workgroup
// sum.
//
// Forward / backward-data (one kernel, MODE 0 / 1).  The GEMM unit is a block of 32 consecutive channels: it holds
// 32 / Cg whole groups, so its 32 outputs read exactly its own 32 inputs, and per tap the weight is one 32 x 32 matrix
// that is block-diagonal inside (the pack kernel writes the zeros).  A wave owns one channel block and tiles of 16
// output pixels.  Per tap one MFMA K step: A = the weight matrix (rows = output channels, k = input channels), B = the
// tap's 16 pixels x 32 input channels, which is the lane's 16-byte load as it stands (B[k = 8 (l >> 4) + j][col = l & 15]
// = pixel l & 15, channels 8 (l >> 4) .. + 7).  Two accumulators cover the 32 output channels; the pack kernel orders
// the rows so that accumulator i's row 4 q + r is output channel 8 q + 4 i + r: lane (q, pixel) then holds the 8
// consecutive output channels 8 q .. 8 q + 7 of its pixel and stores them as 16 bytes.  Taps outside the image (and, in
// the strided backward-data, taps whose source parity does not match) load from offset 0 and are replaced by zeros:
// no divergent branch, no out-of-range address.  The 18 weight fragments of the block stay in registers over the
// wave's tiles.  The matrix cores do 32 / Cg x the algorithmic FLOPs (8 x at Cg = 4: ~10 GFLOP, a few microseconds).
// Backward-data is the same kernel over dy with a second packed form: taps flipped, each block transposed.
// Stride 1 on images at least 16 pixels wide takes a second form of the same kernel (gconv_s1_kernel): a wave walks
// down kRows rows of a 16-pixel-wide strip and keeps the loaded input rows in registers, 3 loads per output row
// instead of 9 (measured at layer1: 50 -> 30 us).
//
// Backward-weight.  dW[co][ci][tap] = sum_p dy[p][co] x[p * stride + tap - 1][ci], K over pixels: both MFMA operands
// want 8 consecutive PIXELS of one channel per lane, the transpose of what NHWC gives.  The transpose is done by the
// matrix core itself: a 16-pixel x 32-channel tile, loaded as above, times a 32 x 16 selection matrix (ones on one
// diagonal) is that tile's 16 x 16 half with the pixel on the register index and the channel on the lane -- exact,
// since every product is a bf16 value times 1 or 0.  Two such tiles give a lane its 8 K values; the K order inside a
// 32-pixel chunk is therefore (tile, row) interleaved, the same for dy and x, which a sum over K does not see.  (A
// non-finite activation would spread over its tile through 0 x inf; the step is lost in that case either way.)
// A workgroup's 4 waves take the chunks of one partial range round-robin, sum their accumulators through LDS in wave
// order and write one partial in fragment order; the fold kernel sums the partials in order and picks the in-group
// entries into the torch [C][Cg][3][3] gradient.  No float atomics: bitwise reproducible.
#include "common.h"

namespace sv {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kCB = 32;                        // channels per GEMM unit
constexpr int kFragsPerBlock = 9 * 2;          // (tap, accumulator) A fragments of one channel block
constexpr int kPackPerBlock = kFragsPerBlock * 64 * 8;  // bf16 elements of one packed channel block (one form)

__host__ __device__ inline bool gconv_supported(const sv_gconv_shape& s) {
  if (s.B <= 0 || s.H <= 0 || s.W <= 0 || s.C <= 0 || s.groups <= 0) return false;
  if (s.KH != 3 || s.KW != 3 || s.pad != 1 || (s.stride != 1 && s.stride != 2)) return false;
  if (s.C % kCB != 0 || s.C % s.groups != 0) return false;
  const int cg = s.C / s.groups;
  return cg == 4 || cg == 8 || cg == 16 || cg == 32;
}
inline int out_dim(int n, int stride) { return (n + 2 - 3) / stride + 1; }

// ---- weight pack ---------------------------------------------------------------------------------------------
struct GPackSegs {
  sv_gconv_pack_seg s[SV_MAX_GPACK_SEGS];
  int64_t first_block[SV_MAX_GPACK_SEGS + 1];
  int n;
};

// element e of a packed form: [C/32][9 taps][2 accumulators][64 lanes][8]
__global__ void __launch_bounds__(256) gconv_pack_kernel(const GPackSegs segs) {
  int k = 0;
  while (k + 1 < segs.n && (int64_t)blockIdx.x >= segs.first_block[k + 1]) ++k;  // block-uniform
  const sv_gconv_pack_seg& g = segs.s[k];
  const int64_t per_form = (int64_t)(g.C / kCB) * kPackPerBlock;
  const int64_t i = ((int64_t)blockIdx.x - segs.first_block[k]) * 256 + threadIdx.x;
  if (i >= 2 * per_form) return;
  const int form = i >= per_form;
  const int64_t e = i - (int64_t)form * per_form;
  const int j = (int)(e & 7), l = (int)((e >> 3) & 63), mi = (int)((e >> 9) & 1);
  const int t = (int)((e >> 10) % 9), cb = (int)(e / kPackPerBlock);
  const int m = l & 15, q = l >> 4;
  const int row = 8 * (m >> 2) + 4 * mi + (m & 3);  // the channel this accumulator row is stored as
  const int kk = 8 * q + j;                         // the channel this K slot reads
  const int cg = g.C / g.groups;
  const int co = form == 0 ? row : kk, ci = form == 0 ? kk : row, tap = form == 0 ? t : 8 - t;
  float v = 0.f;
  if (co / cg == ci / cg) v = g.w[((int64_t)(cb * kCB + co) * cg + (ci % cg)) * 9 + tap];
  (form == 0 ? g.wp_fwd : g.wp_bwd)[e] = f2bf(v);
}

// ---- forward / backward-data ---------------------------------------------------------------------------------
struct GArgs {
  const uint16_t* src;  // [B][Hs][Ws][C]
  const uint16_t* wp;   // packed form of the pass
  uint16_t* dst;        // [B][Hd][Wd][C]
  int Hs, Ws, Hd, Wd, C, stride;
  int64_t Md;           // B * Hd * Wd
  int ntiles;           // ceil(Md / 16)
};

template <int MODE>
__global__ void __launch_bounds__(256) gconv_kernel(const GArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, n = lane & 15;
  const int cb = blockIdx.y * 4 + wave;
  if (cb >= a.C / kCB) return;  // (no barrier in this kernel)
  const uint4* wv = reinterpret_cast<const uint4*>(a.wp) + (size_t)cb * (kFragsPerBlock * 64) + lane;
  bf16x8 wf[9][2];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 2; ++i) wf[t][i] = __builtin_bit_cast(bf16x8, wv[(t * 2 + i) * 64]);
  const int coff = cb * kCB + 8 * q;
  const int sh = a.stride - 1;  // stride 1 / 2 -> shift 0 / 1
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t p = (int64_t)tile * 16 + n;
    const bool pv = p < a.Md;
    const int64_t pc = pv ? p : 0;
    const int x = (int)(pc % a.Wd), y = (int)((pc / a.Wd) % a.Hd);
    const int64_t b = pc / ((int64_t)a.Wd * a.Hd);
    uint4 xv[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int th = t / 3, tw = t % 3;
      int sy, sx;
      bool ok = pv;
      if (MODE == 0) {
        sy = (y << sh) - 1 + th, sx = (x << sh) - 1 + tw;
        ok = ok && sy >= 0 && sx >= 0;
      } else {
        const int ny = y - 1 + th, nx = x - 1 + tw;
        ok = ok && ny >= 0 && nx >= 0 && ((ny | nx) & sh) == 0;
        sy = ny >> sh, sx = nx >> sh;
      }
      ok = ok && sy < a.Hs && sx < a.Ws;
      const int64_t off = ok ? ((b * a.Hs + sy) * a.Ws + sx) * (int64_t)a.C + coff : 0;
      const uint4 v = *reinterpret_cast<const uint4*>(a.src + off);
      xv[t] = ok ? v : make_uint4(0u, 0u, 0u, 0u);
    }
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const bf16x8 bx = __builtin_bit_cast(bf16x8, xv[t]);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[t][0], bx, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[t][1], bx, acc1, 0, 0, 0);
    }
    // lane (q, pixel n): acc0[r] = channel 8 q + r, acc1[r] = channel 8 q + 4 + r of the block
    if (pv)
      *reinterpret_cast<uint4*>(a.dst + p * a.C + coff) =
          make_uint4(pack2bf(acc0[0], acc0[1]), pack2bf(acc0[2], acc0[3]), pack2bf(acc1[0], acc1[1]),
                     pack2bf(acc1[2], acc1[3]));
  }
}

// Stride 1 on images at least 16 pixels wide (forward and backward-data are the same computation there, only the
// packed form differs): a wave owns a strip of 16 consecutive x of one image and kRows output rows, walks down the
// rows and keeps the input rows it has loaded in registers -- an output row needs one new input row (3 loads, its
// x - 1 / x / x + 1 taps) instead of 9, and the next row's loads are in flight while this row's MFMAs run.  The
// generic kernel above reads every input row three times from different workgroups, i.e. through L2: 1.3 TB/s of
// algorithmic bytes at layer1 (C = 128, 64 x 64).
constexpr int kRows = 4;

struct Row3 {
  uint4 v[3];
};

__global__ void __launch_bounds__(256) gconv_s1_kernel(const GArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, n = lane & 15;
  const int cb = blockIdx.y * 4 + wave;
  if (cb >= a.C / kCB) return;  // (no barrier in this kernel)
  const int H = a.Hs, W = a.Ws;  // stride 1: source and destination grids are equal
  const int strips = (W + 15) / 16, nseg = (H + kRows - 1) / kRows;
  const int strip = blockIdx.x % strips, seg = (blockIdx.x / strips) % nseg;
  const int64_t b = blockIdx.x / (strips * nseg);
  const uint4* wv = reinterpret_cast<const uint4*>(a.wp) + (size_t)cb * (kFragsPerBlock * 64) + lane;
  bf16x8 wf[9][2];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 2; ++i) wf[t][i] = __builtin_bit_cast(bf16x8, wv[(t * 2 + i) * 64]);
  const int coff = cb * kCB + 8 * q;
  const int x = strip * 16 + n;
  const int y0 = seg * kRows, y1 = y0 + kRows < H ? y0 + kRows : H;
  // the three x taps of input row yy (zeros outside the image; an out-of-range tap loads offset 0)
  auto load_row = [&](int yy) {
    Row3 r;
#pragma unroll
    for (int tw = 0; tw < 3; ++tw) {
      const int sx = x - 1 + tw;
      const bool ok = yy >= 0 && yy < H && sx >= 0 && sx < W;
      const int64_t off = ok ? ((b * H + yy) * W + sx) * (int64_t)a.C + coff : 0;
      const uint4 v = *reinterpret_cast<const uint4*>(a.src + off);
      r.v[tw] = ok ? v : make_uint4(0u, 0u, 0u, 0u);
    }
    return r;
  };
  Row3 top = load_row(y0 - 1), mid = load_row(y0), bot = load_row(y0 + 1);
  for (int y = y0; y < y1; ++y) {
    const Row3 nxt = load_row(y + 2);  // (for the last row of the range: loaded, not used)
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const uint4 u = t < 3 ? top.v[t % 3] : t < 6 ? mid.v[t % 3] : bot.v[t % 3];
      const bf16x8 bx = __builtin_bit_cast(bf16x8, u);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[t][0], bx, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[t][1], bx, acc1, 0, 0, 0);
    }
    if (x < W)
      *reinterpret_cast<uint4*>(a.dst + ((b * H + y) * W + x) * (int64_t)a.C + coff) =
          make_uint4(pack2bf(acc0[0], acc0[1]), pack2bf(acc0[2], acc0[3]), pack2bf(acc1[0], acc1[1]),
                     pack2bf(acc1[2], acc1[3]));
    top = mid, mid = bot, bot = nxt;
  }
}

int launch_gconv(int mode, const void* src, const uint16_t* wp, void* dst, const sv_gconv_shape* s, hipStream_t st) {
  const int OH = out_dim(s->H, s->stride), OW = out_dim(s->W, s->stride);
  if (s->stride == 1 && s->W >= 16) {
    GArgs a{};
    a.src = (const uint16_t*)src, a.wp = wp, a.dst = (uint16_t*)dst;
    a.C = s->C, a.stride = 1, a.Hs = a.Hd = s->H, a.Ws = a.Wd = s->W;
    const int64_t gx = (int64_t)s->B * ((s->H + kRows - 1) / kRows) * ((s->W + 15) / 16);
    if (gx > 0x7fffffff) return set_error(SV_ERR_UNSUPPORTED, "sv_gconv: too many pixels");
    gconv_s1_kernel<<<dim3((unsigned)gx, (s->C / kCB + 3) / 4), 256, 0, st>>>(a);
    return SV_OK;
  }
  GArgs a{};
  a.src = (const uint16_t*)src, a.wp = wp, a.dst = (uint16_t*)dst;
  a.C = s->C, a.stride = s->stride;
  if (mode == 0) a.Hs = s->H, a.Ws = s->W, a.Hd = OH, a.Wd = OW;
  else a.Hs = OH, a.Ws = OW, a.Hd = s->H, a.Wd = s->W;
  a.Md = (int64_t)s->B * a.Hd * a.Wd;
  const int64_t tiles = (a.Md + 15) / 16;
  if (tiles > 0x7fffffff / 16) return set_error(SV_ERR_UNSUPPORTED, "sv_gconv: too many pixels");
  a.ntiles = (int)tiles;
  const int gy = (s->C / kCB + 3) / 4;
  // ~4 workgroups per CU in all; a wave keeps its 18 weight fragments over its tiles
  const int target = 4 * device_cus(st);
  int gx = (int)tiles;
  if (gx > (target + gy - 1) / gy) gx = (target + gy - 1) / gy;
  if (gx < 1) gx = 1;
  if (mode == 0) gconv_kernel<0><<<dim3(gx, gy), 256, 0, st>>>(a);
  else gconv_kernel<1><<<dim3(gx, gy), 256, 0, st>>>(a);
  return SV_OK;
}

// ---- backward-weight -----------------------------------------------------------------------------------------
struct WArgs {
  const uint16_t* dy;  // [B][OH][OW][C]
  const uint16_t* x;   // [B][H][W][C]
  float* part;         // [P][C/32][9 * NB * 4][64]
  int H, W, OH, OW, C, stride;
  int64_t M;           // B * OH * OW
  int nchunks;         // ceil(M / 32)
  int cpp;             // chunks per partial
};

inline int wgrad_nb(const sv_gconv_shape& s) { return s.C / s.groups == 32 ? 4 : 2; }
// chunks of 32 output pixels per partial: at least 16 (4 per wave), and at most ~256 workgroups in all
inline void wgrad_geometry(const sv_gconv_shape& s, int& nchunks, int& cpp, int& P) {
  const int64_t M = (int64_t)s.B * out_dim(s.H, s.stride) * out_dim(s.W, s.stride);
  nchunks = (int)((M + 31) / 32);
  int pmax = 256 / (s.C / kCB);
  if (pmax < 1) pmax = 1;
  cpp = (nchunks + pmax - 1) / pmax;
  if (cpp < 16) cpp = 16;
  P = (nchunks + cpp - 1) / cpp;
  if (P < 1) P = 1;
}

__device__ __forceinline__ bf16x8 pack_t(const f32x4& d0, const f32x4& d1) {
  const uint4 u = make_uint4(pack2bf(d0[0], d0[1]), pack2bf(d0[2], d0[3]), pack2bf(d1[0], d1[1]), pack2bf(d1[2], d1[3]));
  return __builtin_bit_cast(bf16x8, u);
}

template <int NB>
__global__ void __launch_bounds__(256) gconv_wgrad_kernel(const WArgs a) {
  constexpr int NACC = 9 * NB * 4;
  __shared__ float red[NACC * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, n = lane & 15;
  const int cb = blockIdx.y, part = blockIdx.x;
  const int coff = cb * kCB + 8 * q;
  const int sh = a.stride - 1;
  // selection matrices of the transposing MFMAs: sel[h] = B[k = 8 q + j][col n] = (k == 16 h + n)
  bf16x8 sel[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    uint32_t u[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const uint32_t lo = (8 * q + 2 * jj == 16 * h + n) ? 0x3f80u : 0u;
      const uint32_t hi = (8 * q + 2 * jj + 1 == 16 * h + n) ? 0x3f80u : 0u;
      u[jj] = lo | (hi << 16);
    }
    sel[h] = __builtin_bit_cast(bf16x8, make_uint4(u[0], u[1], u[2], u[3]));
  }
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[9][NB];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < NB; ++i) acc[t][i] = zero;
  const int c0 = part * a.cpp;
  const int c1 = c0 + a.cpp < a.nchunks ? c0 + a.cpp : a.nchunks;
  for (int c = c0 + wave; c < c1; c += 4) {
    bool pv[2];
    int oy[2], ox[2];
    int64_t bb[2];
    bf16x8 dyv[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t p = (int64_t)c * 32 + 16 * u + n;
      pv[u] = p < a.M;
      const int64_t pc = pv[u] ? p : 0;
      ox[u] = (int)(pc % a.OW), oy[u] = (int)((pc / a.OW) % a.OH);
      bb[u] = pc / ((int64_t)a.OW * a.OH);
      const uint4 v = *reinterpret_cast<const uint4*>(a.dy + pc * a.C + coff);
      dyv[u] = __builtin_bit_cast(bf16x8, pv[u] ? v : make_uint4(0u, 0u, 0u, 0u));
    }
    // dyT[h]: lane (q', col) = output channel 16 h + col, K slots j < 4: tile 0 pixel 4 q' + j, j >= 4: tile 1
    bf16x8 dyT[2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
      dyT[h] = pack_t(__builtin_amdgcn_mfma_f32_16x16x32_bf16(dyv[0], sel[h], zero, 0, 0, 0),
                      __builtin_amdgcn_mfma_f32_16x16x32_bf16(dyv[1], sel[h], zero, 0, 0, 0));
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int th = t / 3, tw = t % 3;
      bf16x8 xv[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int sy = (oy[u] << sh) - 1 + th, sx = (ox[u] << sh) - 1 + tw;
        const bool ok = pv[u] && sy >= 0 && sx >= 0 && sy < a.H && sx < a.W;
        const int64_t off = ok ? ((bb[u] * a.H + sy) * a.W + sx) * (int64_t)a.C + coff : 0;
        const uint4 v = *reinterpret_cast<const uint4*>(a.x + off);
        xv[u] = __builtin_bit_cast(bf16x8, ok ? v : make_uint4(0u, 0u, 0u, 0u));
      }
      bf16x8 xT[2];
#pragma unroll
      for (int h = 0; h < 2; ++h)
        xT[h] = pack_t(__builtin_amdgcn_mfma_f32_16x16x32_bf16(xv[0], sel[h], zero, 0, 0, 0),
                       __builtin_amdgcn_mfma_f32_16x16x32_bf16(xv[1], sel[h], zero, 0, 0, 0));
      // D[co][ci]: lane (q'', n) reg r = output channel 16 hco + 4 q'' + r, input channel 16 hci + n
      if (NB == 4) {
#pragma unroll
        for (int hco = 0; hco < 2; ++hco)
#pragma unroll
          for (int hci = 0; hci < 2; ++hci)
            acc[t][(hco * 2 + hci) % NB] =
                __builtin_amdgcn_mfma_f32_16x16x32_bf16(dyT[hco], xT[hci], acc[t][(hco * 2 + hci) % NB], 0, 0, 0);
      } else {
#pragma unroll
        for (int h = 0; h < 2; ++h)
          acc[t][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dyT[h], xT[h], acc[t][h], 0, 0, 0);
      }
    }
  }
  // sum the 4 waves' accumulators in wave order (each lane touches only its own slots)
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int idx = ((t * NB + i) * 4 + r) * 64 + lane;
            red[idx] = w == 0 ? acc[t][i][r] : red[idx] + acc[t][i][r];
          }
    }
    __syncthreads();
  }
  float* out = a.part + ((size_t)part * gridDim.y + cb) * (size_t)(NACC * 64);
  for (int i = threadIdx.x; i < NACC * 64; i += 256) out[i] = red[i];
}

// dw[co][cig][tap] (+)= sum_p part[p][...], partials in order; one thread per gradient element
__global__ void __launch_bounds__(256) gconv_wgrad_fold_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                               int C, int cg, int NB, int P, int accumulate) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)C * cg * 9) return;
  const int tap = (int)(idx % 9), cig = (int)((idx / 9) % cg), co = (int)(idx / (9 * cg));
  const int cb = co / kCB, col = co % kCB, cil = (col / cg) * cg + cig;
  const int blk = NB == 4 ? (col >> 4) * 2 + (cil >> 4) : (col >> 4);
  const int reg = (tap * NB + blk) * 4 + (col & 3);
  const int lane = 16 * ((col & 15) >> 2) + (cil & 15);
  const size_t per_block = (size_t)9 * NB * 4 * 64, per_part = per_block * (size_t)(C / kCB);
  const float* p = part + (size_t)cb * per_block + (size_t)reg * 64 + lane;
  float s = 0.f;
  for (int k = 0; k < P; ++k) s += p[(size_t)k * per_part];
  dw[idx] = accumulate ? dw[idx] + s : s;
}

int check_shape(const char* who, const sv_gconv_shape* s) {
  if (!s) return set_error(SV_ERR_INVALID_ARG, "%s: null shape", who);
  if (!gconv_supported(*s))
    return set_error(SV_ERR_UNSUPPORTED,
                     "%s: unsupported grouped conv B=%d H=%d W=%d C=%d groups=%d k=%dx%d stride=%d pad=%d (3x3, pad 1, "
                     "stride 1|2, C %% 32 == 0, C / groups in {4, 8, 16, 32})",
                     who, s->B, s->H, s->W, s->C, s->groups, s->KH, s->KW, s->stride, s->pad);
  return SV_OK;
}

}  // namespace
}  // namespace sv

using namespace sv;

extern "C" int sv_gconv_weight_pack(const sv_gconv_pack_seg* segs, int32_t nseg, sv_stream_t stream) {
  SV_REQUIRE(segs && nseg >= 1 && nseg <= SV_MAX_GPACK_SEGS, "sv_gconv_weight_pack: 1..%d segments", SV_MAX_GPACK_SEGS);
  GPackSegs a{};
  a.n = nseg;
  int64_t blocks = 0;
  for (int k = 0; k < nseg; ++k) {
    const sv_gconv_pack_seg& g = segs[k];
    SV_REQUIRE(g.w && g.wp_fwd && g.wp_bwd, "sv_gconv_weight_pack: null pointer in segment %d", k);
    SV_REQUIRE((((uintptr_t)g.wp_fwd | (uintptr_t)g.wp_bwd) & 15) == 0, "sv_gconv_weight_pack: misaligned segment %d", k);
    sv_gconv_shape s{1, 3, 3, g.C, g.groups, 3, 3, 1, 1};
    if (int rc = check_shape("sv_gconv_weight_pack", &s)) return rc;
    a.s[k] = g;
    a.first_block[k] = blocks;
    blocks += (2 * (int64_t)(g.C / kCB) * kPackPerBlock + 255) / 256;
  }
  a.first_block[nseg] = blocks;
  gconv_pack_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(a);
  return check_launch("sv_gconv_weight_pack");
}

extern "C" int sv_gconv_fwd(const void* x, const uint16_t* wp_fwd, void* y, const sv_gconv_shape* s, sv_stream_t stream) {
  if (int rc = check_shape("sv_gconv_fwd", s)) return rc;
  SV_REQUIRE(x && wp_fwd && y, "sv_gconv_fwd: null pointer");
  SV_REQUIRE((((uintptr_t)x | (uintptr_t)wp_fwd | (uintptr_t)y) & 15) == 0, "sv_gconv_fwd: pointers must be 16-byte aligned");
  if (int rc = launch_gconv(0, x, wp_fwd, y, s, (hipStream_t)stream)) return rc;
  return check_launch("sv_gconv_fwd");
}

extern "C" int sv_gconv_bwd_data(const void* dy, const uint16_t* wp_bwd, void* dx, const sv_gconv_shape* s,
                                 sv_stream_t stream) {
  if (int rc = check_shape("sv_gconv_bwd_data", s)) return rc;
  SV_REQUIRE(dy && wp_bwd && dx, "sv_gconv_bwd_data: null pointer");
  SV_REQUIRE((((uintptr_t)dy | (uintptr_t)wp_bwd | (uintptr_t)dx) & 15) == 0,
             "sv_gconv_bwd_data: pointers must be 16-byte aligned");
  if (int rc = launch_gconv(1, dy, wp_bwd, dx, s, (hipStream_t)stream)) return rc;
  return check_launch("sv_gconv_bwd_data");
}

extern "C" int sv_gconv_bwd_weight_nparts(const sv_gconv_shape* s) {
  if (!s || !gconv_supported(*s)) return 0;
  int nchunks, cpp, P;
  wgrad_geometry(*s, nchunks, cpp, P);
  return P;
}

extern "C" int64_t sv_gconv_bwd_weight_work_floats(const sv_gconv_shape* s) {
  if (!s || !gconv_supported(*s)) return 0;
  return (int64_t)sv_gconv_bwd_weight_nparts(s) * (s->C / kCB) * 9 * wgrad_nb(*s) * 4 * 64;
}

extern "C" int sv_gconv_bwd_weight(const void* dy, const void* x, float* work, float* dw, int32_t accumulate,
                                   const sv_gconv_shape* s, sv_stream_t stream) {
  if (int rc = check_shape("sv_gconv_bwd_weight", s)) return rc;
  SV_REQUIRE(dy && x && work && dw, "sv_gconv_bwd_weight: null pointer");
  SV_REQUIRE((((uintptr_t)dy | (uintptr_t)x | (uintptr_t)work) & 15) == 0,
             "sv_gconv_bwd_weight: dy, x and work must be 16-byte aligned");
  WArgs a{};
  a.dy = (const uint16_t*)dy, a.x = (const uint16_t*)x, a.part = work;
  a.H = s->H, a.W = s->W, a.OH = out_dim(s->H, s->stride), a.OW = out_dim(s->W, s->stride);
  a.C = s->C, a.stride = s->stride;
  a.M = (int64_t)s->B * a.OH * a.OW;
  SV_REQUIRE(a.M <= 0x7fffffff / 32 * 32LL, "sv_gconv_bwd_weight: too many pixels");
  int P;
  wgrad_geometry(*s, a.nchunks, a.cpp, P);
  const int NB = wgrad_nb(*s), cg = s->C / s->groups;
  const dim3 grid(P, s->C / kCB);
  if (NB == 4) gconv_wgrad_kernel<4><<<grid, 256, 0, (hipStream_t)stream>>>(a);
  else gconv_wgrad_kernel<2><<<grid, 256, 0, (hipStream_t)stream>>>(a);
  if (int rc = check_launch("sv_gconv_bwd_weight")) return rc;
  const int64_t n = (int64_t)s->C * cg * 9;
  gconv_wgrad_fold_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(work, dw, s->C, cg, NB, P,
                                                                                       accumulate);
  return check_launch("sv_gconv_bwd_weight (fold)");
}
