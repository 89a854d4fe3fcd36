// ViT / DeiT-III patch embedding operand and token assembly.
//
// timm's PatchEmbed is Conv2d(3, C, 16, stride 16): a GEMM over non-overlapping 16x16 patches,
//   z[p][c] = b[c] + sum_k patch[p][k] * w[c][k],  k = ci * 256 + ky * 16 + kx  (= proj.weight [C,3,16,16] flattened),
// so proj.weight.view(C, 768) (and its bf16 shadow) is the GEMM's B operand as stored.  sv_patchify16 writes the
// patch rows, 768 wide, patches in row-major order per image; image b's patch p goes to row
// b * rows_per_img + row0 + p (rows_per_img = patches per image, row0 = 0: the plain [B * P, 768] matrix; the ViT
// module places them inside its padded token rows).  Rows it does not own are left untouched.
//
// Input kinds (the reference's host transforms, applied in flight with the same f32 operations as torchvision,
// (u / 255 - mean[c]) / std[c]):
//   SV_IMG_F32_NCHW  [B,3,H,W] f32, already normalised;
//   SV_IMG_U8_GRAY   [B,H,W] uint8 (localization): gray -> RGB replication, ToTensor, Normalize;
//   SV_IMG_U8_HWC    [B,H,W,3] uint8 (classification): ToTensor, Normalize.
// A thread owns 8 consecutive k (one channel, one patch row, 8 pixels): one 16-byte (bf16) or two (f32) stores.
#include "common.h"

namespace sv {
namespace {

constexpr int kThreads = 256;

template <int KIND, typename TO>
__global__ void __launch_bounds__(kThreads) patchify16_kernel(const void* __restrict__ img, float m0, float m1, float m2,
                                                               float s0, float s1, float s2, TO* __restrict__ patches,
                                                               int B, int H, int W, int64_t rows_per_img, int row0) {
  const int Hp = H >> 4, Wp = W >> 4;
  const int64_t total = (int64_t)B * Hp * Wp * 96;  // 768 / 8 chunks per patch
  for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads) {
    const int chunk = (int)(t % 96);
    const int64_t p = t / 96;
    const int px = (int)(p % Wp), py = (int)((p / Wp) % Hp), b = (int)(p / ((int64_t)Wp * Hp));
    const int ci = chunk >> 5, ky = (chunk >> 1) & 15, kx0 = (chunk & 1) * 8;
    const int y = py * 16 + ky, x = px * 16 + kx0;
    float v[8];
    if constexpr (KIND == SV_IMG_F32_NCHW) {
      const float* base = reinterpret_cast<const float*>(img) + (((size_t)b * 3 + ci) * H + y) * W + x;
      const float4 r0 = *reinterpret_cast<const float4*>(base);
      const float4 r1 = *reinterpret_cast<const float4*>(base + 4);
      v[0] = r0.x; v[1] = r0.y; v[2] = r0.z; v[3] = r0.w;
      v[4] = r1.x; v[5] = r1.y; v[6] = r1.z; v[7] = r1.w;
    } else {
      const float mean = ci == 0 ? m0 : (ci == 1 ? m1 : m2);
      const float sd = ci == 0 ? s0 : (ci == 1 ? s1 : s2);
      if constexpr (KIND == SV_IMG_U8_GRAY) {
        const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint8_t*>(img) + ((size_t)b * H + y) * W + x);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          v[q] = ((float)((u.x >> (8 * q)) & 0xffu) / 255.0f - mean) / sd;
          v[4 + q] = ((float)((u.y >> (8 * q)) & 0xffu) / 255.0f - mean) / sd;
        }
      } else {
        const uint8_t* base = reinterpret_cast<const uint8_t*>(img) + (((size_t)b * H + y) * W + x) * 3 + ci;
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = ((float)base[3 * q] / 255.0f - mean) / sd;
      }
    }
    TO* o = patches + ((size_t)b * rows_per_img + row0 + (size_t)py * Wp + px) * 768 + chunk * 8;
    st4<TO>(o, 0, make_float4(v[0], v[1], v[2], v[3]));
    st4<TO>(o, 4, make_float4(v[4], v[5], v[6], v[7]));
  }
}

// x[b][t][:] of the padded token matrix [B][rows_per_img][C] (f32) from the patch-embedding rows pe (same row layout):
//   cls_first (ViT):      t = 0: cls + pos[0];  1 <= t <= P: pe + pos[t]      (pos [P + 1][C])
//   else (DeiT-III):      t = 0: cls;           1 <= t <= P: pe + pos[t - 1]  (pos [P][C])
//   t > P: 0 (pad rows)
__global__ void __launch_bounds__(kThreads) vit_tokens_kernel(const float* __restrict__ pe, const float* __restrict__ cls,
                                                               const float* __restrict__ pos, float* __restrict__ x,
                                                               int B, int P, int rows_per_img, int C, int pos_has_cls) {
  const int C4 = C >> 2;
  const int64_t total = (int64_t)B * rows_per_img * C4;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int c = (int)(i % C4) * 4;
    const int64_t row = i / C4;
    const int t = (int)(row % rows_per_img);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t == 0) {
      v = *reinterpret_cast<const float4*>(cls + c);
      if (pos_has_cls) {
        const float4 q = *reinterpret_cast<const float4*>(pos + c);
        v = make_float4(v.x + q.x, v.y + q.y, v.z + q.z, v.w + q.w);
      }
    } else if (t <= P) {
      const float4 a = *reinterpret_cast<const float4*>(pe + row * C + c);
      const float4 q = *reinterpret_cast<const float4*>(pos + (size_t)(pos_has_cls ? t : t - 1) * C + c);
      v = make_float4(a.x + q.x, a.y + q.y, a.z + q.z, a.w + q.w);
    }
    *reinterpret_cast<float4*>(x + row * C + c) = v;
  }
}

static int grid_for(int64_t work) {
  const int64_t g = (work + kThreads - 1) / kThreads;
  return (int)(g < 65536 ? (g > 0 ? g : 1) : 65536);
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace sv

using namespace sv;

extern "C" {

int sv_patchify16(const void* img, int32_t img_kind, const float* norm_mean, const float* norm_std, void* patches,
                  int32_t out_dtype, int32_t B, int32_t H, int32_t W, int64_t rows_per_img, int32_t row0,
                  sv_stream_t stream) {
  SV_REQUIRE(img && patches, "sv_patchify16: null pointer");
  SV_REQUIRE(B > 0 && H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0, "sv_patchify16: H, W must be multiples of 16");
  const int64_t P = (int64_t)(H / 16) * (W / 16);
  if (rows_per_img == 0) rows_per_img = P;
  SV_REQUIRE(row0 >= 0 && rows_per_img >= row0 + P, "sv_patchify16: rows_per_img must hold row0 + %lld patch rows",
             (long long)P);
  SV_REQUIRE(al16(patches), "sv_patchify16: patches must be 16-byte aligned");
  SV_REQUIRE(out_dtype == SV_F32 || out_dtype == SV_BF16, "sv_patchify16: bad output dtype");
  hipStream_t s = (hipStream_t)stream;
  const int grid = grid_for((int64_t)B * P * 96);
  float m[3] = {0.f, 0.f, 0.f}, sd[3] = {1.f, 1.f, 1.f};
  if (img_kind == SV_IMG_F32_NCHW) {
    SV_REQUIRE(al16(img), "sv_patchify16: f32 image must be 16-byte aligned");
  } else if (img_kind == SV_IMG_U8_GRAY || img_kind == SV_IMG_U8_HWC) {
    SV_REQUIRE(norm_mean && norm_std, "sv_patchify16: u8 input needs the normalisation constants");
    SV_REQUIRE(img_kind != SV_IMG_U8_GRAY || ((uintptr_t)img & 7) == 0, "sv_patchify16: u8 image must be 8-byte aligned");
    for (int i = 0; i < 3; ++i) m[i] = norm_mean[i], sd[i] = norm_std[i];
  } else {
    return set_error(SV_ERR_INVALID_ARG, "sv_patchify16: bad image kind %d", img_kind);
  }
#define SV_P16(KIND, TO)                                                                                             \
  patchify16_kernel<KIND, TO><<<grid, kThreads, 0, s>>>(img, m[0], m[1], m[2], sd[0], sd[1], sd[2], (TO*)patches, B, H, \
                                                        W, rows_per_img, row0)
  if (out_dtype == SV_BF16) {
    if (img_kind == SV_IMG_F32_NCHW) SV_P16(SV_IMG_F32_NCHW, uint16_t);
    else if (img_kind == SV_IMG_U8_GRAY) SV_P16(SV_IMG_U8_GRAY, uint16_t);
    else SV_P16(SV_IMG_U8_HWC, uint16_t);
  } else {
    if (img_kind == SV_IMG_F32_NCHW) SV_P16(SV_IMG_F32_NCHW, float);
    else if (img_kind == SV_IMG_U8_GRAY) SV_P16(SV_IMG_U8_GRAY, float);
    else SV_P16(SV_IMG_U8_HWC, float);
  }
#undef SV_P16
  return check_launch("sv_patchify16");
}

int sv_vit_tokens(const float* pe, const float* cls, const float* pos, float* x, int32_t B, int32_t P,
                  int32_t rows_per_img, int32_t C, int32_t pos_has_cls, sv_stream_t stream) {
  SV_REQUIRE(pe && cls && pos && x, "sv_vit_tokens: null pointer");
  SV_REQUIRE(B > 0 && P > 0 && rows_per_img > P && C > 0 && C % 4 == 0,
             "sv_vit_tokens: need rows_per_img > P patches and C a multiple of 4");
  SV_REQUIRE(al16(pe) && al16(cls) && al16(pos) && al16(x), "sv_vit_tokens: operands must be 16-byte aligned");
  vit_tokens_kernel<<<grid_for((int64_t)B * rows_per_img * (C / 4)), kThreads, 0, (hipStream_t)stream>>>(
      pe, cls, pos, x, B, P, rows_per_img, C, pos_has_cls);
  return check_launch("sv_vit_tokens");
}

}  // extern "C"
