// On-device input pipeline of the BCD train step: what the reference does per sample on the
// host with numpy / cv2 before the tensors ever reach the GPU (reference data/transforms.py:100-154:
// random_flip -> random_exchange -> normalize -> to_tensor, composed at scripts/train_BCD.py:262-270) runs here
// as ONE pass over the raw uint8 batch already resident in HBM:
//
//   image u8 [B][H][W][6] (pre RGB | post RGB, the reference's 6-channel HWC array), label u8 [B][H][W]
//   flags u8 [B][3] = (flip around the x axis = cv2.flip(.,0), flip around the y axis = cv2.flip(.,1), exchange)
//   -> pre f32 [B][3][H][W], post f32 [B][3][H][W] = ((u8 / 255) - mean) / std   (f32, IEEE division: bit-identical
//      to numpy's `image.astype(float32) / 255.0`, `(image - mean) / std`),  label f32 [B][1][H][W] = ceil(u8/255).
//
// HBM-bound byte shuffling: 7 B read, 28 B written per pixel; each thread owns 4 consecutive output pixels of one
// row so that the f32 stores are 16-byte vectors (the u8 reads of a wave cover a contiguous 6 KB span).
#include "common.h"
#include "../../include/change3d_hip.h"

namespace {

__global__ __launch_bounds__(256) void bcd_preprocess_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ lab,
                                                             const uint8_t* __restrict__ flags, const float* __restrict__ mean,
                                                             const float* __restrict__ stdv, float* __restrict__ pre,
                                                             float* __restrict__ post, float* __restrict__ label, int B, int H,
                                                             int W) {
  const int wq = (W + 3) >> 2;                                    // 4-pixel groups per row
  const int64_t total = (int64_t)B * H * wq;
  float m[6], s[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) { m[c] = mean[c]; s[c] = stdv[c]; }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int q = (int)(i % wq);
    const int64_t r = i / wq;
    const int y = (int)(r % H), b = (int)(r / H);
    const bool fy = flags && flags[b * 3 + 0], fx = flags && flags[b * 3 + 1], ex = flags && flags[b * 3 + 2];
    const int ys = fy ? H - 1 - y : y;                            // source row
    float o[6][4];
    float l[4];
    const int x0 = q * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = x0 + k;
      const int xs = x < W ? (fx ? W - 1 - x : x) : 0;
      const uint8_t* p = img + (((int64_t)b * H + ys) * W + xs) * 6;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        // channel c of the OUTPUT 6-channel image: after an exchange the first three come from post
        const int cs = ex ? (c < 3 ? c + 3 : c - 3) : c;
        const float v = (float)p[cs] / 255.0f;
        o[c][k] = (v - m[c]) / s[c];
      }
      l[k] = lab ? (lab[((int64_t)b * H + ys) * W + xs] ? 1.0f : 0.0f) : 0.0f;
    }
    const int64_t plane = (int64_t)H * W;
    const int64_t base = (int64_t)y * W + x0;
    if (x0 + 3 < W && (W & 3) == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        *reinterpret_cast<float4*>(pre + ((int64_t)b * 3 + c) * plane + base) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
        *reinterpret_cast<float4*>(post + ((int64_t)b * 3 + c) * plane + base) = make_float4(o[c + 3][0], o[c + 3][1], o[c + 3][2], o[c + 3][3]);
      }
      if (label) *reinterpret_cast<float4*>(label + (int64_t)b * plane + base) = make_float4(l[0], l[1], l[2], l[3]);
    } else {
      for (int k = 0; k < 4 && x0 + k < W; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          pre[((int64_t)b * 3 + c) * plane + base + k] = o[c][k];
          post[((int64_t)b * 3 + c) * plane + base + k] = o[c + 3][k];
        }
        if (label) label[(int64_t)b * plane + base + k] = l[k];
      }
    }
  }
}

// clip[b][c][t][y][x] (f32 NCDHW, what the stem reads): t = 0 <- pre, t = 1..K <- perception frames (shared by the
// batch), t = K+1 <- post.  One 16-byte vector per thread per step; replaces expand + torch.cat
// (reference model/trainer.py:155-162).
__global__ __launch_bounds__(256) void build_clip_kernel(const float* __restrict__ pre, const float* __restrict__ post,
                                                         const float* __restrict__ P, float* __restrict__ clip, int B, int K,
                                                         int64_t hw4) {
  const int T = K + 2;
  const int64_t total = (int64_t)B * 3 * T * hw4;
  const float4* p4 = reinterpret_cast<const float4*>(pre);
  const float4* q4 = reinterpret_cast<const float4*>(post);
  const float4* f4 = reinterpret_cast<const float4*>(P);
  float4* o4 = reinterpret_cast<float4*>(clip);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i % hw4;
    int64_t q = i / hw4;
    const int t = (int)(q % T); q /= T;
    const int c = (int)(q % 3);
    const int b = (int)(q / 3);
    float4 v;
    if (t == 0) v = p4[((int64_t)b * 3 + c) * hw4 + r];
    else if (t == T - 1) v = q4[((int64_t)b * 3 + c) * hw4 + r];
    else v = f4[((int64_t)c * K + (t - 1)) * hw4 + r];
    o4[i] = v;
  }
}

}  // namespace

extern "C" int c3d_build_clip(const float* pre, const float* post, const float* frames, float* clip, int32_t B, int32_t K,
                              int32_t H, int32_t W, void* stream) {
  if (!pre || !post || !frames || !clip || B <= 0 || K <= 0 || H <= 0 || W <= 0) return C3D_E_BADARG;
  if (((int64_t)H * W) & 3) return C3D_E_UNSUPPORTED;
  const int64_t hw4 = (int64_t)H * W / 4, total = (int64_t)B * 3 * (K + 2) * hw4;
  int64_t grid = (total + 255) / 256;
  if (grid > 256 * 32) grid = 256 * 32;
  build_clip_kernel<<<dim3((unsigned)grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(pre, post, frames, clip, B,
                                                                                                  K, hw4);
  C3D_CHECK_LAUNCH();
  return 0;
}

// SCD labels (reference data/transforms.py:300-326 SCDTransforms.random_flip / random_exchange, :341-357 to_tensor;
// scripts/train_SCD.py:207-213 `.long()`): label u8 [B][H][W][3] = (pre classes, post classes, change) with the same
// flip / exchange flags as the image (c3d_bcd_preprocess handles the image: the 6-channel arithmetic is identical)
// -> int64 [B][3][H][W]; an exchange swaps the two class maps.
__global__ __launch_bounds__(256) void scd_label_kernel(const uint8_t* __restrict__ lab, const uint8_t* __restrict__ flags,
                                                        int64_t* __restrict__ out, int B, int H, int W) {
  const int64_t total = (int64_t)B * H * W;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    const int64_t r = i / W;
    const int y = (int)(r % H), b = (int)(r / H);
    const bool fy = flags && flags[b * 3 + 0], fx = flags && flags[b * 3 + 1], ex = flags && flags[b * 3 + 2];
    const uint8_t* p = lab + (((int64_t)b * H + (fy ? H - 1 - y : y)) * W + (fx ? W - 1 - x : x)) * 3;
    const int64_t plane = (int64_t)H * W, o = (int64_t)b * 3 * plane + (int64_t)y * W + x;
    out[o] = p[ex ? 1 : 0];
    out[o + plane] = p[ex ? 0 : 1];
    out[o + 2 * plane] = p[2];
  }
}

// BDA labels (reference data/transforms.py:502-526 BDATransforms.random_flip / random_exchange, :541-556 to_tensor;
// scripts/train_BDA.py:194-195 `label[:, 0].float()`, `torch.prod(label, dim=1).long()`): label u8 [B][H][W][2] =
// (localisation, damage class) with the two flips of the image pass -> label_loc f32 [B][1][H][W] and
// label_cls int64 [B][H][W] = localisation x damage class.  The exchange flag swaps the IMAGES only: the labels describe
// the post-disaster state whichever way round the pair is fed (flags[b][2] is not read here).
__global__ __launch_bounds__(256) void bda_label_kernel(const uint8_t* __restrict__ lab, const uint8_t* __restrict__ flags,
                                                        float* __restrict__ loc, int64_t* __restrict__ cls, int B, int H, int W) {
  const int64_t total = (int64_t)B * H * W;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    const int64_t r = i / W;
    const int y = (int)(r % H), b = (int)(r / H);
    const bool fy = flags && flags[b * 3 + 0], fx = flags && flags[b * 3 + 1];
    const uint8_t* p = lab + (((int64_t)b * H + (fy ? H - 1 - y : y)) * W + (fx ? W - 1 - x : x)) * 2;
    const uint8_t l0 = p[0], l1 = p[1];
    loc[i] = (float)l0;
    cls[i] = (int64_t)l0 * (int64_t)l1;       // torch.prod of a uint8 tensor accumulates in int64: no wrap
  }
}

// Change-captioning image pairs (reference data/dataset.py:411-424 CaptionDataset.__getitem__ + scripts/train_CC.py:466-469
// transforms.Normalize): img u8 [B][2][3][H][W] (planar, as the HDF5 file stores them) -> pre, post f32 [B][3][H][W] =
// Normalize(FloatTensor(u8 / 255.)) through a 3 x 256 table built by the HOST with exactly that arithmetic (f64 division,
// rounded to f32, then f32 sub / div), so every value is bit-identical to the reference's; swap[b] != 0 exchanges the
// pair (the TRAIN split's p = 0.3 augmentation).  8 B read / 32 B written per 4 pixels and plane.
__global__ __launch_bounds__(256) void cc_preprocess_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ swap,
                                                            const float* __restrict__ lut, float* __restrict__ pre,
                                                            float* __restrict__ post, int B, int64_t hw4) {
  __shared__ float tab[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += blockDim.x) tab[i] = lut[i];
  __syncthreads();
  const int64_t total = (int64_t)B * 6 * hw4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = i % hw4;
    const int pc = (int)((i / hw4) % 6), b = (int)(i / (hw4 * 6));   // pc = image (0 / 1) * 3 + channel
    const uchar4 v = reinterpret_cast<const uchar4*>(img)[i];
    const float* t = tab + (pc % 3) * 256;
    const bool second = (pc >= 3) != (swap && swap[b]);
    float* dst = (second ? post : pre) + ((int64_t)b * 3 + pc % 3) * hw4 * 4 + q * 4;
    *reinterpret_cast<float4*>(dst) = make_float4(t[v.x], t[v.y], t[v.z], t[v.w]);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// File-data-set input pipeline: gather + the whole training augmentation chain in one pass over a uint8 store that
// stays resident in HBM (reference data/transforms.py:166-207 get_transform_pipelines and its SCD / BDA siblings:
// normalize -> scale -> random_crop_resize -> random_flip -> random_exchange -> to_tensor).
//
//   store u8 [N][Hs][Ws][6], label store u8 [N][Hs][Ws][L], table i32 [B][8] = (index, do_crop, x1, y1, flip0, flip1,
//   exchange, reserved) -> pre, post f32 [B][3][H][W] and the task's label tensors (those of c3d_bcd_preprocess /
//   c3d_scd_label_preprocess / c3d_bda_label_preprocess).
//
// An output pixel is un-flipped first (the flips follow the resize), then mapped into the source window: the whole
// image (scale; the identity when the sizes agree) or [y1 : H - y1, x1 : W - x1] (random_crop_resize).  Images are
// resampled as cv2.INTER_LINEAR does on the NORMALISED f32 image: source coordinate (d + 0.5) * (src / dst) - 0.5 in
// double, rounded to f32, floor + fraction in f32, index clamped with fraction 0 at the borders, the horizontal lerp
// S[sx] * (1 - fx) + S[sx + 1] * fx on both rows, then the vertical one (separate multiplies and add, no fma).  A
// fraction of 0 copies the tap, so a sample without crop at the store's own size is bit-identical to the plain passes
// above.  Labels are resampled as cv2.INTER_NEAREST with the exact integer quotient min(d * src / dst, src - 1).
//
// One wave owns one output row (4 waves = 4 rows per workgroup).  The workgroup builds the 6 x 256 table of normalised
// byte values once in LDS (the same two IEEE divisions as the plain pass, 6 per lane instead of 24), each wave stages
// the one or two source rows it needs into LDS with 16-byte loads and interpolates from there; every lane owns 4
// consecutive output pixels, so the f32 stores are 16-byte vectors.  SRC_F32 is the second launch of the two-resample
// case (store size != H x W together with a crop): the image taps come from the already scaled and normalised planar
// f32 batch the first launch wrote, straight from global memory; the labels still come from the u8 store through the
// composition of the two nearest-neighbour index maps, which is exact.
enum { AUG_SCALE_ONLY = 1 };

struct AugArgs {
  const uint8_t* img; const float* spre; const float* spost; const uint8_t* lab; const int32_t* table;
  const float* mean; const float* stdv;
  float* pre; float* post; float* lab_f; int64_t* lab_i;
  int64_t img_bytes;
  int N, Hs, Ws, B, H, W, task, mode, row_lds;
};

struct alignas(16) I64x2 { int64_t a, b; };

__device__ __forceinline__ void aug_lin_coord(int d, int src, int dst, int& s0, float& f) {
  if (src == dst) { s0 = d; f = 0.f; return; }
  const float c = (float)(((double)d + 0.5) * ((double)src / (double)dst) - 0.5);
  int s = (int)floorf(c);
  f = c - (float)s;
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= src - 1) { s = src - 1; f = 0.f; }
  s0 = s;
}

__device__ __forceinline__ int aug_near_coord(int d, int src, int dst) {
  if (src == dst) return d;
  const int s = (int)(((int64_t)d * src) / dst);
  return s < src - 1 ? s : src - 1;
}

__device__ __forceinline__ float aug_lerp(float a, float b, float f) {
  return f == 0.f ? a : __fadd_rn(__fmul_rn(a, 1.0f - f), __fmul_rn(b, f));
}

__device__ __forceinline__ int aug_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the 6 bytes of source pixel `col` of a staged row (2-byte aligned: the row starts at a multiple of 6 bytes)
__device__ __forceinline__ void aug_tap_u8(const uint8_t* row, int col, int (&v)[6]) {
  const uint16_t* p = reinterpret_cast<const uint16_t*>(row + col * 6);
  const uint32_t a = p[0], b = p[1], c = p[2];
  v[0] = a & 255; v[1] = a >> 8; v[2] = b & 255; v[3] = b >> 8; v[4] = c & 255; v[5] = c >> 8;
}

template <bool SRC_F32>
__global__ __launch_bounds__(256) void augment_gather_kernel(const AugArgs a) {
  extern __shared__ uint4 aug_smem[];
  float* lut = reinterpret_cast<float*>(aug_smem);                                  // [6][256], u8 source only
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint8_t* rowbuf = reinterpret_cast<uint8_t*>(aug_smem) + 6 * 256 * 4 + (size_t)wave * 2 * a.row_lds;
  if (!SRC_F32) {
    for (int i = threadIdx.x; i < 6 * 256; i += 256) {
      const int c = i >> 8;
      const float v = (float)(i & 255) / 255.0f;
      lut[i] = (v - a.mean[c]) / a.stdv[c];
    }
  }
  const int H = a.H, W = a.W;
  const int IH = SRC_F32 ? H : a.Hs, IW = SRC_F32 ? W : a.Ws;                       // image source extent
  const int64_t nrows = (int64_t)a.B * H, plane = (int64_t)H * W;
  const bool plain = a.mode & AUG_SCALE_ONLY;
  for (int64_t g = blockIdx.x; g * 4 < nrows; g += gridDim.x) {
    const int64_t row = g * 4 + wave;
    const bool valid = row < nrows;
    const int b = valid ? (int)(row / H) : 0, y = valid ? (int)(row % H) : 0;
    const int32_t* t = (a.table && valid) ? a.table + (int64_t)b * 8 : nullptr;
    const int n = aug_clamp(t ? t[0] : b, 0, a.N - 1);
    // a crop needs a source of the output's own size (the two-launch path provides it); offsets are clamped so that the
    // window keeps at least one pixel whatever the table holds
    const bool crop = t && !plain && t[1] != 0 && IH == H && IW == W;
    const int x1 = crop ? aug_clamp(t[2], 0, (W - 1) >> 1) : 0, y1 = crop ? aug_clamp(t[3], 0, (H - 1) >> 1) : 0;
    const bool fl0 = t && !plain && t[4] != 0, fl1 = t && !plain && t[5] != 0, ex = t && !plain && t[6] != 0;
    const int cw = crop ? W - 2 * x1 : IW, ch = crop ? H - 2 * y1 : IH;
    const int yf = fl0 ? H - 1 - y : y;
    int sy; float fy;
    aug_lin_coord(yf, ch, H, sy, fy);
    const int r0 = aug_clamp(y1 + sy, 0, IH - 1), r1 = fy != 0.f ? aug_clamp(r0 + 1, 0, IH - 1) : r0;
    const bool identity = cw == W && ch == H;                                        // every fraction is 0
    int lead0 = 0, lead1 = 0;
    if (!SRC_F32) {
      __syncthreads();                        // the table of normalised values; the previous row's taps are consumed
      if (valid) {
        for (int k = 0; k < (r1 != r0 ? 2 : 1); ++k) {
          // 16-byte chunks on 16-byte ADDRESS boundaries (the store may start anywhere even: a view that begins at
          // sample n0); a chunk that sticks out of the store at either end is fetched byte by byte, inside it
          const int64_t s = (((int64_t)n * IH + (k ? r1 : r0)) * IW) * 6;
          const int lead = (int)((reinterpret_cast<uintptr_t>(a.img) + (uint64_t)s) & 15), chunks = (lead + IW * 6 + 15) >> 4;
          (k ? lead1 : lead0) = lead;
          uint8_t* dst = rowbuf + (size_t)k * a.row_lds;
          for (int i = lane; i < chunks; i += 64) {
            const int64_t off = s - lead + 16 * (int64_t)i;
            if (off >= 0 && off + 16 <= a.img_bytes) {
              reinterpret_cast<uint4*>(dst)[i] = *reinterpret_cast<const uint4*>(a.img + off);
            } else {
              for (int j = 0; j < 16; ++j) dst[16 * i + j] = (off + j >= 0 && off + j < a.img_bytes) ? a.img[off + j] : (uint8_t)0;
            }
          }
        }
        if (r1 == r0) lead1 = lead0;
      }
      __syncthreads();
    }
    if (!valid) continue;
    const uint8_t* row0 = rowbuf + lead0;
    const uint8_t* row1 = r1 != r0 ? rowbuf + a.row_lds + lead1 : row0;
    // labels: nearest through the crop (in H x W coordinates), then through the scale (store coordinates)
    const bool labels = a.lab && !plain && a.task != 0;
    const int ly = aug_near_coord(crop ? y1 + aug_near_coord(yf, ch, H) : yf, a.Hs, H);
    const int L = a.task == 1 ? 1 : (a.task == 2 ? 3 : 2);
    const uint8_t* lrow = labels ? a.lab + (((int64_t)n * a.Hs + aug_clamp(ly, 0, a.Hs - 1)) * a.Ws) * L : nullptr;
    for (int q = lane; q < (W >> 2); q += 64) {
      const int x0 = q * 4;
      float o[6][4];
      int lx[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int x = x0 + k, xf = fl1 ? W - 1 - x : x;
        int sx; float fx;
        aug_lin_coord(xf, cw, W, sx, fx);
        const int c0 = aug_clamp(x1 + sx, 0, IW - 1), c1 = fx != 0.f ? aug_clamp(c0 + 1, 0, IW - 1) : c0;
        lx[k] = aug_clamp(aug_near_coord(crop ? x1 + aug_near_coord(xf, cw, W) : xf, a.Ws, W), 0, a.Ws - 1);
        if (SRC_F32) {
#pragma unroll
          for (int c = 0; c < 6; ++c) {
            const int cs = ex ? (c < 3 ? c + 3 : c - 3) : c;
            const float* sp = (cs < 3 ? a.spre : a.spost) + ((int64_t)b * 3 + (cs % 3)) * plane;
            const float* p0 = sp + (int64_t)r0 * W;
            const float* p1 = sp + (int64_t)r1 * W;
            if (identity) {
              o[c][k] = p0[c0];
            } else {
              const float h0 = aug_lerp(p0[c0], p0[c1], fx), h1 = fy != 0.f ? aug_lerp(p1[c0], p1[c1], fx) : h0;
              o[c][k] = aug_lerp(h0, h1, fy);
            }
          }
        } else if (identity) {
          int v[6];
          aug_tap_u8(row0, c0, v);
#pragma unroll
          for (int c = 0; c < 6; ++c) {
            const int cs = ex ? (c < 3 ? c + 3 : c - 3) : c;
            o[c][k] = lut[cs * 256 + v[cs]];
          }
        } else {
          int v00[6], v01[6], v10[6], v11[6];
          aug_tap_u8(row0, c0, v00);
          aug_tap_u8(row0, c1, v01);
          aug_tap_u8(row1, c0, v10);
          aug_tap_u8(row1, c1, v11);
#pragma unroll
          for (int c = 0; c < 6; ++c) {
            // normalize precedes the exchange in the reference: the source channel's constants apply
            const int cs = ex ? (c < 3 ? c + 3 : c - 3) : c;
            const float* lc = lut + cs * 256;
            const float h0 = aug_lerp(lc[v00[cs]], lc[v01[cs]], fx);
            const float h1 = fy != 0.f ? aug_lerp(lc[v10[cs]], lc[v11[cs]], fx) : h0;
            o[c][k] = aug_lerp(h0, h1, fy);
          }
        }
      }
      const int64_t base = (int64_t)y * W + x0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        *reinterpret_cast<float4*>(a.pre + ((int64_t)b * 3 + c) * plane + base) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
        *reinterpret_cast<float4*>(a.post + ((int64_t)b * 3 + c) * plane + base) =
            make_float4(o[c + 3][0], o[c + 3][1], o[c + 3][2], o[c + 3][3]);
      }
      if (!labels) continue;
      if (a.task == 1) {                               // BCD: ceil(u8 / 255)
        float l[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) l[k] = lrow[lx[k]] ? 1.0f : 0.0f;
        *reinterpret_cast<float4*>(a.lab_f + (int64_t)b * plane + base) = make_float4(l[0], l[1], l[2], l[3]);
      } else if (a.task == 2) {                        // SCD: int64 [B][3][H][W], the exchange swaps the two class maps
        int64_t l[3][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint8_t* p = lrow + (int64_t)lx[k] * 3;
          l[0][k] = p[ex ? 1 : 0]; l[1][k] = p[ex ? 0 : 1]; l[2][k] = p[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          I64x2* d = reinterpret_cast<I64x2*>(a.lab_i + ((int64_t)b * 3 + c) * plane + base);
          d[0] = I64x2{l[c][0], l[c][1]};
          d[1] = I64x2{l[c][2], l[c][3]};
        }
      } else {                                         // BDA: loc f32, cls int64 = loc x class; the exchange leaves them alone
        float lo[4];
        int64_t cl[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint8_t* p = lrow + (int64_t)lx[k] * 2;
          lo[k] = (float)p[0];
          cl[k] = (int64_t)p[0] * (int64_t)p[1];
        }
        *reinterpret_cast<float4*>(a.lab_f + (int64_t)b * plane + base) = make_float4(lo[0], lo[1], lo[2], lo[3]);
        I64x2* d = reinterpret_cast<I64x2*>(a.lab_i + (int64_t)b * plane + base);
        d[0] = I64x2{cl[0], cl[1]};
        d[1] = I64x2{cl[2], cl[3]};
      }
    }
  }
}

extern "C" int c3d_augment_gather(const uint8_t* store, const uint8_t* label_store, const int32_t* table, const float* mean6,
                                  const float* std6, float* pre, float* post, void* label_a, void* label_b, float* scratch,
                                  int32_t task, int32_t N, int32_t Hs, int32_t Ws, int32_t B, int32_t H, int32_t W,
                                  void* stream) {
  if (!store || !mean6 || !std6 || !pre || !post || N <= 0 || Hs <= 0 || Ws <= 0 || B <= 0 || H <= 0 || W <= 0)
    return C3D_E_BADARG;
  if (task < C3D_AUG_NONE || task > C3D_AUG_BDA) return C3D_E_BADARG;
  if ((task != C3D_AUG_NONE) != (label_store != nullptr) || (task != C3D_AUG_NONE) != (label_a != nullptr)) return C3D_E_BADARG;
  if ((task == C3D_AUG_BDA) != (label_b != nullptr)) return C3D_E_BADARG;
  if (!table && B > N) return C3D_E_BADARG;                       // index = b must exist
  if (reinterpret_cast<uintptr_t>(store) & 1) return C3D_E_BADARG;   // the staged rows are read as 16-bit words
  const bool two = table && (Hs != H || Ws != W);                 // scale, then crop: the reference resamples twice
  if (two && !scratch) return C3D_E_BADARG;
  if (W & 3) return C3D_E_UNSUPPORTED;
  if (H > 32768 || W > 32768 || Hs > 32768) return C3D_E_UNSUPPORTED;
  AugArgs a;
  a.img = store; a.spre = nullptr; a.spost = nullptr; a.lab = label_store; a.table = table; a.mean = mean6; a.stdv = std6;
  a.pre = pre; a.post = post;
  a.lab_f = task == C3D_AUG_SCD ? nullptr : static_cast<float*>(label_a);
  a.lab_i = task == C3D_AUG_SCD ? static_cast<int64_t*>(label_a) : static_cast<int64_t*>(label_b);
  a.img_bytes = (int64_t)N * Hs * Ws * 6;
  a.N = N; a.Hs = Hs; a.Ws = Ws; a.B = B; a.H = H; a.W = W; a.task = task; a.mode = 0;
  a.row_lds = ((Ws * 6 + 15) & ~15) + 32;
  const size_t lds = 6 * 256 * 4 + (size_t)8 * a.row_lds;
  if (lds > 64 * 1024) return C3D_E_UNSUPPORTED;                  // Ws <= 1232: two staged rows per wave in 64 KB of LDS
  int64_t grid = ((int64_t)B * H + 3) / 4;
  if (grid > 256 * 8) grid = 256 * 8;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!two) {
    augment_gather_kernel<false><<<dim3((unsigned)grid), dim3(256), lds, st>>>(a);
    C3D_CHECK_LAUNCH();
    return 0;
  }
  AugArgs s = a;                                                  // launch 1: gather + normalize + scale into the scratch batch
  s.mode = AUG_SCALE_ONLY;
  s.pre = scratch; s.post = scratch + (int64_t)B * 3 * H * W;
  augment_gather_kernel<false><<<dim3((unsigned)grid), dim3(256), lds, st>>>(s);
  C3D_CHECK_LAUNCH();
  a.spre = s.pre; a.spost = s.post;                               // launch 2: crop-resize, flips, exchange; labels from the store
  augment_gather_kernel<true><<<dim3((unsigned)grid), dim3(256), 0, st>>>(a);
  C3D_CHECK_LAUNCH();
  return 0;
}

extern "C" int c3d_scd_label_preprocess(const uint8_t* label3, const uint8_t* flags, int64_t* out, int32_t B, int32_t H,
                                        int32_t W, void* stream) {
  if (!label3 || !out || B <= 0 || H <= 0 || W <= 0) return C3D_E_BADARG;
  int64_t grid = ((int64_t)B * H * W + 255) / 256;
  if (grid > 256 * 32) grid = 256 * 32;
  scd_label_kernel<<<dim3((unsigned)grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(label3, flags, out, B, H, W);
  C3D_CHECK_LAUNCH();
  return 0;
}

extern "C" int c3d_bda_label_preprocess(const uint8_t* label2, const uint8_t* flags, float* label_loc, int64_t* label_cls,
                                        int32_t B, int32_t H, int32_t W, void* stream) {
  if (!label2 || !label_loc || !label_cls || B <= 0 || H <= 0 || W <= 0) return C3D_E_BADARG;
  int64_t grid = ((int64_t)B * H * W + 255) / 256;
  if (grid > 256 * 32) grid = 256 * 32;
  bda_label_kernel<<<dim3((unsigned)grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(label2, flags, label_loc,
                                                                                                 label_cls, B, H, W);
  C3D_CHECK_LAUNCH();
  return 0;
}

extern "C" int c3d_cc_preprocess(const uint8_t* img, const uint8_t* swap, const float* lut, float* pre, float* post,
                                 int32_t B, int32_t H, int32_t W, void* stream) {
  if (!img || !lut || !pre || !post || B <= 0 || H <= 0 || W <= 0 || (((int64_t)H * W) & 3)) return C3D_E_BADARG;
  const int64_t hw4 = (int64_t)H * W / 4;
  int64_t grid = ((int64_t)B * 6 * hw4 + 255) / 256;
  if (grid > 256 * 32) grid = 256 * 32;
  cc_preprocess_kernel<<<dim3((unsigned)grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(img, swap, lut, pre, post,
                                                                                                     B, hw4);
  C3D_CHECK_LAUNCH();
  return 0;
}

extern "C" int c3d_bcd_preprocess(const uint8_t* image6, const uint8_t* label, const uint8_t* flags, const float* mean6,
                                  const float* std6, float* pre, float* post, float* label_out, int32_t B, int32_t H,
                                  int32_t W, void* stream) {
  if (!image6 || !mean6 || !std6 || !pre || !post || B <= 0 || H <= 0 || W <= 0) return C3D_E_BADARG;
  if ((label == nullptr) != (label_out == nullptr)) return C3D_E_BADARG;
  const int64_t total = (int64_t)B * H * ((W + 3) / 4);
  int64_t grid = (total + 255) / 256;
  if (grid > 256 * 32) grid = 256 * 32;
  bcd_preprocess_kernel<<<dim3((unsigned)grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(
      image6, label, flags, mean6, std6, pre, post, label_out, B, H, W);
  C3D_CHECK_LAUNCH();
  return 0;
}
