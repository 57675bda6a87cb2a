// Whole-scene inference (change3d_amd/infer.py): cut a co-registered uint8 scene pair that stays resident in HBM into
// overlapping model-sized tiles, and put the per-tile predictions back together.  The reference has no counterpart: its
// val() only sees pre-cut 256 x 256 crops (reference scripts/train_BCD.py:92-154, scripts/train_SCD.py:104-178).
//
// Geometry, per axis (tile t, stride s, 1 <= s <= t, t - s even): margin m = (t - s) / 2, n = ceil(extent / s) tiles, tile i
// starts at i*s - m, so that every scene pixel lies in the central s-wide region of some tile, and k = ceil(t / s) tile
// rows cover any scene row.  Coordinates outside the scene fold back as numpy's `reflect` does, for any overhang (period
// 2*(extent-1), extent 1 -> 0), so a scene smaller than a tile or than the margin is legal.
//
//   c3d_scene_gather   scene u8 [Hs][Ws][6] + origins i32 [n][2] -> pre, post f32 [n][3][th][tw] = ((u8/255) - mean)/std,
//                      the arithmetic of c3d_bcd_preprocess through the 6 x 256 table of c3d_augment_gather (bit-identical
//                      for a tile inside the scene).  6 B read, 24 B written per tile pixel.
//   c3d_scene_stitch   a ring of ky tile rows of predictions f32 [ky][ncols][C][th][tw] -> the scene rows that became final
//                      with tile row `row`: per pixel and channel sum(w*p) / sum(w) over the covering tiles in a FIXED order
//                      (tile row ascending, then tile column ascending), w = wy[y] * wx[x].  Gather form: every output
//                      pixel is written once by one thread, no atomics, so two runs agree bit for bit.
//
//   c3d_scene_gather_views / c3d_scene_fold_views   test-time augmentation: the same tiles under the views of a mask over
//                      the eight flips and rotations of the square, and the mean of the model's outputs with each view
//                      undone, written straight into a slot range of the stitch ring (see "test-time augmentation" below).
//
// All are streaming kernels: a thread owns 4 consecutive pixels of one output row and stores them as one 16-byte vector;
// rows of a scene whose width is no multiple of 4 are shifted so that the vectors stay aligned and the edges go out as
// scalars.  Tables (normalised byte values, window vectors) live in LDS; a thread's tile set is found once, outside its
// channel / tap loops.
#include <initializer_list>

#include "common.h"
#include "../../include/change3d_hip.h"

namespace {

// numpy `reflect` for any overhang, then clamped: no origin can address outside the scene
__device__ __forceinline__ int scene_fold(int64_t c, int E) {
  if (c < 0 || c >= E) {
    if (E == 1) return 0;
    const int64_t P = 2 * (int64_t)(E - 1);
    c %= P;
    if (c < 0) c += P;
    if (c >= E) c = P - c;
  }
  const int r = (int)c;
  return r < 0 ? 0 : (r > E - 1 ? E - 1 : r);
}

// One workgroup per (tile, band of `band` tile rows); item = 4 consecutive pixels of one tile row.
__global__ __launch_bounds__(256) void scene_gather_kernel(const uint8_t* __restrict__ scene, const int32_t* __restrict__ origins,
                                                           const float* __restrict__ mean, const float* __restrict__ stdv,
                                                           float* __restrict__ pre, float* __restrict__ post, int Hs, int Ws,
                                                           int n, int th, int tw, int band, int vec) {
  extern __shared__ float lut[];                           // [6][256]; dynamic, because c3d_launch_lds raises the dynamic limit
  for (int i = threadIdx.x; i < 6 * 256; i += 256) {
    const int c = i >> 8;                                  // to the CU's whole LDS, which leaves no room for a static array
    const float v = (float)(i & 255) / 255.0f;
    lut[i] = (v - mean[c]) / stdv[c];
  }
  __syncthreads();
  const int wq = (tw + 3) >> 2, bands = (th + band - 1) / band;
  const int64_t plane = (int64_t)th * tw;
  for (int64_t g = blockIdx.x; g < (int64_t)n * bands; g += gridDim.x) {
    const int tile = (int)(g / bands), ya = (int)(g % bands) * band, yb = ya + band < th ? ya + band : th;
    const int64_t oy = origins[2 * tile], ox = origins[2 * tile + 1];
    int qprev = -1, xs[4];
    for (int i = threadIdx.x; i < (yb - ya) * wq; i += 256) {
      const int q = i % wq, y = ya + i / wq;
      if (q != qprev) {                                    // 256 % wq == 0 (tw = 32, 64, 256, ...): folded once per thread
#pragma unroll
        for (int k = 0; k < 4; ++k) xs[k] = scene_fold(ox + 4 * q + k, Ws);
        qprev = q;
      }
      const uint8_t* row = scene + (int64_t)scene_fold(oy + y, Hs) * Ws * 6;
      float o[6][4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint16_t* p = reinterpret_cast<const uint16_t*>(row + (int64_t)xs[k] * 6);   // even address: 6 B pixels
        const uint32_t a = p[0], b = p[1], c = p[2];
        o[0][k] = lut[a & 255]; o[1][k] = lut[256 + (a >> 8)]; o[2][k] = lut[512 + (b & 255)];
        o[3][k] = lut[768 + (b >> 8)]; o[4][k] = lut[1024 + (c & 255)]; o[5][k] = lut[1280 + (c >> 8)];
      }
      const int x0 = q * 4;
      const int64_t base = (int64_t)tile * 3 * plane + (int64_t)y * tw + x0;
      if (vec) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          *reinterpret_cast<float4*>(pre + base + c * plane) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
          *reinterpret_cast<float4*>(post + base + c * plane) = make_float4(o[c + 3][0], o[c + 3][1], o[c + 3][2], o[c + 3][3]);
        }
      } else {
        for (int k = 0; k < 4 && x0 + k < tw; ++k) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            pre[base + c * plane + k] = o[c][k];
            post[base + c * plane + k] = o[c + 3][k];
          }
        }
      }
    }
  }
}

struct StitchArgs {
  const float* ring; const float* wy; const float* wx; float* blend; uint8_t* cls; const uint8_t* gate;
  int Hs, Ws, C, th, tw, sy, sx, my, mx, ky, ncols, row, y0, y1, vec_in, vec_blend, vec_cls;
};

// Item = (scene row Y of the strip, quad q): the 4 pixels X0 .. X0 + 3 with X0 = 4q - ((Y * Ws) & 3), so that Y * Ws + X0
// is a multiple of 4 whatever Ws is: the u8 quad and channel 0's f32 quad are aligned, the row's two edges are partial.
__global__ __launch_bounds__(256) void scene_stitch_kernel(const StitchArgs a) {
  extern __shared__ float4 stitch_smem[];
  float* wy = reinterpret_cast<float*>(stitch_smem);
  float* wx = wy + ((a.th + 3) & ~3);
  for (int i = threadIdx.x; i < a.th; i += 256) wy[i] = a.wy[i];
  for (int i = threadIdx.x; i < a.tw; i += 256) wx[i] = a.wx[i];
  __syncthreads();
  const int nq = (a.Ws + 6) >> 2;                          // quads of the longest shifted row
  const int64_t total = (int64_t)(a.y1 - a.y0) * nq, pix = (int64_t)a.Hs * a.Ws;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i % nq), Y = a.y0 + (int)(i / nq);
    const int64_t e0 = (int64_t)Y * a.Ws;
    const int X0 = 4 * q - (int)(e0 & 3);
    if (X0 >= a.Ws) continue;
    const int Xa = X0 < 0 ? 0 : X0, Xb = X0 + 3 < a.Ws ? X0 + 3 : a.Ws - 1;   // first and last pixel of the scene in the quad
    const bool full = X0 >= 0 && X0 + 3 < a.Ws;
    // tile rows r with 0 <= Y - (r*sy - my) < th that exist so far (all of them are in the ring), tile columns likewise
    // (r_lo >= row - ky + 1 for every Y >= row*sy - my, since (th - 1) / sy = ky - 1: the ring holds all of them)
    const int r_lo = Y + a.my - a.th + 1 <= 0 ? 0 : (Y + a.my - a.th + a.sy) / a.sy;
    const int r_hi = (Y + a.my) / a.sy < a.row ? (Y + a.my) / a.sy : a.row;
    const int c_lo = Xa + a.mx - a.tw + 1 <= 0 ? 0 : (Xa + a.mx - a.tw + a.sx) / a.sx;
    const int c_hi = (Xb + a.mx) / a.sx < a.ncols - 1 ? (Xb + a.mx) / a.sx : a.ncols - 1;
    float den[4] = {0.f, 0.f, 0.f, 0.f}, best[4] = {0.f, 0.f, 0.f, 0.f};
    int arg[4] = {0, 0, 0, 0};
    for (int ch = 0; ch < a.C; ++ch) {
      float num[4] = {0.f, 0.f, 0.f, 0.f};
      for (int r = r_lo; r <= r_hi; ++r) {
        const int yl = Y - (r * a.sy - a.my);
        const float wr = wy[yl];
        const float* trow = a.ring + ((((int64_t)(r % a.ky) * a.ncols + c_lo) * a.C + ch) * a.th + yl) * a.tw;
        for (int c = c_lo; c <= c_hi; ++c, trow += (int64_t)a.C * a.th * a.tw) {
          const int xl = X0 - (c * a.sx - a.mx);           // tile-local x of the quad's first pixel
          if (full && a.vec_in && xl >= 0 && xl + 3 < a.tw && !(xl & 3)) {
            const float4 p = *reinterpret_cast<const float4*>(trow + xl);
            const float4 w4 = *reinterpret_cast<const float4*>(wx + xl);
            const float w0 = wr * w4.x, w1 = wr * w4.y, w2 = wr * w4.z, w3 = wr * w4.w;
            num[0] = fmaf(w0, p.x, num[0]); num[1] = fmaf(w1, p.y, num[1]);
            num[2] = fmaf(w2, p.z, num[2]); num[3] = fmaf(w3, p.w, num[3]);
            if (ch == 0) { den[0] += w0; den[1] += w1; den[2] += w2; den[3] += w3; }
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int x = xl + k, X = X0 + k;
              if (X < 0 || X >= a.Ws || x < 0 || x >= a.tw) continue;
              const float w = wr * wx[x];
              num[k] = fmaf(w, trow[x], num[k]);
              if (ch == 0) den[k] += w;
            }
          }
        }
      }
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[k] = num[k] / den[k];                            // den > 0 for a pixel of the scene: some tile's centre holds it
        if (ch == 0 || v[k] > best[k]) { best[k] = v[k]; arg[k] = ch; }   // strict: the lowest index wins a tie
      }
      if (a.blend) {
        float* o = a.blend + ch * pix + e0 + X0;
        if (full && a.vec_blend && !((ch * pix) & 3)) {
          *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (X0 + k >= 0 && X0 + k < a.Ws) o[k] = v[k];
        }
      }
    }
    if (a.cls) {
      uint8_t u[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        u[k] = a.C == 1 ? (uint8_t)(best[k] > 0.5f) : (uint8_t)arg[k];
        if (a.gate && X0 + k >= 0 && X0 + k < a.Ws) u[k] *= a.gate[e0 + X0 + k];
      }
      uint8_t* o = a.cls + e0 + X0;
      if (full && a.vec_cls) {
        *reinterpret_cast<uchar4*>(o) = make_uchar4(u[0], u[1], u[2], u[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (X0 + k >= 0 && X0 + k < a.Ws) o[k] = u[k];
      }
    }
  }
}

// ---- test-time augmentation: the eight views of the square (include/change3d_hip.h "Views") ----
// V_v: transpose if v & 4, then reverse the rows if v & 2, then the columns if v & 1.  Both kernels below walk a plane in
// 32 x 32 blocks, one block per workgroup pass: thread (r, q) = (tid >> 3, tid & 7) owns the quad 4q .. 4q + 3 of block row r,
// so 8 neighbouring lanes read and write 128 B (192 B of scene) runs of one row whatever the view is.  A transposing view
// goes through an LDS block [32][33] (pitch 33 dwords): written by rows, lane (r, q) word k at r*33 + 4q + k, read by columns,
// lane (r, q) word k at (4q + k)*33 + r.  A 32-lane half holds 4 consecutive r and all 8 q, and r + 4q takes 32 different
// values mod 32 there, so both directions touch every bank once (tools/tta_lds_check.py prints the model's cycle counts).
// A column-reversing view keeps its 16-byte accesses: the quad at x0 maps to the quad at tw - 4 - x0 with its words reversed.
constexpr int kVB = 32, kVP = kVB + 1;                       // block edge, LDS pitch in dwords

__device__ __forceinline__ int view_slot(int mask, int v) { return __popc(mask & ((1 << v) - 1)); }

// 4 words of row `row` of a th x tw plane that view bit 0 (`rev`) maps onto columns x0 .. x0 + 3: d[k] = p[row][rev ? tw-1-(x0+k) : x0+k]
template <bool VEC>
__device__ __forceinline__ void quad_load(const float* __restrict__ p, int row, int x0, bool rev, int tw, float (&d)[4]) {
  const float* r = p + (int64_t)row * tw;
  if (VEC) {                                                 // tw % 4 == 0: the quad is whole and aligned on either side
    const float4 a = *reinterpret_cast<const float4*>(r + (rev ? tw - 4 - x0 : x0));
    d[0] = rev ? a.w : a.x; d[1] = rev ? a.z : a.y; d[2] = rev ? a.y : a.z; d[3] = rev ? a.x : a.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = x0 + k < tw ? r[rev ? tw - 1 - (x0 + k) : x0 + k] : 0.f;
  }
}

template <bool VEC>
__device__ __forceinline__ void quad_store(float* __restrict__ p, int row, int x0, bool rev, int tw, const float (&d)[4]) {
  float* r = p + (int64_t)row * tw;
  if (VEC) {
    *reinterpret_cast<float4*>(r + (rev ? tw - 4 - x0 : x0)) =
        rev ? make_float4(d[3], d[2], d[1], d[0]) : make_float4(d[0], d[1], d[2], d[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x0 + k < tw) r[rev ? tw - 1 - (x0 + k) : x0 + k] = d[k];
  }
}

// Work item = (tile, 32 x 32 block of the tile): the block's pixels are read and normalised once, every plain view of the
// mask is stored from registers, every transposing one from the LDS copy of the block (6 channels).  A block that overhangs
// the tile (th no multiple of 32) keeps its out-of-tile lanes idle on both sides of the LDS: they neither write nor read it.
template <bool VEC>
__global__ __launch_bounds__(256) void scene_gather_views_kernel(const uint8_t* __restrict__ scene, const int32_t* __restrict__ origins,
                                                                 const float* __restrict__ mean, const float* __restrict__ stdv,
                                                                 float* __restrict__ pre, float* __restrict__ post, int Hs, int Ws,
                                                                 int n, int th, int tw, int mask, int nv) {
  extern __shared__ float views_smem[];
  float* lut = views_smem;                                   // [6][256], as in scene_gather_kernel
  float* blk = views_smem + 6 * 256;                         // [6][32][33], transposing views only
  for (int i = threadIdx.x; i < 6 * 256; i += 256) {
    const int c = i >> 8;
    const float v = (float)(i & 255) / 255.0f;
    lut[i] = (v - mean[c]) / stdv[c];
  }
  __syncthreads();
  const int q = threadIdx.x & 7, r = threadIdx.x >> 3;
  const int nby = (th + kVB - 1) / kVB, nbx = (tw + kVB - 1) / kVB;
  const int64_t plane = (int64_t)th * tw;
  for (int64_t g = blockIdx.x; g < (int64_t)n * nby * nbx; g += gridDim.x) {
    const int tile = (int)(g / (nby * nbx)), b = (int)(g % (nby * nbx)), Y0 = (b / nbx) * kVB, X0 = (b % nbx) * kVB;
    const int y = Y0 + r, x0 = X0 + 4 * q;
    const bool live = y < th && x0 < tw;
    int64_t e = (int64_t)tile * nv * 3 * plane;              // entry tile * nv + j of both outputs, j counting the mask's views
    float o[6][4];
    if (live) {
      const int64_t oy = origins[2 * tile], ox = origins[2 * tile + 1];
      const uint8_t* row = scene + (int64_t)scene_fold(oy + y, Hs) * Ws * 6;
#pragma unroll
      for (int k = 0; k < 4; ++k) {                          // a column past the tile folds to a pixel of the scene: read, never stored
        const uint16_t* p = reinterpret_cast<const uint16_t*>(row + (int64_t)scene_fold(ox + x0 + k, Ws) * 6);
        const uint32_t a = p[0], bb = p[1], c = p[2];
        o[0][k] = lut[a & 255]; o[1][k] = lut[256 + (a >> 8)]; o[2][k] = lut[512 + (bb & 255)];
        o[3][k] = lut[768 + (bb >> 8)]; o[4][k] = lut[1024 + (c & 255)]; o[5][k] = lut[1280 + (c >> 8)];
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        if (!(mask >> v & 1)) continue;
        const int64_t ev = e + (int64_t)view_slot(mask, v) * 3 * plane;
        const int yo = v & 2 ? th - 1 - y : y;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          quad_store<VEC>(pre + ev + c * plane, yo, x0, v & 1, tw, o[c]);
          quad_store<VEC>(post + ev + c * plane, yo, x0, v & 1, tw, o[c + 3]);
        }
      }
    }
    if (mask >> 4) {                                         // uniform over the grid: th == tw here
      __syncthreads();                                       // the previous block's column reads are done
      if (live) {
#pragma unroll
        for (int c = 0; c < 6; ++c)
#pragma unroll
          for (int k = 0; k < 4; ++k) blk[(c * kVB + r) * kVP + 4 * q + k] = o[c][k];
      }
      __syncthreads();
      // the transposed block: T[X0 + r][Y0 + 4q + k] = A[Y0 + 4q + k][X0 + r]
      const int yt = X0 + r, xt = Y0 + 4 * q;
      if (yt < tw && xt < th) {
#pragma unroll
        for (int c = 0; c < 6; ++c)
#pragma unroll
          for (int k = 0; k < 4; ++k) o[c][k] = blk[(c * kVB + 4 * q + k) * kVP + r];   // rows past th: stale words, never stored
#pragma unroll
        for (int v = 4; v < 8; ++v) {
          if (!(mask >> v & 1)) continue;
          const int64_t ev = e + (int64_t)view_slot(mask, v) * 3 * plane;
          const int yo = v & 2 ? th - 1 - yt : yt;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            quad_store<VEC>(pre + ev + c * plane, yo, xt, v & 1, tw, o[c]);
            quad_store<VEC>(post + ev + c * plane, yo, xt, v & 1, tw, o[c + 3]);
          }
        }
      }
    }
  }
}

// Work item = (entry, channel, 32 x 32 block of the OUTPUT plane).  V_v^-1 of a plain view reads row f2(y), quad f1(x0 ..) of
// that view's plane directly; of a transposing one, A[y][x] = B[f2(x)][f1(y)]: the block B[f2(X0 + r)][f1(Y0 + 4q + k)] is
// read by rows into LDS slot s (one slot per transposing view of the mask) and summed by columns.  The sum runs in
// ascending view order from the first view's value (plain views are codes 0 .. 3, so they come first), then one divide.
template <bool VEC>
__global__ __launch_bounds__(256) void scene_fold_views_kernel(const float* __restrict__ values, float* __restrict__ dst, int cnt,
                                                               int C, int th, int tw, int mask, int nv) {
  extern __shared__ float views_smem[];                      // [popcount(mask >> 4)][32][33]
  const int q = threadIdx.x & 7, r = threadIdx.x >> 3;
  const int nby = (th + kVB - 1) / kVB, nbx = (tw + kVB - 1) / kVB;
  const int64_t plane = (int64_t)th * tw;
  const float fnv = (float)nv;
  for (int64_t g = blockIdx.x; g < (int64_t)cnt * C * nby * nbx; g += gridDim.x) {
    const int64_t ic = g / (nby * nbx);                      // entry * C + channel
    const int b = (int)(g % (nby * nbx)), Y0 = (b / nbx) * kVB, X0 = (b % nbx) * kVB;
    const int64_t i = ic / C;
    const int c = (int)(ic % C);
    const float* src = values + (i * nv * C + c) * plane;    // view j of this entry and channel: + j * C * plane
    const int y = Y0 + r, x0 = X0 + 4 * q;
    const bool live = y < th && x0 < tw;
    if (mask >> 4) {
      __syncthreads();
      const int xs = X0 + r, ys = Y0 + 4 * q;                // this lane stages A[ys + k][xs], k = 0 .. 3, of every transposing view
      if (xs < tw && ys < th) {
#pragma unroll
        for (int v = 4; v < 8; ++v) {
          if (!(mask >> v & 1)) continue;
          float d[4];
          quad_load<VEC>(src + (int64_t)view_slot(mask, v) * C * plane, v & 2 ? th - 1 - xs : xs, ys, v & 1, tw, d);
          float* s = views_smem + (view_slot(mask >> 4, v - 4) * kVB + r) * kVP + 4 * q;
#pragma unroll
          for (int k = 0; k < 4; ++k) s[k] = d[k];
        }
      }
      __syncthreads();
    }
    if (!live) continue;
    float acc[4];
    bool first = true;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (!(mask >> v & 1)) continue;
      float d[4];
      quad_load<VEC>(src + (int64_t)view_slot(mask, v) * C * plane, v & 2 ? th - 1 - y : y, x0, v & 1, tw, d);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = first ? d[k] : acc[k] + d[k];
      first = false;
    }
#pragma unroll
    for (int v = 4; v < 8; ++v) {
      if (!(mask >> v & 1)) continue;
      const float* s = views_smem + (view_slot(mask >> 4, v - 4) * kVB + 4 * q) * kVP + r;
#pragma unroll
      for (int k = 0; k < 4; ++k) {                          // words past tw: stale, never stored
        const float d = s[k * kVP];
        acc[k] = first ? d : acc[k] + d;
      }
      first = false;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = acc[k] / fnv;
    quad_store<VEC>(dst + ic * plane, y, x0, false, tw, acc);
  }
}

// margin, tile count and ring depth of one axis; false where the geometry is refused
bool scene_axis(int extent, int t, int s, int& m, int& n, int& k) {
  if (extent <= 0 || t <= 0 || s < 1 || s > t || ((t - s) & 1)) return false;
  m = (t - s) / 2;
  n = (int)(((int64_t)extent + s - 1) / s);
  k = (t + s - 1) / s;
  return true;
}

}  // namespace

extern "C" int c3d_scene_gather(const uint8_t* scene, const int32_t* origins, const float* mean6, const float* std6, float* pre,
                                float* post, int32_t Hs, int32_t Ws, int32_t n, int32_t th, int32_t tw, void* stream) {
  if (!scene || !origins || !mean6 || !std6 || !pre || !post || Hs <= 0 || Ws <= 0 || n <= 0 || th <= 0 || tw <= 0)
    return C3D_E_BADARG;
  if (reinterpret_cast<uintptr_t>(scene) & 1) return C3D_E_BADARG;   // pixels are read as three 16-bit words
  if (th > 32768 || tw > 32768) return C3D_E_UNSUPPORTED;
  const int band = 16;
  const int vec = !(tw & 3) && !((reinterpret_cast<uintptr_t>(pre) | reinterpret_cast<uintptr_t>(post)) & 15);
  int64_t grid = (int64_t)n * ((th + band - 1) / band);
  if (grid > 256 * 8) grid = 256 * 8;
  return c3d_launch_lds<scene_gather_kernel>(dim3((unsigned)grid), dim3(256), 6 * 256 * sizeof(float),
                                             reinterpret_cast<hipStream_t>(stream), scene, origins, mean6, std6, pre, post, (int)Hs,
                                             (int)Ws, (int)n, (int)th, (int)tw, band, vec);
}

extern "C" int c3d_scene_stitch(const float* ring, const float* wy, const float* wx, float* blend, uint8_t* cls,
                                const uint8_t* gate, int32_t Hs, int32_t Ws, int32_t C, int32_t th, int32_t tw, int32_t sy,
                                int32_t sx, int32_t row, void* stream) {
  if (!ring || !wy || !wx || (!blend && !cls) || (gate && !cls) || C <= 0 || C > 256) return C3D_E_BADARG;
  StitchArgs a;
  int nrows, kx;
  if (!scene_axis(Hs, th, sy, a.my, nrows, a.ky) || !scene_axis(Ws, tw, sx, a.mx, a.ncols, kx)) return C3D_E_BADARG;
  if (row < 0 || row >= nrows) return C3D_E_BADARG;
  if (th > 4096 || tw > 4096) return C3D_E_UNSUPPORTED;              // the two window vectors live in LDS
  int64_t ring_bytes = 4;                                            // factor by factor: the whole product can pass 2^63
  for (const int64_t f : {(int64_t)a.ky, (int64_t)a.ncols, (int64_t)C, (int64_t)th, (int64_t)tw}) {
    if (ring_bytes > ((1ll << 31) - 1) / f) return C3D_E_UNSUPPORTED;
    ring_bytes *= f;
  }
  a.ring = ring; a.wy = wy; a.wx = wx; a.blend = blend; a.cls = cls; a.gate = gate;
  a.Hs = Hs; a.Ws = Ws; a.C = C; a.th = th; a.tw = tw; a.sy = sy; a.sx = sx; a.row = row;
  // rows [row*sy - my, (row+1)*sy - my) are final once tile row `row` exists; the last tile row also closes the scene
  // (its centre ends at nrows*sy >= Hs, and nothing comes after it)
  a.y0 = row * sy - a.my < 0 ? 0 : row * sy - a.my;
  a.y1 = row == nrows - 1 ? Hs : ((row + 1) * sy - a.my < Hs ? (row + 1) * sy - a.my : Hs);
  if (a.y1 <= a.y0) return 0;                                        // a margin of a stride or more: nothing final yet
  a.vec_in = !(tw & 3) && !(reinterpret_cast<uintptr_t>(ring) & 15);
  a.vec_blend = !(reinterpret_cast<uintptr_t>(blend) & 15);
  a.vec_cls = !(reinterpret_cast<uintptr_t>(cls) & 3);
  int64_t grid = ((int64_t)(a.y1 - a.y0) * ((Ws + 6) >> 2) + 255) / 256;
  if (grid > 256 * 8) grid = 256 * 8;
  const size_t lds = (size_t)(((th + 3) & ~3) + ((tw + 3) & ~3)) * 4;
  return c3d_launch_lds<scene_stitch_kernel>(dim3((unsigned)grid), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), a);
}

namespace {
// C3D_E_BADARG for an empty mask, bits above 7, or a transposing view of a tile that is not square
bool views_ok(int32_t view_mask, int32_t th, int32_t tw) {
  return view_mask >= 1 && view_mask <= 255 && !((view_mask >> 4) && th != tw);
}
}  // namespace

extern "C" int c3d_scene_gather_views(const uint8_t* scene, const int32_t* origins, const float* mean6, const float* std6,
                                      float* pre, float* post, int32_t Hs, int32_t Ws, int32_t n, int32_t th, int32_t tw,
                                      int32_t view_mask, void* stream) {
  if (!scene || !origins || !mean6 || !std6 || !pre || !post || Hs <= 0 || Ws <= 0 || n <= 0 || th <= 0 || tw <= 0)
    return C3D_E_BADARG;
  if (reinterpret_cast<uintptr_t>(scene) & 1) return C3D_E_BADARG;
  if (!views_ok(view_mask, th, tw)) return C3D_E_BADARG;
  if (th > 32768 || tw > 32768) return C3D_E_UNSUPPORTED;
  const int nv = __builtin_popcount((unsigned)view_mask);
  const bool vec = !(tw & 3) && !((reinterpret_cast<uintptr_t>(pre) | reinterpret_cast<uintptr_t>(post)) & 15);
  int64_t grid = (int64_t)n * ((th + kVB - 1) / kVB) * ((tw + kVB - 1) / kVB);
  if (grid > 256 * 8) grid = 256 * 8;
  const size_t lds = (size_t)(6 * 256 + ((view_mask >> 4) ? 6 * kVB * kVP : 0)) * sizeof(float);
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return vec ? c3d_launch_lds<scene_gather_views_kernel<true>>(dim3((unsigned)grid), dim3(256), lds, st, scene, origins, mean6, std6,
                                                               pre, post, (int)Hs, (int)Ws, (int)n, (int)th, (int)tw,
                                                               (int)view_mask, nv)
             : c3d_launch_lds<scene_gather_views_kernel<false>>(dim3((unsigned)grid), dim3(256), lds, st, scene, origins, mean6,
                                                                std6, pre, post, (int)Hs, (int)Ws, (int)n, (int)th, (int)tw,
                                                                (int)view_mask, nv);
}

extern "C" int c3d_scene_fold_views(const float* values, float* dst, int32_t cnt, int32_t C, int32_t th, int32_t tw,
                                    int32_t view_mask, void* stream) {
  if (!values || !dst || cnt <= 0 || C <= 0 || th <= 0 || tw <= 0) return C3D_E_BADARG;
  if (!views_ok(view_mask, th, tw)) return C3D_E_BADARG;
  if (th > 32768 || tw > 32768) return C3D_E_UNSUPPORTED;
  const int nv = __builtin_popcount((unsigned)view_mask), nt = __builtin_popcount((unsigned)view_mask >> 4);
  const bool vec = !(tw & 3) && !((reinterpret_cast<uintptr_t>(values) | reinterpret_cast<uintptr_t>(dst)) & 15);
  int64_t grid = (int64_t)cnt * C * ((th + kVB - 1) / kVB) * ((tw + kVB - 1) / kVB);
  if (grid > 256 * 8) grid = 256 * 8;
  const size_t lds = (size_t)(nt ? nt : 1) * kVB * kVP * sizeof(float);
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return vec ? c3d_launch_lds<scene_fold_views_kernel<true>>(dim3((unsigned)grid), dim3(256), lds, st, values, dst, (int)cnt, (int)C,
                                                             (int)th, (int)tw, (int)view_mask, nv)
             : c3d_launch_lds<scene_fold_views_kernel<false>>(dim3((unsigned)grid), dim3(256), lds, st, values, dst, (int)cnt,
                                                              (int)C, (int)th, (int)tw, (int)view_mask, nv);
}
