// Objects of a whole-scene map (change3d_amd/infer.py, predict(objects=True)): connected-component labelling of a u8 mask
// that stays in HBM, a minimum-area filter, raster numbering, and one row of statistics per object (area, inclusive box,
// majority class of a class map, mean score).  The reference has no counterpart: xBD's per-building majority vote is done
// on the host there, after a download.  All arithmetic is integer: every output is exact and two runs agree bit for bit.
//
// Union-find over linear pixel indices.  The invariant of every phase: a foreground pixel's parent is a pixel of the same
// component with an index <= its own, so a tree's root is the smallest index it holds, parents only ever decrease
// (atomicMin), and every walk towards a root ends.  Every walk and every union loop is ALSO capped at Hs*Ws steps; a loop
// that reaches the cap sets the error word of the workspace, which c3d_scene_objects folds into counts[0] = -1.  No loop
// waits for another workgroup: phases are separate launches on one stream, there is no grid barrier.
//
//   1 label_local    one workgroup per 64 x 64 tile, the i32 tile in LDS (16 KB).  A wave owns a row: the ballot of the row's
//                    foreground gives every pixel the start of its run as first parent.  Then each pixel unites with its
//                    backward neighbours in the row above (LDS atomicMin), skipping the edges that its left neighbour's
//                    edges already imply, and writes the GLOBAL index of its tile-local root.
//   2 label_seam     one thread per pixel of a tile's first row / first column unites across the seam in global memory.
//   3 label_flatten  every pixel gets its root; area per root with u32 atomics, pre-aggregated per wave.
//   4 count_roots    kept roots (area >= min_area) per chunk of 1024 pixels,
//   5 scan_chunks    exclusive scan of the chunk counts by one workgroup,
//   6 number_roots   id = chunk offset + rank in the chunk + 1: raster order of the first pixel, no tickets; writes the
//                    table row's area / first and the empty box, and replaces the root's area by its id.
//   7 relabel_stats  labels = id of the root; box (atomicMin / atomicMax), votes (u32) and score sum (u64 of 16-bit fixed
//                    point) per object, pre-aggregated where a wave's objects pixels share one id.
//   8 finalise       majority class (lowest index wins a tie), score_q, counts.
//   9 paint          object_cls.
//
// Which edges are united.  A row run inside a tile is united by construction.  For pixel p with left neighbour l, upper
// neighbours ul, u, ur, where l only counts when it lies in p's tile column (x % 64 != 0):
//   4-connectivity: p-u unless l and ul are foreground (then l-ul, united earlier or implied, and the two runs join them);
//   8-connectivity: u foreground: p-u unless l is foreground (u is l's upper right); otherwise p-ul unless l is foreground
//                   (ul is l's upper neighbour), and p-ur always.
// Rows y % 64 == 0 get these edges from label_seam, the others from label_local.  A row edge across a tile column (x % 64
// == 0) is united by label_seam unless u and ul are foreground (p-u is never skipped in that column, u-ul is the same seam
// one row up, ul-l is an edge of l); with 8-connectivity the two diagonals across the column are united unless a third
// foreground pixel of the 2 x 2 block joins them.  Each skipped edge is implied by edges whose later end point comes
// earlier in raster order, or by p's own vertical edge, which that column never skips: the induction is well founded.
#include <climits>

#include "scene_wave.h"
#include "scene_detail.h"
#include "../../include/change3d_hip.h"

namespace {

using namespace c3d_wave;

constexpr int TH = 64, TW = 64;                            // tile of the local phase: a wave is a row
static_assert(TH * TW == C3D_DETAIL_TILE, "the walks of scene_detail.h are capped by the tile");
constexpr int CHUNK = 1024;                                // pixels per chunk of the numbering scan
constexpr int MAX_GRID = 256 * 8;

enum { WS_ERR = 0, WS_FOUND = 1 };                         // words of the workspace header

struct Workspace {
  int64_t area, chunks, ssum, hist, bytes;                 // byte offsets; `area` [N] u32 becomes the id per root
  int64_t n_chunks, cap;                                   // cap = most objects a scene can hold = ceil(N / 2)
};

Workspace workspace_plan(int64_t N, int n_cls) {
  Workspace w;
  auto up = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  w.n_chunks = (N + CHUNK - 1) / CHUNK;
  w.cap = (N + 1) / 2;
  w.area = 256;
  w.chunks = w.area + up(N * 4);
  w.ssum = w.chunks + up(w.n_chunks * 4);
  w.hist = w.ssum + up(w.cap * 8);
  w.bytes = w.hist + up(w.cap * 4 * n_cls);
  return w;
}

__global__ __launch_bounds__(256) void label_local_kernel(const uint8_t* __restrict__ mask, int32_t* __restrict__ L,
                                                          uint32_t* __restrict__ err, int Hs, int Ws, int tiles_x, int n_tiles,
                                                          int conn8) {
  extern __shared__ int32_t lab[];                         // [TH][TW]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int ty0 = (tile / tiles_x) * TH, tx0 = (tile % tiles_x) * TW;
    const int gx = tx0 + lane;
    for (int y = wave; y < TH; y += 4) {
      const int gy = ty0 + y;
      const bool fg = gy < Hs && gx < Ws && mask[(int64_t)gy * Ws + gx] != 0;
      const unsigned long long gaps = ~__ballot(fg) & ((1ull << lane) - 1ull);   // background pixels left of this lane
      const int start = gaps ? 64 - __clzll((long long)gaps) : 0;
      lab[y * TW + lane] = fg ? y * TW + start : -1;
    }
    __syncthreads();
    for (int y = wave ? wave : 4; y < TH; y += 4) {        // row 0 has no row above it in the tile
      const int p = y * TW + lane;
      if (ld_wg(lab + p) < 0) continue;                    // the sign of an entry never changes
      const bool l = lane > 0 && ld_wg(lab + p - 1) >= 0, u = ld_wg(lab + p - TW) >= 0;
      const bool ul = lane > 0 && ld_wg(lab + p - TW - 1) >= 0, ur = lane < TW - 1 && ld_wg(lab + p - TW + 1) >= 0;
      if (conn8) {
        if (u) {
          if (!l) lds_unite(lab, p, p - TW, err);
        } else {
          if (ul && !l) lds_unite(lab, p, p - TW - 1, err);
          if (ur) lds_unite(lab, p, p - TW + 1, err);
        }
      } else if (u && !(l && ul)) {
        lds_unite(lab, p, p - TW, err);
      }
    }
    __syncthreads();
    for (int y = wave; y < TH; y += 4) {
      const int gy = ty0 + y;
      if (gy >= Hs || gx >= Ws) continue;
      const int p = y * TW + lane;
      int r = -1;
      if (lab[p] >= 0) {
        r = lds_find(lab, p, err);
        r = (ty0 + r / TW) * Ws + tx0 + r % TW;            // < Hs * Ws < 2^31: the root is a foreground pixel of the scene
      }
      L[(int64_t)gy * Ws + gx] = r;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void label_seam_kernel(const uint8_t* __restrict__ mask, int32_t* __restrict__ L,
                                                         uint32_t* __restrict__ err, int Hs, int Ws, int64_t row_items,
                                                         int64_t items, int cap, int conn8) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    if (it < row_items) {                                  // pixel (y, x) of a tile's first row, y >= TH
      const int x = (int)(it % Ws), y = ((int)(it / Ws) + 1) * TH;
      const int p = y * Ws + x;
      if (!mask[p]) continue;
      const bool l = (x % TW) != 0 && mask[p - 1], u = mask[p - Ws];
      const bool ul = x > 0 && mask[p - Ws - 1], ur = x < Ws - 1 && mask[p - Ws + 1];
      if (conn8) {
        if (u) {
          if (!l) g_unite(L, p, p - Ws, cap, err);
        } else {
          if (ul && !l) g_unite(L, p, p - Ws - 1, cap, err);
          if (ur) g_unite(L, p, p - Ws + 1, cap, err);
        }
      } else if (u && !(l && ul)) {
        g_unite(L, p, p - Ws, cap, err);
      }
    } else {                                               // pixel (y, x) of a tile's first column, x >= TW
      const int64_t j = it - row_items;
      const int y = (int)(j % Hs), x = ((int)(j / Hs) + 1) * TW;
      const int p = y * Ws + x;
      const bool c = mask[p], l = mask[p - 1], u = y > 0 && mask[p - Ws], ul = y > 0 && mask[p - Ws - 1];
      if (c && l && !(u && ul)) g_unite(L, p, p - 1, cap, err);
      if (conn8) {
        if (c && ul && !l && !u) g_unite(L, p, p - Ws - 1, cap, err);
        if (l && u && !c && !ul) g_unite(L, p - 1, p - Ws, cap, err);
      }
    }
  }
}

// Every pixel gets its root; the areas per root through c3d_detail_wave_area_add (scene_detail.h).  AREA = false only
// flattens (csrc/scene_split.hip counts the areas of its pieces itself).
template <bool AREA>
__global__ __launch_bounds__(256) void label_flatten_kernel(int32_t* __restrict__ L, uint32_t* __restrict__ area,
                                                            uint32_t* __restrict__ err, int N, int cap) {
  for (int64_t base = (int64_t)blockIdx.x * 256; base < N; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    int r = -1;
    if (i < N) {
      const int p = ld_agent(L + i);
      if (p >= 0) {
        r = g_find(L, p, cap, err);                        // other threads flatten the same trees meanwhile: every value
        if (r != p) __hip_atomic_store(L + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ever stored is an ancestor
      }
    }
    if (AREA) c3d_detail_wave_area_add(area, r);
  }
}

__device__ __forceinline__ bool kept_root(const int32_t* L, const uint32_t* area, int64_t i, int N, uint32_t min_area) {
  return i < N && L[i] == (int32_t)i && area[i] >= min_area;
}

__global__ __launch_bounds__(256) void count_roots_kernel(const int32_t* __restrict__ L, const uint32_t* __restrict__ area,
                                                          uint32_t* __restrict__ chunks, int N, int64_t n_chunks,
                                                          uint32_t min_area) {
  extern __shared__ uint32_t part[];                       // [4]; dynamic: c3d_launch_lds refuses a static array
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    uint32_t n = 0;
    for (int k = 0; k < CHUNK / 256; ++k)
      n += (uint32_t)__popcll(__ballot(kept_root(L, area, c * CHUNK + k * 256 + threadIdx.x, N, min_area)));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) chunks[c] = part[0] + part[1] + part[2] + part[3];
    __syncthreads();
  }
}

// in place: chunks[c] = kept roots before chunk c; header[WS_FOUND] = all of them.  One workgroup.
__global__ __launch_bounds__(256) void scan_chunks_kernel(uint32_t* __restrict__ chunks, uint32_t* __restrict__ header,
                                                          int64_t n_chunks) {
  extern __shared__ uint32_t s[];                          // [256]
  uint32_t running = 0;
  for (int64_t base = 0; base < n_chunks; base += 256) {
    const int64_t c = base + threadIdx.x;
    const uint32_t v = c < n_chunks ? chunks[c] : 0u;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const uint32_t add = threadIdx.x >= d ? s[threadIdx.x - d] : 0u;
      __syncthreads();
      s[threadIdx.x] += add;
      __syncthreads();
    }
    if (c < n_chunks) chunks[c] = running + s[threadIdx.x] - v;
    running += s[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) header[WS_FOUND] = running;
}

__global__ __launch_bounds__(256) void number_roots_kernel(const int32_t* __restrict__ L, uint32_t* __restrict__ area,
                                                           const uint32_t* __restrict__ chunks, int32_t* __restrict__ table,
                                                           int N, int64_t n_chunks, uint32_t min_area, int max_objects) {
  extern __shared__ uint32_t part[];                       // [4]; dynamic: c3d_launch_lds refuses a static array
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    uint32_t run = chunks[c];
    for (int k = 0; k < CHUNK / 256; ++k) {
      const int64_t i = c * CHUNK + k * 256 + threadIdx.x;
      const bool root = i < N && L[i] == (int32_t)i;
      const uint32_t a = root ? area[i] : 0u;
      const bool keep = root && a >= min_area;
      const unsigned long long b = __ballot(keep);
      if (lane == 0) part[wave] = (uint32_t)__popcll(b);
      __syncthreads();
      uint32_t before = 0, all = 0;
      for (int w = 0; w < 4; ++w) {
        before += w < wave ? part[w] : 0u;
        all += part[w];
      }
      if (root) {
        const uint32_t id = keep ? run + before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull)) + 1u : 0u;
        area[i] = id;                                      // from here on this word is the root's id (0: removed)
        if (id && id <= (uint32_t)max_objects) {
          int32_t* row = table + (int64_t)(id - 1) * 8;
          row[0] = (int32_t)a; row[1] = INT_MAX; row[2] = INT_MAX; row[3] = -1; row[4] = -1; row[5] = 0; row[6] = (int32_t)i; row[7] = 0;
        }
      }
      run += all;
      __syncthreads();
    }
  }
}


// 16-bit fixed point of a probability: NaN and negatives count as 0 (fmaxf returns the operand that is a number)
__device__ __forceinline__ uint32_t score_fixed(float p) { return __float2uint_rn(fminf(fmaxf(p, 0.0f), 1.0f) * 65535.0f); }

__global__ __launch_bounds__(256) void relabel_stats_kernel(int32_t* __restrict__ L, const uint32_t* __restrict__ ids,
                                                            const uint8_t* __restrict__ cls_map, const float* __restrict__ score,
                                                            int32_t* __restrict__ table, uint32_t* __restrict__ hist,
                                                            unsigned long long* __restrict__ ssum, int N, int Ws, int n_cls,
                                                            int max_objects) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < N; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    int id = 0;
    if (i < N) {
      const int r = L[i];                                  // the root since label_flatten; only this thread touches L[i]
      id = r >= 0 ? (int)ids[r] : 0;
      L[i] = id;
    }
    const bool in = id >= 1 && id <= max_objects;          // a pixel of an object that has a table row
    const int x = in ? (int)(i % Ws) : 0, y = in ? (int)(i / Ws) : 0;
    const int c = in && cls_map ? cls_map[i] : 255;
    const uint32_t q = in && score ? score_fixed(score[i]) : 0u;
    const unsigned long long m = __ballot(in);
    if (!m) continue;
    const int id0 = __shfl(id, __ffsll((long long)m) - 1);
    if (__ballot(in && id != id0) == 0) {                  // one object in this wave: reduce first, one lane does the atomics
      const int x0 = wave_min32(in ? x : INT_MAX), y0 = wave_min32(in ? y : INT_MAX);
      const int x1 = wave_max32(in ? x : -1), y1 = wave_max32(in ? y : -1);
      const uint32_t qs = wave_sum32(q);                   // <= 64 * 65535
      int32_t* row = table + (int64_t)(id0 - 1) * 8;
      if (lane == 0) {
        atomicMin(row + 1, x0); atomicMin(row + 2, y0); atomicMax(row + 3, x1); atomicMax(row + 4, y1);
        if (score) atomicAdd(ssum + (id0 - 1), (unsigned long long)qs);
      }
      if (cls_map) {
        for (int k = 0; k < n_cls; ++k) {
          const unsigned long long v = __ballot(c == k);
          if (lane == 0 && v) atomicAdd(hist + (int64_t)(id0 - 1) * n_cls + k, (uint32_t)__popcll(v));
        }
      }
    } else if (in) {
      int32_t* row = table + (int64_t)(id - 1) * 8;
      atomicMin(row + 1, x); atomicMin(row + 2, y); atomicMax(row + 3, x); atomicMax(row + 4, y);
      if (score) atomicAdd(ssum + (id - 1), (unsigned long long)q);
      if (c < n_cls) atomicAdd(hist + (int64_t)(id - 1) * n_cls + c, 1u);
    }
  }
}

__global__ __launch_bounds__(256) void finalise_kernel(int32_t* __restrict__ table, const uint32_t* __restrict__ hist,
                                                       const unsigned long long* __restrict__ ssum,
                                                       const uint32_t* __restrict__ header, int32_t* __restrict__ counts,
                                                       int n_cls, int first_class, int max_objects, int has_cls, int has_score) {
  const uint32_t found = header[WS_FOUND];
  const int rows = found < (uint32_t)max_objects ? (int)found : max_objects;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    counts[0] = header[WS_ERR] ? -1 : (int32_t)found;
    counts[1] = rows;
  }
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < max_objects; k += (int64_t)gridDim.x * 256) {
    int32_t* row = table + k * 8;
    if (k >= rows) {                                       // no object owns this row: nothing has written it yet
      for (int j = 0; j < 8; ++j) row[j] = 0;
      continue;
    }
    if (has_cls) {
      uint32_t best = 0;
      int arg = 0;
      for (int c = first_class; c < n_cls; ++c) {
        const uint32_t v = hist[k * n_cls + c];
        if (v > best) { best = v; arg = c; }               // strict: the lowest class wins a tie; no vote: 0
      }
      row[5] = arg;
    }
    if (has_score) {
      const unsigned long long a = (unsigned long long)(uint32_t)row[0];
      row[7] = (int32_t)((ssum[k] + a / 2) / a);           // a >= 1 for a numbered object; the mean is <= 65535
    }
  }
}

__global__ __launch_bounds__(256) void paint_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ table,
                                                    uint8_t* __restrict__ object_cls, int N, int max_objects) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
    const int id = labels[i];
    object_cls[i] = id >= 1 && id <= max_objects ? (uint8_t)table[(int64_t)(id - 1) * 8 + 5] : (uint8_t)0;
  }
}

unsigned grid_for(int64_t items, int per_block) {
  int64_t g = (items + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > MAX_GRID ? MAX_GRID : g));
}

}  // namespace

extern "C" int64_t c3d_scene_label_ws_bytes(int32_t Hs, int32_t Ws, int32_t n_cls) {
  if (Hs <= 0 || Ws <= 0 || n_cls < 1 || n_cls > 16) return C3D_E_BADARG;
  if ((int64_t)Hs * Ws >= (1ll << 31)) return C3D_E_UNSUPPORTED;
  return workspace_plan((int64_t)Hs * Ws, n_cls).bytes;
}

extern "C" int c3d_scene_label_tile(int32_t* th, int32_t* tw) {
  if (!th || !tw) return C3D_E_BADARG;
  *th = TH;
  *tw = TW;
  return 0;
}

// ---- the stages as host functions (scene_detail.h): c3d_scene_objects below, and csrc/scene_split.hip
int64_t c3d_detail_label_ws_bytes(int64_t N, int n_cls) { return workspace_plan(N, n_cls).bytes; }
int64_t c3d_detail_area_offset() { return workspace_plan(1, 1).area; }
int64_t c3d_detail_ssum_offset(int64_t N) { return workspace_plan(N, 1).ssum; }

// header and area; the sums and votes of the rows that can be used.  The table needs none: number_roots writes the rows of
// the objects, finalise zeroes the others.
int c3d_detail_objects_clear(void* ws, int64_t N, const uint8_t* cls_map, const float* score, int n_cls, uint32_t* hist,
                             int max_objects, hipStream_t st) {
  if (!cls_map) { n_cls = 1; hist = nullptr; }
  const Workspace w = workspace_plan(N, n_cls);
  char* base = static_cast<char*>(ws);
  const int64_t rows_cap = max_objects < w.cap ? max_objects : w.cap;   // no id with a table row can be larger
  uint32_t* votes = hist ? hist : reinterpret_cast<uint32_t*>(base + w.hist);
  hipError_t e = hipMemsetAsync(base, 0, (size_t)(w.chunks), st);
  if (e == hipSuccess && score) e = hipMemsetAsync(base + w.ssum, 0, (size_t)rows_cap * 8, st);
  if (e == hipSuccess && cls_map) e = hipMemsetAsync(votes, 0, (size_t)(hist ? (int64_t)max_objects : rows_cap) * n_cls * 4, st);
  return (int)e;
}

int c3d_detail_label_roots(const uint8_t* mask, int32_t* L, uint32_t* err, uint32_t* area, int Hs, int Ws, int conn8, int phases,
                           hipStream_t st) {
  const int N = Hs * Ws;
  const int tiles_x = (Ws + TW - 1) / TW, tiles_y = (Hs + TH - 1) / TH;
  const int n_tiles = tiles_x * tiles_y;                   // <= N / 4096 + ...: far below 2^31
  int rc = c3d_launch_lds<label_local_kernel>(dim3((unsigned)(n_tiles > 65536 ? 65536 : n_tiles)), dim3(256), TH * TW * 4, st,
                                              mask, L, err, Hs, Ws, tiles_x, n_tiles, conn8);
  if (rc || phases == 1) return rc;
  const int64_t row_items = (int64_t)(tiles_y - 1) * Ws, items = row_items + (int64_t)(tiles_x - 1) * Hs;
  if (items > 0) {
    rc = c3d_launch_lds<label_seam_kernel>(dim3(grid_for(items, 256)), dim3(256), 0, st, mask, L, err, Hs, Ws, row_items, items, N,
                                           conn8);
    if (rc) return rc;
  }
  if (phases == 2) return 0;
  if (area) return c3d_launch_lds<label_flatten_kernel<true>>(dim3(grid_for(N, 256)), dim3(256), 0, st, L, area, err, N, N);
  return c3d_launch_lds<label_flatten_kernel<false>>(dim3(grid_for(N, 256)), dim3(256), 0, st, L, area, err, N, N);
}

int c3d_detail_label_flatten(int32_t* L, uint32_t* err, uint32_t* area, int N, hipStream_t st) {
  return c3d_launch_lds<label_flatten_kernel<true>>(dim3(grid_for(N, 256)), dim3(256), 0, st, L, area, err, N, N);
}

int c3d_detail_objects_tail(const uint8_t* cls_map, const float* score, int Hs, int Ws, int min_area, int n_cls, int first_class,
                            int max_objects, int32_t* labels, int32_t* table, uint32_t* hist, uint8_t* object_cls, int32_t* counts,
                            void* ws, int phases, hipStream_t st) {
  if (!cls_map) { n_cls = 1; hist = nullptr; }            // no class map, no votes: `hist` is left alone
  const int N = Hs * Ws;
  const Workspace w = workspace_plan(N, n_cls);
  char* base = static_cast<char*>(ws);
  uint32_t* header = reinterpret_cast<uint32_t*>(base);
  uint32_t* area = reinterpret_cast<uint32_t*>(base + w.area);
  uint32_t* chunks = reinterpret_cast<uint32_t*>(base + w.chunks);
  unsigned long long* ssum = reinterpret_cast<unsigned long long*>(base + w.ssum);
  uint32_t* votes = hist ? hist : reinterpret_cast<uint32_t*>(base + w.hist);
  const uint32_t min_a = min_area < 1 ? 1u : (uint32_t)min_area;
  int rc = c3d_launch_lds<count_roots_kernel>(dim3(grid_for(w.n_chunks, 1)), dim3(256), 16, st, (const int32_t*)labels,
                                              (const uint32_t*)area, chunks, N, w.n_chunks, min_a);
  if (rc || phases == 4) return rc;
  rc = c3d_launch_lds<scan_chunks_kernel>(dim3(1), dim3(256), 1024, st, chunks, header, w.n_chunks);
  if (rc || phases == 5) return rc;
  rc = c3d_launch_lds<number_roots_kernel>(dim3(grid_for(w.n_chunks, 1)), dim3(256), 16, st, (const int32_t*)labels, area,
                                           (const uint32_t*)chunks, table, N, w.n_chunks, min_a, max_objects);
  if (rc || phases == 6) return rc;
  rc = c3d_launch_lds<relabel_stats_kernel>(dim3(grid_for(N, 256)), dim3(256), 0, st, labels, (const uint32_t*)area, cls_map,
                                            score, table, votes, ssum, N, Ws, n_cls, max_objects);
  if (rc || phases == 7) return rc;
  rc = c3d_launch_lds<finalise_kernel>(dim3(grid_for(max_objects, 256)), dim3(256), 0, st, table, (const uint32_t*)votes,
                                       (const unsigned long long*)ssum, (const uint32_t*)header, counts, n_cls, first_class,
                                       max_objects, cls_map ? 1 : 0, score ? 1 : 0);
  if (rc || phases == 8) return rc;
  if (object_cls)
    rc = c3d_launch_lds<paint_kernel>(dim3(grid_for(N, 256)), dim3(256), 0, st, (const int32_t*)labels, (const int32_t*)table,
                                      object_cls, N, max_objects);
  return rc;
}

extern "C" int c3d_scene_objects(const uint8_t* mask, const uint8_t* cls_map, const float* score, int32_t Hs, int32_t Ws,
                                 int32_t connectivity, int32_t min_area, int32_t n_cls, int32_t first_class, int32_t max_objects,
                                 int32_t* labels, int32_t* table, uint32_t* hist, uint8_t* object_cls, int32_t* counts, void* ws,
                                 void* stream) {
  if (!mask || !labels || !table || !counts || !ws || Hs <= 0 || Ws <= 0 || max_objects < 1 || first_class < 0) return C3D_E_BADARG;
  if (connectivity != 4 && connectivity != 8) return C3D_E_BADARG;
  if ((int64_t)Hs * Ws >= (1ll << 31)) return C3D_E_UNSUPPORTED;
  if (cls_map && (n_cls < 1 || n_cls > 16)) return C3D_E_BADARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint32_t* header = static_cast<uint32_t*>(ws);
  uint32_t* area = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + c3d_detail_area_offset());

  // instrumented build only (common.h c3d_knob): tools/objects_step.py times prefixes of the nine launches.  The product
  // library compiles this to 9, and every `phases == k` in the stages to false.
  const int phases = c3d_knob("C3D_OBJECTS_PHASES", 9);

  int rc = c3d_detail_objects_clear(ws, (int64_t)Hs * Ws, cls_map, score, n_cls, hist, max_objects, st);
  if (rc) return rc;
  rc = c3d_detail_label_roots(mask, labels, header + WS_ERR, area, Hs, Ws, connectivity == 8, phases, st);
  if (rc || phases <= 3) return rc;
  return c3d_detail_objects_tail(cls_map, score, Hs, Ws, min_area, n_cls, first_class, max_objects, labels, table, hist, object_cls,
                                 counts, ws, phases, st);
}
