// Class regions of a scene map (change3d_amd/infer.py, predict(objects=True, regions=..)): the connected components of EQUAL
// nonzero key of a u8 key map that stays in HBM -- scipy.ndimage.label(key == k) for every k, taken together -- numbered in
// raster order of their first pixel over all keys, with the table of c3d_scene_objects and the key as the exact class.
// The reference has no counterpart.  All arithmetic is integer: every output is exact and two runs agree bit for bit.
//
// The union-find of csrc/scene_objects.hip with "foreground" read as "has my key".  For a pixel of key k every test below is
// the binary one on the mask (key == k), the edges it unites join pixels of that mask only, and the masks of different keys
// share no pixel: the argument of scene_objects.hip holds for each k on its own, and so does its invariant (a pixel's parent
// is a pixel of the same region with an index <= its own; parents only decrease; every walk is also capped at Hs*Ws steps and
// sets the error word at the cap).
//
//   1 region_local    one workgroup per 64 x 64 tile; the i32 tile and the u8 keys in LDS (20 KB).  A wave owns a row: a run
//                     starts where the key differs from the left neighbour's (the ballot of that, highest start at or below
//                     the lane), then each pixel unites with the backward neighbours of its key in the row above, with the
//                     skips of label_local under key equality, and writes the GLOBAL index of its tile-local root.
//   2 region_seam     one thread per pixel of a tile's first row / first column unites across the seam in global memory.
//   3 flatten         c3d_detail_label_flatten (the kernel of scene_objects.hip), or its gated twin for the sieve's rounds.
//   4..8              c3d_detail_objects_tail without a class map (count, scan, number, relabel_stats, finalise).
//   9 region_keys     table column 5 = the key at the region's first pixel; object_key.
//
// At connectivity 8 two regions of different keys may cross at a lattice point (A B / B A): each diagonal is an edge of its
// own key's mask, and both are united.
#include "common.h"
#include "scene_detail.h"
#include "../../include/change3d_hip.h"

namespace {

constexpr int TH = 64, TW = 64;                            // tile of the local phase: a wave is a row
static_assert(TH * TW == C3D_DETAIL_TILE, "the walks of scene_detail.h are capped by the tile");
constexpr int LOCAL_LDS = TH * TW * 4 + TH * TW;           // parents, then keys

__global__ __launch_bounds__(256) void region_local_kernel(const uint8_t* __restrict__ key, int32_t* __restrict__ L,
                                                           uint32_t* __restrict__ err, const uint32_t* __restrict__ stop, int Hs,
                                                           int Ws, int tiles_x, int n_tiles, int conn8) {
  extern __shared__ int32_t lab[];                         // [TH][TW]
  uint8_t* kk = reinterpret_cast<uint8_t*>(lab + TH * TW); // [TH][TW]
  if (stop && *stop) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int ty0 = (tile / tiles_x) * TH, tx0 = (tile % tiles_x) * TW;
    const int gx = tx0 + lane;
    for (int y = wave; y < TH; y += 4) {
      const int gy = ty0 + y;
      const int k = gy < Hs && gx < Ws ? (int)key[(int64_t)gy * Ws + gx] : 0;   // outside the scene: background
      kk[y * TW + lane] = (uint8_t)k;
      const int left = __shfl_up(k, 1);
      const unsigned long long below = lane == 63 ? ~0ull : (2ull << lane) - 1ull;   // lanes 0 .. lane
      const unsigned long long starts = __ballot(lane == 0 || left != k) & below;    // lane 0 is always a start
      lab[y * TW + lane] = k ? y * TW + 63 - __clzll((long long)starts) : -1;
    }
    __syncthreads();
    for (int y = wave ? wave : 4; y < TH; y += 4) {        // row 0 has no row above it in the tile
      const int p = y * TW + lane;
      const int k = kk[p];
      if (!k) continue;
      const bool l = lane > 0 && kk[p - 1] == k, u = kk[p - TW] == k;
      const bool ul = lane > 0 && kk[p - TW - 1] == k, ur = lane < TW - 1 && kk[p - TW + 1] == k;
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
      if (kk[p]) {
        r = lds_find(lab, p, err);
        r = (ty0 + r / TW) * Ws + tx0 + r % TW;            // < Hs * Ws < 2^31: the root is a pixel of the scene
      }
      L[(int64_t)gy * Ws + gx] = r;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void region_seam_kernel(const uint8_t* __restrict__ key, int32_t* __restrict__ L,
                                                          uint32_t* __restrict__ err, const uint32_t* __restrict__ stop, int Hs,
                                                          int Ws, int64_t row_items, int64_t items, int cap, int conn8) {
  if (stop && *stop) return;
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    if (it < row_items) {                                  // pixel (y, x) of a tile's first row, y >= TH
      const int x = (int)(it % Ws), y = ((int)(it / Ws) + 1) * TH;
      const int p = y * Ws + x;
      const int k = key[p];
      if (!k) continue;
      const bool l = (x % TW) != 0 && key[p - 1] == k, u = key[p - Ws] == k;
      const bool ul = x > 0 && key[p - Ws - 1] == k, ur = x < Ws - 1 && key[p - Ws + 1] == k;
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
      const int c = key[p], l = key[p - 1], u = y > 0 ? (int)key[p - Ws] : 0, ul = y > 0 ? (int)key[p - Ws - 1] : 0;
      if (c && l == c && !(u == c && ul == c)) g_unite(L, p, p - 1, cap, err);
      if (conn8) {
        if (c && ul == c && l != c && u != c) g_unite(L, p, p - Ws - 1, cap, err);
        if (l && u == l && c != l && ul != l) g_unite(L, p - 1, p - Ws, cap, err);
      }
    }
  }
}

// label_flatten_kernel<true> of scene_objects.hip behind the stop word
__global__ __launch_bounds__(256) void region_flatten_gated_kernel(int32_t* __restrict__ L, uint32_t* __restrict__ area,
                                                                   uint32_t* __restrict__ err, const uint32_t* __restrict__ stop,
                                                                   int N) {
  if (*stop) return;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < N; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    int r = -1;
    if (i < N) {
      const int p = ld_agent(L + i);
      if (p >= 0) {
        r = g_find(L, p, N, err);
        if (r != p) __hip_atomic_store(L + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // every value stored is an ancestor
      }
    }
    c3d_detail_wave_area_add(area, r);
  }
}

__global__ __launch_bounds__(256) void region_keys_kernel(const uint8_t* __restrict__ key, const int32_t* __restrict__ labels,
                                                          int32_t* __restrict__ table, const int32_t* __restrict__ counts,
                                                          uint8_t* __restrict__ object_key, int N, int max_objects) {
  const int c = counts[1];
  const int rows = c < 0 ? 0 : (c > max_objects ? max_objects : c);
  const int64_t items = N > rows ? N : rows;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (int64_t)gridDim.x * 256) {
    if (object_key && i < N) object_key[i] = labels[i] > 0 ? key[i] : (uint8_t)0;
    if (i < rows) {
      const int first = table[i * 8 + 6];
      table[i * 8 + 5] = first >= 0 && first < N ? (int32_t)key[first] : 0;
    }
  }
}

unsigned grid_cus(int64_t items, int per_block) {
  static const int cus = c3d_device_cus();
  const int64_t most = (int64_t)(cus > 0 ? cus : 256) * 8;
  const int64_t g = (items + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > most ? most : g));
}

}  // namespace

int c3d_detail_region_roots(const uint8_t* key, int32_t* L, uint32_t* err, uint32_t* area, int Hs, int Ws, int conn8,
                            const uint32_t* stop, hipStream_t st) {
  const int N = Hs * Ws;
  const int tiles_x = (Ws + TW - 1) / TW, tiles_y = (Hs + TH - 1) / TH;
  const int n_tiles = tiles_x * tiles_y;
  int rc = c3d_launch_lds<region_local_kernel>(dim3((unsigned)(n_tiles > 65536 ? 65536 : n_tiles)), dim3(256), LOCAL_LDS, st, key, L,
                                               err, stop, Hs, Ws, tiles_x, n_tiles, conn8);
  if (rc) return rc;
  const int64_t row_items = (int64_t)(tiles_y - 1) * Ws, items = row_items + (int64_t)(tiles_x - 1) * Hs;
  if (items > 0) {
    rc = c3d_launch_lds<region_seam_kernel>(dim3(grid_cus(items, 256)), dim3(256), 0, st, key, L, err, stop, Hs, Ws, row_items,
                                            items, N, conn8);
    if (rc) return rc;
  }
  if (!stop) return c3d_detail_label_flatten(L, err, area, N, st);
  return c3d_launch_lds<region_flatten_gated_kernel>(dim3(grid_cus(N, 256)), dim3(256), 0, st, L, area, err, stop, N);
}

// the score sums start where the label workspace has them and run over its votes (unused without a class map) to N rows
int64_t c3d_detail_region_ws_bytes(int64_t N) {
  const int64_t plain = c3d_detail_label_ws_bytes(N, 1), sums = c3d_detail_ssum_offset(N) + ((N * 8 + 255) & ~(int64_t)255);
  return plain > sums ? plain : sums;
}

int c3d_detail_region_clear(void* ws, int64_t N, const float* score, int max_objects, hipStream_t st) {
  const int rc = c3d_detail_objects_clear(ws, N, nullptr, nullptr, 1, nullptr, max_objects, st);   // header and areas
  if (rc || !score) return rc;
  const int64_t rows = max_objects < N ? max_objects : N;  // no id with a table row can be larger
  return (int)hipMemsetAsync(static_cast<char*>(ws) + c3d_detail_ssum_offset(N), 0, (size_t)rows * 8, st);
}

int c3d_detail_region_keys(const uint8_t* key, const int32_t* labels, int32_t* table, const int32_t* counts, uint8_t* object_key,
                           int Hs, int Ws, int max_objects, hipStream_t st) {
  const int N = Hs * Ws;
  return c3d_launch_lds<region_keys_kernel>(dim3(grid_cus(N > max_objects ? N : max_objects, 256)), dim3(256), 0, st, key, labels,
                                            table, counts, object_key, N, max_objects);
}

extern "C" int64_t c3d_scene_regions_ws_bytes(int32_t Hs, int32_t Ws) {
  if (Hs <= 0 || Ws <= 0) return C3D_E_BADARG;
  if ((int64_t)Hs * Ws >= (1ll << 31)) return C3D_E_UNSUPPORTED;
  return c3d_detail_region_ws_bytes((int64_t)Hs * Ws);
}

extern "C" int c3d_scene_regions_tile(int32_t* th, int32_t* tw) {
  if (!th || !tw) return C3D_E_BADARG;
  *th = TH;
  *tw = TW;
  return 0;
}

extern "C" int c3d_scene_regions(const uint8_t* key, const float* score, int32_t Hs, int32_t Ws, int32_t connectivity,
                                 int32_t min_area, int32_t max_objects, int32_t* labels, int32_t* table, uint8_t* object_key,
                                 int32_t* counts, void* ws, void* stream) {
  if (!key || !labels || !table || !counts || !ws || Hs <= 0 || Ws <= 0 || max_objects < 1) return C3D_E_BADARG;
  if (connectivity != 4 && connectivity != 8) return C3D_E_BADARG;
  if ((int64_t)Hs * Ws >= (1ll << 31)) return C3D_E_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint32_t* header = static_cast<uint32_t*>(ws);
  uint32_t* area = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + c3d_detail_area_offset());
  int rc = c3d_detail_region_clear(ws, (int64_t)Hs * Ws, score, max_objects, st);
  if (rc) return rc;
  rc = c3d_detail_region_roots(key, labels, header + C3D_DETAIL_WS_ERR, area, Hs, Ws, connectivity == 8, nullptr, st);
  if (rc) return rc;
  rc = c3d_detail_objects_tail(nullptr, score, Hs, Ws, min_area, 1, 0, max_objects, labels, table, nullptr, nullptr, counts, ws, 9, st);
  if (rc) return rc;
  return c3d_detail_region_keys(key, labels, table, counts, object_key, Hs, Ws, max_objects, st);
}
