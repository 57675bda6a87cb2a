// What the consumers of a ring table share (csrc/scene_polis.hip for each of its two sides, csrc/scene_valid.hip,
// csrc/scene_conflicts.hip): the pass that marks the used rows of a table, the incomplete ids and K, the scan that settles
// which ids are complete and where their edges go, the passes that regroup the rows into per-id edge lists (place, gather),
// and the class of a pair of live edges.  The rule is the header's (include/change3d_hip.h, c3d_rings_valid); the files
// include this one and none keeps a copy: their __global__ kernels are thin wrappers around the ..._pass bodies below.
// Everything is an integer: coordinate differences stay below 2^25 and every cross or dot product below 2^51, so the doubles
// that carry them are exact and only their signs and orders are used.
#pragma once
#include <climits>

#include "scene_wave.h"
#include "../../include/change3d_hip.h"

namespace c3d_rings {

using namespace c3d_wave;

constexpr int RING_LIMIT = 16384;                          // rings of an id whose order the gather step restores
constexpr int BIG_RING = 4096;                             // a longer ring is checked and copied by many workgroups
constexpr int SCAN_T = 1024;
constexpr int COORD_UNIT = 32768;

enum : uint8_t { ROW_SKIP = 0, ROW_USED = 1 };             // ROW_USED: valid, n >= 3, listed under its id
enum { ID_INCOMPLETE = 1 };
enum { PAIR_NONE = 0, PAIR_CROSS = 1, PAIR_OVERLAP = 2, PAIR_VV = 3, PAIR_VE = 4 };

// the table and the workspace arrays of the shared passes; a file's own view derives from it
struct Rows {
  const int32_t* rings;
  const int2* vertices;
  const int32_t* counts;
  int max_rings, max_vertices, max_ids;
  int64_t coord_max;                                       // 32768 << frac_bits
  // two words of the workspace header (zeroed by the call's memset), wherever the file keeps them
  uint32_t* top;                                           // the largest id of a row
  uint32_t* n_big;                                         // the rings above BIG_RING
  // workspace
  uint8_t* kind;                                           // [max_rings]
  uint32_t* big;                                           // [max_rings] the rows of the rings above BIG_RING, in any order
  uint32_t* id_rings;                                      // [max_ids] used rings with n >= 3
  u64* id_verts;                                           // [max_ids] their edges, degenerate ones included
  uint32_t* id_flags;                                      // [max_ids]
  uint32_t* id_list;                                       // [max_ids] start among the listed rings
  uint32_t* id_start;                                      // [max_ids] start among the edges
};

__device__ __forceinline__ int rows_of(const Rows& s) {
  return (s.counts[4] & C3D_OUTLINE_ST_BAD_COUNTS) ? 0 : clampi(s.counts[1], 0, s.max_rings);
}
__device__ __forceinline__ bool coord_ok(const Rows& s, int2 p) {
  return p.x >= -s.coord_max && p.x <= s.coord_max && p.y >= -s.coord_max && p.y <= s.coord_max;
}
__device__ __forceinline__ int sign_of(double v) { return (v > 0.0) - (v < 0.0); }

// The bounding boxes of two segments that share a point meet, so this reject in front of pair_class changes no class.  The
// callers branch on it wave by wave (__any): left to itself the compiler turns the test into selects and runs the fifty
// double-precision instructions of pair_class for every pair: 12.6 ms against 5.1 ms on one id at the default cap.
__device__ __forceinline__ bool boxes_meet(int4 p, int4 q) {
  return !(max(p.x, p.z) < min(q.x, q.z) || max(q.x, q.z) < min(p.x, p.z) || max(p.y, p.w) < min(q.y, q.w) ||
           max(q.y, q.w) < min(p.y, p.w));
}
// The class of the pair of live edges p = (a, b) and q = (c, d) by the header's rule.  Differences are below 2^25 in an int,
// products below 2^50 and their sums and differences below 2^51 in a double: exact, fused or not.
static __device__ __noinline__ int pair_class(int4 p, int4 q, bool adjacent) {
  const double ex = (double)(p.z - p.x), ey = (double)(p.w - p.y), fx = (double)(q.z - q.x), fy = (double)(q.w - q.y);
  const double cx = (double)(q.x - p.x), cy = (double)(q.y - p.y), dx = (double)(q.z - p.x), dy = (double)(q.w - p.y);
  const double bx = (double)(p.z - q.x), by = (double)(p.w - q.y);
  const int o1 = sign_of(ex * cy - ey * cx), o2 = sign_of(ex * dy - ey * dx);
  const int o3 = sign_of(fy * cx - fx * cy), o4 = sign_of(fx * by - fy * bx);   // a - c = -(c - a)
  if (o1 * o2 < 0 && o3 * o4 < 0) return PAIR_CROSS;
  if ((o1 | o2 | o3 | o4) == 0) {
    const double tc = cx * ex + cy * ey, td = dx * ex + dy * ey, L = ex * ex + ey * ey;
    const double lo = fmax(fmin(tc, td), 0.0), hi = fmin(fmax(tc, td), L);
    if (lo < hi) return PAIR_OVERLAP;
    return (lo == hi && !adjacent) ? PAIR_VV : PAIR_NONE;
  }
  if (o1 * o2 > 0 || o3 * o4 > 0 || adjacent) return PAIR_NONE;
  const bool ends = (p.x == q.x && p.y == q.y) || (p.x == q.z && p.y == q.w) || (p.z == q.x && p.w == q.y) ||
                    (p.z == q.z && p.w == q.w);
  return ends ? PAIR_VV : PAIR_VE;
}
__device__ __forceinline__ bool live_of(int4 e) { return e.x != e.z || e.y != e.w; }

// --------------------------------------------------------------------------------------------------------------- rows
// A wave per ring row (256 threads, r uniform over the wave): classifies the row and adds it to its id (ring count, vertex
// count, the incomplete mark); the rings above BIG_RING vertices are only listed.
__device__ __forceinline__ void rows_pass(const Rows& s) {
  const int rows = rows_of(s), lane = threadIdx.x & 63;
  const int64_t vlimit = clampi(s.counts[3], 0, s.max_vertices);
  // what a wave adds to an id is kept in registers while the id stays the same (the holes of a scene-filling object are
  // thousands of rows of one id); integer sums: the grouping changes nothing
  int top = 0, held = 0;
  uint32_t held_rings = 0;
  u64 held_verts = 0;
  for (int r = blockIdx.x * 4 + (int)(threadIdx.x >> 6); r < rows; r += gridDim.x * 4) {   // r is uniform over the wave
    const int id = s.rings[(int64_t)r * 8], start = s.rings[(int64_t)r * 8 + 1], n = s.rings[(int64_t)r * 8 + 2];
    uint8_t kind = ROW_SKIP;
    if (id >= 1 && id <= s.max_ids) {
      bool bad = start < 0 || n < 0 || (int64_t)start + n > vlimit;
      if (!bad && n <= BIG_RING) {
        bool out = false;
        for (int k = lane; k < n; k += 64) out |= !coord_ok(s, s.vertices[(int64_t)start + k]);
        bad = __any(out);
      }
      // a longer ring is counted now and checked by the next kernel: a bad coordinate there makes the id incomplete
      if (!bad && n > BIG_RING && lane == 0) s.big[atomicAdd(s.n_big, 1u)] = (uint32_t)r;
      top = id > top ? id : top;
      if (bad) {
        if (lane == 0) atomicOr(s.id_flags + (id - 1), (uint32_t)ID_INCOMPLETE);
      } else if (n >= 3) {
        if (id != held) {
          if (held_rings && lane == 0) {
            atomicAdd(s.id_rings + (held - 1), held_rings);
            atomicAdd(s.id_verts + (held - 1), held_verts);
          }
          held = id;
          held_rings = 0;
          held_verts = 0;
        }
        held_rings += 1;
        held_verts += (u64)n;
        kind = ROW_USED;
      }
    }
    if (lane == 0) s.kind[r] = kind;
  }
  if (lane == 0) {
    if (held_rings) {
      atomicAdd(s.id_rings + (held - 1), held_rings);
      atomicAdd(s.id_verts + (held - 1), held_verts);
    }
    if (top) atomicMax(s.top, (uint32_t)top);
  }
}

// the coordinates of the rings above BIG_RING vertices, which rows_pass only lists: many workgroups of 256, a chunk each
__device__ __forceinline__ uint32_t big_of(const Rows& s) { return min(*s.n_big, (uint32_t)s.max_rings); }
__device__ __forceinline__ void check_big_pass(const Rows& s) {
  const uint32_t n_big = big_of(s);
  for (uint32_t li = 0; li < n_big; ++li) {
    const int r = (int)s.big[li];
    const int id = s.rings[(int64_t)r * 8], n = s.rings[(int64_t)r * 8 + 2];
    const int64_t start = s.rings[(int64_t)r * 8 + 1];
    bool out = false;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) out |= !coord_ok(s, s.vertices[start + k]);
    if (out) atomicOr(s.id_flags + (id - 1), (uint32_t)ID_INCOMPLETE);
  }
}

// ---------------------------------------------------------------------------------------------------------------- ids
// One workgroup of SCAN_T threads, `part` = u64 [2][SCAN_T / 64] of LDS: exclusive scans over the ids up to the largest one
// seen.  An id with more than RING_LIMIT rings, or whose edges no longer fit below max_vertices (only tables whose rows share
// vertices get there), becomes incomplete and takes no room.
__device__ __forceinline__ int top_of(const Rows& s) { return clampi((int)*s.top, 0, s.max_ids); }
__device__ __forceinline__ void ids_pass(const Rows& s, u64 (*part)[SCAN_T / 64]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int top = top_of(s);                               // the ids above it have no row: their words stay 0
  u64 run_r = 0, run_v = 0;
  for (int base = 0; base < top; base += SCAN_T) {
    const int i = base + (int)threadIdx.x;
    u64 nr = 0, nv = 0;
    uint32_t fl = 0;
    if (i < top) {
      nr = s.id_rings[i];
      nv = s.id_verts[i];
      fl = s.id_flags[i];
      if (nr > (u64)RING_LIMIT) fl |= ID_INCOMPLETE;
      if (fl & ID_INCOMPLETE) nr = nv = 0;
    }
    u64 ir = nr, iv = nv;
    for (int d = 1; d < 64; d <<= 1) {
      const int from = lane >= d ? lane - d : lane;
      const u64 tr = shfl64(ir, from), tv = shfl64(iv, from);
      if (lane >= d) { ir += tr; iv += tv; }
    }
    if (lane == 63) { part[0][wave] = ir; part[1][wave] = iv; }
    __syncthreads();
    u64 br = 0, bv = 0, ar = 0, av = 0;
    for (int w = 0; w < SCAN_T / 64; ++w) {
      br += w < wave ? part[0][w] : 0ull;
      bv += w < wave ? part[1][w] : 0ull;
      ar += part[0][w];
      av += part[1][w];
    }
    if (i < top) {
      const u64 at_r = run_r + br + ir - nr, at_v = run_v + bv + iv - nv;
      // at_v only grows: an id that does not fit takes its place in the sum all the same, so that no later id fits either
      const bool fits = at_v + nv <= (u64)s.max_vertices;
      if (!fits) fl |= ID_INCOMPLETE;
      s.id_flags[i] = fl;
      s.id_list[i] = (uint32_t)at_r;                       // at most max_rings
      s.id_start[i] = fits ? (uint32_t)at_v : 0u;
      if (fl & ID_INCOMPLETE) { s.id_rings[i] = 0; s.id_verts[i] = 0; }
    }
    run_r += ar;
    run_v += av;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------ place, gather
// The rows regrouped into one edge list per id, in row order.  What is written per edge is the file's: a writer W with
//   w.edge(at, before, n, a, b)   edge (a, b) of a ring of n edges that starts `before` edges into its id; `at` = its place
//                                 among the edges of all ids; returns whether the file counts the edge (W::COUNTS only)
//   w.counted(id, c)              one lane per wave and ring: c edges of the id were counted (W::COUNTS only)
struct Lists : Rows {
  uint2* list;                                             // [max_rings] (ring row, its n) grouped by id
  uint32_t* row_at;                                        // [max_rings] where a ring above BIG_RING goes within its id
  uint32_t* id_claim;                                      // [max_ids]
};

// a thread per row: claims a slot in the ring list of its id (the order of the list varies and is never used)
__device__ __forceinline__ void place_pass(const Lists& s) {
  const int rows = rows_of(s);
  for (int r = blockIdx.x * 256 + (int)threadIdx.x; r < rows; r += gridDim.x * 256) {
    if (s.kind[r] != ROW_USED) continue;
    const int id = s.rings[(int64_t)r * 8];
    const uint32_t k = s.id_rings[id - 1];                 // 0: the id became incomplete
    if (!k) continue;
    const uint32_t slot = atomicAdd(s.id_claim + (id - 1), 1u);
    if (slot < k) s.list[(u64)s.id_list[id - 1] + slot] = make_uint2((uint32_t)r, (uint32_t)s.rings[(int64_t)r * 8 + 2]);
  }
}

// a wave per row (256 threads): the row's place among the edges of its id = the n of the listed rings with a smaller row
// index (an integer sum); then its edges go to that place.  A ring above BIG_RING only gets its place here
template <class W>
__device__ __forceinline__ void gather_pass(const Lists& s, const W& w) {
  const int rows = rows_of(s), lane = threadIdx.x & 63;
  for (int r = blockIdx.x * 4 + (int)(threadIdx.x >> 6); r < rows; r += gridDim.x * 4) {   // r is uniform over the wave
    if (s.kind[r] != ROW_USED) continue;
    const int id = s.rings[(int64_t)r * 8], n = s.rings[(int64_t)r * 8 + 2];
    const int64_t start = s.rings[(int64_t)r * 8 + 1];
    const int k = (int)s.id_rings[id - 1];                 // at most RING_LIMIT
    if (!k) continue;
    const uint2* list = s.list + s.id_list[id - 1];
    u64 before = 0;                                        // edges of the id's rings with a smaller row index
    for (int j = lane; j < k; j += 64) {
      const uint2 q = list[j];
      if (q.x < (uint32_t)r) before += (u64)q.y;
    }
    before = wave_sum64(before);
    const u64 total = s.id_verts[id - 1];
    if (before + (u64)n > total) continue;                 // cannot happen: the sums are those of rows_pass
    if (n > BIG_RING) {                                    // copied by gather_big_pass
      if (lane == 0) s.row_at[r] = (uint32_t)before;
      continue;
    }
    const u64 at = (u64)s.id_start[id - 1] + before;       // id_start + total <= max_vertices
    if constexpr (W::COUNTS) {
      uint32_t c = 0;
      for (int j0 = 0; j0 < n; j0 += 64) {                 // uniform trip count: the ballot sees every lane
        const int j = j0 + lane;
        bool hit = false;
        if (j < n) hit = w.edge(at + j, before, n, s.vertices[start + j], s.vertices[start + (j + 1 < n ? j + 1 : 0)]);
        c += (uint32_t)__popcll(__ballot(hit));
      }
      if (c && lane == 0) w.counted(id, c);
    } else {
      for (int j = lane; j < n; j += 64) w.edge(at + j, before, n, s.vertices[start + j], s.vertices[start + (j + 1 < n ? j + 1 : 0)]);
    }
  }
}

// the same for the rings above BIG_RING, whose place gather_pass left in row_at: many workgroups of 256, a chunk each
template <class W>
__device__ __forceinline__ void gather_big_pass(const Lists& s, const W& w) {
  const uint32_t n_big = big_of(s);
  for (uint32_t li = 0; li < n_big; ++li) {
    const int r = (int)s.big[li];
    if (s.kind[r] != ROW_USED) continue;
    const int id = s.rings[(int64_t)r * 8], n = s.rings[(int64_t)r * 8 + 2];
    const int64_t start = s.rings[(int64_t)r * 8 + 1];
    if (!s.id_rings[id - 1]) continue;                     // the id became incomplete
    const u64 before = s.row_at[r];
    if (before + (u64)n > s.id_verts[id - 1]) continue;    // cannot happen
    const u64 at = (u64)s.id_start[id - 1] + before;
    uint32_t c = 0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256)
      c += w.edge(at + j, before, n, s.vertices[start + j], s.vertices[start + (j + 1 < n ? j + 1 : 0)]) ? 1u : 0u;
    if constexpr (W::COUNTS) {
      c = wave_sum32(c);
      if (c && (threadIdx.x & 63) == 0) w.counted(id, c);
    }
  }
}

}  // namespace c3d_rings
