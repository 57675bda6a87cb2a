// Grouping the rows of a ring table by id, as csrc/scene_hull.hip and csrc/scene_fill.hip both do it before they work id by
// id: the pass that validates the rows and counts the rings of every id, the scan of the counts and the scatter of the row
// indices.  Both files include this header and neither keeps a copy: their __global__ kernels are thin wrappers around the
// ..._pass bodies below.  What a file checks per vertex and adds up per id is its policy P (see group_pass).
#pragma once
#include "scene_wave.h"
#include "../../include/change3d_hip.h"

namespace c3d_groups {

using namespace c3d_wave;

constexpr int SMALL_RING = 16;                             // most vertices of a ring that one lane walks alone
constexpr int SCAN_T = 1024, SCAN_ROWS = 8;
constexpr int ROW_SKIP = 0, ROW_USED = 1;

__device__ __forceinline__ int rows_of(const int32_t* counts, int max_rings) {
  if (counts[4] & C3D_OUTLINE_ST_BAD_COUNTS) return 0;
  return clampi(counts[1], 0, max_rings);
}

// the ring table and the arrays of the three passes
struct Groups {
  const int32_t* rings;
  const int2* vertices;
  const int32_t* counts;
  int max_rings, max_vertices, max_objects;
  uint32_t* cnt;                                           // [max_objects] used rings of the id
  uint32_t* off;                                           // [max_objects] exclusive scan of cnt
  uint32_t* cursor;                                        // [max_objects] slots claimed so far
  uint32_t* grouped;                                       // [max_rings] row indices grouped by id
  uint8_t* valid;                                          // [max_rings] ROW_USED / ROW_SKIP
  uint32_t* top;                                           // the header word of K, the largest used id
};

// 64 ring rows per wave and step (256 threads): a small ring is read by its own lane, a larger one by the whole wave.  What
// the rows of a wave add to the same word goes out as one atomic per wave for its two most frequent ids (a checkerboard is
// half a million rings of ONE id).  The policy:
//   P::Ring               what the vertices of a ring reduce to
//   p.vertex(ring, v)     accumulates one vertex; false: its coordinates are out of range
//   p.merge(ring)         the wave's partial results of one larger ring into the whole (every lane calls it)
//   p.status(...)         raises the file's status words for the rows of this wave that were looked at and not used
//   P::Sum                what a ring adds to its id
//   p.ring(r, n, used, ring)   the Sum of this lane's row (and whatever the file keeps per row)
//   p.fold(same, sum)     the wave's Sum over the lanes with `same` (every lane calls it)
//   p.add(id, sum)        one lane adds a Sum to the id's words
template <class P>
__device__ __forceinline__ void group_pass(const Groups& g, const P& p) {
  const int lane = threadIdx.x & 63, rows = rows_of(g.counts, g.max_rings);
  const int64_t vlimit = clampi(g.counts[3], 0, g.max_vertices);
  for (int base = (blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * 64; base < rows; base += gridDim.x * 256) {   // uniform over the wave
    const int r = base + lane;
    const bool in = r < rows;
    int id = 0, start = -1, n = 0;
    if (in) {
      id = g.rings[(int64_t)r * 8];
      start = g.rings[(int64_t)r * 8 + 1];
      n = g.rings[(int64_t)r * 8 + 2];
    }
    const bool look = in && start >= 0;                    // start < 0: a ring that had no room, skipped silently
    const bool id_ok = id >= 1 && id <= g.max_objects, range_ok = look && n >= 0 && (int64_t)start + n <= vlimit;
    typename P::Ring ring = p.empty();
    bool bad = false;
    if (range_ok && n <= SMALL_RING)
      for (int k = 0; k < n; ++k) bad |= !p.vertex(ring, g.vertices[(int64_t)start + k]);
    u64 big = __ballot(range_ok && n > SMALL_RING);
    for (int step = 0; step < 64 && big; ++step) {         // uniform: the shuffles see every lane
      const int src = __ffsll((long long)big) - 1;
      big &= big - 1;
      const int64_t s0 = __shfl(start, src);
      const int n0 = __shfl(n, src);
      typename P::Ring part = p.empty();
      bool b0 = false;
      for (int k = lane; k < n0; k += 64) b0 |= !p.vertex(part, g.vertices[s0 + k]);
      p.merge(part);
      const bool any_bad = __any(b0) != 0;
      if (lane == src) {
        ring = part;
        bad = any_bad;
      }
    }
    const bool ring_ok = range_ok && !bad, used = look && id_ok && ring_ok;
    if (in) g.valid[r] = used ? ROW_USED : ROW_SKIP;
    p.status(look, id_ok, ring_ok, used);
    const int k_max = wave_max32(used ? id : 0);
    if (lane == 0 && (uint32_t)k_max > *g.top) atomicMax(g.top, (uint32_t)k_max);
    const typename P::Sum mine = p.ring(r, n, used, ring);
    bool open = used;
    for (int round = 0; round < 2; ++round) {              // one set of atomics per wave for its two most frequent ids
      const u64 m = __ballot(open);
      if (!m) break;
      const int leader = __ffsll((long long)m) - 1, id0 = __shfl(id, leader);
      const bool same = open && id == id0;
      const int c = __popcll(__ballot(same));
      const typename P::Sum all = p.fold(same, mine);
      if (lane == leader) {
        atomicAdd(g.cnt + (id0 - 1), (uint32_t)c);
        p.add(id0, all);
      }
      if (same) open = false;
    }
    if (open) {
      atomicAdd(g.cnt + (id - 1), 1u);
      p.add(id, mine);
    }
  }
}

// off[i] = rings of the ids before i + 1, for the ids up to K (the ids above K own no ring and are never looked up).  One
// workgroup of SCAN_T threads; part: u32 [SCAN_T / 64] of LDS.
__device__ __forceinline__ void scan_pass(const Groups& g, uint32_t* part) {
  const int K = (int)*g.top;
  uint32_t running = 0;
  for (int base = 0; base < K; base += SCAN_T * SCAN_ROWS) {
    uint32_t n[SCAN_ROWS], mine = 0;
    for (int j = 0; j < SCAN_ROWS; ++j) {
      const int i = base + (int)threadIdx.x * SCAN_ROWS + j;
      n[j] = i < K ? g.cnt[i] : 0u;
      mine += n[j];
    }
    uint32_t all;
    uint32_t at = running + block_excl_scan32<SCAN_T / 64>(mine, part, &all);
    for (int j = 0; j < SCAN_ROWS; ++j) {
      const int i = base + (int)threadIdx.x * SCAN_ROWS + j;
      if (i < K) g.off[i] = at;
      at += n[j];
    }
    running += all;
    __syncthreads();
  }
}

// Row indices grouped by id.  The slot inside a group is claimed by an atomic, so the order inside a group varies from run to
// run; one claim per wave for its two most frequent ids.
__device__ __forceinline__ void scatter_pass(const Groups& g) {
  const int rows = rows_of(g.counts, g.max_rings), lane = threadIdx.x & 63;
  for (int base = blockIdx.x * 256; base < rows; base += gridDim.x * 256) {   // whole waves stay together
    const int r = base + (int)threadIdx.x;
    bool open = r < rows && g.valid[r] == ROW_USED;
    const int id = open ? g.rings[(int64_t)r * 8] : 0;     // 1 .. max_objects: the group pass checked it
    uint32_t slot = 0xFFFFFFFFu;
    for (int round = 0; round < 2; ++round) {
      const u64 m = __ballot(open);
      if (!m) break;
      const int leader = __ffsll((long long)m) - 1, id0 = __shfl(id, leader);
      const bool same = open && id == id0;
      const u64 sm = __ballot(same);
      uint32_t first = 0;
      if (lane == leader) first = atomicAdd(g.cursor + (id0 - 1), (uint32_t)__popcll(sm));
      first = (uint32_t)__shfl((int)first, leader);
      if (same) {
        slot = g.off[id0 - 1] + first + (uint32_t)__popcll(sm & ((1ull << lane) - 1ull));
        open = false;
      }
    }
    if (open) slot = g.off[id - 1] + atomicAdd(g.cursor + (id - 1), 1u);
    if (slot < (uint32_t)g.max_rings) g.grouped[slot] = (uint32_t)r;   // the used rows number at most max_rings
  }
}

}  // namespace c3d_groups
