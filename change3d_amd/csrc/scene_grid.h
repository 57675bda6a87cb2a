// The uniform grid of edge cells that csrc/scene_conflicts.hip and the detector of csrc/scene_safe.hip both build: per candidate
// shift the entries it would cost, the smallest shift within the entry and the cell budget, a count per cell, where the
// entries of every cell start (and the jobs of a crowded cell), and the edge indices grouped by cell.  Both files include this
// one and neither keeps a copy: their __global__ kernels are thin wrappers around the ..._pass bodies below.
//
// A caller hands in its arrays as a Cells view, its header (32-bit words; the 64-bit words start at byte 64) and a table W of
// the word indices it keeps the grid's state at: LO_X, LO_Y, HI_X, HI_Y (the biased box of the edges), SHIFT, CX, CY, X0, Y0,
// AT, JOBS, and the 64-bit Q_WORK, Q_ENTRIES, Q_COST.  LIVE = true skips the edges with a == b, which the list of the safe call
// keeps in place; the list of the conflicts call holds live edges only.  Any gate (a done word, the work limit) is the caller's.
#pragma once
#include "scene_wave.h"

namespace c3d_grid {

using namespace c3d_wave;

constexpr int CELL_WAVE_LIMIT = 64;                        // entries of a cell in the wave tier: a lane each
constexpr int CHUNK = 256;                                 // entries of a chunk: a thread each; an LDS tile is one chunk
constexpr int BUDGET_E = 2;                                // entries the grid may hold per live edge
constexpr int BUDGET_C = 4;                                // cells the grid may have per live edge
constexpr int N_SHIFT = 26;                                // candidate shifts 0 .. 25: extents stay below 2^25, so s = 25 is one cell
constexpr int BIAS = 1 << 24;                              // above every |coordinate|: biased values are positive, 0 means none

struct Cells {
  const int4* e_xy;                                        // (a.x, a.y, b.x, b.y) of every listed edge
  uint32_t* cell_n;                                        // [cap_c] entries of the cell
  uint32_t* cell_at;                                       // [cap_c] where they start; after the fill, where they end
  uint32_t* entry;                                         // [cap_e] edge indices grouped by cell
  uint2* jobs;                                             // [cap_j] (cell, chunk)
  int64_t cap_e, cap_c, cap_j;
};
template <class S>
__device__ __forceinline__ Cells cells_of(const S& s) {
  return Cells{s.e_xy, s.cell_n, s.cell_at, s.entry, s.jobs, s.cap_e, s.cap_c, s.cap_j};
}
// a cell above CELL_WAVE_LIMIT entries has ceil(n / CHUNK) jobs: at most entries / CHUNK + entries / (CELL_WAVE_LIMIT + 1) in all
inline int64_t jobs_cap(int64_t cap_e) { return cap_e / CHUNK + cap_e / (CELL_WAVE_LIMIT + 1) + 1; }

__device__ __forceinline__ u64* quad(uint32_t* header) { return reinterpret_cast<u64*>(header + 16); }
__device__ __forceinline__ const u64* quad(const uint32_t* header) { return reinterpret_cast<const u64*>(header + 16); }
__device__ __forceinline__ bool is_dead(int4 e) { return e.x == e.z && e.y == e.w; }
__device__ __forceinline__ u64 entry_budget(const Cells& s, uint32_t n) { return min((u64)BUDGET_E * n, (u64)s.cap_e); }
__device__ __forceinline__ u64 cell_budget(const Cells& s, uint32_t n) { return min((u64)BUDGET_C * max(n, 1u), (u64)s.cap_c); }

// the grid as the later launches read it
struct Grid {
  int shift, x0, y0;
  uint32_t cx, cy;
};
template <class W>
__device__ __forceinline__ Grid grid_of(const uint32_t* header) {
  Grid g;
  g.shift = (int)header[W::SHIFT]; g.x0 = (int)header[W::X0]; g.y0 = (int)header[W::Y0];
  g.cx = header[W::CX]; g.cy = header[W::CY];
  return g;
}
// the cells (x0 .. x1, y0 .. y1) that the bounding box of e covers; e lies inside the box of all edges, so no index leaves the grid
__device__ __forceinline__ void span_of(const Grid& g, int4 e, uint32_t& x0, uint32_t& x1, uint32_t& y0, uint32_t& y1) {
  x0 = (uint32_t)(min(e.x, e.z) - g.x0) >> g.shift; x1 = (uint32_t)(max(e.x, e.z) - g.x0) >> g.shift;
  y0 = (uint32_t)(min(e.y, e.w) - g.y0) >> g.shift; y1 = (uint32_t)(max(e.y, e.w) - g.y0) >> g.shift;
  x1 = min(x1, g.cx - 1u); y1 = min(y1, g.cy - 1u);        // cannot bind: the box was taken over these edges
}

// ------------------------------------------------------------------------------------------------------------------ cost
// 256 threads, a thread per listed edge (n of them, `live` of them live).  Per candidate s the entries that s would cost.  A sum
// only has to tell "within the budget" from "above it": an edge adds at most budget + 1 and a wave keeps its sum at or below
// that, so no 64-bit counter overflows.
template <class W, bool LIVE>
__device__ __forceinline__ void cost_pass(const Cells& s, uint32_t* __restrict__ header, uint32_t n, uint32_t live) {
  const int lane = threadIdx.x & 63;
  if ((uint32_t)blockIdx.x * 256u >= n) return;             // the launch is sized by the caller's maximum
  if constexpr (LIVE)
    if (!live) return;
  const int x0 = BIAS - (int)header[W::LO_X], y0 = BIAS - (int)header[W::LO_Y];
  const u64 top = entry_budget(s, live) + 1ull;
  u64 cost[N_SHIFT];
#pragma unroll
  for (int k = 0; k < N_SHIFT; ++k) cost[k] = 0;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int4 e = s.e_xy[i];
    if constexpr (LIVE)
      if (is_dead(e)) continue;
    const uint32_t ax = (uint32_t)(min(e.x, e.z) - x0), bx = (uint32_t)(max(e.x, e.z) - x0);
    const uint32_t ay = (uint32_t)(min(e.y, e.w) - y0), by = (uint32_t)(max(e.y, e.w) - y0);
#pragma unroll
    for (int k = 0; k < N_SHIFT; ++k) {
      const u64 c = (u64)((bx >> k) - (ax >> k) + 1u) * (u64)((by >> k) - (ay >> k) + 1u);   // below 2^50
      cost[k] = min(cost[k] + min(c, top), top);
    }
  }
#pragma unroll
  for (int k = 0; k < N_SHIFT; ++k) {
    u64 v = cost[k];
    for (int o = 32; o > 0; o >>= 1) v = min(v + shfl64(v, lane ^ o), top);
    if (lane == 0 && v) atomicAdd(quad(header) + W::Q_COST + k, v);
  }
}

// ---------------------------------------------------------------------------------------------------------------- choose
// one wave, a lane per candidate: the smallest s within the entry and the cell budget, both taken per live edge (n of them): a
// list that fills a fraction of its room gets a grid sized for what it holds
template <class W>
__device__ __forceinline__ void choose_pass(const Cells& s, uint32_t* __restrict__ header, uint32_t n) {
  const int k = threadIdx.x;
  int x0 = 0, y0 = 0;
  uint32_t wx = 0, wy = 0;                                 // the extent of the box: below 2^25
  if (n) {
    x0 = BIAS - (int)header[W::LO_X]; y0 = BIAS - (int)header[W::LO_Y];
    wx = (uint32_t)((int)header[W::HI_X] - BIAS - x0); wy = (uint32_t)((int)header[W::HI_Y] - BIAS - y0);
  }
  bool ok = false;
  u64 cells = 0, cost = 0;
  if (k < N_SHIFT) {
    cells = (u64)((wx >> k) + 1u) * (u64)((wy >> k) + 1u);
    cost = quad(header)[W::Q_COST + k];
    ok = cost <= entry_budget(s, n) && cells <= cell_budget(s, n);
  }
  const u64 fit = __ballot(ok);
  const int pick = fit ? __ffsll((long long)fit) - 1 : N_SHIFT - 1;   // s = 25 always fits: one cell, an entry per edge
  if (k == pick) {
    header[W::SHIFT] = (uint32_t)pick;
    header[W::CX] = (wx >> pick) + 1u;
    header[W::CY] = (wy >> pick) + 1u;
    header[W::X0] = (uint32_t)x0;
    header[W::Y0] = (uint32_t)y0;
    quad(header)[W::Q_ENTRIES] = min(cost, entry_budget(s, n));
  }
}

// ----------------------------------------------------------------------------------------------------------- zero, count
// 256 threads, a thread per cell: for a caller that builds the grid more than once
template <class W>
__device__ __forceinline__ void zero_pass(const Cells& s, const uint32_t* __restrict__ header) {
  const u64 cells = min((u64)header[W::CX] * header[W::CY], (u64)s.cap_c);
  for (u64 c = (u64)blockIdx.x * 256 + threadIdx.x; c < cells; c += (u64)gridDim.x * 256) s.cell_n[c] = 0u;
}

// 256 threads, a thread per listed edge: one atomic per covered cell
template <class W, bool LIVE>
__device__ __forceinline__ void count_pass(const Cells& s, const uint32_t* __restrict__ header, uint32_t n) {
  const Grid g = grid_of<W>(header);
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int4 e = s.e_xy[i];
    if constexpr (LIVE)
      if (is_dead(e)) continue;
    uint32_t x0, x1, y0, y1;
    span_of(g, e, x0, x1, y0, y1);
    for (uint32_t y = y0; y <= y1; ++y)                    // at most cap_e cells in all: the chosen s is within the budget
      for (uint32_t x = x0; x <= x1; ++x) atomicAdd(s.cell_n + ((u64)y * g.cx + x), 1u);
  }
}

// ---------------------------------------------------------------------------------------------------------------- starts
// 256 threads, a thread per cell: where its entries go (a wave scan, one atomic per wave), its share of `work`, and the jobs of
// a cell above CELL_WAVE_LIMIT entries
template <class W>
__device__ __forceinline__ void starts_pass(const Cells& s, uint32_t* __restrict__ header) {
  const Grid g = grid_of<W>(header);
  const u64 cells = min((u64)g.cx * g.cy, (u64)s.cap_c);   // cannot bind: choose kept the cells within the budget
  const int lane = threadIdx.x & 63;
  u64 work = 0;
  for (u64 c0 = ((u64)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; c0 < cells; c0 += (u64)gridDim.x * 256) {   // uniform over the wave
    const u64 c = c0 + lane;
    const uint32_t cnt = c < cells ? s.cell_n[c] : 0u;
    uint32_t all;
    const uint32_t before = wave_excl_scan32(cnt, &all);
    uint32_t base = 0;
    if (lane == 0 && all) base = atomicAdd(header + W::AT, all);
    base = (uint32_t)__shfl((int)base, 0);
    if (c < cells) s.cell_at[c] = base + before;
    work += (u64)cnt * (u64)(cnt ? cnt - 1u : 0u) / 2ull;   // cnt < 2^31: an edge enters a cell once
    if (cnt > (uint32_t)CELL_WAVE_LIMIT) {
      const uint32_t chunks = (cnt + CHUNK - 1) / CHUNK;
      const uint32_t at = atomicAdd(header + W::JOBS, chunks);
      for (uint32_t i = 0; i < chunks; ++i)                // at most cap_e / CHUNK + 1 steps
        if ((u64)at + i < (u64)s.cap_j) s.jobs[at + i] = make_uint2((uint32_t)c, i);   // cannot fail: see jobs_cap
    }
  }
  work = wave_sum64(work);
  if (lane == 0 && work) atomicAdd(quad(header) + W::Q_WORK, work);
}

// ------------------------------------------------------------------------------------------------------------------ fill
// 256 threads, a thread per listed edge: its index into every covered cell
template <class W, bool LIVE>
__device__ __forceinline__ void fill_pass(const Cells& s, const uint32_t* __restrict__ header, uint32_t n) {
  const Grid g = grid_of<W>(header);
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int4 e = s.e_xy[i];
    if constexpr (LIVE)
      if (is_dead(e)) continue;
    uint32_t x0, x1, y0, y1;
    span_of(g, e, x0, x1, y0, y1);
    for (uint32_t y = y0; y <= y1; ++y)
      for (uint32_t x = x0; x <= x1; ++x) {
        const uint32_t at = atomicAdd(s.cell_at + ((u64)y * g.cx + x), 1u);
        if ((u64)at < (u64)s.cap_e) s.entry[at] = i;       // cannot fail: the counts are those of count_pass
      }
  }
}

}  // namespace c3d_grid
