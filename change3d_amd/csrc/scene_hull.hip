// Convex hulls and minimum-area rectangles of the objects of a scene map: the ring table and vertex list of
// c3d_scene_outlines (or any table of that shape with integer pixel corners) turned into one strictly convex hull and one
// oriented bounding rectangle per id while they stay in HBM.  The rule -- the point set of an id, the walk from the smallest
// (y, x), the farthest of collinear points, the rectangle of the smallest area by an exact 128-bit comparison, the smallest
// edge on ties -- is the header's (include/change3d_hip.h); this file is one way to compute it.  Integer arithmetic and
// integer atomics only.  No workgroup waits for another, nothing is read back, every loop is capped.
//
//   1 init      per-id state in the workspace (ring count, point count, cursor)
//   2 group     validates the ring rows (a lane per small ring, the wave together on a larger one), counts the rings and the
//               points of every id, K = the largest used id; one atomic per wave and word where its rows share the id
//   3 scan      one workgroup: off[id] = exclusive scan of the ring counts
//   4 scatter   ring indices grouped by id.  The slot inside a group is claimed by an atomic, so the order varies from run to
//               run; the hull of a point SET does not
//   5 wave      ids of up to WAVE_LIMIT points, one wave each: a lane per point, the point in registers; a step of the walk is
//               one arg-reduction by shuffles; hull vertex k stays in lane k, which then owns hull edge k of the rectangle
//               search.  Writes the id's hull row (all but `start`) and rectangle row, lists the larger ids for 6, zeroes the
//               rows past K
//   6 block     larger ids, one workgroup of 1024 each.  Two sweeps over the id's rings: the eight directional extreme POINTS,
//               then every point that is not strictly inside their octagon (Akl-Toussaint: such a point is strictly inside
//               the hull, dropping it is exact) goes to LDS.  An id of up to LDS_LIMIT points always fits; a larger one whose
//               candidates do not fit walks over its rings in HBM instead, unfiltered.  A step of the walk is a reduction over
//               the candidates (shuffles, then one LDS word per wave); the hull lives in LDS, a thread per hull edge searches
//               the rectangle
//   7 starts    one workgroup: start = exclusive scan of the hull sizes in id order, -1 from the first id that does not
//               fit; counts_out
//   8, 9        5 and 6 again for the ids with start >= 0, this time writing the hull's vertices where they belong.  A wave
//               walks its few points again.  A workgroup of 6 has kept its hull in a staging list of max_vertices points
//               (claimed by an atomic: the place varies, the content does not) and 9 copies it.  Rows of a table may share
//               vertices, so the hulls of all ids together have no O(max_vertices) bound: a hull that found the list full is
//               walked again by 9, which needs no room at all
#include <climits>

#include "scene_groups.h"
#include "scene_host.h"

namespace {

using namespace c3d_groups;                                // the group, scan and scatter passes (steps 2-4)
using c3d_host::grid_for;

typedef unsigned long long u64;
typedef unsigned __int128 u128;

constexpr int WAVE_LIMIT = 64;                             // one lane per point
constexpr int LDS_LIMIT = 16384;                           // points or candidates of an id that one workgroup keeps in LDS
// The edges of a strictly convex lattice polygon have distinct directions, and inside [0, 16384]^2 their |dx| + |dy| add up
// to at most 4 * 16384: the shortest primitive vectors spend that on 2273 edges (tests/test_hull_cpu.py counts them), so no
// hull comes near HULL_CAP.  The walk is capped by it all the same.
constexpr int HULL_CAP = 4096;
constexpr int BLOCK_T = 1024;                              // threads of an id's workgroup: a step of the walk is latency
constexpr int WAVES = BLOCK_T / 64;
constexpr int COORD_MAX = 16384;
constexpr int MID_RING = 2048;                             // most vertices of a ring that one wave walks; all threads beyond
constexpr int BIG_LIST = 1024;                             // larger rings of an id that the workgroup lists in LDS per sweep
constexpr int MAX_GRID = 8192;
constexpr int LIST_GRID = 256;                             // workgroups that share the list of large ids
constexpr uint32_t NONE = 0xFFFFFFFFu;                     // no point; a point is y << 16 | x, so that the order is (y, x)

// LDS of the block kernel: candidates, hull, the list of larger rings, then the scratch of the reductions
constexpr int LDS_BYTES = LDS_LIMIT * 4 + HULL_CAP * 4 + BIG_LIST * 8 + 8 * 8 + WAVES * 24 + 16;

// words of the workspace header (256 bytes, zeroed by the call's memset)
enum { WS_STATUS = 0, WS_K = 1, WS_LARGE = 2, WS_STAGED = 4 };   // WS_STAGED: a u64, the hull vertices staged so far

struct Plan {
  Groups g;
  u64* npts;                                               // [max_objects] points of the id
  uint32_t* large;                                         // [max_objects] the ids above WAVE_LIMIT points, in any order
  uint32_t* stage_at;                                      // [max_objects] where the id's hull starts in `stage`
  uint32_t* stage;                                         // [max_vertices] hulls kept by the first block pass
  int64_t bytes;
};

// ws: the workspace, or nullptr where only the sizes are asked for
Plan plan_of(void* ws, int64_t max_rings, int64_t max_vertices, int64_t max_objects) {
  Plan pl{};
  c3d_host::Layout l{static_cast<char*>(ws), 256};
  l.take(pl.npts, max_objects * 8);
  l.take(pl.g.cnt, max_objects * 4);
  l.take(pl.g.off, max_objects * 4);
  l.take(pl.g.cursor, max_objects * 4);
  l.take(pl.large, max_objects * 4);
  l.take(pl.stage_at, max_objects * 4);
  l.take(pl.g.grouped, max_rings * 4);
  l.take(pl.g.valid, max_rings);
  l.take(pl.stage, max_vertices * 4);
  pl.bytes = l.at;
  pl.g.max_rings = (int)max_rings; pl.g.max_vertices = (int)max_vertices; pl.g.max_objects = (int)max_objects;
  if (ws) pl.g.top = static_cast<uint32_t*>(ws) + WS_K;
  return pl;
}

// 64-bit reductions by the xor shuffle, which the walks below use on pairs of words too: another shuffle pattern than
// scene_wave.h's, so these three stay here
__device__ __forceinline__ u64 shfl_xor64(u64 v, int d) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_sum64(u64 v) {
  for (int d = 32; d; d >>= 1) v += shfl_xor64(v, d);
  return v;
}
__device__ __forceinline__ u64 wave_min64(u64 v) {
  for (int d = 32; d; d >>= 1) {
    const u64 o = shfl_xor64(v, d);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ u64 wave_max64(u64 v) {
  for (int d = 32; d; d >>= 1) {
    const u64 o = shfl_xor64(v, d);
    v = o > v ? o : v;
  }
  return v;
}

__device__ __forceinline__ bool coord_ok(int2 p) { return p.x >= 0 && p.x <= COORD_MAX && p.y >= 0 && p.y <= COORD_MAX; }
__device__ __forceinline__ uint32_t pack(int2 p) { return ((uint32_t)p.y << 16) | (uint32_t)p.x; }
__device__ __forceinline__ int px(uint32_t v) { return (int)(v & 0xFFFFu); }
__device__ __forceinline__ int py(uint32_t v) { return (int)(v >> 16); }
// cross(a, b, c) of the header; every product stays under 2^28 and the difference under 2^29
__device__ __forceinline__ int cross3(uint32_t a, uint32_t b, uint32_t c) {
  return (px(b) - px(a)) * (py(c) - py(a)) - (py(b) - py(a)) * (px(c) - px(a));
}
__device__ __forceinline__ int dist2(uint32_t a, uint32_t b) {
  const int dx = px(b) - px(a), dy = py(b) - py(a);
  return dx * dx + dy * dy;
}
// The better successor of the hull vertex `cur` among a and b, neither equal to cur: b wins if a does not have b on its
// left-or-on side, or if both lie on one ray and b is farther.  Seen from a hull vertex all points lie within less than a
// half turn, so this is a total order and any reduction tree gives the same point.
__device__ __forceinline__ uint32_t better(uint32_t cur, uint32_t a, uint32_t b) {
  if (a == NONE) return b;
  if (b == NONE) return a;
  const int c = cross3(cur, a, b);
  if (c < 0) return b;
  if (c > 0) return a;
  return dist2(cur, b) > dist2(cur, a) ? b : a;
}
__device__ __forceinline__ uint32_t wave_better(uint32_t cur, uint32_t v) {
  for (int d = 32; d; d >>= 1) v = better(cur, v, (uint32_t)__shfl_xor((int)v, d));
  return v;
}

// the rectangle on one hull edge, and the order the header gives rectangles: by area w * c / L, compared exactly, then by k
struct Rect {
  u64 wc, L;                                               // (t_max - t_min) * c_max < 2^59, |d|^2 <= 2^29
  int k;                                                   // the edge, INT_MAX: none
  int64_t t_min, t_max, c_max;
  int j_tmin, j_tmax, j_cmax;
};
__device__ __forceinline__ bool rect_less(u64 wc_a, u64 L_a, int k_a, u64 wc_b, u64 L_b, int k_b) {
  if (k_b == INT_MAX) return k_a != INT_MAX;
  if (k_a == INT_MAX) return false;
  const u128 lhs = (u128)wc_a * L_b, rhs = (u128)wc_b * L_a;   // under 2^88
  return lhs < rhs || (lhs == rhs && k_a < k_b);
}
// hull(j) for j < m gives the packed hull vertex j
template <class Hull>
__device__ __forceinline__ Rect edge_rect(Hull hull, int m, int k) {
  const uint32_t P = hull(k), Q = hull(k + 1 == m ? 0 : k + 1);
  const int64_t dx = px(Q) - px(P), dy = py(Q) - py(P);
  Rect r;
  r.k = k;
  r.L = (u64)(dx * dx + dy * dy);
  r.t_min = LLONG_MAX;
  r.t_max = LLONG_MIN;
  r.c_max = -1;
  r.j_tmin = r.j_tmax = r.j_cmax = 0;
  for (int j = 0; j < m; ++j) {
    const uint32_t h = hull(j);
    const int64_t qx = px(h) - px(P), qy = py(h) - py(P);
    const int64_t t = qx * dx + qy * dy, c = dx * qy - dy * qx;
    if (t < r.t_min) { r.t_min = t; r.j_tmin = j; }
    if (t > r.t_max) { r.t_max = t; r.j_tmax = j; }
    if (c > r.c_max) { r.c_max = c; r.j_cmax = j; }
  }
  r.wc = (u64)(r.t_max - r.t_min) * (u64)r.c_max;
  return r;
}
__device__ __forceinline__ void write_rect(int64_t* __restrict__ rects, int id, const Rect& r) {
  int64_t* row = rects + (int64_t)(id - 1) * 8;
  row[0] = r.k;
  row[1] = (int64_t)r.L;
  row[2] = r.t_min;
  row[3] = r.t_max;
  row[4] = r.c_max;
  row[5] = r.j_tmin;
  row[6] = r.j_tmax;
  row[7] = r.j_cmax;
}
__device__ __forceinline__ void write_no_rect(int64_t* __restrict__ rects, int id) {
  int64_t* row = rects + (int64_t)(id - 1) * 8;
  row[0] = -1;
  for (int j = 1; j < 8; ++j) row[j] = 0;
}
__device__ __forceinline__ int npts_i32(u64 n) { return n > (u64)INT_MAX ? INT_MAX : (int)n; }

__global__ __launch_bounds__(256) void hull_init_kernel(u64* __restrict__ npts, uint32_t* __restrict__ cnt,
                                                        uint32_t* __restrict__ cursor, int max_objects) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < max_objects; i += gridDim.x * 256) {
    npts[i] = 0;
    cnt[i] = 0;
    cursor[i] = 0;
  }
}

// what the group pass checks and adds up here: coordinates inside the scene, the points of every id
struct GroupPolicy {
  u64* npts;
  uint32_t* header;
  struct Ring {};                                          // nothing is kept per ring but its n
  typedef u64 Sum;
  __device__ __forceinline__ Ring empty() const { return Ring{}; }
  __device__ __forceinline__ bool vertex(Ring&, int2 v) const { return coord_ok(v); }
  __device__ __forceinline__ void merge(Ring&) const {}
  __device__ __forceinline__ void status(bool look, bool, bool, bool used) const {
    const bool any_skipped = __any(look && !used) != 0;
    if ((threadIdx.x & 63) == 0 && any_skipped) atomicOr(header + WS_STATUS, (uint32_t)C3D_HULL_ST_BAD_ROW);
  }
  __device__ __forceinline__ Sum ring(int, int n, bool, const Ring&) const { return (u64)n; }
  __device__ __forceinline__ Sum fold(bool same, Sum n) const { return wave_sum64(same ? n : 0ull); }
  __device__ __forceinline__ void add(int id, Sum pts) const {
    if (pts) atomicAdd(npts + (id - 1), pts);
  }
};
__global__ __launch_bounds__(256) void hull_group_kernel(Groups g, u64* __restrict__ npts, uint32_t* __restrict__ header) {
  group_pass(g, GroupPolicy{npts, header});
}
__global__ __launch_bounds__(SCAN_T) void hull_scan_kernel(Groups g) {
  extern __shared__ uint32_t part[];                       // [SCAN_T / 64]
  scan_pass(g, part);
}
__global__ __launch_bounds__(256) void hull_scatter_kernel(Groups g) { scatter_pass(g); }

// ------------------------------------------------------------------------------------------------- one wave per id
// WRITE false: the hull row (all but start) and the rectangle row of every id up to K, the list of the larger ids, zeros
// past K.  WRITE true: the hull's vertices, for the ids whose start the scan set.
template <bool WRITE>
__global__ __launch_bounds__(256) void hull_wave_kernel(const int32_t* __restrict__ rings, const int2* __restrict__ vertices,
                                                        const u64* __restrict__ npts, const uint32_t* __restrict__ cnt,
                                                        const uint32_t* __restrict__ off, const uint32_t* __restrict__ grouped,
                                                        uint32_t* __restrict__ large, uint32_t* __restrict__ header,
                                                        int max_objects, int max_hull_vertices, int32_t* __restrict__ hulls,
                                                        int2* __restrict__ hull_vertices, int64_t* __restrict__ rects) {
  const int lane = threadIdx.x & 63, K = (int)header[WS_K];
  const int last = WRITE ? K : max_objects;
  for (int id = 1 + blockIdx.x * 4 + (threadIdx.x >> 6); id <= last; id += gridDim.x * 4) {   // id is uniform over the wave
    int4* row = reinterpret_cast<int4*>(hulls + (int64_t)(id - 1) * 8);
    if (id > K) {                                          // WRITE false only
      if (lane < 2) row[lane] = make_int4(0, 0, 0, 0);
      if (lane < 8) rects[(int64_t)(id - 1) * 8 + lane] = 0;
      continue;
    }
    const u64 np = npts[id - 1];
    if (np == 0) {
      if (!WRITE && lane == 0) {
        row[0] = make_int4(id, -1, 0, 0);
        row[1] = make_int4(0, 0, 0, 0);
        write_no_rect(rects, id);
      }
      continue;
    }
    if (np > (u64)WAVE_LIMIT) {                            // for the workgroup tier; the order of the list is of no consequence
      if (!WRITE && lane == 0) large[atomicAdd(header + WS_LARGE, 1u)] = (uint32_t)id;
      continue;
    }
    const int start_out = WRITE ? hulls[(int64_t)(id - 1) * 8 + 1] : -1;
    if (WRITE && start_out < 0) continue;
    // the id's points, one per lane, in the order of its ring list (which varies; the result does not depend on it)
    const int n_in = (int)np;
    uint32_t p = NONE;
    const uint32_t nr = cnt[id - 1], at = off[id - 1];
    int pos = 0;
    for (uint32_t i = 0; i < nr && pos < n_in; ++i) {
      const int r = (int)grouped[at + i];
      const int64_t start = rings[(int64_t)r * 8 + 1];
      const int n = rings[(int64_t)r * 8 + 2];
      const int k = lane - pos;
      if (k >= 0 && k < n && lane < n_in) p = pack(vertices[start + k]);
      pos += n;
    }
    // the walk
    const uint32_t h0 = wave_min32u(p);
    uint32_t cur = h0, mine = NONE;                        // mine = hull vertex `lane`
    int m = 0;
    for (int step = 0; step < WAVE_LIMIT; ++step) {        // a hull has no more vertices than the id has points
      if (lane == step) mine = cur;
      m = step + 1;
      const uint32_t next = wave_better(cur, p != cur ? p : NONE);
      if (next == NONE || next == h0) break;               // uniform
      cur = next;
    }
    if (WRITE) {
      if (lane < m && (int64_t)start_out + lane < max_hull_vertices) hull_vertices[(int64_t)start_out + lane] = make_int2(px(mine), py(mine));
      continue;
    }
    const uint32_t nxt = (uint32_t)__shfl((int)mine, lane + 1 < m ? lane + 1 : 0);
    const uint32_t area2 = wave_sum32(lane < m ? (uint32_t)(px(mine) * py(nxt) - px(nxt) * py(mine)) : 0u);   // below 2^30: exact
    if (lane == 0) {
      row[0] = make_int4(id, -1, m, (int)area2);           // start: the scan's
      row[1] = make_int4(0, px(h0), py(h0), n_in);
    }
    if (m < 3) {
      if (lane == 0) write_no_rect(rects, id);
      continue;
    }
    Rect best;
    best.k = INT_MAX;
    best.wc = best.L = 0;
    {                                                      // every lane walks an edge: the shuffles see the whole wave
      const Rect r = edge_rect([&](int j) { return (uint32_t)__shfl((int)mine, j); }, m, lane < m ? lane : m - 1);
      if (lane < m) best = r;
    }
    u64 wc = best.wc, L = best.L;
    int k = best.k;
    for (int d = 32; d; d >>= 1) {
      const u64 owc = shfl_xor64(wc, d), oL = shfl_xor64(L, d);
      const int ok = __shfl_xor(k, d);
      if (rect_less(owc, oL, ok, wc, L, k)) { wc = owc; L = oL; k = ok; }
    }
    if (lane == k) write_rect(rects, id, best);
  }
}

// -------------------------------------------------------------------------------------------- one workgroup per id
// fn(point) for every point of the id, spread over the workgroup.  The waves take the id's rings 64 at a time; a small ring is
// walked by its lane, a larger one goes to a list in LDS that is shared out afterwards -- a medium ring to one wave, a long one
// to all threads: an object is typically one long outline and many short holes.  A ring that finds the list full is walked by
// its wave at once.  Every thread of the workgroup calls it; it holds barriers
template <class Fn>
__device__ __forceinline__ void each_point(const int32_t* __restrict__ rings, const int2* __restrict__ vertices,
                                           const uint32_t* __restrict__ grouped, uint32_t at, uint32_t nr, int2* s_big,
                                           uint32_t* s_nbig, Fn fn) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                                         // the sweep before is done with the list
  if (threadIdx.x == 0) *s_nbig = 0;
  __syncthreads();
  for (uint32_t base = (uint32_t)wave * 64; base < nr; base += (uint32_t)WAVES * 64) {
    int start = 0, n = 0;
    if (base + lane < nr) {
      const int r = (int)grouped[at + base + lane];
      start = rings[(int64_t)r * 8 + 1];
      n = rings[(int64_t)r * 8 + 2];
    }
    bool full = false;
    if (n <= SMALL_RING) {
      for (int k = 0; k < n; ++k) fn(pack(vertices[(int64_t)start + k]));
    } else {
      const uint32_t slot = atomicAdd(s_nbig, 1u);         // at most max_rings
      if (slot < (uint32_t)BIG_LIST) s_big[slot] = make_int2(start, n);
      else full = true;
    }
    u64 big = __ballot(full);
    for (int step = 0; step < 64 && big; ++step) {         // uniform: the shuffles see every lane
      const int src = __ffsll((long long)big) - 1;
      big &= big - 1;
      const int64_t s0 = __shfl(start, src);
      const int n0 = __shfl(n, src);
      for (int k = lane; k < n0; k += 64) fn(pack(vertices[s0 + k]));
    }
  }
  __syncthreads();
  const int listed = (int)(*s_nbig < (uint32_t)BIG_LIST ? *s_nbig : (uint32_t)BIG_LIST);
  for (int i = 0; i < listed; ++i) {
    const int2 d = s_big[i];
    if (d.y > MID_RING) {
      for (int k = threadIdx.x; k < d.y; k += BLOCK_T) fn(pack(vertices[(int64_t)d.x + k]));
    } else if (i % WAVES == wave) {
      for (int k = lane; k < d.y; k += 64) fn(pack(vertices[(int64_t)d.x + k]));
    }
  }
}

// the eight extremes: the value in the high word, the point in the low one; slots 0..3 are minima, 4..7 maxima.  In the order
// of the walk (top goes +x, then +y) the extreme points are: min y, max x-y, max x, max x+y, max y, min x-y, min x, min x+y
__device__ __forceinline__ u64 ext_key(int value, uint32_t p) { return ((u64)(uint32_t)(value + 32768) << 32) | p; }

template <bool WRITE>
__global__ __launch_bounds__(BLOCK_T) void hull_block_kernel(const int32_t* __restrict__ rings, const int2* __restrict__ vertices,
                                                             const u64* __restrict__ npts, const uint32_t* __restrict__ cnt,
                                                             const uint32_t* __restrict__ off, const uint32_t* __restrict__ grouped,
                                                             const uint32_t* __restrict__ large, const uint32_t* __restrict__ header,
                                                             int max_hull_vertices, int32_t* __restrict__ hulls,
                                                             int2* __restrict__ hull_vertices, int64_t* __restrict__ rects,
                                                             u64* __restrict__ stage_ctr, uint32_t* __restrict__ stage_at,
                                                             uint32_t* __restrict__ stage, int max_vertices) {
  extern __shared__ u64 lds[];
  u64* s_ext = lds;                                        // [8]
  u64* s_wc = s_ext + 8;                                   // [WAVES]
  u64* s_L = s_wc + WAVES;                                 // [WAVES]
  int* s_k = reinterpret_cast<int*>(s_L + WAVES);          // [WAVES]
  uint32_t* s_part = reinterpret_cast<uint32_t*>(s_k + WAVES);   // [WAVES]
  uint32_t* s_n = s_part + WAVES;                          // candidates found; [1] the shoelace sum; [2] the listed rings
  uint32_t* s_nbig = s_n + 2;
  int2* s_big = reinterpret_cast<int2*>(s_n + 4);          // [BIG_LIST]
  uint32_t* s_pts = reinterpret_cast<uint32_t*>(s_big + BIG_LIST);   // [LDS_LIMIT]
  uint32_t* s_hull = s_pts + LDS_LIMIT;                    // [HULL_CAP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t n_large = header[WS_LARGE];
  for (uint32_t li = blockIdx.x; li < n_large; li += gridDim.x) {
    const int id = (int)large[li];
    const int start_out = WRITE ? hulls[(int64_t)(id - 1) * 8 + 1] : -1;
    if (WRITE && start_out < 0) continue;                  // uniform
    if (WRITE && stage_at[id - 1] != NONE) {               // uniform: the first pass kept this hull, the usual case
      const int64_t sa = stage_at[id - 1];
      const int m = hulls[(int64_t)(id - 1) * 8 + 2];
      for (int k = tid; k < m; k += BLOCK_T) {
        const uint32_t p = stage[sa + k];
        if ((int64_t)start_out + k < max_hull_vertices) hull_vertices[(int64_t)start_out + k] = make_int2(px(p), py(p));
      }
      continue;
    }
    const u64 np = npts[id - 1];
    const uint32_t nr = cnt[id - 1], at = off[id - 1];
    __syncthreads();                                       // the id before is done with the LDS
    if (tid < 8) s_ext[tid] = tid < 4 ? ~0ull : 0ull;
    if (tid == 8) s_n[0] = s_n[1] = 0;
    __syncthreads();
    {                                                      // sweep 1: the extreme points of eight directions
      u64 e[8];
      for (int j = 0; j < 8; ++j) e[j] = j < 4 ? ~0ull : 0ull;
      each_point(rings, vertices, grouped, at, nr, s_big, s_nbig, [&](uint32_t p) {
        const int x = px(p), y = py(p);
        const u64 k0 = ext_key(y, p), k1 = ext_key(x, p), k2 = ext_key(x - y, p), k3 = ext_key(x + y, p);
        e[0] = k0 < e[0] ? k0 : e[0];
        e[1] = k1 < e[1] ? k1 : e[1];
        e[2] = k2 < e[2] ? k2 : e[2];
        e[3] = k3 < e[3] ? k3 : e[3];
        e[4] = k0 > e[4] ? k0 : e[4];
        e[5] = k1 > e[5] ? k1 : e[5];
        e[6] = k2 > e[6] ? k2 : e[6];
        e[7] = k3 > e[7] ? k3 : e[7];
      });
      for (int j = 0; j < 4; ++j) {
        const u64 lo = wave_min64(e[j]), hi = wave_max64(e[4 + j]);
        if (lane == 0) {
          atomicMin(s_ext + j, lo);
          atomicMax(s_ext + 4 + j, hi);
        }
      }
    }
    __syncthreads();
    uint32_t oct[8];                                       // in the order of the walk
    {
      const int order[8] = {0, 6, 5, 7, 4, 2, 1, 3};       // min y, max x-y, max x, max x+y, max y, min x-y, min x, min x+y
      for (int j = 0; j < 8; ++j) oct[j] = (uint32_t)s_ext[order[j]];
    }
    int sides = 0;
    for (int j = 0; j < 8; ++j) sides += oct[j] != oct[(j + 1) & 7];
    // sweep 2: what is not strictly inside the octagon of these points is a candidate
    each_point(rings, vertices, grouped, at, nr, s_big, s_nbig, [&](uint32_t p) {
      bool inside = sides > 0;
      for (int j = 0; j < 8; ++j) {
        const uint32_t a = oct[j], b = oct[(j + 1) & 7];
        if (a != b) inside = inside && cross3(a, b, p) > 0;
      }
      if (inside) return;
      const uint32_t slot = atomicAdd(s_n, 1u);            // fewer than 2^32: the points of the used rows of one table
      if (slot < (uint32_t)LDS_LIMIT) s_pts[slot] = p;
    });
    __syncthreads();
    const uint32_t found = s_n[0];
    const bool in_lds = found <= (uint32_t)LDS_LIMIT;      // always, for an id of up to LDS_LIMIT points
    const int n_cand = in_lds ? (int)found : 0;
    // one step of the walk: the best successor of cur over all points, the same in every thread
    auto successor = [&](uint32_t cur) {
      uint32_t b = NONE;
      if (in_lds) {
        for (int k = tid; k < n_cand; k += BLOCK_T) {
          const uint32_t p = s_pts[k];
          if (p != cur) b = better(cur, b, p);
        }
      } else {
        each_point(rings, vertices, grouped, at, nr, s_big, s_nbig, [&](uint32_t p) {
          if (p != cur) b = better(cur, b, p);
        });
      }
      b = wave_better(cur, b);
      if (lane == 0) s_part[wave] = b;
      __syncthreads();
      b = s_part[lane & (WAVES - 1)];                      // every wave reduces the WAVES partial results once more
      for (int d = WAVES / 2; d; d >>= 1) b = better(cur, b, (uint32_t)__shfl_xor((int)b, d));
      __syncthreads();
      return b;
    };
    const uint32_t h0 = oct[0];                            // min (y, x): the key of slot 0 orders by y, then by the point
    const u64 cap64 = np < (u64)HULL_CAP ? np : (u64)HULL_CAP;
    const int cap = (int)cap64;
    uint32_t cur = h0;
    int m = 0;
    for (int step = 0; step < cap; ++step) {
      if (tid == 0) s_hull[step] = cur;
      m = step + 1;
      const uint32_t next = successor(cur);
      if (next == NONE || next == h0) break;               // uniform
      cur = next;
    }
    __syncthreads();
    if (WRITE) {
      for (int k = tid; k < m; k += BLOCK_T)
        if ((int64_t)start_out + k < max_hull_vertices) hull_vertices[(int64_t)start_out + k] = make_int2(px(s_hull[k]), py(s_hull[k]));
      continue;
    }
    uint32_t acc = 0;
    for (int k = tid; k < m; k += BLOCK_T) {
      const uint32_t a = s_hull[k], b = s_hull[k + 1 == m ? 0 : k + 1];
      acc += (uint32_t)(px(a) * py(b) - px(b) * py(a));    // modular; the sum is below 2^30
    }
    acc = wave_sum32(acc);
    if (lane == 0 && acc) atomicAdd(s_n + 1, acc);
    if (tid == 0) {                                        // room for the hull in the staging list, so that 9 need not walk again
      const u64 slot = atomicAdd(stage_ctr, (u64)m);
      s_n[3] = slot + (u64)m <= (u64)max_vertices ? (uint32_t)slot : NONE;
      stage_at[id - 1] = s_n[3];
    }
    Rect best;
    best.k = INT_MAX;
    best.wc = best.L = 0;
    if (m >= 3) {
      for (int k = tid; k < m; k += BLOCK_T) {             // ascending k: a tie keeps the earlier edge
        const Rect r = edge_rect([&](int j) { return s_hull[j]; }, m, k);
        if (rect_less(r.wc, r.L, r.k, best.wc, best.L, best.k)) best = r;
      }
    }
    u64 wc = best.wc, L = best.L;
    int k = best.k;
    for (int d = 32; d; d >>= 1) {
      const u64 owc = shfl_xor64(wc, d), oL = shfl_xor64(L, d);
      const int ok = __shfl_xor(k, d);
      if (rect_less(owc, oL, ok, wc, L, k)) { wc = owc; L = oL; k = ok; }
    }
    if (lane == 0) { s_wc[wave] = wc; s_L[wave] = L; s_k[wave] = k; }
    __syncthreads();
    for (int w = 0; w < WAVES; ++w)
      if (rect_less(s_wc[w], s_L[w], s_k[w], wc, L, k)) { wc = s_wc[w]; L = s_L[w]; k = s_k[w]; }
    if (tid == 0) {
      int4* row = reinterpret_cast<int4*>(hulls + (int64_t)(id - 1) * 8);
      row[0] = make_int4(id, -1, m, (int)s_n[1]);          // start: the scan's
      row[1] = make_int4(0, px(h0), py(h0), npts_i32(np));
      if (m < 3) write_no_rect(rects, id);
    }
    if (m >= 3 && best.k == k) write_rect(rects, id, best);   // one thread: the edges are distinct
    const uint32_t sa = s_n[3];                            // written before the barrier above
    if (sa != NONE)
      for (int j = tid; j < m; j += BLOCK_T) stage[(int64_t)sa + j] = s_hull[j];
  }
}

// start = the hull vertices of the ids before, -1 from the first id whose hull does not fit; counts_out.  One workgroup.
__global__ __launch_bounds__(SCAN_T) void hull_starts_kernel(const int32_t* __restrict__ counts, const u64* __restrict__ npts,
                                                             const uint32_t* __restrict__ header, int max_hull_vertices,
                                                             int32_t* __restrict__ hulls, int32_t* __restrict__ counts_out) {
  extern __shared__ u64 spart[];                            // [SCAN_T / 64], then the vertices written and the ids with points
  u64& s_written = spart[SCAN_T / 64];
  uint32_t& s_ids = *reinterpret_cast<uint32_t*>(spart + SCAN_T / 64 + 1);
  const int K = (int)header[WS_K];
  const int lane = threadIdx.x & 63;
  if (threadIdx.x == 0) { s_written = ~0ull; s_ids = 0; }
  __syncthreads();
  u64 running = 0;
  for (int base = 0; base < K; base += SCAN_T * SCAN_ROWS) {
    uint32_t n[SCAN_ROWS], with_points = 0;
    u64 mine = 0;
    for (int j = 0; j < SCAN_ROWS; ++j) {
      const int i = base + (int)threadIdx.x * SCAN_ROWS + j;
      n[j] = i < K ? (uint32_t)hulls[(int64_t)i * 8 + 2] : 0u;
      with_points += i < K && npts[i] != 0;
      mine += n[j];
    }
    with_points = wave_sum32(with_points);
    if (lane == 0 && with_points) atomicAdd(&s_ids, with_points);
    u64 all;
    u64 at = running + block_excl_scan64(mine, spart, &all);
    for (int j = 0; j < SCAN_ROWS; ++j) {
      const int i = base + (int)threadIdx.x * SCAN_ROWS + j;
      if (i < K && n[j]) {
        // `at` only grows: once at + n exceeds the room it does so for every later id with a vertex, the prefix shape
        const bool fits = at + n[j] <= (u64)max_hull_vertices;
        hulls[(int64_t)i * 8 + 1] = fits ? (int)at : -1;
        if (!fits) atomicMin(&s_written, at);
      }
      at += n[j];
    }
    running += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const bool truncated = s_written != ~0ull;
    if (counts[4] & C3D_OUTLINE_ST_BAD_COUNTS) {
      counts_out[0] = counts_out[1] = counts_out[2] = counts_out[3] = 0;
      counts_out[4] = C3D_OUTLINE_ST_BAD_COUNTS;
    } else {
      counts_out[0] = (int32_t)s_ids;
      counts_out[1] = K;
      counts_out[2] = running > (u64)INT_MAX ? INT_MAX : (int32_t)running;
      counts_out[3] = (int32_t)(truncated ? s_written : running);   // at most max_hull_vertices
      counts_out[4] = (int32_t)((uint32_t)counts[4] | header[WS_STATUS] | (truncated ? (uint32_t)C3D_HULL_ST_TRUNCATED : 0u));
    }
  }
}

int refuse(int32_t max_rings, int32_t max_vertices, int32_t max_objects) {
  if (max_rings < 1 || max_vertices < 1 || max_objects < 1) return C3D_E_BADARG;
  return 0;
}

}  // namespace

extern "C" void c3d_rings_hull_limits(int32_t out[2]) {
  if (!out) return;
  out[0] = WAVE_LIMIT;
  out[1] = LDS_LIMIT;
}

extern "C" int64_t c3d_rings_hull_ws_bytes(int32_t max_rings, int32_t max_vertices, int32_t max_objects) {
  const int rc = refuse(max_rings, max_vertices, max_objects);
  if (rc) return rc;
  return plan_of(nullptr, max_rings, max_vertices, max_objects).bytes;
}

extern "C" int c3d_rings_hull(const int32_t* rings, const int32_t* vertices, const int32_t* counts, int32_t max_rings,
                              int32_t max_vertices, int32_t max_objects, int32_t max_hull_vertices, int32_t* hulls,
                              int32_t* hull_vertices, int64_t* rects, int32_t* counts_out, void* ws, void* stream) {
  if (!rings || !vertices || !counts || !hulls || !hull_vertices || !rects || !counts_out || !ws) return C3D_E_BADARG;
  if (max_hull_vertices < 1) return C3D_E_BADARG;
  int rc = refuse(max_rings, max_vertices, max_objects);
  if (rc) return rc;
  const Plan pl = plan_of(ws, max_rings, max_vertices, max_objects);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint32_t* header = static_cast<uint32_t*>(ws);
  Groups g = pl.g;
  g.rings = rings; g.vertices = reinterpret_cast<const int2*>(vertices); g.counts = counts;
  u64* npts = pl.npts;
  uint32_t *cnt = g.cnt, *off = g.off, *large = pl.large, *grouped = g.grouped, *stage_at = pl.stage_at, *stage = pl.stage;
  u64* stage_ctr = reinterpret_cast<u64*>(header + WS_STAGED);
  const int2* v_in = g.vertices;
  int2* hv = reinterpret_cast<int2*>(hull_vertices);

  // only the header: every other word of the workspace is written by the call before the call reads it
  hipError_t e = hipMemsetAsync(ws, 0, 256, st);
  if (e != hipSuccess) return (int)e;
  // ring and id counts are known on the device only: grids are sized by the limits and surplus waves and workgroups return
  const unsigned g_ids = grid_for(max_objects, 256, MAX_GRID), g_idw = grid_for(max_objects, 4, MAX_GRID);
  const unsigned g_rows = grid_for(max_rings, 256, MAX_GRID);
  const unsigned g_list = (unsigned)(max_objects < LIST_GRID ? max_objects : LIST_GRID);
  rc = c3d_launch_lds<hull_init_kernel>(dim3(g_ids), dim3(256), 0, st, npts, cnt, g.cursor, (int)max_objects);
  if (rc) return rc;
  rc = c3d_launch_lds<hull_group_kernel>(dim3(g_rows), dim3(256), 0, st, g, npts, header);
  if (rc) return rc;
  rc = c3d_launch_lds<hull_scan_kernel>(dim3(1), dim3(SCAN_T), SCAN_T / 64 * 4, st, g);
  if (rc) return rc;
  rc = c3d_launch_lds<hull_scatter_kernel>(dim3(g_rows), dim3(256), 0, st, g);
  if (rc) return rc;
  rc = c3d_launch_lds<hull_wave_kernel<false>>(dim3(g_idw), dim3(256), 0, st, rings, v_in, (const u64*)npts, (const uint32_t*)cnt,
                                               (const uint32_t*)off, (const uint32_t*)grouped, large, header, (int)max_objects,
                                               (int)max_hull_vertices, hulls, hv, rects);
  if (rc) return rc;
  rc = c3d_launch_lds<hull_block_kernel<false>>(dim3(g_list), dim3(BLOCK_T), LDS_BYTES, st, rings, v_in, (const u64*)npts,
                                                (const uint32_t*)cnt, (const uint32_t*)off, (const uint32_t*)grouped,
                                                (const uint32_t*)large, (const uint32_t*)header, (int)max_hull_vertices, hulls, hv,
                                                rects, stage_ctr, stage_at, stage, (int)max_vertices);
  if (rc) return rc;
  rc = c3d_launch_lds<hull_starts_kernel>(dim3(1), dim3(SCAN_T), SCAN_T / 8 + 16, st, counts, (const u64*)npts,
                                          (const uint32_t*)header, (int)max_hull_vertices, hulls, counts_out);
  if (rc) return rc;
  rc = c3d_launch_lds<hull_wave_kernel<true>>(dim3(g_idw), dim3(256), 0, st, rings, v_in, (const u64*)npts, (const uint32_t*)cnt,
                                              (const uint32_t*)off, (const uint32_t*)grouped, large, header, (int)max_objects,
                                              (int)max_hull_vertices, hulls, hv, rects);
  if (rc) return rc;
  return c3d_launch_lds<hull_block_kernel<true>>(dim3(g_list), dim3(BLOCK_T), LDS_BYTES, st, rings, v_in, (const u64*)npts,
                                                 (const uint32_t*)cnt, (const uint32_t*)off, (const uint32_t*)grouped,
                                                 (const uint32_t*)large, (const uint32_t*)header, (int)max_hull_vertices, hulls, hv,
                                                 rects, stage_ctr, stage_at, stage, (int)max_vertices);
}
