// Crossing-free shared walls: the shared-wall simplification of csrc/scene_shared.hip run in rounds, each arc with a tolerance
// of its own.  A round simplifies every ring with the current levels, finds the defective pairs of output edges and the defective
// rings, and raises the level of every arc that takes part in one; the loop ends when a round finds nothing.  The rule -- the
// arc key, the level, the defective pair and ring, the stopping rules -- is the header's (include/change3d_hip.h,
// c3d_outlines_simplify_safe); this file is one way to compute it.  Integer arithmetic and integer atomics only.  The passes
// from the node bitmaps to the scatter, the three-tier Douglas-Peucker body among them, are csrc/scene_walls.h's, which
// csrc/scene_shared.hip runs too; the policy `Levelled` below says what the rounds add to them.  The build of the cell grid is
// csrc/scene_grid.h's, which csrc/scene_conflicts.hip runs too, and the class of a pair is csrc/scene_rings.h's.  This file holds
// the policy and the kernels around those passes, the level store, the key pass, the detector's entry and pair rule, raise, tail
// and the entries.
//
// Once, before round 0:
//   nodes, count, scan_rows, augment   scene_walls.h's, as in scene_shared.hip; augment also keeps the direction of the edge leaving every vertex
//   keys       whoever owns a ring (a wave up to WAVE_LIMIT augmented vertices, a workgroup beyond): the arc of every vertex by
//              an exclusive max-scan over the node flags, the key of every arc from its two end steps, the key of its arc for
//              every vertex, and the `present` bit of the key in the level store; arcs, closed arcs, arcs with a left label
// Every round, each kernel returning at once when the device word WS_DONE is set:
//   dp         the three tiers of scene_shared.hip; the level of an arc is read at its first vertex when the chord starts of
//              round 0 are set up and kept in the arc word of that vertex, so the split test costs two LDS reads more
//   scan_kept, scatter   as there; the scatter also writes level_out, the row, index and key of the edge leaving every output
//              vertex, and marks every arc of a defective ring
//   edges      a thread per output vertex: the edge (a, b) that leaves it, the live count, the box of the live edges
//   cost, choose, zero, count, starts, fill   the grid of scene_grid.h over the live edges
//   wave, jobs the pairs of a cell by the lower-corner rule, same-id pairs included; a defective pair ORs the mark bit of both
//              keys into the level store and counts once
//   raise      a thread per word of the level store (a word per lattice point, a byte per direction): counts the arcs above
//              level 0 and at the cap, clears the marks, adds 1 below the cap
//   tail       one workgroup: the stopping rules, `safe`, the grid columns of info, and zeroes the round's header
// Every ring is simplified again in every round: a round is a fixed sequence of launches without a list of rings to redo.
// No workgroup waits for another, nothing is read back, every loop is capped by a count that was checked against the workspace.
#include <climits>

#include "scene_grid.h"
#include "scene_rings.h"
#include "scene_walls.h"

namespace {

using namespace c3d_walls;
using namespace c3d_grid;
using c3d_rings::live_of;

// the level store: a byte per arc key = a word per lattice point, the byte of direction d at bits 8 d
constexpr uint32_t LV_LEVEL = 0x3Fu, LV_PRESENT = 0x40u, LV_MARK = 0x80u;
constexpr int PAIR_T = 256;
constexpr int CELL_GRID = 4096;

// words of the call's header (256 bytes, zeroed by the memset) behind those of scene_walls.h
enum { WS_WRITTEN = 6, WS_DONE = 16, WS_ROUND = 17, WS_RUN = 18, WS_RAISED = 19, WS_RINGS0 = 20, WS_PAIRS0 = 22 /* u64 */ };
// words of the round's header (512 bytes behind the call's; zeroed by the memset and by every round's tail)
enum { RH_EDGES = 0, RH_LO_X = 1, RH_LO_Y = 2, RH_HI_X = 3, RH_HI_Y = 4, RH_SHIFT = 5, RH_CX = 6, RH_CY = 7, RH_X0 = 8, RH_Y0 = 9,
       RH_AT = 10, RH_JOBS = 11, RH_BAD_RINGS = 12, RH_UP = 13, RH_ABOVE = 14, RH_AT_CAP = 15 };
// 64-bit words of the round's header, counted from its byte 64
enum { RQ_WORK = 0, RQ_ENTRIES = 1, RQ_PAIRS = 2, RQ_COST = 4 /* N_SHIFT of them */ };
constexpr int HEADER_BYTES = 256 + 512;
static_assert(64 + (RQ_COST + N_SHIFT) * 8 <= 512, "the round's header holds the cost of every shift");
// where scene_grid.h finds the grid's words in the round's header
struct Words {
  enum { LO_X = RH_LO_X, LO_Y = RH_LO_Y, HI_X = RH_HI_X, HI_Y = RH_HI_Y, SHIFT = RH_SHIFT, CX = RH_CX, CY = RH_CY, X0 = RH_X0, Y0 = RH_Y0,
         AT = RH_AT, JOBS = RH_JOBS, Q_WORK = RQ_WORK, Q_ENTRIES = RQ_ENTRIES, Q_COST = RQ_COST };
};

struct Workspace : Space {                                 // the arrays of scene_walls.h behind the two headers, then this file's
  int64_t dirs, vkey, levels, e_key, e_info, e_xy, cell_n, cell_at, entry, jobs, bytes;   // byte offsets
  int64_t level_words, cap_e, cap_c, cap_j;
};

Workspace workspace_plan(int64_t Hs, int64_t Ws, int64_t max_rings, int64_t max_vertices, int64_t max_out) {
  Workspace w;
  static_cast<Space&>(w) = space_plan(HEADER_BYTES, Hs, Ws, max_rings, max_vertices);
  auto up = up256;
  const int64_t A = 2 * max_vertices;
  w.dirs = w.end;
  w.vkey = w.dirs + up(A);
  w.level_words = (Hs + 1) * (Ws + 1);
  w.levels = w.vkey + up(A * 4);
  // both budgets hold for one cell whatever the output holds (at most max_out live edges, one entry each): the sizes are a
  // function of max_vertices_out alone
  w.cap_e = BUDGET_E * max_out;
  w.cap_c = BUDGET_C * max_out;
  w.cap_j = jobs_cap(w.cap_e);
  w.e_key = w.levels + up(w.level_words * 4);
  w.e_info = w.e_key + up(max_out * 4);
  w.e_xy = w.e_info + up(max_out * 16);
  w.cell_n = w.e_xy + up(max_out * 16);
  w.cell_at = w.cell_n + up(w.cap_c * 4);
  w.entry = w.cell_at + up(w.cap_c * 4);
  w.jobs = w.entry + up(w.cap_e * 4);
  w.bytes = w.jobs + up(w.cap_j * 8);
  return w;
}

// the word and the shift of a key's byte in the level store
__device__ __forceinline__ uint32_t key_of(int2 v, int dir, int Ws) { return 4u * (uint32_t)(v.y * (Ws + 1) + v.x) + (uint32_t)dir; }
__device__ __forceinline__ void level_or(uint32_t* __restrict__ level_words, uint32_t key, uint32_t bit) {
  atomicOr(level_words + (key >> 2), bit << (8 * (key & 3u)));
}

// ------------------------------------------------------------------------------------------- keys: once, a ring per owner
// vkey[k] = the key of the arc of vertex k of the rotated ring: min(key(s, first unit step), key(e, reverse of the last unit
// step)) of the arc s .. e.  link and arc are the dp's workspace arrays, free until round 0.  T = 64: the rings of up to
// WAVE_LIMIT augmented vertices; T = BLOCK_T: the listed larger ones.
template <int T>
__global__ __launch_bounds__(T) void safe_keys_kernel(const int32_t* __restrict__ naug, const uint32_t* __restrict__ off,
                                                      const uint32_t* __restrict__ rot, const uint32_t* __restrict__ ap,
                                                      const uint32_t* __restrict__ meta, const uint8_t* __restrict__ dirs,
                                                      int32_t* __restrict__ g_link, int32_t* __restrict__ g_arc,
                                                      uint32_t* __restrict__ g_vkey, uint32_t* __restrict__ level_words,
                                                      const uint32_t* __restrict__ large, uint32_t* __restrict__ header, int Ws) {
  extern __shared__ int part_k[];                          // [16]
  const bool wave_tier = T == 64;
  const uint32_t items = wave_tier ? header[WS_ROWS] : header[WS_LARGE];
  const int tid = threadIdx.x;
  for (uint32_t at = blockIdx.x; at < items; at += gridDim.x) {
    const int r = wave_tier ? (int)at : (int)large[at];
    const int n = naug[r];
    if (n < 0 || (wave_tier ? n > WAVE_LIMIT : n <= WAVE_LIMIT)) continue;   // uniform over the workgroup
    const int64_t o = off[r];
    const int s = (int)rot[r];
    auto where = [&](int k) { const int j = k + s; return o + (j >= n ? j - n : j); };
    int* link = g_link + o;
    int* arc = g_arc + o;
    uint32_t* vkey = g_vkey + o;
    int last = -1;
    for (int base = 0; base < n; base += T) {              // arc[k] = the first vertex of the arc of k, link[a] = its end
      const int k = base + tid;
      const bool node = k < n && (k == 0 || (meta[where(k)] & NODE_BIT));
      int top;
      int e = block_excl_max32(node ? k : -1, part_k, &top);
      e = e > last ? e : last;
      last = top > last ? top : last;
      if (k < n) {
        arc[k] = node ? k : e;
        if (node && k > 0) link[e] = k;
      }
      __syncthreads();                                     // part_k is reused by the next step
    }
    if (tid == 0) link[last] = n;                          // the arc of the last node ends at the closing repeat of vertex 0
    __syncthreads();
    for (int k = tid; k < n; k += T) {
      if (arc[k] != k) continue;
      const int end = link[k];                             // k < end <= n
      const int2 p = unpack(ap[where(k)]), q = unpack(ap[where(end == n ? 0 : end)]);
      const uint32_t fwd = key_of(p, dirs[where(k)], Ws), back = key_of(q, (dirs[where(end - 1)] + 2) & 3, Ws);
      const uint32_t key = fwd < back ? fwd : back;
      vkey[k] = key;
      level_or(level_words, key, LV_PRESENT);
      atomicAdd(header + WS_INFO + INFO_ARCS, 1u);
      if (p.x == q.x && p.y == q.y) atomicAdd(header + WS_INFO + INFO_CLOSED, 1u);
      if (meta[where(k)] & ~NODE_BIT) atomicAdd(header + WS_INFO + INFO_SHARED, 1u);
    }
    __syncthreads();
    for (int k = tid; k < n; k += T)
      if (arc[k] != k) vkey[k] = vkey[arc[k]];
    __syncthreads();                                       // the next ring reuses part_k
  }
}

// what the scatter adds to the shared call's: the level and the key of the arc of every output edge, its place in the table, and
// the marks of the arcs of a defective ring
struct Marks {
  const uint32_t* vkey;                                    // [2 max_vertices] in rotated order
  uint32_t* level_words;
  int32_t* level_out;
  uint32_t* e_key;                                         // [max_vertices_out]
  int4* e_info;                                            // [max_vertices_out] (id, ring row, k, n')
  uint32_t* round;                                         // the round's header
};

// ------------------------------------------------------------------------------------ the passes of scene_walls.h, levelled
// An arc word carries the level above the closed bit; the key pass counts the arcs; every pass of a round returns at once when
// the done word is set; the kept-scan leaves the written count for the detector; the scatters fill Marks.
struct Levelled {
  static constexpr bool LEVELLED = true;
  struct Levels {
    const uint32_t* vkey;                                  // [2 max_vertices] in rotated order
    const uint8_t* levels;                                 // the level store by bytes
  };
  typedef ::Marks Marks;
  static __device__ __forceinline__ int level(const Levels& lv, int64_t i) { return (int)(lv.levels[lv.vkey[i]] & LV_LEVEL); }
  static __device__ __forceinline__ int arc_word(bool closed, int level) { return ~((closed ? 1 : 0) | (level << 1)); }
  static __device__ __forceinline__ bool arc_closed(int word) { return (~word) & 1; }
  static __device__ __forceinline__ int arc_level(int word) { return (~word) >> 1; }
  static __device__ __forceinline__ bool done(const uint32_t* header) { return header[WS_DONE] != 0; }
  static __device__ __forceinline__ void written(uint32_t* header, uint32_t v) { header[WS_WRITTEN] = v; }
  static __device__ __forceinline__ uint32_t key_at(const Marks& mk, int64_t i) { return mk.vkey[i]; }
  static __device__ __forceinline__ uint32_t out_key(const Marks& mk, int64_t to) { return mk.e_key[to]; }
  static __device__ __forceinline__ void edge_out(const Marks& mk, int64_t to, uint32_t key, int id, int row, int k, int n) {
    mk.level_out[to] = (int32_t)(reinterpret_cast<const uint8_t*>(mk.level_words)[key] & LV_LEVEL);
    mk.e_key[to] = key;
    mk.e_info[to] = make_int4(id, row, k, n);
  }
  // n' < 3, or an area whose sign is not that of the input row
  static __device__ __forceinline__ bool ring_defective(int count, int area2, int area_in) {
    return count < 3 || ((area2 > 0) - (area2 < 0)) != ((area_in > 0) - (area_in < 0));
  }
  static __device__ __forceinline__ void mark(const Marks& mk, uint32_t key) { level_or(mk.level_words, key, LV_MARK); }
  static __device__ __forceinline__ void bad_ring(const Marks& mk) { atomicAdd(mk.round + RH_BAD_RINGS, 1u); }
};

template <bool COLS>
__global__ __launch_bounds__(256) void safe_nodes_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ counts_obj,
                                                           int Hs, int Ws, int max_objects, uint32_t* __restrict__ bits, int words) {
  nodes_pass<COLS>(labels, counts_obj, Hs, Ws, max_objects, bits, words);
}

__global__ __launch_bounds__(256) void safe_count_rows_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ counts_obj,
                                                           int Hs, int Ws, int max_objects, const int32_t* __restrict__ rings,
                                                           const int2* __restrict__ vertices, const int32_t* __restrict__ counts,
                                                           int max_rings, int max_vertices, int32_t* __restrict__ naug, Bits bits) {
  count_pass(labels, counts_obj, Hs, Ws, max_objects, rings, vertices, counts, max_rings, max_vertices, naug, bits);
}

__global__ __launch_bounds__(BLOCK_T) void safe_scan_rows_kernel(const int32_t* __restrict__ counts, int32_t* __restrict__ naug,
                                                               uint32_t* __restrict__ off, uint32_t* __restrict__ large,
                                                               uint32_t* __restrict__ header, int max_rings, int max_vertices) {
  extern __shared__ u64 part[];                            // [BLOCK_T / 64]
  scan_rows_pass(counts, naug, off, large, header, max_rings, max_vertices, part);
}

__global__ __launch_bounds__(256) void safe_augment_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ counts_obj,
                                                             int Hs, int Ws, int max_objects, const int32_t* __restrict__ rings,
                                                             const int2* __restrict__ vertices, const int32_t* __restrict__ naug,
                                                             const uint32_t* __restrict__ off, uint32_t* __restrict__ rot,
                                                             uint32_t* __restrict__ ap, uint32_t* __restrict__ meta,
                                                             uint8_t* __restrict__ dirs, uint32_t* __restrict__ header, Bits bits) {
  augment_pass<Levelled>(labels, counts_obj, Hs, Ws, max_objects, rings, vertices, naug, off, rot, ap, meta, dirs, header, bits);
}

// T = 64: the rings of up to WAVE_LIMIT augmented vertices, a wave each; T = BLOCK_T: the listed larger ones
template <int T, int LIMIT>
__global__ __launch_bounds__(T) void safe_dp_kernel(const int32_t* __restrict__ naug, const uint32_t* __restrict__ off,
                                                      const uint32_t* __restrict__ rot, const uint32_t* __restrict__ ap,
                                                      const uint32_t* __restrict__ meta, int32_t* __restrict__ kept,
                                                      uint8_t* __restrict__ flags, int32_t* __restrict__ g_link,
                                                      int32_t* __restrict__ g_arc, u64* __restrict__ g_idx, u64* __restrict__ g_best,
                                                      const uint32_t* __restrict__ large, const uint32_t* __restrict__ header,
                                                      const uint32_t* __restrict__ vkey, const uint8_t* __restrict__ levels, u64 tol2_q) {
  extern __shared__ u64 lds[];
  dp_pass<Levelled, T, LIMIT>(naug, off, rot, ap, meta, kept, flags, g_link, g_arc, g_idx, g_best, large, header,
                              Levelled::Levels{vkey, levels}, tol2_q, lds);
}

__global__ __launch_bounds__(BLOCK_T) void safe_scan_kept_kernel(const int32_t* __restrict__ kept, uint32_t* __restrict__ startp,
                                                               uint32_t* __restrict__ header, int32_t* __restrict__ counts_out,
                                                               int32_t* __restrict__ info, int max_vertices_out) {
  extern __shared__ u64 part[];                            // [BLOCK_T / 64], then the first start without room
  scan_kept_pass<Levelled>(kept, startp, header, counts_out, info, max_vertices_out, part);
}

__global__ __launch_bounds__(256) void safe_scatter_wave_kernel(const int32_t* __restrict__ rings, const int32_t* __restrict__ naug,
                                                                  const uint32_t* __restrict__ off, const uint32_t* __restrict__ rot,
                                                                  const uint32_t* __restrict__ ap, const uint32_t* __restrict__ meta,
                                                                  const int32_t* __restrict__ kept, const uint32_t* __restrict__ startp,
                                                                  const uint8_t* __restrict__ flags, const uint32_t* __restrict__ header,
                                                                  int32_t* __restrict__ rings_out, int2* __restrict__ vertices_out,
                                                                  int32_t* __restrict__ left_out, int32_t* __restrict__ info,
                                                                  int max_rings, Marks mk) {
  scatter_wave_pass<Levelled>(rings, naug, off, rot, ap, meta, kept, startp, flags, header, rings_out, vertices_out, left_out, info,
                              max_rings, mk);
}

__global__ __launch_bounds__(256) void safe_scatter_block_kernel(const int32_t* __restrict__ rings, const int32_t* __restrict__ naug,
                                                                   const uint32_t* __restrict__ off, const uint32_t* __restrict__ rot,
                                                                   const uint32_t* __restrict__ ap, const uint32_t* __restrict__ meta,
                                                                   const int32_t* __restrict__ kept, const uint32_t* __restrict__ startp,
                                                                   const uint8_t* __restrict__ flags, const uint32_t* __restrict__ large,
                                                                   const uint32_t* __restrict__ header, int32_t* __restrict__ rings_out,
                                                                   int2* __restrict__ vertices_out, int32_t* __restrict__ left_out,
                                                                   int32_t* __restrict__ info, Marks mk) {
  extern __shared__ u64 part[];                            // [4], then the area
  scatter_block_pass<Levelled>(rings, naug, off, rot, ap, meta, kept, startp, flags, large, header, rings_out, vertices_out, left_out,
                               info, mk, part);
}

// ------------------------------------------------------------------------------------------------- the detector's grid
// The flat list of output edges is the output's own vertex order: edge i leaves vertex i.  e_xy[i] = (a, b); a dead edge has
// a == b and takes part in nothing.
struct Det {
  const int2* vertices_out;
  const uint32_t* e_key;
  const int4* e_info;
  int4* e_xy;
  uint32_t* cell_n;                                        // [cap_c] entries of the cell
  uint32_t* cell_at;                                       // [cap_c] where they start; after the fill, where they end
  uint32_t* entry;                                         // [cap_e] edge indices grouped by cell
  uint2* jobs;                                             // [cap_j] (cell, chunk)
  uint32_t* level_words;
  int64_t cap_e, cap_c, cap_j, max_work;
  int max_out;
};
__device__ __forceinline__ uint32_t written_of(const Det& s, const uint32_t* header) {
  return min(header[WS_WRITTEN], (uint32_t)s.max_out);
}
__device__ __forceinline__ bool over_work(const Det& s, const uint32_t* round) { return quad(round)[RQ_WORK] > (u64)s.max_work; }

// a thread per output vertex: the edge that leaves it, the number of live edges and their box
__global__ __launch_bounds__(256) void safe_edges_kernel(Det s, const uint32_t* __restrict__ header, uint32_t* __restrict__ round) {
  if (header[WS_DONE]) return;
  const uint32_t n = written_of(s, header);
  const int lane = threadIdx.x & 63;
  int lo_x = 0, lo_y = 0, hi_x = 0, hi_y = 0;              // biased: BIAS - min and BIAS + max, 0 where nothing was seen
  uint32_t cnt = 0;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int4 in = s.e_info[i];                           // (id, row, k, n'): the ring starts at i - k
    const int2 a = s.vertices_out[i], b = s.vertices_out[i - (uint32_t)in.z + (uint32_t)(in.z + 1 == in.w ? 0 : in.z + 1)];
    const int4 e = make_int4(a.x, a.y, b.x, b.y);
    s.e_xy[i] = e;
    if (live_of(e)) {
      ++cnt;
      lo_x = max(lo_x, BIAS - min(e.x, e.z)); lo_y = max(lo_y, BIAS - min(e.y, e.w));
      hi_x = max(hi_x, BIAS + max(e.x, e.z)); hi_y = max(hi_y, BIAS + max(e.y, e.w));
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo_x = max(lo_x, __shfl_xor(lo_x, o, 64)); lo_y = max(lo_y, __shfl_xor(lo_y, o, 64));
    hi_x = max(hi_x, __shfl_xor(hi_x, o, 64)); hi_y = max(hi_y, __shfl_xor(hi_y, o, 64));
  }
  cnt = wave_sum32(cnt);
  if (lane == 0 && cnt) {
    atomicAdd(round + RH_EDGES, cnt);
    atomicMax(round + RH_LO_X, (uint32_t)lo_x); atomicMax(round + RH_LO_Y, (uint32_t)lo_y);
    atomicMax(round + RH_HI_X, (uint32_t)hi_x); atomicMax(round + RH_HI_Y, (uint32_t)hi_y);
  }
}

// cost, choose, zero, count, starts, fill: csrc/scene_grid.h's, over the live ones of the written edges
__global__ __launch_bounds__(256) void safe_cost_kernel(Det s, const uint32_t* __restrict__ header, uint32_t* __restrict__ round) {
  if (header[WS_DONE]) return;
  cost_pass<Words, true>(cells_of(s), round, written_of(s, header), round[RH_EDGES]);
}
__global__ __launch_bounds__(64) void safe_choose_kernel(Det s, const uint32_t* __restrict__ header, uint32_t* __restrict__ round) {
  if (header[WS_DONE]) return;
  choose_pass<Words>(cells_of(s), round, round[RH_EDGES]);
}
__global__ __launch_bounds__(256) void safe_zero_cells_kernel(Det s, const uint32_t* __restrict__ header, const uint32_t* __restrict__ round) {
  if (header[WS_DONE]) return;
  zero_pass<Words>(cells_of(s), round);
}
__global__ __launch_bounds__(256) void safe_count_kernel(Det s, const uint32_t* __restrict__ header, const uint32_t* __restrict__ round) {
  if (header[WS_DONE]) return;
  count_pass<Words, true>(cells_of(s), round, written_of(s, header));
}
__global__ __launch_bounds__(256) void safe_starts_kernel(Det s, const uint32_t* __restrict__ header, uint32_t* __restrict__ round) {
  if (header[WS_DONE]) return;
  starts_pass<Words>(cells_of(s), round);
}
__global__ __launch_bounds__(256) void safe_fill_kernel(Det s, const uint32_t* __restrict__ header, const uint32_t* __restrict__ round) {
  if (header[WS_DONE] || over_work(s, round)) return;
  fill_pass<Words, true>(cells_of(s), round, written_of(s, header));
}

// ------------------------------------------------------------------------------------------------------------ the pairs
// one entry as the pair kernels hold it: in = (id, ring row, k, n'); a dead e stands for no entry
struct Ent {
  int4 e, in;
  uint32_t key;
};
__device__ __forceinline__ Ent ent_of(const Det& s, uint32_t i) { return Ent{s.e_xy[i], s.e_info[i], s.e_key[i]}; }
// does this cell evaluate the pair: boxes that meet, and the lower corner of their intersection in the cell
__device__ __forceinline__ bool owned(const Grid& g, uint32_t cell_x, uint32_t cell_y, const Ent& p, const Ent& q) {
  if (!live_of(p.e) || !live_of(q.e) || !c3d_rings::boxes_meet(p.e, q.e)) return false;
  const int px = max(min(p.e.x, p.e.z), min(q.e.x, q.e.z)), py = max(min(p.e.y, p.e.w), min(q.e.y, q.e.w));
  return ((uint32_t)(px - g.x0) >> g.shift) == cell_x && ((uint32_t)(py - g.y0) >> g.shift) == cell_y;
}
// the header's defective pair: a cross, a collinear overlap that is no shared wall, a vertex strictly inside a non-adjacent edge
__device__ __forceinline__ bool defective(const Ent& p, const Ent& q) {
  const int d = p.in.z > q.in.z ? p.in.z - q.in.z : q.in.z - p.in.z;
  const bool adjacent = p.in.y == q.in.y && (d == 1 || d == p.in.w - 1);
  const int cls = c3d_rings::pair_class(p.e, q.e, adjacent);
  if (cls == c3d_rings::PAIR_CROSS || cls == c3d_rings::PAIR_VE) return true;
  if (cls != c3d_rings::PAIR_OVERLAP) return false;
  const int64_t dot = (int64_t)(p.e.z - p.e.x) * (q.e.z - q.e.x) + (int64_t)(p.e.w - p.e.y) * (q.e.w - q.e.y);
  return !(p.in.x != q.in.x && dot < 0);
}
__device__ __forceinline__ void pairs_out(uint32_t tally, uint32_t* round) {
  u64 v = wave_sum64((u64)tally);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(quad(round) + RQ_PAIRS, v);
}

// a wave per 64 cells: each cell of 2 .. CELL_WAVE_LIMIT entries in turn, a lane per entry, the partner by shuffle
__global__ __launch_bounds__(256) void safe_pairs_wave_kernel(Det s, const uint32_t* __restrict__ header, uint32_t* __restrict__ round) {
  if (header[WS_DONE] || over_work(s, round)) return;
  const Grid g = grid_of<Words>(round);
  const u64 cells = min((u64)g.cx * g.cy, (u64)s.cap_c);
  const int lane = threadIdx.x & 63;
  uint32_t tally = 0;
  for (u64 c0 = ((u64)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; c0 < cells; c0 += (u64)gridDim.x * 256) {   // uniform over the wave
    const uint32_t mine = c0 + lane < cells ? s.cell_n[c0 + lane] : 0u;
    u64 todo = __ballot(mine >= 2u && mine <= (uint32_t)CELL_WAVE_LIMIT);
    while (todo) {                                         // at most 64 cells
      const int which = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      const u64 c = c0 + which;
      const int cnt = (int)(uint32_t)__shfl((int)mine, which);
      const uint32_t first = s.cell_at[c] - (uint32_t)cnt;   // cell_at is the end since the fill
      const uint32_t cell_x = (uint32_t)(c % g.cx), cell_y = (uint32_t)(c / g.cx);
      Ent own = {make_int4(0, 0, 0, 0), make_int4(0, 0, 0, 0), 0u};
      if (lane < cnt) own = ent_of(s, s.entry[first + lane]);
      // rotation r pairs lane l with lane (l + r) mod cnt: each unordered pair is met at r and at cnt - r, and counts where l
      // is the smaller one
      for (int r = 1; r < cnt; ++r) {
        int other = lane + r;
        other = other >= cnt ? other - cnt : other;
        Ent q;
        q.e = make_int4(__shfl(own.e.x, other), __shfl(own.e.y, other), __shfl(own.e.z, other), __shfl(own.e.w, other));
        const bool near = lane < cnt && lane < other && owned(g, cell_x, cell_y, own, q);
        if (!__any(near)) continue;                        // uniform over the wave: scene_rings.h says why
        q.in = make_int4(__shfl(own.in.x, other), __shfl(own.in.y, other), __shfl(own.in.z, other), __shfl(own.in.w, other));
        q.key = (uint32_t)__shfl((int)own.key, other);
        if (near && defective(own, q)) {
          level_or(s.level_words, own.key, LV_MARK);
          level_or(s.level_words, q.key, LV_MARK);
          ++tally;
        }
      }
    }
  }
  pairs_out(tally, round);
}

// The job (cell, chunk i) of a cell of c chunks compares chunk i with the chunks i, i + 1, .., i + floor(c / 2) (mod c): every
// unordered pair of chunks belongs to exactly one job.  For even c the offset c / 2 joins i and i + c / 2 from both ends, so
// only i < c / 2 takes it; inside chunk i itself a thread takes the partners with a larger index.
__global__ __launch_bounds__(PAIR_T) void safe_pairs_jobs_kernel(Det s, const uint32_t* __restrict__ header, uint32_t* __restrict__ round) {
  extern __shared__ int4 t_edge[];                         // [CHUNK], then int4 [CHUNK], then u32 [CHUNK]
  int4* t_in = t_edge + CHUNK;
  uint32_t* t_key = reinterpret_cast<uint32_t*>(t_in + CHUNK);
  if (header[WS_DONE] || over_work(s, round)) return;
  const Grid g = grid_of<Words>(round);
  const int tid = threadIdx.x;
  const u64 n_jobs = min((u64)round[RH_JOBS], (u64)s.cap_j);
  uint32_t tally = 0;
  for (u64 job = blockIdx.x; job < n_jobs; job += gridDim.x) {
    const uint2 jb = s.jobs[job];
    const u64 cell = jb.x;
    const uint32_t cnt = s.cell_n[cell], first = s.cell_at[cell] - cnt;
    const uint32_t c = (cnt + CHUNK - 1) / CHUNK, i = jb.y;
    if (i >= c) continue;                                  // cannot happen
    const uint32_t cell_x = (uint32_t)(cell % g.cx), cell_y = (uint32_t)(cell / g.cx);
    const uint32_t k = i * CHUNK + (uint32_t)tid;
    Ent own = {make_int4(0, 0, 0, 0), make_int4(0, 0, 0, 0), 0u};
    if (k < cnt) own = ent_of(s, s.entry[first + k]);
    const uint32_t half = c / 2;
    for (uint32_t kk = 0; kk <= half; ++kk) {              // at most cap_e / (2 CHUNK) + 1 steps
      if (kk * 2 == c && i >= half) break;
      const uint32_t base = ((i + kk) % c) * CHUNK;
      const int here = cnt - base < (uint32_t)CHUNK ? (int)(cnt - base) : CHUNK;
      __syncthreads();                                     // the tile before has been read
      Ent mine = {make_int4(0, 0, 0, 0), make_int4(0, 0, 0, 0), 0u};   // past the end: no entry, which takes part in no pair
      if (tid < here) mine = ent_of(s, s.entry[first + base + tid]);
      t_edge[tid] = mine.e; t_in[tid] = mine.in; t_key[tid] = mine.key;
      __syncthreads();
      const int from = !live_of(own.e) ? CHUNK : (kk == 0 ? tid + 1 : 0);   // the diagonal chunk: partners with a larger index only
      for (int t = 0; t < here; ++t) {                     // the same address in every lane
        Ent q;
        q.e = t_edge[t];
        const bool near = t >= from && owned(g, cell_x, cell_y, own, q);
        if (!__any(near)) continue;                        // uniform over the wave; most partners are far away
        q.in = t_in[t];
        q.key = t_key[t];
        if (near && defective(own, q)) {
          level_or(s.level_words, own.key, LV_MARK);
          level_or(s.level_words, q.key, LV_MARK);
          ++tally;
        }
      }
    }
  }
  pairs_out(tally, round);
}

// -------------------------------------------------------------------------------------------------------- raise and tail
// a thread per word of the level store: the arcs above level 0 and at the cap as this round's simplify read them, then every
// marked byte loses its mark and, below the cap, gains a level
__global__ __launch_bounds__(256) void safe_raise_kernel(Det s, const uint32_t* __restrict__ header, uint32_t* __restrict__ round,
                                                         int64_t level_words, int cap) {
  if (header[WS_DONE]) return;
  const bool over = over_work(s, round);
  uint32_t above = 0, at_cap = 0;
  bool up = false;
  for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < level_words; w += (int64_t)gridDim.x * 256) {
    const uint32_t v = s.level_words[w];
    if (!v) continue;
    uint32_t out = v;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const uint32_t b = (v >> (8 * d)) & 0xFFu, level = b & LV_LEVEL;
      if (!(b & LV_PRESENT)) continue;
      above += level > 0;
      at_cap += level == (uint32_t)cap;
      if ((b & LV_MARK) && !over) {
        const bool raise = level < (uint32_t)cap;
        up |= raise;
        out = (out & ~(0xFFu << (8 * d))) | ((LV_PRESENT | (level + (raise ? 1u : 0u))) << (8 * d));
      }
    }
    if (out != v) s.level_words[w] = out;
  }
  above = wave_sum32(above);
  at_cap = wave_sum32(at_cap);
  const bool any_up = __any(up);
  if ((threadIdx.x & 63) == 0) {
    if (above) atomicAdd(round + RH_ABOVE, above);
    if (at_cap) atomicAdd(round + RH_AT_CAP, at_cap);
    if (any_up) atomicOr(round + RH_UP, 1u);
  }
}

// one workgroup: the stopping rules; `safe`, the grid columns of info; the round's header is zeroed for the next round
__global__ __launch_bounds__(128) void safe_tail_kernel(Det s, uint32_t* __restrict__ header, uint32_t* __restrict__ round,
                                                        int32_t* __restrict__ info, int64_t* __restrict__ safe, int max_rounds) {
  extern __shared__ uint32_t was_done[];                   // thread 0 sets the word below: every thread decides on the old one
  if (threadIdx.x == 0) was_done[0] = header[WS_DONE];
  __syncthreads();
  if (was_done[0]) return;
  if (threadIdx.x == 0) {
    const uint32_t rnd = header[WS_ROUND];
    const bool over = over_work(s, round), bad_counts = header[WS_BADCOUNTS] != 0;
    const u64 pairs = over ? 0ull : quad(round)[RQ_PAIRS], work = quad(round)[RQ_WORK];
    const uint32_t bad_rings = round[RH_BAD_RINGS];
    u64* pairs0 = reinterpret_cast<u64*>(header + WS_PAIRS0);
    if (rnd == 0) {
      *pairs0 = pairs;
      header[WS_RINGS0] = bad_rings;
    }
    int status = C3D_SAFE_ST_CONVERGED;
    bool done = true;
    if (over) status = C3D_SAFE_ST_OVER_WORK;
    else if (pairs == 0 && bad_rings == 0) status = C3D_SAFE_ST_CONVERGED;
    else if (!round[RH_UP]) status = C3D_SAFE_ST_DEFECTS_LEFT;
    else {
      header[WS_RAISED] += 1u;
      status = C3D_SAFE_ST_NOT_CONVERGED;                  // stands if this was the last round
      done = rnd + 1u >= (uint32_t)max_rounds;
    }
    header[WS_RUN] = rnd + 1u;
    header[WS_ROUND] = rnd + 1u;
    safe[0] = rnd + 1u;
    safe[1] = header[WS_RAISED];
    safe[2] = round[RH_ABOVE];
    safe[3] = round[RH_AT_CAP];
    safe[4] = (int64_t)*pairs0;
    safe[5] = (int64_t)pairs;
    safe[6] = header[WS_RINGS0];
    safe[7] = status;
    if (!bad_counts) {
      info[6] = (int32_t)round[RH_SHIFT];
      info[7] = (int32_t)(work > (u64)INT_MAX ? (u64)INT_MAX : work);
    }
    if (done) header[WS_DONE] = 1u;
  }
  __syncthreads();
  round[threadIdx.x] = 0u;                                 // 128 words
}

}  // namespace

extern "C" void c3d_outlines_simplify_safe_limits(int32_t out[6]) {
  if (!out) return;
  out[0] = WAVE_LIMIT;
  out[1] = LDS_LIMIT;
  out[2] = CELL_WAVE_LIMIT;
  out[3] = CHUNK;
  out[4] = BUDGET_E;
  out[5] = BUDGET_C;
}

extern "C" int64_t c3d_outlines_simplify_safe_ws_bytes(int32_t Hs, int32_t Ws, int32_t max_rings, int32_t max_vertices,
                                                       int32_t max_vertices_out) {
  if (Hs < 1 || Ws < 1 || max_rings < 1 || max_vertices < 1 || max_vertices > (1 << 30) || max_vertices_out < 1 ||
      max_vertices_out > (1 << 29))
    return C3D_E_BADARG;
  if (Hs > COORD_MAX || Ws > COORD_MAX) return C3D_E_UNSUPPORTED;
  return workspace_plan(Hs, Ws, max_rings, max_vertices, max_vertices_out).bytes;
}

extern "C" int c3d_outlines_simplify_safe(const int32_t* labels, const int32_t* counts_obj, int32_t Hs, int32_t Ws, int32_t max_objects,
                                          const int32_t* rings, const int32_t* vertices, const int32_t* counts, int32_t max_rings,
                                          int32_t max_vertices, int64_t tol2_q, int32_t max_rounds, int64_t max_work,
                                          int32_t max_vertices_out, int32_t* rings_out, int32_t* vertices_out, int32_t* left_out,
                                          int32_t* level_out, int32_t* counts_out, int32_t* info, int64_t* safe, void* ws, void* stream) {
  if (!labels || !counts_obj || !rings || !vertices || !counts || !rings_out || !vertices_out || !left_out || !level_out || !counts_out ||
      !info || !safe || !ws)
    return C3D_E_BADARG;
  if (Hs < 1 || Ws < 1 || max_objects < 1 || max_objects >= (1 << 30) || max_rings < 1 || max_vertices < 1 || max_vertices > (1 << 30) ||
      max_vertices_out < 1 || max_vertices_out > (1 << 29) || tol2_q < 0 || tol2_q > C3D_SIMPLIFY_TOL2_Q_MAX || max_rounds < 1 ||
      max_rounds > 64 || max_work < 0)
    return C3D_E_BADARG;
  if (Hs > COORD_MAX || Ws > COORD_MAX) return C3D_E_UNSUPPORTED;
  const Workspace w = workspace_plan(Hs, Ws, max_rings, max_vertices, max_vertices_out);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  uint32_t* header = reinterpret_cast<uint32_t*>(base);
  uint32_t* round = header + 64;
  int32_t* naug = reinterpret_cast<int32_t*>(base + w.naug);
  uint32_t* off = reinterpret_cast<uint32_t*>(base + w.off);
  uint32_t* rot = reinterpret_cast<uint32_t*>(base + w.rot);
  int32_t* kept = reinterpret_cast<int32_t*>(base + w.kept);
  uint32_t* startp = reinterpret_cast<uint32_t*>(base + w.startp);
  uint32_t* large = reinterpret_cast<uint32_t*>(base + w.large);
  uint32_t* ap = reinterpret_cast<uint32_t*>(base + w.ap);
  uint32_t* meta = reinterpret_cast<uint32_t*>(base + w.meta);
  uint8_t* flags = reinterpret_cast<uint8_t*>(base + w.flags);
  int32_t* link = reinterpret_cast<int32_t*>(base + w.link);
  int32_t* arc = reinterpret_cast<int32_t*>(base + w.arc);
  u64* idx = reinterpret_cast<u64*>(base + w.idx);
  u64* best = reinterpret_cast<u64*>(base + w.best);
  uint32_t* rowbits = reinterpret_cast<uint32_t*>(base + w.rowbits);
  uint32_t* colbits = reinterpret_cast<uint32_t*>(base + w.colbits);
  uint8_t* dirs = reinterpret_cast<uint8_t*>(base + w.dirs);
  uint32_t* vkey = reinterpret_cast<uint32_t*>(base + w.vkey);
  uint32_t* level_words = reinterpret_cast<uint32_t*>(base + w.levels);
  const Bits bits{rowbits, colbits, w.WR, w.WC};
  const int2* v_in = reinterpret_cast<const int2*>(vertices);
  int2* v_out = reinterpret_cast<int2*>(vertices_out);
  Marks mk{vkey, level_words, level_out, reinterpret_cast<uint32_t*>(base + w.e_key), reinterpret_cast<int4*>(base + w.e_info), round};
  Det det{v_out, mk.e_key, mk.e_info, reinterpret_cast<int4*>(base + w.e_xy), reinterpret_cast<uint32_t*>(base + w.cell_n),
          reinterpret_cast<uint32_t*>(base + w.cell_at), reinterpret_cast<uint32_t*>(base + w.entry),
          reinterpret_cast<uint2*>(base + w.jobs), level_words, w.cap_e, w.cap_c, w.cap_j, max_work, (int)max_vertices_out};
  int cap = 0;                                             // L_cap: the smallest L with tol2_q >> 2 L == 0
  while (tol2_q >> (2 * cap)) ++cap;

  // the two headers and the level store: every other word of the workspace is written by the call before the call reads it
  hipError_t e = hipMemsetAsync(base, 0, HEADER_BYTES, st);
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(level_words, 0, (size_t)w.level_words * 4, st);
  if (e != hipSuccess) return (int)e;
  // the ring count is known on the device only: grids are sized by max_rings and surplus waves and workgroups return
  const unsigned g_wave = grid_for(max_rings, 4), g_block = grid_for(max_rings, 1);
  int rc = c3d_launch_lds<safe_nodes_kernel<false>>(dim3(grid_for((int64_t)(Hs + 1) * w.WR * 32, 256)), dim3(256), 0, st, labels, counts_obj,
                                                    (int)Hs, (int)Ws, (int)max_objects, rowbits, w.WR);
  if (rc) return rc;
  rc = c3d_launch_lds<safe_nodes_kernel<true>>(dim3(grid_for((int64_t)(Ws + 1) * w.WC * 32, 256)), dim3(256), 0, st, labels, counts_obj,
                                               (int)Hs, (int)Ws, (int)max_objects, colbits, w.WC);
  if (rc) return rc;
  rc = c3d_launch_lds<safe_count_rows_kernel>(dim3(g_wave), dim3(256), 0, st, labels, counts_obj, (int)Hs, (int)Ws, (int)max_objects, rings,
                                              v_in, counts, (int)max_rings, (int)max_vertices, naug, bits);
  if (rc) return rc;
  rc = c3d_launch_lds<safe_scan_rows_kernel>(dim3(1), dim3(BLOCK_T), BLOCK_T / 8, st, counts, naug, off, large, header, (int)max_rings,
                                             (int)max_vertices);
  if (rc) return rc;
  rc = c3d_launch_lds<safe_augment_kernel>(dim3(g_wave), dim3(256), 0, st, labels, counts_obj, (int)Hs, (int)Ws, (int)max_objects, rings,
                                           v_in, (const int32_t*)naug, (const uint32_t*)off, rot, ap, meta, dirs, header, bits);
  if (rc) return rc;
  rc = c3d_launch_lds<safe_keys_kernel<64>>(dim3(g_block), dim3(64), 64, st, (const int32_t*)naug, (const uint32_t*)off,
                                            (const uint32_t*)rot, (const uint32_t*)ap, (const uint32_t*)meta, (const uint8_t*)dirs, link,
                                            arc, vkey, level_words, (const uint32_t*)large, header, (int)Ws);
  if (rc) return rc;
  rc = c3d_launch_lds<safe_keys_kernel<BLOCK_T>>(dim3(g_block), dim3(BLOCK_T), 64, st, (const int32_t*)naug, (const uint32_t*)off,
                                                 (const uint32_t*)rot, (const uint32_t*)ap, (const uint32_t*)meta, (const uint8_t*)dirs,
                                                 link, arc, vkey, level_words, (const uint32_t*)large, header, (int)Ws);
  if (rc) return rc;

  // the rounds are launched ahead: after the stopping one every kernel returns at once on header[WS_DONE]
  const uint32_t* hdr = header;
  const uint32_t* rnd = round;
  const unsigned g_edge = grid_for(max_vertices_out, 256);
  const unsigned g_cell = (unsigned)((w.cap_c + 255) / 256 < CELL_GRID ? (w.cap_c + 255) / 256 : CELL_GRID);
  const unsigned g_jobs = (unsigned)(w.cap_j < CELL_GRID ? w.cap_j : CELL_GRID);
  const unsigned g_level = grid_for(w.level_words, 256);
  for (int r = 0; r < max_rounds; ++r) {
    rc = c3d_launch_lds<safe_dp_kernel<64, WAVE_LIMIT>>(dim3(g_block), dim3(64), WAVE_LDS_BYTES, st, (const int32_t*)naug,
                                                        (const uint32_t*)off, (const uint32_t*)rot, (const uint32_t*)ap,
                                                        (const uint32_t*)meta, kept, flags, link, arc, idx, best, (const uint32_t*)large,
                                                        hdr, (const uint32_t*)vkey, (const uint8_t*)level_words, (u64)tol2_q);
    if (rc) return rc;
    rc = c3d_launch_lds<safe_dp_kernel<BLOCK_T, LDS_LIMIT>>(dim3(g_block), dim3(BLOCK_T), LDS_BYTES, st, (const int32_t*)naug,
                                                            (const uint32_t*)off, (const uint32_t*)rot, (const uint32_t*)ap,
                                                            (const uint32_t*)meta, kept, flags, link, arc, idx, best,
                                                            (const uint32_t*)large, hdr, (const uint32_t*)vkey,
                                                            (const uint8_t*)level_words, (u64)tol2_q);
    if (rc) return rc;
    rc = c3d_launch_lds<safe_scan_kept_kernel>(dim3(1), dim3(BLOCK_T), BLOCK_T / 8 + 8, st, (const int32_t*)kept, startp, header, counts_out,
                                               info, (int)max_vertices_out);
    if (rc) return rc;
    rc = c3d_launch_lds<safe_scatter_wave_kernel>(dim3(g_wave), dim3(256), 0, st, rings, (const int32_t*)naug, (const uint32_t*)off,
                                                  (const uint32_t*)rot, (const uint32_t*)ap, (const uint32_t*)meta, (const int32_t*)kept,
                                                  (const uint32_t*)startp, (const uint8_t*)flags, hdr, rings_out, v_out, left_out, info,
                                                  (int)max_rings, mk);
    if (rc) return rc;
    rc = c3d_launch_lds<safe_scatter_block_kernel>(dim3(g_block), dim3(256), 40, st, rings, (const int32_t*)naug, (const uint32_t*)off,
                                                   (const uint32_t*)rot, (const uint32_t*)ap, (const uint32_t*)meta, (const int32_t*)kept,
                                                   (const uint32_t*)startp, (const uint8_t*)flags, (const uint32_t*)large, hdr, rings_out,
                                                   v_out, left_out, info, mk);
    if (rc) return rc;
    rc = c3d_launch_lds<safe_edges_kernel>(dim3(g_edge), dim3(256), 0, st, det, hdr, round);
    if (rc) return rc;
    rc = c3d_launch_lds<safe_cost_kernel>(dim3(g_edge), dim3(256), 0, st, det, hdr, round);
    if (rc) return rc;
    rc = c3d_launch_lds<safe_choose_kernel>(dim3(1), dim3(64), 0, st, det, hdr, round);
    if (rc) return rc;
    rc = c3d_launch_lds<safe_zero_cells_kernel>(dim3(g_cell), dim3(256), 0, st, det, hdr, rnd);
    if (rc) return rc;
    rc = c3d_launch_lds<safe_count_kernel>(dim3(g_edge), dim3(256), 0, st, det, hdr, rnd);
    if (rc) return rc;
    rc = c3d_launch_lds<safe_starts_kernel>(dim3(g_cell), dim3(256), 0, st, det, hdr, round);
    if (rc) return rc;
    rc = c3d_launch_lds<safe_fill_kernel>(dim3(g_edge), dim3(256), 0, st, det, hdr, rnd);
    if (rc) return rc;
    rc = c3d_launch_lds<safe_pairs_wave_kernel>(dim3(g_cell), dim3(256), 0, st, det, hdr, round);
    if (rc) return rc;
    rc = c3d_launch_lds<safe_pairs_jobs_kernel>(dim3(g_jobs), dim3(PAIR_T), (size_t)CHUNK * 36, st, det, hdr, round);
    if (rc) return rc;
    rc = c3d_launch_lds<safe_raise_kernel>(dim3(g_level), dim3(256), 0, st, det, hdr, round, w.level_words, cap);
    if (rc) return rc;
    rc = c3d_launch_lds<safe_tail_kernel>(dim3(1), dim3(128), 16, st, det, header, round, info, safe, (int)max_rounds);
    if (rc) return rc;
  }
  return 0;
}
