// Polygon conflicts between the objects of a ring table: the proper crossings, collinear overlaps and touches of every pair
// of live edges of DIFFERENT ids, while the table stays in HBM.  The rule is the header's (include/change3d_hip.h); this file
// is one way to compute it.  The all-pairs walk across ids is quadratic in the edges of the whole scene, so the edges are
// binned into a uniform grid of square cells and only the entries of one cell are compared.  The rows pass, the ids scan and
// the pair predicate are those of csrc/scene_valid.hip (csrc/scene_rings.h); the grid build (4 .. 8) is csrc/scene_grid.h's, which the
// detector of csrc/scene_safe.hip runs too.  Everything is an integer, every sum an integer
// atomic or a ballot count, and nothing depends on the order in which entries land in a cell.  No workgroup waits for
// another, nothing is read back, every loop is capped.
//
//   1 rows     a wave per ring row: the used rows, the incomplete ids, K                                   (scene_rings.h)
//     check    the coordinates of the rings above BIG_RING vertices                                        (scene_rings.h)
//   2 ids      one workgroup: which ids are complete                                                       (scene_rings.h)
//   3 edges    a wave per used row of a complete id: its live edges go to one flat list (id, a, b), 64 at a time behind one
//              atomic; m per id; the bounding box of all of them
//     edges    the same for the rings above BIG_RING: many workgroups, 64 edges of a wave at a time
//   4 cost     a thread per edge: for every candidate shift s the cells its bounding box would cover; a saturating sum per
//              wave, then one 64-bit atomic per wave and candidate
//   5 choose   one wave, a lane per candidate: the smallest s within the entry and the cell budget, both taken per live edge:
//              a table that fills a fraction of max_vertices gets a grid sized for what it holds
//   6 count    a thread per edge: one atomic per covered cell
//   7 starts   a thread per cell: where its entries go (a wave scan, one atomic per wave), its share of `work`, and the jobs
//              of a cell above WAVE_LIMIT entries
//   8 scatter  a thread per edge: its index into every covered cell
//   9 rows     a thread per id: flag, m and zeros; the rows past K
//  10 wave     a wave per 64 cells: each cell of 2 .. WAVE_LIMIT entries in turn, a lane per entry, the partner by shuffle
//  11 jobs     a workgroup per (cell, chunk i): a thread per entry, the chunks i, i+1, .., i + floor(c/2) (mod c) through LDS
//  12 tail     one workgroup: the partner column, counts, info, totals
//
// A pair of entries of one cell is evaluated iff the ids differ, the bounding boxes meet, and the cell holds the lower corner
// of the boxes' intersection: that point lies in both boxes, so exactly one cell that holds both edges evaluates the pair.
#include <climits>

#include "scene_grid.h"
#include "scene_host.h"
#include "scene_rings.h"

namespace {

using namespace c3d_rings;
using namespace c3d_grid;
using c3d_host::grid_for;

constexpr int WAVE_LIMIT = CELL_WAVE_LIMIT;                // entries of a cell in the wave tier: a lane each
constexpr int TILE = 256;                                  // entries of an LDS tile: 20 bytes each; a chunk is one tile
constexpr int BLOCK_T = 256;
constexpr int MAX_GRID = 4096;
constexpr u64 NO_PARTNER = ~0ull;

// 32-bit words of the workspace header (512 bytes, zeroed by the call's memset): the largest id of a row, the jobs, the long
// rings, the live edges, the grid's words
enum { WS_K = 1, WS_JOBS = 2, WS_BIG = 3, WS_EDGES = 4, WS_LO_X = 5, WS_LO_Y = 6, WS_HI_X = 7, WS_HI_Y = 8, WS_SHIFT = 9, WS_CX = 10, WS_CY = 11, WS_X0 = 12,
       WS_Y0 = 13, WS_AT = 14 };
// 64-bit words of the header, counted from byte 64
enum { WQ_WORK = 0, WQ_ENTRIES = 1, WQ_SUM = 2 /* cross, same, opposite, vv, ve */, WQ_COST = 8 /* N_SHIFT of them */ };
enum { COL_FLAG = 0, COL_PARTNER = 1, COL_M = 2, COL_CROSS = 3, COL_SAME = 4, COL_OPP = 5, COL_VV = 6, COL_VE = 7 };
enum { HIT_CROSS = 0, HIT_SAME = 1, HIT_OPP = 2, HIT_VV = 3, HIT_VE = 4, HIT_NONE = 5 };
// where scene_grid.h finds the grid's words in this header
struct Words {
  enum { LO_X = WS_LO_X, LO_Y = WS_LO_Y, HI_X = WS_HI_X, HI_Y = WS_HI_Y, SHIFT = WS_SHIFT, CX = WS_CX, CY = WS_CY, X0 = WS_X0, Y0 = WS_Y0,
         AT = WS_AT, JOBS = WS_JOBS, Q_WORK = WQ_WORK, Q_ENTRIES = WQ_ENTRIES, Q_COST = WQ_COST };
};

struct Tab : Rows {
  uint32_t* id_live;                                       // [max_ids] live edges of the id
  int4* e_xy;                                              // [max_vertices] (a.x, a.y, b.x, b.y) of the live edges, in any order
  uint32_t* e_id;                                          // [max_vertices]
  uint32_t* cell_n;                                        // [cap_c] entries of the cell
  uint32_t* cell_at;                                       // [cap_c] where they start; after the scatter, where they end
  uint32_t* entry;                                         // [cap_e] edge indices grouped by cell
  uint2* jobs;                                             // [cap_j] (cell, chunk)
  int64_t cap_e, cap_c, cap_j;
  int64_t max_work;
};

struct Plan {
  Tab t;
  int64_t zero_bytes, bytes;
};

// ws: the workspace, or nullptr where only the sizes are asked for
Plan plan_of(void* ws, int64_t max_rings, int64_t max_vertices, int64_t max_ids) {
  Plan pl{};
  c3d_host::Layout l{static_cast<char*>(ws), 512};
  Tab& t = pl.t;
  // both budgets hold for one cell whatever the table holds (at most max_vertices live edges, one entry each), and a grid
  // within the budgets of the live edges is within those of max_vertices, so the sizes are a function of the maxima alone;
  // the caps keep every index in 32 bits
  t.cap_e = BUDGET_E * max_vertices < 0xFFFFFFF0ll ? BUDGET_E * max_vertices : 0xFFFFFFF0ll;
  t.cap_c = BUDGET_C * max_vertices < 0x7FFFFFF0ll ? BUDGET_C * max_vertices : 0x7FFFFFF0ll;
  t.cap_j = jobs_cap(t.cap_e);
  l.take(t.id_rings, max_ids * 4);                           // zeroed part first
  l.take(t.id_verts, max_ids * 8);
  l.take(t.id_flags, max_ids * 4);
  l.take(t.id_live, max_ids * 4);
  l.take(t.cell_n, t.cap_c * 4);
  pl.zero_bytes = l.at;
  l.take(t.kind, max_rings);
  l.take(t.big, max_rings * 4);
  l.take(t.id_list, max_ids * 4);
  l.take(t.id_start, max_ids * 4);
  l.take(t.e_xy, max_vertices * 16);
  l.take(t.e_id, max_vertices * 4);
  l.take(t.cell_at, t.cap_c * 4);
  l.take(t.entry, t.cap_e * 4);
  l.take(t.jobs, t.cap_j * 8);
  pl.bytes = l.at;
  t.max_rings = (int)max_rings; t.max_vertices = (int)max_vertices; t.max_ids = (int)max_ids;
  if (ws) {
    t.top = static_cast<uint32_t*>(ws) + WS_K;
    t.n_big = static_cast<uint32_t*>(ws) + WS_BIG;
  }
  return pl;
}

__device__ __forceinline__ uint32_t edges_of(const Tab& s, const uint32_t* header) {
  return min(header[WS_EDGES], (uint32_t)s.max_vertices);
}
__device__ __forceinline__ bool over_work(const Tab& s, const uint32_t* header) { return quad(header)[WQ_WORK] > (u64)s.max_work; }

// ---------------------------------------------------------------------------------------------------------- 1, 2: shared
__global__ __launch_bounds__(256) void conflicts_rows_kernel(Tab s) { rows_pass(s); }
__global__ __launch_bounds__(256) void conflicts_check_big_kernel(Tab s) { check_big_pass(s); }
__global__ __launch_bounds__(SCAN_T) void conflicts_ids_kernel(Tab s) {
  extern __shared__ u64 part_ids[];                        // [2][SCAN_T / 64]
  ids_pass(s, reinterpret_cast<u64(*)[SCAN_T / 64]>(part_ids));
}

// -------------------------------------------------------------------------------------------------------------- 3: edges
// What a wave keeps while it walks: the box of its live edges, folded into the header once at the end.
struct Box {
  int lo_x, lo_y, hi_x, hi_y;                              // biased: BIAS - min and BIAS + max, 0 where nothing was seen
};
__device__ __forceinline__ void box_out(Box b, uint32_t* header) {
  for (int o = 32; o > 0; o >>= 1) {
    b.lo_x = max(b.lo_x, __shfl_xor(b.lo_x, o, 64)); b.lo_y = max(b.lo_y, __shfl_xor(b.lo_y, o, 64));
    b.hi_x = max(b.hi_x, __shfl_xor(b.hi_x, o, 64)); b.hi_y = max(b.hi_y, __shfl_xor(b.hi_y, o, 64));
  }
  if ((threadIdx.x & 63) == 0 && b.lo_x) {
    atomicMax(header + WS_LO_X, (uint32_t)b.lo_x); atomicMax(header + WS_LO_Y, (uint32_t)b.lo_y);
    atomicMax(header + WS_HI_X, (uint32_t)b.hi_x); atomicMax(header + WS_HI_Y, (uint32_t)b.hi_y);
  }
}
// 64 edges j0 + lane of the ring (start, n) of `id`, the same j0 in every lane of the wave: the live ones are appended
__device__ __forceinline__ uint32_t emit64(const Tab& s, uint32_t* header, int id, int64_t start, int n, int64_t j0, Box& box) {
  const int lane = threadIdx.x & 63;
  const int64_t j = j0 + lane;
  int4 e = make_int4(0, 0, 0, 0);
  if (j < n) {
    const int2 a = s.vertices[start + j], b = s.vertices[start + (j + 1 < n ? j + 1 : 0)];
    e = make_int4(a.x, a.y, b.x, b.y);
  }
  const bool live = live_of(e);
  const u64 mask = __ballot(live);
  const uint32_t cnt = (uint32_t)__popcll(mask);
  if (!cnt) return 0;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(header + WS_EDGES, cnt);
  base = (uint32_t)__shfl((int)base, 0);
  if (live) {
    const u64 at = (u64)base + (u64)__popcll(mask & ((1ull << lane) - 1ull));
    if (at < (u64)s.max_vertices) {                        // cannot fail: the complete ids fit (ids_pass)
      s.e_xy[at] = e;
      s.e_id[at] = (uint32_t)id;
    }
    box.lo_x = max(box.lo_x, BIAS - min(e.x, e.z)); box.lo_y = max(box.lo_y, BIAS - min(e.y, e.w));
    box.hi_x = max(box.hi_x, BIAS + max(e.x, e.z)); box.hi_y = max(box.hi_y, BIAS + max(e.y, e.w));
  }
  return cnt;
}

__global__ __launch_bounds__(256) void conflicts_edges_kernel(Tab s, uint32_t* __restrict__ header) {
  const int rows = rows_of(s), lane = threadIdx.x & 63;
  Box box = {0, 0, 0, 0};
  for (int r = blockIdx.x * 4 + (int)(threadIdx.x >> 6); r < rows; r += gridDim.x * 4) {   // r is uniform over the wave
    if (s.kind[r] != ROW_USED) continue;
    const int id = s.rings[(int64_t)r * 8], n = s.rings[(int64_t)r * 8 + 2];
    const int64_t start = s.rings[(int64_t)r * 8 + 1];
    if (!s.id_rings[id - 1] || n > BIG_RING) continue;     // the id became incomplete; a long ring is the next kernel's
    uint32_t m = 0;
    for (int j0 = 0; j0 < n; j0 += 64) m += emit64(s, header, id, start, n, j0, box);
    if (m && lane == 0) atomicAdd(s.id_live + (id - 1), m);
  }
  box_out(box, header);
}

__global__ __launch_bounds__(256) void conflicts_edges_big_kernel(Tab s, uint32_t* __restrict__ header) {
  const uint32_t n_big = min(header[WS_BIG], (uint32_t)s.max_rings);
  const int lane = threadIdx.x & 63;
  Box box = {0, 0, 0, 0};
  for (uint32_t li = 0; li < n_big; ++li) {
    const int r = (int)s.big[li];
    if (s.kind[r] != ROW_USED) continue;
    const int id = s.rings[(int64_t)r * 8], n = s.rings[(int64_t)r * 8 + 2];
    const int64_t start = s.rings[(int64_t)r * 8 + 1];
    if (!s.id_rings[id - 1]) continue;
    uint32_t m = 0;
    for (int64_t j0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; j0 < n; j0 += (int64_t)gridDim.x * 256)
      m += emit64(s, header, id, start, n, j0, box);
    if (m && lane == 0) atomicAdd(s.id_live + (id - 1), m);
  }
  box_out(box, header);
}

// ------------------------------------------------------------------------------------------------- 4 .. 8: scene_grid.h
// the list holds live edges only, all of them: no filter
__global__ __launch_bounds__(256) void conflicts_cost_kernel(Tab s, uint32_t* __restrict__ header) {
  const uint32_t n = edges_of(s, header);
  cost_pass<Words, false>(cells_of(s), header, n, n);
}
__global__ __launch_bounds__(64) void conflicts_choose_kernel(Tab s, uint32_t* __restrict__ header) {
  choose_pass<Words>(cells_of(s), header, edges_of(s, header));
}
__global__ __launch_bounds__(256) void conflicts_count_kernel(Tab s, const uint32_t* __restrict__ header) {
  count_pass<Words, false>(cells_of(s), header, edges_of(s, header));
}
__global__ __launch_bounds__(256) void conflicts_starts_kernel(Tab s, uint32_t* __restrict__ header) {
  starts_pass<Words>(cells_of(s), header);
}
__global__ __launch_bounds__(256) void conflicts_scatter_kernel(Tab s, const uint32_t* __restrict__ header) {
  if (over_work(s, header)) return;
  fill_pass<Words, false>(cells_of(s), header, edges_of(s, header));
}

// --------------------------------------------------------------------------------------------------------------- 9: rows
__global__ __launch_bounds__(256) void conflicts_init_kernel(Tab s, const uint32_t* __restrict__ header, u64* __restrict__ conflict) {
  const int top = clampi((int)header[WS_K], 0, s.max_ids);
  const bool over = over_work(s, header);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < s.max_ids; i += (int64_t)gridDim.x * 256) {
    u64* row = conflict + i * 8;
    u64 flag = 0, m = 0, partner = 0;
    if (i < top) {
      m = s.id_live[i];
      if (s.id_flags[i] & ID_INCOMPLETE) { flag = 2; m = 0; }
      else if (m == 0) flag = 1;
      else if (over) flag = 3;
      else partner = NO_PARTNER;                           // what atomicMin starts from; the tail turns it into 0
    }
    row[COL_FLAG] = flag; row[COL_PARTNER] = partner; row[COL_M] = m;
    for (int k = COL_CROSS; k < 8; ++k) row[k] = 0;
  }
}

// ---------------------------------------------------------------------------------------------------------- 10, 11: pairs
// one entry as the pair kernels hold it
struct Ent {
  int4 e;
  uint32_t id;                                             // 0: no entry
};
// the header's classes for a pair of different ids: cross, same, opposite, touch_vv, touch_ve
__device__ __forceinline__ int hit_class(int4 p, int4 q) {
  const int cls = pair_class(p, q, false);
  if (cls == PAIR_NONE) return HIT_NONE;
  if (cls == PAIR_CROSS) return HIT_CROSS;
  if (cls == PAIR_VV) return HIT_VV;
  if (cls == PAIR_VE) return HIT_VE;
  const int64_t dot = (int64_t)(p.z - p.x) * (q.z - q.x) + (int64_t)(p.w - p.y) * (q.w - q.y);   // below 2^51; never 0 here
  return dot > 0 ? HIT_SAME : HIT_OPP;
}
// does this cell evaluate the pair: different ids, boxes that meet, and the lower corner of their intersection in the cell
__device__ __forceinline__ bool owned(const Grid& g, uint32_t cell_x, uint32_t cell_y, const Ent& p, const Ent& q) {
  if (!p.id || !q.id || p.id == q.id || !boxes_meet(p.e, q.e)) return false;
  const int px = max(min(p.e.x, p.e.z), min(q.e.x, q.e.z)), py = max(min(p.e.y, p.e.w), min(q.e.y, q.e.w));
  return ((uint32_t)(px - g.x0) >> g.shift) == cell_x && ((uint32_t)(py - g.y0) >> g.shift) == cell_y;
}
// Adds 1 to column `col` of the row of `id` for every lane with `hit`; the lanes that share the first such lane's id are
// counted by one ballot and added by one atomic.  Called by every lane of the wave.
__device__ __forceinline__ void wave_add(u64* __restrict__ conflict, uint32_t id, int col, bool hit) {
  const u64 mask = __ballot(hit);
  if (!mask) return;
  const int lane = threadIdx.x & 63, leader = __ffsll((long long)mask) - 1;
  const uint32_t lid = (uint32_t)__shfl((int)id, leader);
  const u64 same = __ballot(hit && id == lid);
  if (lane == leader) atomicAdd(conflict + (u64)(lid - 1) * 8 + col, (u64)__popcll(same));
  else if (hit && id != lid) atomicAdd(conflict + (u64)(id - 1) * 8 + col, 1ull);
}
// what every lane of a wave does with the class of its pair (HIT_NONE where it had none): both rows, both partner columns,
// and the lane's own tally of pairs, each counted once
__device__ __forceinline__ void record(u64* __restrict__ conflict, uint32_t id_p, uint32_t id_q, int hit, uint32_t (&tally)[5]) {
  if (!__any(hit != HIT_NONE)) return;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    wave_add(conflict, id_p, COL_CROSS + k, hit == k);
    wave_add(conflict, id_q, COL_CROSS + k, hit == k);
    tally[k] += hit == k;
  }
  if (hit == HIT_CROSS || hit == HIT_SAME) {
    atomicMin(conflict + (u64)(id_p - 1) * 8 + COL_PARTNER, (u64)id_q);
    atomicMin(conflict + (u64)(id_q - 1) * 8 + COL_PARTNER, (u64)id_p);
  }
}
__device__ __forceinline__ void tally_out(uint32_t (&tally)[5], uint32_t* header) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    u64 v = tally[k];
    for (int o = 32; o > 0; o >>= 1) v += shfl64(v, lane ^ o);
    if (lane == 0 && v) atomicAdd(quad(header) + WQ_SUM + k, v);
  }
}

__global__ __launch_bounds__(256) void conflicts_wave_kernel(Tab s, uint32_t* __restrict__ header, u64* __restrict__ conflict) {
  if (over_work(s, header)) return;
  const Grid g = grid_of<Words>(header);
  const u64 cells = (u64)g.cx * g.cy;
  const int lane = threadIdx.x & 63;
  uint32_t tally[5] = {0, 0, 0, 0, 0};
  for (u64 c0 = ((u64)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; c0 < cells; c0 += (u64)gridDim.x * 256) {   // uniform over the wave
    const uint32_t mine = c0 + lane < cells ? s.cell_n[c0 + lane] : 0u;
    u64 todo = __ballot(mine >= 2u && mine <= (uint32_t)WAVE_LIMIT);
    while (todo) {                                         // at most 64 cells
      const int which = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      const u64 c = c0 + which;
      const int cnt = (int)(uint32_t)__shfl((int)mine, which);
      const uint32_t first = s.cell_at[c] - (uint32_t)cnt;   // cell_at is the end since the scatter
      const uint32_t cell_x = (uint32_t)(c % g.cx), cell_y = (uint32_t)(c / g.cx);
      Ent own = {make_int4(0, 0, 0, 0), 0u};
      if (lane < cnt) {
        const uint32_t i = s.entry[first + lane];
        own.e = s.e_xy[i];
        own.id = s.e_id[i];
      }
      // most cells of a traced scene hold the edges of one object only
      if (!__any(lane < cnt && own.id != (uint32_t)__shfl((int)own.id, 0))) continue;
      // rotation r pairs lane l with lane (l + r) mod cnt: each unordered pair is met at r and at cnt - r, and counts where l
      // is the smaller one
      for (int r = 1; r < cnt; ++r) {
        int other = lane + r;
        other = other >= cnt ? other - cnt : other;
        Ent q;
        q.e = make_int4(__shfl(own.e.x, other), __shfl(own.e.y, other), __shfl(own.e.z, other), __shfl(own.e.w, other));
        q.id = (uint32_t)__shfl((int)own.id, other);
        const bool near = lane < cnt && lane < other && owned(g, cell_x, cell_y, own, q);
        if (!__any(near)) continue;                        // uniform over the wave
        int hit = HIT_NONE;
        if (near) hit = hit_class(own.e, q.e);
        record(conflict, own.id, q.id, hit, tally);
      }
    }
  }
  tally_out(tally, header);
}

// The job (cell, chunk i) of a cell of c chunks compares chunk i with the chunks i, i + 1, .., i + floor(c / 2) (mod c): every
// unordered pair of chunks belongs to exactly one job.  For even c the offset c / 2 joins i and i + c / 2 from both ends, so
// only i < c / 2 takes it; inside chunk i itself a thread takes the partners with a larger index.
__global__ __launch_bounds__(BLOCK_T) void conflicts_jobs_kernel(Tab s, uint32_t* __restrict__ header, u64* __restrict__ conflict) {
  extern __shared__ int4 t_edge[];                         // [TILE], then u32 [TILE]
  uint32_t* t_id = reinterpret_cast<uint32_t*>(t_edge + TILE);
  if (over_work(s, header)) return;
  const Grid g = grid_of<Words>(header);
  const int tid = threadIdx.x;
  const u64 n_jobs = min((u64)header[WS_JOBS], (u64)s.cap_j);
  uint32_t tally[5] = {0, 0, 0, 0, 0};
  for (u64 job = blockIdx.x; job < n_jobs; job += gridDim.x) {
    const uint2 jb = s.jobs[job];
    const u64 cell = jb.x;
    const uint32_t cnt = s.cell_n[cell], first = s.cell_at[cell] - cnt;
    const uint32_t c = (cnt + CHUNK - 1) / CHUNK, i = jb.y;
    if (i >= c) continue;                                  // cannot happen
    const uint32_t cell_x = (uint32_t)(cell % g.cx), cell_y = (uint32_t)(cell / g.cx);
    const uint32_t k = i * CHUNK + (uint32_t)tid;
    Ent own = {make_int4(0, 0, 0, 0), 0u};
    if (k < cnt) {
      const uint32_t e = s.entry[first + k];
      own.e = s.e_xy[e];
      own.id = s.e_id[e];
    }
    const uint32_t half = c / 2;
    for (uint32_t kk = 0; kk <= half; ++kk) {              // at most cap_e / (2 CHUNK) + 1 steps
      if (kk * 2 == c && i >= half) break;
      const uint32_t base = ((i + kk) % c) * CHUNK;
      const int here = cnt - base < (uint32_t)TILE ? (int)(cnt - base) : TILE;
      __syncthreads();                                     // the tile before has been read
      if (tid < here) {
        const uint32_t e = s.entry[first + base + tid];
        t_edge[tid] = s.e_xy[e];
        t_id[tid] = s.e_id[e];
      } else {
        t_edge[tid] = make_int4(0, 0, 0, 0);
        t_id[tid] = 0u;                                    // past the end: no entry, which takes part in no pair
      }
      __syncthreads();
      const int from = !own.id ? TILE : (kk == 0 ? tid + 1 : 0);   // the diagonal chunk: partners with a larger index only
      for (int t0 = 0; t0 < here; t0 += 4) {               // four partners at a time: the same addresses in every lane
        Ent q[4];
        bool near[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          q[u].e = t_edge[t0 + u];                         // TILE is a multiple of 4 and the tile is padded
          q[u].id = t_id[t0 + u];
          near[u] = t0 + u >= from && owned(g, cell_x, cell_y, own, q[u]);
        }
        if (!__any(near[0] || near[1] || near[2] || near[3])) continue;   // uniform over the wave; most partners are far away
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (!__any(near[u])) continue;
          int hit = HIT_NONE;
          if (near[u]) hit = hit_class(own.e, q[u].e);
          record(conflict, own.id, q[u].id, hit, tally);
        }
      }
    }
  }
  tally_out(tally, header);
}

// -------------------------------------------------------------------------------------------------------------- 12: tail
__global__ __launch_bounds__(256) void conflicts_tail_kernel(Tab s, const uint32_t* __restrict__ header, int64_t* __restrict__ conflict,
                                                              int64_t* __restrict__ counts, int64_t* __restrict__ info,
                                                              int64_t* __restrict__ totals) {
  extern __shared__ long long s_tail[];                    // [5][256]
  long long(*s_i)[256] = reinterpret_cast<long long(*)[256]>(s_tail);
  const int tid = threadIdx.x;
  const int top = clampi((int)header[WS_K], 0, s.max_ids);
  long long c[5] = {0, 0, 0, 0, 0};
  for (int i = tid; i < top; i += 256) {
    int64_t* row = conflict + (int64_t)i * 8;
    const int flag = (int)row[COL_FLAG];
    if (flag == 0) {
      if ((u64)row[COL_PARTNER] == NO_PARTNER) row[COL_PARTNER] = 0;
      c[0] += 1;
      c[1] += (row[COL_CROSS] != 0 || row[COL_SAME] != 0) ? 1 : 0;
    } else {
      c[1 + flag] += 1;                                    // 1 empty, 2 incomplete, 3 over work
    }
  }
  for (int k = 0; k < 5; ++k) s_i[k][tid] = c[k];
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d)
      for (int k = 0; k < 5; ++k) s_i[k][tid] += s_i[k][tid + d];
    __syncthreads();
  }
  if (tid == 0) {
    const u64* q = quad(header);
    const int64_t status = (int64_t)(uint32_t)s.counts[4];
    for (int k = 0; k < 5; ++k) counts[k] = s_i[k][0];
    counts[5] = (int64_t)q[WQ_SUM + HIT_CROSS];
    counts[6] = (int64_t)q[WQ_SUM + HIT_SAME];
    counts[7] = status;
    info[0] = edges_of(s, header);
    info[1] = header[WS_SHIFT]; info[2] = header[WS_CX]; info[3] = header[WS_CY];
    info[4] = (int64_t)q[WQ_ENTRIES];
    info[5] = (int64_t)q[WQ_WORK];
    info[6] = (int64_t)q[WQ_SUM + HIT_OPP];
    info[7] = (int64_t)(q[WQ_SUM + HIT_VV] + q[WQ_SUM + HIT_VE]);
    if (totals) {
      for (int k = 0; k < 7; ++k) totals[k] += counts[k];
      totals[7] |= status;
    }
  }
}

int refuse(int32_t max_rings, int32_t max_vertices, int32_t max_ids) {
  if (max_rings < 1 || max_vertices < 1 || max_ids < 1) return C3D_E_BADARG;
  return 0;
}

}  // namespace

extern "C" void c3d_rings_conflicts_limits(int32_t out[6]) {
  if (!out) return;
  out[0] = WAVE_LIMIT;
  out[1] = CHUNK;
  out[2] = TILE;
  out[3] = RING_LIMIT;
  out[4] = BUDGET_E;
  out[5] = BUDGET_C;
}

extern "C" int64_t c3d_rings_conflicts_ws_bytes(int32_t max_rings, int32_t max_vertices, int32_t max_ids) {
  const int rc = refuse(max_rings, max_vertices, max_ids);
  if (rc) return rc;
  return plan_of(nullptr, max_rings, max_vertices, max_ids).bytes;
}

extern "C" int c3d_rings_conflicts(const int32_t* rings, const int32_t* vertices, const int32_t* counts_in, int32_t max_rings,
                                   int32_t max_vertices, int32_t frac_bits, int32_t max_ids, int64_t max_work, int64_t* conflict,
                                   int64_t* counts, int64_t* info, int64_t* totals, void* ws, void* stream) {
  if (!rings || !vertices || !counts_in || !conflict || !counts || !info || !ws) return C3D_E_BADARG;
  if (frac_bits < 0 || frac_bits > 8 || max_work < 0) return C3D_E_BADARG;
  int rc = refuse(max_rings, max_vertices, max_ids);
  if (rc) return rc;
  const Plan pl = plan_of(ws, max_rings, max_vertices, max_ids);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Tab s = pl.t;
  s.rings = rings; s.vertices = reinterpret_cast<const int2*>(vertices); s.counts = counts_in;
  s.coord_max = (int64_t)COORD_UNIT << frac_bits;
  s.max_work = max_work;
  uint32_t* header = static_cast<uint32_t*>(ws);
  const uint32_t* hdr = header;
  u64* rows = reinterpret_cast<u64*>(conflict);

  // the header, the per-id sums and the cell counts: every other word of the workspace is written by the call before the call
  // reads it
  hipError_t e = hipMemsetAsync(ws, 0, (size_t)pl.zero_bytes, st);
  if (e != hipSuccess) return (int)e;
  // the ring, id, edge and cell counts are known on the device only: grids are sized by the maxima and surplus workgroups return
  const unsigned g_rows = grid_for(max_rings, 4, MAX_GRID), g_edge = grid_for(max_vertices, 256, MAX_GRID);
  const unsigned g_cell = grid_for(s.cap_c, 256, MAX_GRID), g_big = grid_for(max_vertices, 4 * 256, 1024);
  rc = c3d_launch_lds<conflicts_rows_kernel>(dim3(g_rows), dim3(256), 0, st, s);
  if (rc) return rc;
  rc = c3d_launch_lds<conflicts_check_big_kernel>(dim3(g_big), dim3(256), 0, st, s);
  if (rc) return rc;
  rc = c3d_launch_lds<conflicts_ids_kernel>(dim3(1), dim3(SCAN_T), 2 * (SCAN_T / 64) * 8, st, s);
  if (rc) return rc;
  rc = c3d_launch_lds<conflicts_edges_kernel>(dim3(g_rows), dim3(256), 0, st, s, header);
  if (rc) return rc;
  rc = c3d_launch_lds<conflicts_edges_big_kernel>(dim3(g_big), dim3(256), 0, st, s, header);
  if (rc) return rc;
  rc = c3d_launch_lds<conflicts_cost_kernel>(dim3(g_edge), dim3(256), 0, st, s, header);
  if (rc) return rc;
  rc = c3d_launch_lds<conflicts_choose_kernel>(dim3(1), dim3(64), 0, st, s, header);
  if (rc) return rc;
  rc = c3d_launch_lds<conflicts_count_kernel>(dim3(g_edge), dim3(256), 0, st, s, hdr);
  if (rc) return rc;
  rc = c3d_launch_lds<conflicts_starts_kernel>(dim3(g_cell), dim3(256), 0, st, s, header);
  if (rc) return rc;
  rc = c3d_launch_lds<conflicts_scatter_kernel>(dim3(g_edge), dim3(256), 0, st, s, hdr);
  if (rc) return rc;
  rc = c3d_launch_lds<conflicts_init_kernel>(dim3(grid_for(max_ids, 256, MAX_GRID)), dim3(256), 0, st, s, hdr, rows);
  if (rc) return rc;
  rc = c3d_launch_lds<conflicts_wave_kernel>(dim3(g_cell), dim3(256), 0, st, s, header, rows);
  if (rc) return rc;
  rc = c3d_launch_lds<conflicts_jobs_kernel>(dim3(grid_for(s.cap_j, 1, MAX_GRID)), dim3(BLOCK_T), (size_t)TILE * 20, st, s, header, rows);
  if (rc) return rc;
  return c3d_launch_lds<conflicts_tail_kernel>(dim3(1), dim3(256), 5 * 256 * 8, st, s, hdr, conflict, counts, info, totals);
}
