// Crossing-free shared walls: the shared-wall simplification of csrc/scene_shared.hip run in rounds, each arc with a tolerance
// of its own.  A round simplifies every ring with the current levels, finds the defective pairs of output edges and the defective
// rings, and raises the level of every arc that takes part in one; the loop ends when a round finds nothing.  The rule -- the
// arc key, the level, the defective pair and ring, the stopping rules -- is the header's (include/change3d_hip.h,
// c3d_outlines_simplify_safe); this file is one way to compute it.  Integer arithmetic and integer atomics only.  The passes up
// to the augmented ring and the three-tier Douglas-Peucker body are copies of csrc/scene_shared.hip, which stays as it is; the
// cell grid is a copy of csrc/scene_conflicts.hip's, and the class of a pair is csrc/scene_rings.h's.
//
// Once, before round 0:
//   nodes, count, scan_rows, augment   as in scene_shared.hip; augment also keeps the direction of the edge leaving every vertex
//   keys       whoever owns a ring (a wave up to WAVE_LIMIT augmented vertices, a workgroup beyond): the arc of every vertex by
//              an exclusive max-scan over the node flags, the key of every arc from its two end steps, the key of its arc for
//              every vertex, and the `present` bit of the key in the level store; arcs, closed arcs, arcs with a left label
// Every round, each kernel returning at once when the device word WS_DONE is set:
//   dp         the three tiers of scene_shared.hip; the level of an arc is read at its first vertex when the chord starts of
//              round 0 are set up and kept in the arc word of that vertex, so the split test costs two LDS reads more
//   scan_kept, scatter   as there; the scatter also writes level_out, the row, index and key of the edge leaving every output
//              vertex, and marks every arc of a defective ring
//   edges      a thread per output vertex: the edge (a, b) that leaves it, the live count, the box of the live edges
//   cost, choose, zero, count, starts, fill   the grid of scene_conflicts.hip over the live edges
//   wave, jobs the pairs of a cell by the lower-corner rule, same-id pairs included; a defective pair ORs the mark bit of both
//              keys into the level store and counts once
//   raise      a thread per word of the level store (a word per lattice point, a byte per direction): counts the arcs above
//              level 0 and at the cap, clears the marks, adds 1 below the cap
//   tail       one workgroup: the stopping rules, `safe`, the grid columns of info, and zeroes the round's header
// Every ring is simplified again in every round: a round is a fixed sequence of launches without a list of rings to redo.
// No workgroup waits for another, nothing is read back, every loop is capped by a count that was checked against the workspace.
#include <climits>
#include <type_traits>

#include "scene_rings.h"

namespace {

typedef unsigned long long u64;

constexpr int WAVE_LIMIT = 64;
// 28 bytes of state per augmented vertex (best and idx 8 each, link, arc and the packed position 4 each) and 96 for the workgroup
constexpr int LDS_LIMIT = 5800;
constexpr int LDS_MISC = 96;
static_assert(LDS_LIMIT % 2 == 0 && LDS_LIMIT * 28 + LDS_MISC <= 160 * 1024, "the ring state of the LDS tier fills at most one CU's LDS");
constexpr int LDS_BYTES = LDS_LIMIT * 28 + LDS_MISC;
constexpr int WAVE_LDS_BYTES = WAVE_LIMIT * 28 + LDS_MISC;
constexpr int BLOCK_T = 1024;
constexpr int COORD_MAX = 16384;
constexpr int MAX_GRID = 2048;
constexpr int SCAN_ROWS = 8;
constexpr int ROW_PASS = -1, ROW_BAD = -2;                 // naug[r] / kept[r] of a row that is not simplified
constexpr uint32_t NODE_BIT = 0x80000000u;                 // of a meta word; the rest is the left label
constexpr uint32_t NO_ROOM = 0xFFFFFFFFu;                  // startp[r] of a ring that max_vertices_out cuts off
constexpr u64 IDX_NONE = ~0ull, SPLIT_MARK = ~0ull - 1;    // keys stay below 2^61
// the level store: a byte per arc key = a word per lattice point, the byte of direction d at bits 8 d
constexpr uint32_t LV_LEVEL = 0x3Fu, LV_PRESENT = 0x40u, LV_MARK = 0x80u;
// the detector's grid, as in scene_conflicts.hip
constexpr int CELL_WAVE_LIMIT = 64;                        // entries of a cell in the wave tier: a lane each
constexpr int CHUNK = 256;                                 // entries of a chunk: a thread each; an LDS tile is one chunk
constexpr int BUDGET_E = 2;                                // entries the grid may hold per live edge
constexpr int BUDGET_C = 4;                                // cells the grid may have per live edge
constexpr int N_SHIFT = 26;
constexpr int PAIR_T = 256;
constexpr int CELL_GRID = 4096;
constexpr int BIAS = 1 << 24;                              // above every coordinate: biased values are positive, 0 means none

// words of the call's header (256 bytes, zeroed by the memset)
enum { WS_ERR = 0, WS_ROWS = 1, WS_FOUND = 2, WS_STATUS = 3, WS_BADCOUNTS = 4, WS_LARGE = 5, WS_WRITTEN = 6, WS_INFO = 8,
       WS_DONE = 16, WS_ROUND = 17, WS_RUN = 18, WS_RAISED = 19, WS_RINGS0 = 20, WS_PAIRS0 = 22 /* u64 */ };
enum { INFO_INSERTED = 0, INFO_NODES = 1, INFO_ARCS = 2, INFO_CLOSED = 3, INFO_SHARED = 4, INFO_COLLAPSED = 5 };
// words of the round's header (512 bytes behind the call's; zeroed by the memset and by every round's tail)
enum { RH_EDGES = 0, RH_LO_X = 1, RH_LO_Y = 2, RH_HI_X = 3, RH_HI_Y = 4, RH_SHIFT = 5, RH_CX = 6, RH_CY = 7, RH_X0 = 8, RH_Y0 = 9,
       RH_AT = 10, RH_JOBS = 11, RH_BAD_RINGS = 12, RH_UP = 13, RH_ABOVE = 14, RH_AT_CAP = 15 };
// 64-bit words of the round's header, counted from its byte 64
enum { RQ_WORK = 0, RQ_ENTRIES = 1, RQ_PAIRS = 2, RQ_COST = 4 /* N_SHIFT of them */ };
constexpr int HEADER_BYTES = 256 + 512;
static_assert(64 + (RQ_COST + N_SHIFT) * 8 <= 512, "the round's header holds the cost of every shift");

struct Workspace {
  int64_t naug, off, rot, kept, startp, large, ap, meta, flags, link, arc, idx, best, rowbits, colbits;   // byte offsets
  int64_t dirs, vkey, levels, e_key, e_info, e_xy, cell_n, cell_at, entry, jobs, bytes;
  int64_t level_words, cap_e, cap_c, cap_j;
  int WR, WC;                                              // words per row of the two node bitmaps
};

Workspace workspace_plan(int64_t Hs, int64_t Ws, int64_t max_rings, int64_t max_vertices, int64_t max_out) {
  Workspace w;
  auto up = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  const int64_t A = 2 * max_vertices;
  w.naug = HEADER_BYTES;
  w.off = w.naug + up(max_rings * 4);
  w.rot = w.off + up(max_rings * 4);
  w.kept = w.rot + up(max_rings * 4);
  w.startp = w.kept + up(max_rings * 4);
  w.large = w.startp + up(max_rings * 4);
  w.ap = w.large + up(max_rings * 4);
  w.meta = w.ap + up(A * 4);
  w.flags = w.meta + up(A * 4);
  w.link = w.flags + up(A);
  w.arc = w.link + up(A * 4);
  w.idx = w.arc + up(A * 4);
  w.best = w.idx + up(A * 8);
  w.WR = (int)((Ws + 1 + 31) / 32);
  w.WC = (int)((Hs + 1 + 31) / 32);
  w.rowbits = w.best + up(A * 8);
  w.colbits = w.rowbits + up((Hs + 1) * w.WR * 4);
  w.dirs = w.colbits + up((Ws + 1) * w.WC * 4);
  w.vkey = w.dirs + up(A);
  w.level_words = (Hs + 1) * (Ws + 1);
  w.levels = w.vkey + up(A * 4);
  // both budgets hold for one cell whatever the output holds (at most max_out live edges, one entry each): the sizes are a
  // function of max_vertices_out alone
  w.cap_e = BUDGET_E * max_out;
  w.cap_c = BUDGET_C * max_out;
  w.cap_j = w.cap_e / CHUNK + w.cap_e / (CELL_WAVE_LIMIT + 1) + 1;
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

struct Scene {
  const int32_t* labels;
  int Hs, Ws, rows;
};

__device__ __forceinline__ int label_at(const Scene& s, int y, int x) {
  if ((unsigned)y >= (unsigned)s.Hs || (unsigned)x >= (unsigned)s.Ws) return 0;
  const int v = s.labels[(int64_t)y * s.Ws + x];
  return (v >= 1 && v <= s.rows) ? v : 0;
}
__device__ __forceinline__ bool is_node(const Scene& s, int vx, int vy) {
  const int a = label_at(s, vy - 1, vx - 1), b = label_at(s, vy - 1, vx), c = label_at(s, vy, vx - 1), d = label_at(s, vy, vx);
  return (a != b) + (c != d) + (a != c) + (b != d) >= 3;
}
// the label left of the unit edge that leaves (vx, vy) in direction (dx, dy): the object is on the right, y points down
__device__ __forceinline__ int left_of(const Scene& s, int vx, int vy, int dx, int dy) {
  if (dx > 0) return label_at(s, vy - 1, vx);
  if (dy > 0) return label_at(s, vy, vx);
  if (dx < 0) return label_at(s, vy, vx - 1);
  return label_at(s, vy - 1, vx - 1);
}
__device__ __forceinline__ Scene scene_of(const int32_t* labels, const int32_t* counts_obj, int Hs, int Ws, int max_objects) {
  const int r = counts_obj[1];
  return Scene{labels, Hs, Ws, r < 0 ? 0 : (r > max_objects ? max_objects : r)};
}

// the node bitmaps: bit vx of row vy of `rows`, bit vy of row vx of `cols`
struct Bits {
  const uint32_t* rows;
  const uint32_t* cols;
  int WR, WC;
};
__device__ __forceinline__ bool node_bit(const Bits& b, int vx, int vy) {
  return (b.rows[(int64_t)vy * b.WR + (vx >> 5)] >> (vx & 31)) & 1u;
}
// the word w of a bitmap row cut to the positions lo .. hi (inclusive; w lies in lo >> 5 .. hi >> 5)
__device__ __forceinline__ uint32_t cut_word(const uint32_t* row, int w, int lo, int hi) {
  uint32_t m = row[w];
  if (w == (lo >> 5)) m &= 0xFFFFFFFFu << (lo & 31);
  if (w == (hi >> 5)) m &= 0xFFFFFFFFu >> (31 - (hi & 31));
  return m;
}
__device__ __forceinline__ uint32_t count_range(const uint32_t* row, int lo, int hi) {
  uint32_t c = 0;
  if (lo <= hi)
    for (int w = lo >> 5; w <= (hi >> 5); ++w) c += (uint32_t)__popc(cut_word(row, w, lo, hi));
  return c;
}

__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_max64(u64 v) {
  for (int d = 32; d; d >>= 1) {
    const u64 o = shfl64(v, (int)((threadIdx.x & 63) ^ d));
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ u64 wave_min64(u64 v) {
  for (int d = 32; d; d >>= 1) {
    const u64 o = shfl64(v, (int)((threadIdx.x & 63) ^ d));
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_min32u(uint32_t v) {
  for (int d = 32; d; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, d);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
  for (int d = 32; d; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
  return v;
}
__device__ __forceinline__ u64 wave_sum64(u64 v) {
  for (int d = 32; d; d >>= 1) v += shfl64(v, (int)((threadIdx.x & 63) ^ d));
  return v;
}
// exclusive prefix sum over the lanes of a wave; *all = the wave's sum
__device__ __forceinline__ uint32_t wave_excl_scan32(uint32_t v, uint32_t* all) {
  const int lane = threadIdx.x & 63;
  uint32_t inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = (uint32_t)__shfl((int)inc, lane >= d ? lane - d : lane);
    if (lane >= d) inc += t;
  }
  *all = (uint32_t)__shfl((int)inc, 63);
  return inc - v;
}

// exclusive prefix of v over the workgroup's threads; `all` = the sum.  part: one word of LDS per wave; the caller syncs
// before reusing it
__device__ __forceinline__ u64 block_excl_scan64(u64 v, u64* part, u64* all) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  u64 inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const u64 t = shfl64(inc, lane >= d ? lane - d : lane);
    if (lane >= d) inc += t;
  }
  if (lane == 63) part[wave] = inc;
  __syncthreads();
  u64 before = 0, sum = 0;
  for (int w = 0; w < waves; ++w) {
    before += w < wave ? part[w] : 0ull;
    sum += part[w];
  }
  *all = sum;
  return before + inc - v;
}

// exclusive prefix maximum of v (>= -1) over the workgroup's threads; `all` = the maximum.  part as above
__device__ __forceinline__ int block_excl_max32(int v, int* part, int* all) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  int inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl(inc, lane >= d ? lane - d : lane);
    if (lane >= d) inc = t > inc ? t : inc;
  }
  const int up = __shfl(inc, lane ? lane - 1 : 0);
  if (lane == 63) part[wave] = inc;
  __syncthreads();
  int before = -1, top = -1;
  for (int w = 0; w < waves; ++w) {
    if (w < wave) before = part[w] > before ? part[w] : before;
    top = part[w] > top ? part[w] : top;
  }
  *all = top;
  const int mine = lane ? up : -1;
  return mine > before ? mine : before;
}

// squared distance of p to the segment (a, b) as num / den
__device__ __forceinline__ u64 seg_num(int2 a, int2 b, int2 p, u64* den) {
  const int64_t dx = b.x - a.x, dy = b.y - a.y, qx = p.x - a.x, qy = p.y - a.y;
  const int64_t L2 = dx * dx + dy * dy, pa2 = qx * qx + qy * qy;
  if (L2 == 0) { *den = 1; return (u64)pa2; }
  *den = (u64)L2;
  const int64_t t = qx * dx + qy * dy;
  if (t <= 0) return (u64)(pa2 * L2);
  if (t >= L2) {
    const int64_t rx = p.x - b.x, ry = p.y - b.y;
    return (u64)((rx * rx + ry * ry) * L2);
  }
  const int64_t c = dx * qy - dy * qx;
  return (u64)(c * c);
}
__device__ __forceinline__ uint32_t abs_cross(int2 a, int2 b, int2 p) {
  const int c = (b.x - a.x) * (p.y - a.y) - (b.y - a.y) * (p.x - a.x);
  return (uint32_t)(c < 0 ? -c : c);
}
__device__ __forceinline__ uint32_t pos_key(int2 p) { return (uint32_t)(p.y * (COORD_MAX + 1) + p.x); }   // below 2^29
__device__ __forceinline__ uint32_t pack(int x, int y) { return (uint32_t)x | ((uint32_t)y << 16); }
__device__ __forceinline__ int2 unpack(uint32_t v) { return make_int2((int)(v & 0xFFFFu), (int)(v >> 16)); }

// the stored edge k of a ring: its direction and length, or len = 0 for one that the rule refuses
struct Edge {
  int2 p;
  int dx, dy, len;
  const uint32_t* row;                                     // the bitmap row along the edge, and the positions strictly inside it
  int lo, hi;
};
__device__ __forceinline__ Edge edge_of(const int2* __restrict__ v, int64_t start, int k, int nv, const Scene& s, const Bits& b) {
  Edge e;
  e.p = v[start + k];
  const int2 q = v[start + (k + 1 == nv ? 0 : k + 1)];
  const bool ok = e.p.x >= 0 && e.p.x <= s.Ws && e.p.y >= 0 && e.p.y <= s.Hs && q.x >= 0 && q.x <= s.Ws && q.y >= 0 && q.y <= s.Hs &&
                  ((e.p.x != q.x) != (e.p.y != q.y));
  e.dx = (q.x > e.p.x) - (q.x < e.p.x);
  e.dy = (q.y > e.p.y) - (q.y < e.p.y);
  const int len = (q.x - e.p.x) * e.dx + (q.y - e.p.y) * e.dy;
  e.len = ok ? len : 0;                                    // at most COORD_MAX: Hs, Ws <= COORD_MAX
  e.row = b.rows;
  e.lo = 1;
  e.hi = 0;
  if (ok) {                                                // the vertex is inside the scene's lattice: so is the row
    const int from = e.dx ? e.p.x : e.p.y, to = e.dx ? q.x : q.y;
    e.row = e.dx ? b.rows + (int64_t)e.p.y * b.WR : b.cols + (int64_t)e.p.x * b.WC;
    e.lo = (from < to ? from : to) + 1;
    e.hi = (from < to ? to : from) - 1;
  }
  return e;
}

struct Limits {
  int rows;
  int64_t vlimit;
};
__device__ __forceinline__ Limits limits_of(const int32_t* counts, int max_rings, int max_vertices) {
  const int rows_in = counts[1], written = counts[3];
  Limits l;
  l.rows = (counts[4] & C3D_OUTLINE_ST_BAD_COUNTS) ? 0 : (rows_in < 0 ? 0 : (rows_in > max_rings ? max_rings : rows_in));
  l.vlimit = written < 0 ? 0 : (written > max_vertices ? max_vertices : written);
  return l;
}

// ------------------------------------------------------------------------------------------------ 0: the node bitmaps
// COLS = false: line = vy, position = vx; COLS = true: line = vx, position = vy.  A wave owns 64 consecutive positions of one
// line or of two (a line is a whole number of words), and writes its two words whole: padding bits are 0
template <bool COLS>
__global__ __launch_bounds__(256) void safe_nodes_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ counts_obj,
                                                           int Hs, int Ws, int max_objects, uint32_t* __restrict__ bits, int words) {
  const Scene s = scene_of(labels, counts_obj, Hs, Ws, max_objects);
  const int64_t per_line = (int64_t)words * 32, total = (int64_t)((COLS ? Ws : Hs) + 1) * per_line;
  const int extent = COLS ? Hs : Ws, lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int line = (int)(i / per_line), pos = (int)(i - (int64_t)line * per_line);
    const bool bit = pos <= extent && (COLS ? is_node(s, line, pos) : is_node(s, pos, line));
    const u64 m = __ballot(bit);                           // total is a multiple of 32: the lanes of a half wave are in or out together
    if ((lane & 31) == 0) bits[i >> 5] = lane ? (uint32_t)(m >> 32) : (uint32_t)m;
  }
}

// --------------------------------------------------------------------------------------------------- 1: one wave per row
__global__ __launch_bounds__(256) void safe_count_rows_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ counts_obj,
                                                           int Hs, int Ws, int max_objects, const int32_t* __restrict__ rings,
                                                           const int2* __restrict__ vertices, const int32_t* __restrict__ counts,
                                                           int max_rings, int max_vertices, int32_t* __restrict__ naug, Bits bits) {
  const Scene s = scene_of(labels, counts_obj, Hs, Ws, max_objects);
  const Limits lim = limits_of(counts, max_rings, max_vertices);
  const int lane = threadIdx.x & 63;
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < lim.rows; r += gridDim.x * 4) {   // r is uniform over the wave
    const int start = rings[(int64_t)r * 8 + 1], nv = rings[(int64_t)r * 8 + 2];
    if (start < 0) {
      if (lane == 0) naug[r] = ROW_PASS;
      continue;
    }
    if (nv < 4 || (int64_t)start + nv > lim.vlimit) {
      if (lane == 0) naug[r] = ROW_BAD;
      continue;
    }
    u64 mine = 0;
    bool bad = false;
    for (int k = lane; k < nv; k += 64) {
      const Edge e = edge_of(vertices, start, k, nv, s, bits);
      bad |= e.len == 0;
      mine += 1u + count_range(e.row, e.lo, e.hi);
    }
    const bool any_bad = __any(bad);
    const u64 total = wave_sum64(mine);
    if (lane == 0) naug[r] = (any_bad || total > (u64)INT_MAX) ? ROW_BAD : (int)total;
  }
}

// ------------------------------------------------------------------------------------------------ 2: one workgroup in all
__global__ __launch_bounds__(BLOCK_T) void safe_scan_rows_kernel(const int32_t* __restrict__ counts, int32_t* __restrict__ naug,
                                                               uint32_t* __restrict__ off, uint32_t* __restrict__ large,
                                                               uint32_t* __restrict__ header, int max_rings, int max_vertices) {
  extern __shared__ u64 part[];                            // [BLOCK_T / 64]
  const Limits lim = limits_of(counts, max_rings, max_vertices);
  const int rows = lim.rows;
  const u64 cap = 2ull * (u64)max_vertices;
  u64 running = 0;
  bool bad = false;
  for (int base = 0; base < rows; base += BLOCK_T * SCAN_ROWS) {
    int n[SCAN_ROWS], cls[SCAN_ROWS];
    u64 mine = 0;
    for (int j = 0; j < SCAN_ROWS; ++j) {
      const int r = base + (int)threadIdx.x * SCAN_ROWS + j;
      const int c = r < rows ? naug[r] : ROW_PASS;
      cls[j] = c < 0 ? c : 0;
      n[j] = c < 0 ? 0 : c;
      mine += (u64)n[j];
    }
    u64 all;
    u64 at = running + block_excl_scan64(mine, part, &all);
    for (int j = 0; j < SCAN_ROWS; ++j) {
      const int r = base + (int)threadIdx.x * SCAN_ROWS + j;
      if (r < rows) {
        if (cls[j] == 0 && at + (u64)n[j] > cap) { cls[j] = ROW_BAD; naug[r] = ROW_BAD; }   // no room for its augmented ring
        bad |= cls[j] == ROW_BAD;
        off[r] = (uint32_t)(at < 0xFFFFFFFFull ? at : 0xFFFFFFFFull);
        if (cls[j] == 0 && n[j] > WAVE_LIMIT) large[atomicAdd(header + WS_LARGE, 1u)] = (uint32_t)r;   // at most rows entries
      }
      at += (u64)n[j];
    }
    running += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    header[WS_ROWS] = (uint32_t)rows;
    header[WS_FOUND] = (uint32_t)counts[0];
    header[WS_STATUS] = (uint32_t)counts[4];
    header[WS_BADCOUNTS] = (counts[4] & C3D_OUTLINE_ST_BAD_COUNTS) ? 1u : 0u;
  }
  if (bad) atomicOr(header + WS_ERR, 1u);
}

// --------------------------------------------------------------------------------------------------- 3: one wave per row
__global__ __launch_bounds__(256) void safe_augment_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ counts_obj,
                                                             int Hs, int Ws, int max_objects, const int32_t* __restrict__ rings,
                                                             const int2* __restrict__ vertices, const int32_t* __restrict__ naug,
                                                             const uint32_t* __restrict__ off, uint32_t* __restrict__ rot,
                                                             uint32_t* __restrict__ ap, uint32_t* __restrict__ meta,
                                                             uint8_t* __restrict__ dirs, uint32_t* __restrict__ header, Bits bits) {
  const Scene s = scene_of(labels, counts_obj, Hs, Ws, max_objects);
  const int lane = threadIdx.x & 63, rows = (int)header[WS_ROWS];
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += gridDim.x * 4) {
    const int n = naug[r];
    if (n < 0) continue;
    const int start = rings[(int64_t)r * 8 + 1], nv = rings[(int64_t)r * 8 + 2];
    const int64_t o = off[r];
    uint32_t run = 0, first_node = 0xFFFFFFFFu, inserted = 0, nodes = 0;
    u64 smallest = ~0ull;
    for (int base = 0; base < nv; base += 64) {
      const int k = base + lane;
      const bool in = k < nv;
      Edge e;
      e.len = 0;
      uint32_t c = 0;
      if (in) {
        e = edge_of(vertices, start, k, nv, s, bits);      // count validated every edge of this row
        c = 1u + count_range(e.row, e.lo, e.hi);
      }
      uint32_t all;
      uint32_t pos = run + wave_excl_scan32(c, &all);
      run += all;
      // the last condition cannot fail: the bits are the ones that count read
      if (in && e.len != 0 && (u64)pos + c <= (u64)n) {
        const uint32_t lf = (uint32_t)left_of(s, e.p.x, e.p.y, e.dx, e.dy);
        const bool corner_node = node_bit(bits, e.p.x, e.p.y);
        const uint8_t dir = (uint8_t)(e.dx > 0 ? 0 : (e.dy > 0 ? 1 : (e.dx < 0 ? 2 : 3)));   // as the tracer numbers sides
        ap[o + pos] = pack(e.p.x, e.p.y);
        meta[o + pos] = lf | (corner_node ? NODE_BIT : 0u);
        dirs[o + pos] = dir;
        const u64 key = ((u64)pos_key(e.p) << 32) | pos;
        smallest = key < smallest ? key : smallest;
        if (corner_node) { first_node = pos < first_node ? pos : first_node; ++nodes; }
        uint32_t at = pos + 1;
        const bool up = e.dx + e.dy > 0;                   // the travel runs towards larger positions
        const int w_first = up ? e.lo >> 5 : e.hi >> 5, w_last = up ? e.hi >> 5 : e.lo >> 5;
        for (int w = w_first; e.lo <= e.hi && (up ? w <= w_last : w >= w_last); w += up ? 1 : -1) {
          uint32_t m = cut_word(e.row, w, e.lo, e.hi);
          while (m && at < pos + c) {                      // the nodes inside the edge, in travel order
            const int b = up ? __ffs((int)m) - 1 : 31 - __clz((int)m);
            m &= ~(1u << b);
            const int t = w * 32 + b, x = e.dx ? t : e.p.x, y = e.dx ? e.p.y : t;
            ap[o + at] = pack(x, y);
            meta[o + at] = (uint32_t)left_of(s, x, y, e.dx, e.dy) | NODE_BIT;
            dirs[o + at] = dir;
            first_node = at < first_node ? at : first_node;
            ++at;
            ++inserted;
            ++nodes;
          }
        }
      }
    }
    first_node = wave_min32u(first_node);
    smallest = wave_min64(smallest);
    inserted = wave_sum32(inserted);
    nodes = wave_sum32(nodes);
    if (lane == 0) {
      const uint32_t st = first_node != 0xFFFFFFFFu ? first_node : (uint32_t)smallest;
      rot[r] = st < (uint32_t)n ? st : 0u;
      if (inserted) atomicAdd(header + WS_INFO + INFO_INSERTED, inserted);
      if (nodes) atomicAdd(header + WS_INFO + INFO_NODES, nodes);
    }
  }
}

// ------------------------------------------------------------------------------------------ 4: one workgroup of T per ring
// The rotated ring has the vertices 0 .. n-1 and the closing repeat n of vertex 0; vertex 0 is a node, or stands for one.
// link[k] >= 0: vertex k is open, link[k] = its chord's first vertex lo; -1: dropped; < -1: kept, ~link[k] = the end of the chord
// that starts at k.  arc[k] >= 0: k is no node, arc[k] = the node its arc starts at; arc[k] < 0: k is a node and ~arc[k] says
// whether the arc that starts at k is closed (bit 0) and its level getL(k) (the bits above).  best / idx are used at chord starts
// only.  sh: 18 words of LDS.  Returns the kept count; flags_out[k] = kept.  Every thread of the workgroup calls it with the
// same arguments.
__device__ __forceinline__ int arc_word(bool closed, int level) { return ~((closed ? 1 : 0) | (level << 1)); }
__device__ __forceinline__ bool arc_closed(int word) { return (~word) & 1; }
__device__ __forceinline__ int arc_level(int word) { return (~word) >> 1; }
template <int T, class GetP, class GetM, class GetL>
__device__ __forceinline__ int ring_dp(GetP getP, GetM getM, GetL getL, int* link, int* arc, u64* idx, u64* best,
                                       uint8_t* __restrict__ flags_out, int n, u64 tol2_q, int* sh) {
  const int tid = threadIdx.x, lane = tid & 63;
  int* part = sh;                                          // [16]
  int* sh_cnt = sh + 16;
  int* sh_far = sh + 17;
  if (tid == 0) *sh_cnt = 0;
  int last = -1;                                           // the last node below the step's vertices
  for (int base = 0; base < n; base += T) {
    const int k = base + tid;
    const uint32_t m = k < n ? getM(k) : 0u;
    const bool node = k < n && (k == 0 || (m & NODE_BIT));
    int top;
    int e = block_excl_max32(node ? k : -1, part, &top);
    e = e > last ? e : last;
    last = top > last ? top : last;
    if (k < n) {
      if (node) {
        best[k] = 0;
        idx[k] = IDX_NONE;
        if (k > 0) {
          const int2 a = getP(e), b = getP(k);
          const bool closed = a.x == b.x && a.y == b.y;
          link[e] = ~k;
          arc[e] = arc_word(closed, getL(e));
        }
      } else {
        link[k] = e;
        arc[k] = e;
      }
    }
    __syncthreads();                                       // part is reused by the next step
  }
  if (tid == 0) {                                          // the arc of the last node ends at the closing repeat of vertex 0
    const int2 a = getP(last), b = getP(0);
    const bool closed = a.x == b.x && a.y == b.y;
    link[last] = ~n;
    arc[last] = arc_word(closed, getL(last));
  }
  __syncthreads();

  // the steps t (vertex k = T t + tid) in which this wave still has an open vertex: open vertices only close
  int t0 = 0, t1 = (n + T - 1) / T;
  auto chord = [&](int lo, int2* a, int2* b, int* hi) {
    *hi = ~link[lo];
    *a = getP(lo);
    *b = getP(*hi == n ? 0 : *hi);
  };
  for (int round = 0; round <= n; ++round) {               // every round but the last keeps a vertex: at most n rounds
    int nt0 = t1, nt1 = t0;
    for (int t = t0; t < t1; ++t) {                        // max
      const int k = t * T + tid, lo = k < n ? link[k] : -1;
      const bool act = lo >= 0;
      const u64 mk = __ballot(act);
      if (!mk) continue;
      nt0 = t < nt0 ? t : nt0;
      nt1 = t + 1;
      u64 num = 0, den;
      if (act) {
        int2 a, b;
        int hi;
        chord(lo, &a, &b, &hi);
        num = seg_num(a, b, getP(k), &den);
      }
      const int leader = __ffsll((long long)mk) - 1, lo0 = __shfl(lo, leader);
      if (__ballot(act && lo != lo0) == 0) {
        const u64 w = wave_max64(num);
        if (lane == leader) atomicMax(best + lo0, w);
      } else if (act) {
        atomicMax(best + lo, num);
      }
    }
    t0 = nt0;
    t1 = nt1;
    __syncthreads();
    if (tid == 0) *sh_far = 0;                             // read after the last barrier of the round before, set after the next
    for (int t = t0; t < t1; ++t) {                        // arg: the smallest (vy, vx) at the maximum, with its index
      const int k = t * T + tid, lo = k < n ? link[k] : -1;
      const bool act = lo >= 0;
      const u64 mk = __ballot(act);
      if (!mk) continue;
      u64 cand = IDX_NONE;
      if (act) {
        int2 a, b;
        int hi;
        u64 den;
        chord(lo, &a, &b, &hi);
        const int2 p = getP(k);
        if (seg_num(a, b, p, &den) == best[lo]) cand = ((u64)pos_key(p) << 32) | (uint32_t)k;
      }
      const int leader = __ffsll((long long)mk) - 1, lo0 = __shfl(lo, leader);
      if (__ballot(act && lo != lo0) == 0) {
        const u64 w = wave_min64(cand);
        if (lane == leader && w != IDX_NONE) atomicMin(idx + lo0, w);
      } else if (cand != IDX_NONE) {
        atomicMin(idx + lo, cand);
      }
    }
    __syncthreads();
    bool any_far = false;
    for (int t = t0; t < t1; ++t) {                        // split: reads chord starts, writes the vertex's own slots
      const int k = t * T + tid, lo = k < n ? link[k] : -1;
      if (lo < 0) continue;
      int2 a, b;
      int hi;
      chord(lo, &a, &b, &hi);
      const int64_t dx = b.x - a.x, dy = b.y - a.y;
      const u64 L2 = (u64)(dx * dx + dy * dy);
      const int aw = arc[lo];                              // the arc's own tolerance: tol2_q >> 2 L
      const u64 tol = tol2_q >> (2 * arc_level(aw < 0 ? aw : arc[aw]));
      if (L2 != 0 && !(16ull * best[lo] > tol * L2)) { link[k] = -1; continue; }   // a chord whose ends coincide always splits
      any_far = true;
      const int m = (int)(uint32_t)idx[lo];
      if (k == m) {
        link[k] = ~hi;
        best[k] = (u64)lo;
        idx[k] = SPLIT_MARK;
      } else if (k > m) {
        link[k] = m;
      }
    }
    if (any_far) *sh_far = 1;                              // every writer stores the same value
    __syncthreads();
    if (!*sh_far) break;
    for (int t = t0; t < t1; ++t) {                        // link: the split vertices of this round were open in it
      const int k = t * T + tid;
      if (k >= n || link[k] >= -1 || idx[k] != SPLIT_MARK) continue;
      const int lo = (int)best[k];
      link[lo] = ~k;
      best[lo] = 0;
      idx[lo] = IDX_NONE;
      best[k] = 0;
      idx[k] = IDX_NONE;
    }
    __syncthreads();
  }

  // the guard of the closed arcs: one that kept a single interior vertex M also keeps the interior vertex farthest from the
  // line through its node and M, unless all of them lie on that line
  for (int k = tid; k < n; k += T)
    if (link[k] < -1) { best[k] = 0; idx[k] = 0; }
  __syncthreads();
  for (int k = tid; k < n; k += T) {                       // idx[a] = the kept interior vertices of the closed arc at a, best[a] = one
    const int a = arc[k];
    if (a < 0 || link[k] >= -1 || !arc_closed(arc[a])) continue;
    atomicAdd(idx + a, 1ull);
    best[a] = (u64)k;
  }
  __syncthreads();
  for (int pass = 0; pass < 2; ++pass) {
    for (int k = tid; k < n; k += T) {
      const int a = arc[k];
      if (a < 0 || link[k] != -1 || !arc_closed(arc[a]) || idx[a] != 1ull) continue;
      const int M = (int)best[a];
      const int2 p = getP(k);
      const uint32_t c = abs_cross(getP(a), getP(M), p);
      if (c == 0) continue;
      const u64 key = ((u64)c << 32) | (0xFFFFFFFFu - pos_key(p));
      if (pass == 0) atomicMax(best + M, key);             // M is kept: its own slot is free, and no vertex of pass 0 reads it
      else if (key == best[M]) link[k] = -3;               // kept; ~(-3) = 2 is never read as a chord end
    }
    __syncthreads();
  }

  for (int base = 0; base < n; base += T) {
    const int k = base + tid;
    const bool f = k < n && link[k] < -1;
    if (k < n) flags_out[k] = f ? 1 : 0;
    const int c = __popcll(__ballot(f));
    if (lane == 0 && c) atomicAdd(sh_cnt, c);
  }
  __syncthreads();
  return *sh_cnt;
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

// T = 64: the rings of up to WAVE_LIMIT augmented vertices, a wave each; T = BLOCK_T: the listed larger ones
template <int T, int LIMIT>
__global__ __launch_bounds__(T) void safe_dp_kernel(const int32_t* __restrict__ naug, const uint32_t* __restrict__ off,
                                                      const uint32_t* __restrict__ rot, const uint32_t* __restrict__ ap,
                                                      const uint32_t* __restrict__ meta, int32_t* __restrict__ kept,
                                                      uint8_t* __restrict__ flags, int32_t* __restrict__ g_link,
                                                      int32_t* __restrict__ g_arc, u64* __restrict__ g_idx, u64* __restrict__ g_best,
                                                      const uint32_t* __restrict__ large, const uint32_t* __restrict__ header,
                                                      const uint32_t* __restrict__ vkey, const uint8_t* __restrict__ levels, u64 tol2_q) {
  if (header[WS_DONE]) return;
  extern __shared__ u64 lds[];                             // best, idx u64 [LIMIT]; link, arc, packed positions u32 [LIMIT]; 18 words
  u64* s_best = lds;
  u64* s_idx = lds + LIMIT;
  int* s_link = reinterpret_cast<int*>(lds + 2 * LIMIT);
  int* s_arc = s_link + LIMIT;
  uint32_t* s_p = reinterpret_cast<uint32_t*>(s_arc + LIMIT);
  int* sh = reinterpret_cast<int*>(s_p + LIMIT);
  const bool wave_tier = T == 64;
  const uint32_t items = wave_tier ? header[WS_ROWS] : header[WS_LARGE];
  for (uint32_t at = blockIdx.x; at < items; at += gridDim.x) {
    const int r = wave_tier ? (int)at : (int)large[at];
    const int n = naug[r];
    if (wave_tier) {
      if (threadIdx.x == 0) kept[r] = n < 0 ? n : 0;       // the workgroup kernel overwrites the larger rings'
      if (n < 0 || n > WAVE_LIMIT) continue;
    } else if (n <= WAVE_LIMIT) {
      continue;                                            // cannot happen: scan_rows listed it
    }
    const int64_t o = off[r];
    const int s = (int)rot[r];
    const bool in_lds = n <= LIMIT;
    auto where = [&](int k) { const int j = k + s; return o + (j >= n ? j - n : j); };
    __syncthreads();                                       // the ring before is done with the LDS
    if (in_lds)
      for (int k = threadIdx.x; k < n; k += T) s_p[k] = ap[where(k)];
    __syncthreads();
    auto getM = [&](int k) { return meta[where(k)]; };
    auto getL = [&](int k) { return (int)(levels[vkey[o + k]] & LV_LEVEL); };   // vkey is kept in rotated order
    int count;
    if (in_lds) {
      count = ring_dp<T>([&](int k) { return unpack(s_p[k]); }, getM, getL, s_link, s_arc, s_idx, s_best, flags + o, n, tol2_q, sh);
    } else {
      count = ring_dp<T>([&](int k) { return unpack(ap[where(k)]); }, getM, getL, g_link + o, g_arc + o, g_idx + o, g_best + o, flags + o,
                         n, tol2_q, sh);
    }
    if (threadIdx.x == 0) kept[r] = count;
  }
}

// start'[r] = kept vertices of the rows before r, or NO_ROOM past max_vertices_out; counts_out; info but for its collapsed rings
__global__ __launch_bounds__(BLOCK_T) void safe_scan_kept_kernel(const int32_t* __restrict__ kept, uint32_t* __restrict__ startp,
                                                               uint32_t* __restrict__ header, int32_t* __restrict__ counts_out,
                                                               int32_t* __restrict__ info, int max_vertices_out) {
  if (header[WS_DONE]) return;
  extern __shared__ u64 part[];                            // [BLOCK_T / 64], then the first start without room
  u64* sh_cut = part + BLOCK_T / 64;
  const int rows = (int)header[WS_ROWS];
  if (threadIdx.x == 0) *sh_cut = ~0ull;
  __syncthreads();
  u64 running = 0;
  for (int base = 0; base < rows; base += BLOCK_T * SCAN_ROWS) {
    int n[SCAN_ROWS];
    u64 mine = 0;
    for (int j = 0; j < SCAN_ROWS; ++j) {
      const int r = base + (int)threadIdx.x * SCAN_ROWS + j;
      const int c = r < rows ? kept[r] : 0;
      n[j] = c > 0 ? c : 0;
      mine += (u64)n[j];
    }
    u64 all;
    u64 at = running + block_excl_scan64(mine, part, &all);
    for (int j = 0; j < SCAN_ROWS; ++j) {
      const int r = base + (int)threadIdx.x * SCAN_ROWS + j;
      if (r < rows) {
        const bool fits = at + (u64)n[j] <= (u64)max_vertices_out;
        startp[r] = fits ? (uint32_t)at : NO_ROOM;
        if (!fits) atomicMin(sh_cut, at);
      }
      at += (u64)n[j];
    }
    running += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    for (int j = 0; j < 8; ++j) info[j] = 0;
    if (header[WS_BADCOUNTS]) {
      counts_out[0] = counts_out[1] = counts_out[2] = counts_out[3] = 0;
      counts_out[4] = C3D_OUTLINE_ST_BAD_COUNTS;
      header[WS_WRITTEN] = 0u;
    } else {
      const u64 written = *sh_cut == ~0ull ? running : *sh_cut;
      counts_out[0] = (int32_t)header[WS_FOUND];
      counts_out[1] = rows;
      counts_out[2] = (int32_t)(running > (u64)INT_MAX ? (u64)INT_MAX : running);
      counts_out[3] = (int32_t)written;
      header[WS_WRITTEN] = (uint32_t)written;
      counts_out[4] = (int32_t)(header[WS_STATUS] | (header[WS_ERR] ? (uint32_t)C3D_SIMPLIFY_ST_BAD_INPUT : 0u) |
                                (written < running ? (uint32_t)C3D_OUTLINE_ST_TRUNCATED : 0u));
      for (int j = 0; j < 5; ++j) info[j] = (int32_t)header[WS_INFO + j];
    }
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
__device__ __forceinline__ void edge_out(const Marks& mk, int64_t to, uint32_t key, int id, int row, int k, int n) {
  mk.level_out[to] = (int32_t)(reinterpret_cast<const uint8_t*>(mk.level_words)[key] & LV_LEVEL);
  mk.e_key[to] = key;
  mk.e_info[to] = make_int4(id, row, k, n);
}
// n' < 3, or an area whose sign is not that of the input row
__device__ __forceinline__ bool ring_defective(int count, int area2, int area_in) {
  return count < 3 || ((area2 > 0) - (area2 < 0)) != ((area_in > 0) - (area_in < 0));
}

__device__ __forceinline__ void write_row(int32_t* __restrict__ rings_out, int r, const int4 r0, const int4 r1, int start, int n,
                                          int area2, int x, int y) {
  int4* dst = reinterpret_cast<int4*>(rings_out + (int64_t)r * 8);
  dst[0] = make_int4(r0.x, start, n, area2);
  dst[1] = make_int4(r1.x, x, y, r0.z);
}

// rows of rings of up to WAVE_LIMIT augmented vertices, rows that are not simplified, and the zero rows past the table
__global__ __launch_bounds__(256) void safe_scatter_wave_kernel(const int32_t* __restrict__ rings, const int32_t* __restrict__ naug,
                                                                  const uint32_t* __restrict__ off, const uint32_t* __restrict__ rot,
                                                                  const uint32_t* __restrict__ ap, const uint32_t* __restrict__ meta,
                                                                  const int32_t* __restrict__ kept, const uint32_t* __restrict__ startp,
                                                                  const uint8_t* __restrict__ flags, const uint32_t* __restrict__ header,
                                                                  int32_t* __restrict__ rings_out, int2* __restrict__ vertices_out,
                                                                  int32_t* __restrict__ left_out, int32_t* __restrict__ info,
                                                                  int max_rings, Marks mk) {
  if (header[WS_DONE]) return;
  const int lane = threadIdx.x & 63, rows = (int)header[WS_ROWS];
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < max_rings; r += gridDim.x * 4) {
    int4* dst = reinterpret_cast<int4*>(rings_out + (int64_t)r * 8);
    if (r >= rows) {
      if (lane < 2) dst[lane] = make_int4(0, 0, 0, 0);
      continue;
    }
    const int4 r0 = reinterpret_cast<const int4*>(rings + (int64_t)r * 8)[0], r1 = reinterpret_cast<const int4*>(rings + (int64_t)r * 8)[1];
    const int count = kept[r];
    const uint32_t at = startp[r];
    if (count < 0 || at == NO_ROOM) {
      if (lane == 0) write_row(rings_out, r, r0, r1, -1, 0, 0, r1.y, r1.z);
      continue;
    }
    const int n = naug[r];
    if (n > WAVE_LIMIT) continue;
    const int64_t o = off[r];
    const int s = (int)rot[r];
    const int j = lane + s, src = j >= n ? j - n : j;
    const bool f = lane < n && flags[o + lane];
    const int2 p = f ? unpack(ap[o + src]) : make_int2(0, 0);
    const u64 mask = __ballot(f), below = mask & ((1ull << lane) - 1ull);
    const u64 from = below ? below : mask;                 // the kept vertex before this one, cyclically
    const int prev = from ? 63 - __clzll((long long)from) : lane;
    const int px = __shfl(p.x, prev), py = __shfl(p.y, prev);
    const uint32_t key = f ? mk.vkey[o + lane] : 0u;      // vkey and flags are kept in rotated order
    if (f) {
      const int64_t to = (int64_t)at + __popcll(below);
      vertices_out[to] = p;
      left_out[to] = (int32_t)(meta[o + src] & ~NODE_BIT);
      edge_out(mk, to, key, r0.x, r, __popcll(below), count);
    }
    const uint32_t area2 = wave_sum32(f ? (uint32_t)(px * p.y - p.x * py) : 0u);   // modular: exact if the total fits i32
    const int x0 = __shfl(p.x, 0), y0 = __shfl(p.y, 0);   // vertex 0 of the rotated ring is always kept
    const bool bad = ring_defective(count, (int)area2, r0.w);
    if (bad && f) level_or(mk.level_words, key, LV_MARK);   // the first vertex of every arc is kept: all its arcs
    if (lane == 0) {
      write_row(rings_out, r, r0, r1, (int)at, count, (int)area2, x0, y0);
      if (count < 3 || area2 == 0) atomicAdd(info + INFO_COLLAPSED, 1);
      if (bad) atomicAdd(mk.round + RH_BAD_RINGS, 1u);
    }
  }
}

__global__ __launch_bounds__(256) void safe_scatter_block_kernel(const int32_t* __restrict__ rings, const int32_t* __restrict__ naug,
                                                                   const uint32_t* __restrict__ off, const uint32_t* __restrict__ rot,
                                                                   const uint32_t* __restrict__ ap, const uint32_t* __restrict__ meta,
                                                                   const int32_t* __restrict__ kept, const uint32_t* __restrict__ startp,
                                                                   const uint8_t* __restrict__ flags, const uint32_t* __restrict__ large,
                                                                   const uint32_t* __restrict__ header, int32_t* __restrict__ rings_out,
                                                                   int2* __restrict__ vertices_out, int32_t* __restrict__ left_out,
                                                                   int32_t* __restrict__ info, Marks mk) {
  if (header[WS_DONE]) return;
  extern __shared__ u64 part[];                            // [4], then the area
  uint32_t& sh_area = *reinterpret_cast<uint32_t*>(part + 4);
  const uint32_t n_large = header[WS_LARGE];
  for (uint32_t li = blockIdx.x; li < n_large; li += gridDim.x) {
    const int r = (int)large[li];
    const int count = kept[r];
    const uint32_t at32 = startp[r];
    if (count < 0 || at32 == NO_ROOM) continue;            // the wave kernel writes this row
    const int4 r0 = reinterpret_cast<const int4*>(rings + (int64_t)r * 8)[0], r1 = reinterpret_cast<const int4*>(rings + (int64_t)r * 8)[1];
    const int n = naug[r], s = (int)rot[r];
    const int64_t o = off[r], at = at32;
    if (threadIdx.x == 0) sh_area = 0;
    u64 run = 0;
    for (int base = 0; base < n; base += 256) {
      const int k = base + (int)threadIdx.x;
      const bool f = k < n && flags[o + k];
      u64 all;
      const u64 pos = run + block_excl_scan64(f ? 1ull : 0ull, part, &all);
      if (f) {
        const int j = k + s, src = j >= n ? j - n : j;
        vertices_out[at + (int64_t)pos] = unpack(ap[o + src]);
        left_out[at + (int64_t)pos] = (int32_t)(meta[o + src] & ~NODE_BIT);
        edge_out(mk, at + (int64_t)pos, mk.vkey[o + k], r0.x, r, (int)pos, count);
      }
      run += all;
      __syncthreads();
    }
    uint32_t acc = 0;
    for (int j = threadIdx.x; j < count; j += 256) {       // the workgroup's own writes, after its barrier
      const int2 c = vertices_out[at + j], q = vertices_out[at + (j ? j - 1 : count - 1)];
      acc += (uint32_t)(q.x * c.y - c.x * q.y);
    }
    acc = wave_sum32(acc);
    if ((threadIdx.x & 63) == 0) atomicAdd(&sh_area, acc);
    __syncthreads();
    const bool bad = ring_defective(count, (int)sh_area, r0.w);
    if (bad)
      for (int j = threadIdx.x; j < count; j += 256) level_or(mk.level_words, mk.e_key[at + j], LV_MARK);
    if (threadIdx.x == 0) {
      const int2 first = vertices_out[at];
      write_row(rings_out, r, r0, r1, (int)at, count, (int)sh_area, first.x, first.y);
      if (count < 3 || sh_area == 0) atomicAdd(info + INFO_COLLAPSED, 1);
      if (bad) atomicAdd(mk.round + RH_BAD_RINGS, 1u);
    }
    __syncthreads();
  }
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
__device__ __forceinline__ u64* quad(uint32_t* round) { return reinterpret_cast<u64*>(round + 16); }
__device__ __forceinline__ const u64* quad(const uint32_t* round) { return reinterpret_cast<const u64*>(round + 16); }
__device__ __forceinline__ uint32_t written_of(const Det& s, const uint32_t* header) {
  return min(header[WS_WRITTEN], (uint32_t)s.max_out);
}
__device__ __forceinline__ bool over_work(const Det& s, const uint32_t* round) { return quad(round)[RQ_WORK] > (u64)s.max_work; }
__device__ __forceinline__ bool live_of(int4 e) { return e.x != e.z || e.y != e.w; }
__device__ __forceinline__ u64 entry_budget(const Det& s, uint32_t n) { return min((u64)BUDGET_E * n, (u64)s.cap_e); }
__device__ __forceinline__ u64 cell_budget(const Det& s, uint32_t n) { return min((u64)BUDGET_C * max(n, 1u), (u64)s.cap_c); }

struct Grid {
  int shift, x0, y0;
  uint32_t cx, cy;
};
__device__ __forceinline__ Grid grid_of(const uint32_t* round) {
  Grid g;
  g.shift = (int)round[RH_SHIFT]; g.x0 = (int)round[RH_X0]; g.y0 = (int)round[RH_Y0];
  g.cx = round[RH_CX]; g.cy = round[RH_CY];
  return g;
}
// the cells that the bounding box of e covers; e lies inside the box of all live edges, so no index leaves the grid
__device__ __forceinline__ void span_of(const Grid& g, int4 e, uint32_t& x0, uint32_t& x1, uint32_t& y0, uint32_t& y1) {
  x0 = (uint32_t)(min(e.x, e.z) - g.x0) >> g.shift; x1 = (uint32_t)(max(e.x, e.z) - g.x0) >> g.shift;
  y0 = (uint32_t)(min(e.y, e.w) - g.y0) >> g.shift; y1 = (uint32_t)(max(e.y, e.w) - g.y0) >> g.shift;
  x1 = min(x1, g.cx - 1u); y1 = min(y1, g.cy - 1u);        // cannot bind: the box was taken over these edges
}

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

// Per candidate shift the entries it would cost.  A sum only has to tell "within the budget" from "above it": an edge adds at
// most budget + 1 and a wave keeps its sum at or below that, so no 64-bit counter overflows.
__global__ __launch_bounds__(256) void safe_cost_kernel(Det s, const uint32_t* __restrict__ header, uint32_t* __restrict__ round) {
  if (header[WS_DONE]) return;
  const uint32_t n = written_of(s, header), live = round[RH_EDGES];
  const int lane = threadIdx.x & 63;
  if ((uint32_t)blockIdx.x * 256u >= n || !live) return;   // the grid is sized by max_vertices_out
  const int x0 = BIAS - (int)round[RH_LO_X], y0 = BIAS - (int)round[RH_LO_Y];
  const u64 top = entry_budget(s, live) + 1ull;
  u64 cost[N_SHIFT];
#pragma unroll
  for (int k = 0; k < N_SHIFT; ++k) cost[k] = 0;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int4 e = s.e_xy[i];
    if (!live_of(e)) continue;
    const uint32_t ax = (uint32_t)(min(e.x, e.z) - x0), bx = (uint32_t)(max(e.x, e.z) - x0);
    const uint32_t ay = (uint32_t)(min(e.y, e.w) - y0), by = (uint32_t)(max(e.y, e.w) - y0);
#pragma unroll
    for (int k = 0; k < N_SHIFT; ++k) {
      const u64 c = (u64)((bx >> k) - (ax >> k) + 1u) * (u64)((by >> k) - (ay >> k) + 1u);
      cost[k] = min(cost[k] + min(c, top), top);
    }
  }
#pragma unroll
  for (int k = 0; k < N_SHIFT; ++k) {
    u64 v = cost[k];
    for (int o = 32; o > 0; o >>= 1) v = min(v + shfl64(v, lane ^ o), top);
    if (lane == 0 && v) atomicAdd(quad(round) + RQ_COST + k, v);
  }
}

// one wave, a lane per candidate: the smallest shift within the entry and the cell budget, both taken per live edge
__global__ __launch_bounds__(64) void safe_choose_kernel(Det s, const uint32_t* __restrict__ header, uint32_t* __restrict__ round) {
  if (header[WS_DONE]) return;
  const int k = threadIdx.x;
  const uint32_t n = round[RH_EDGES];
  int x0 = 0, y0 = 0;
  uint32_t wx = 0, wy = 0;
  if (n) {
    x0 = BIAS - (int)round[RH_LO_X]; y0 = BIAS - (int)round[RH_LO_Y];
    wx = (uint32_t)((int)round[RH_HI_X] - BIAS - x0); wy = (uint32_t)((int)round[RH_HI_Y] - BIAS - y0);
  }
  bool ok = false;
  u64 cells = 0, cost = 0;
  if (k < N_SHIFT) {
    cells = (u64)((wx >> k) + 1u) * (u64)((wy >> k) + 1u);
    cost = quad(round)[RQ_COST + k];
    ok = cost <= entry_budget(s, n) && cells <= cell_budget(s, n);
  }
  const u64 fit = __ballot(ok);
  const int pick = fit ? __ffsll((long long)fit) - 1 : N_SHIFT - 1;   // the last shift always fits: one cell, an entry per edge
  if (k == pick) {
    round[RH_SHIFT] = (uint32_t)pick;
    round[RH_CX] = (wx >> pick) + 1u;
    round[RH_CY] = (wy >> pick) + 1u;
    round[RH_X0] = (uint32_t)x0;
    round[RH_Y0] = (uint32_t)y0;
    quad(round)[RQ_ENTRIES] = min(cost, entry_budget(s, n));
  }
}

__global__ __launch_bounds__(256) void safe_zero_cells_kernel(Det s, const uint32_t* __restrict__ header, const uint32_t* __restrict__ round) {
  if (header[WS_DONE]) return;
  const u64 cells = min((u64)round[RH_CX] * round[RH_CY], (u64)s.cap_c);
  for (u64 c = (u64)blockIdx.x * 256 + threadIdx.x; c < cells; c += (u64)gridDim.x * 256) s.cell_n[c] = 0u;
}

__global__ __launch_bounds__(256) void safe_count_kernel(Det s, const uint32_t* __restrict__ header, const uint32_t* __restrict__ round) {
  if (header[WS_DONE]) return;
  const uint32_t n = written_of(s, header);
  const Grid g = grid_of(round);
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int4 e = s.e_xy[i];
    if (!live_of(e)) continue;
    uint32_t x0, x1, y0, y1;
    span_of(g, e, x0, x1, y0, y1);
    for (uint32_t y = y0; y <= y1; ++y)                    // at most cap_e cells in all: the chosen shift is within the budget
      for (uint32_t x = x0; x <= x1; ++x) atomicAdd(s.cell_n + ((u64)y * g.cx + x), 1u);
  }
}

// a thread per cell: where its entries go, its share of `work`, and the jobs of a cell above CELL_WAVE_LIMIT entries
__global__ __launch_bounds__(256) void safe_starts_kernel(Det s, const uint32_t* __restrict__ header, uint32_t* __restrict__ round) {
  if (header[WS_DONE]) return;
  const Grid g = grid_of(round);
  const u64 cells = min((u64)g.cx * g.cy, (u64)s.cap_c);
  const int lane = threadIdx.x & 63;
  u64 work = 0;
  for (u64 c0 = ((u64)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; c0 < cells; c0 += (u64)gridDim.x * 256) {   // uniform over the wave
    const u64 c = c0 + lane;
    const uint32_t cnt = c < cells ? s.cell_n[c] : 0u;
    uint32_t all;
    const uint32_t before = wave_excl_scan32(cnt, &all);
    uint32_t base = 0;
    if (lane == 0 && all) base = atomicAdd(round + RH_AT, all);
    base = (uint32_t)__shfl((int)base, 0);
    if (c < cells) s.cell_at[c] = base + before;
    work += (u64)cnt * (u64)(cnt ? cnt - 1u : 0u) / 2ull;
    if (cnt > (uint32_t)CELL_WAVE_LIMIT) {
      const uint32_t chunks = (cnt + CHUNK - 1) / CHUNK;
      const uint32_t at = atomicAdd(round + RH_JOBS, chunks);
      for (uint32_t i = 0; i < chunks; ++i)                // at most cap_e / CHUNK + 1 steps
        if ((u64)at + i < (u64)s.cap_j) s.jobs[at + i] = make_uint2((uint32_t)c, i);   // cannot fail: see workspace_plan
    }
  }
  work = wave_sum64(work);
  if (lane == 0 && work) atomicAdd(quad(round) + RQ_WORK, work);
}

__global__ __launch_bounds__(256) void safe_fill_kernel(Det s, const uint32_t* __restrict__ header, const uint32_t* __restrict__ round) {
  if (header[WS_DONE] || over_work(s, round)) return;
  const uint32_t n = written_of(s, header);
  const Grid g = grid_of(round);
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int4 e = s.e_xy[i];
    if (!live_of(e)) continue;
    uint32_t x0, x1, y0, y1;
    span_of(g, e, x0, x1, y0, y1);
    for (uint32_t y = y0; y <= y1; ++y)
      for (uint32_t x = x0; x <= x1; ++x) {
        const uint32_t at = atomicAdd(s.cell_at + ((u64)y * g.cx + x), 1u);
        if ((u64)at < (u64)s.cap_e) s.entry[at] = i;       // cannot fail: the counts are those of the count kernel
      }
  }
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
  const Grid g = grid_of(round);
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
  const Grid g = grid_of(round);
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

unsigned grid_for(int64_t items, int per_block) {
  int64_t g = (items + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > MAX_GRID ? MAX_GRID : g));
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
