// Shared-wall simplification of a scene's traced rings: every boundary is cut at the lattice points where three or more regions
// meet (the nodes, read from the label map), and every arc between two nodes is simplified once by a Douglas-Peucker whose
// result does not depend on the direction of travel, so that both neighbours of a wall get the same chords.  The rule -- the
// four labels of a node, the augmented ring, its start, the tie to the smallest (vy, vx), the guard of a closed arc -- is the
// header's (include/change3d_hip.h); this file is one way to compute it.  Integer arithmetic and integer atomics only.
//
//   0 nodes       two launches over the lattice points: a bitmap of the nodes by rows (a bit per vx) and one by columns (a bit per
//                 vy), written whole words at a time from a wave's ballot.  An edge then finds the nodes inside it by popcount
//                 over a bit range instead of walking its lattice points with four label reads each: one wave owns a ring, and
//                 on the serpentine (2050 edges, half of them 1024 long) the walk took 31 ms beside 2 ms of simplification
//   1 count       one wave per ring row, a lane per stored edge: validates the edge and counts the nodes strictly inside it;
//                 naug[r] = the ring's augmented vertex count, or why the row is not simplified
//   2 scan_rows   one workgroup: off[r] = where ring r keeps its augmented vertices and per-vertex state in the workspace; lists
//                 the rings above WAVE_LIMIT for the workgroup tiers
//   3 augment     one wave per ring: reads the edges' bits again and writes the augmented vertices (packed position; left label and
//                 node flag) in stored order, and the ring's start = its first node, or its smallest (vy, vx) without one.  The
//                 later stages read position k of the rotated ring at (k + start) mod n
//   4 dp          whoever owns a ring loops until no chord of it splits: one wave (a workgroup of 64) with the state in LDS up to
//                 WAVE_LIMIT augmented vertices, one workgroup of 1024 with the state in LDS up to LDS_LIMIT, in the workspace
//                 beyond: the same loop body for all three.  The chord starts of round 0 are the nodes, found by an exclusive
//                 max-scan over the node flags.  A round is the four passes of scene_simplify.hip (max, arg, split, link); arg
//                 takes the minimum of (vy * 16385 + vx) << 32 | k among the vertices at the maximum, which is unique inside an
//                 arc and carries the index with it.  Then the guard of the closed arcs
//   5 scan_kept   one workgroup: start' = exclusive scan of the kept counts, cut prefix-shaped at max_vertices_out; counts, info
//   6 scatter     wave and block variants: ordered compaction into vertices_out and left_out, the shoelace sum, the ring row
// No workgroup waits for another, nothing is read back, every loop is capped by a count that was checked against the workspace.
#include <climits>

#include "common.h"
#include "../../include/change3d_hip.h"

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

// words of the workspace header (256 bytes), zeroed by the memset
enum { WS_ERR = 0, WS_ROWS = 1, WS_FOUND = 2, WS_STATUS = 3, WS_BADCOUNTS = 4, WS_LARGE = 5, WS_INFO = 8 };
enum { INFO_INSERTED = 0, INFO_NODES = 1, INFO_ARCS = 2, INFO_CLOSED = 3, INFO_SHARED = 4, INFO_COLLAPSED = 5 };

struct Workspace {
  int64_t naug, off, rot, kept, startp, large, ap, meta, flags, link, arc, idx, best, rowbits, colbits, bytes;   // byte offsets
  int WR, WC;                                              // words per row of the two node bitmaps
};

Workspace workspace_plan(int64_t Hs, int64_t Ws, int64_t max_rings, int64_t max_vertices) {
  Workspace w;
  auto up = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  const int64_t A = 2 * max_vertices;
  w.naug = 256;
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
  w.bytes = w.colbits + up((Ws + 1) * w.WC * 4);
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
__global__ __launch_bounds__(256) void shared_nodes_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ counts_obj,
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
__global__ __launch_bounds__(256) void shared_count_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ counts_obj,
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
__global__ __launch_bounds__(BLOCK_T) void shared_scan_rows_kernel(const int32_t* __restrict__ counts, int32_t* __restrict__ naug,
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
__global__ __launch_bounds__(256) void shared_augment_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ counts_obj,
                                                             int Hs, int Ws, int max_objects, const int32_t* __restrict__ rings,
                                                             const int2* __restrict__ vertices, const int32_t* __restrict__ naug,
                                                             const uint32_t* __restrict__ off, uint32_t* __restrict__ rot,
                                                             uint32_t* __restrict__ ap, uint32_t* __restrict__ meta,
                                                             uint32_t* __restrict__ header, Bits bits) {
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
        ap[o + pos] = pack(e.p.x, e.p.y);
        meta[o + pos] = lf | (corner_node ? NODE_BIT : 0u);
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
// whether the arc that starts at k is closed.  best / idx are used at chord starts only.  sh: 18 words of LDS.  Returns the kept
// count; flags_out[k] = kept.  Every thread of the workgroup calls it with the same arguments.
template <int T, class GetP, class GetM>
__device__ __forceinline__ int ring_dp(GetP getP, GetM getM, int* link, int* arc, u64* idx, u64* best, uint8_t* __restrict__ flags_out,
                                       int n, u64 tol2_q, int* sh, uint32_t* __restrict__ header) {
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
          arc[e] = ~(closed ? 1 : 0);
          if (closed) atomicAdd(header + WS_INFO + INFO_CLOSED, 1u);
        }
        atomicAdd(header + WS_INFO + INFO_ARCS, 1u);
        if (m & ~NODE_BIT) atomicAdd(header + WS_INFO + INFO_SHARED, 1u);
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
    arc[last] = ~(closed ? 1 : 0);
    if (closed) atomicAdd(header + WS_INFO + INFO_CLOSED, 1u);
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
      if (L2 != 0 && !(16ull * best[lo] > tol2_q * L2)) { link[k] = -1; continue; }   // a chord whose ends coincide always splits
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
    if (a < 0 || link[k] >= -1 || arc[a] != ~1) continue;
    atomicAdd(idx + a, 1ull);
    best[a] = (u64)k;
  }
  __syncthreads();
  for (int pass = 0; pass < 2; ++pass) {
    for (int k = tid; k < n; k += T) {
      const int a = arc[k];
      if (a < 0 || link[k] != -1 || arc[a] != ~1 || idx[a] != 1ull) continue;
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

// T = 64: the rings of up to WAVE_LIMIT augmented vertices, a wave each; T = BLOCK_T: the listed larger ones
template <int T, int LIMIT>
__global__ __launch_bounds__(T) void shared_dp_kernel(const int32_t* __restrict__ naug, const uint32_t* __restrict__ off,
                                                      const uint32_t* __restrict__ rot, const uint32_t* __restrict__ ap,
                                                      const uint32_t* __restrict__ meta, int32_t* __restrict__ kept,
                                                      uint8_t* __restrict__ flags, int32_t* __restrict__ g_link,
                                                      int32_t* __restrict__ g_arc, u64* __restrict__ g_idx, u64* __restrict__ g_best,
                                                      const uint32_t* __restrict__ large, uint32_t* __restrict__ header, u64 tol2_q) {
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
    int count;
    if (in_lds) {
      count = ring_dp<T>([&](int k) { return unpack(s_p[k]); }, getM, s_link, s_arc, s_idx, s_best, flags + o, n, tol2_q, sh, header);
    } else {
      count = ring_dp<T>([&](int k) { return unpack(ap[where(k)]); }, getM, g_link + o, g_arc + o, g_idx + o, g_best + o, flags + o, n,
                         tol2_q, sh, header);
    }
    if (threadIdx.x == 0) kept[r] = count;
  }
}

// start'[r] = kept vertices of the rows before r, or NO_ROOM past max_vertices_out; counts_out; info but for its collapsed rings
__global__ __launch_bounds__(BLOCK_T) void shared_scan_kept_kernel(const int32_t* __restrict__ kept, uint32_t* __restrict__ startp,
                                                               const uint32_t* __restrict__ header, int32_t* __restrict__ counts_out,
                                                               int32_t* __restrict__ info, int max_vertices_out) {
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
    } else {
      const u64 written = *sh_cut == ~0ull ? running : *sh_cut;
      counts_out[0] = (int32_t)header[WS_FOUND];
      counts_out[1] = rows;
      counts_out[2] = (int32_t)(running > (u64)INT_MAX ? (u64)INT_MAX : running);
      counts_out[3] = (int32_t)written;
      counts_out[4] = (int32_t)(header[WS_STATUS] | (header[WS_ERR] ? (uint32_t)C3D_SIMPLIFY_ST_BAD_INPUT : 0u) |
                                (written < running ? (uint32_t)C3D_OUTLINE_ST_TRUNCATED : 0u));
      for (int j = 0; j < 5; ++j) info[j] = (int32_t)header[WS_INFO + j];
    }
  }
}

__device__ __forceinline__ void write_row(int32_t* __restrict__ rings_out, int r, const int4 r0, const int4 r1, int start, int n,
                                          int area2, int x, int y) {
  int4* dst = reinterpret_cast<int4*>(rings_out + (int64_t)r * 8);
  dst[0] = make_int4(r0.x, start, n, area2);
  dst[1] = make_int4(r1.x, x, y, r0.z);
}

// rows of rings of up to WAVE_LIMIT augmented vertices, rows that are not simplified, and the zero rows past the table
__global__ __launch_bounds__(256) void shared_scatter_wave_kernel(const int32_t* __restrict__ rings, const int32_t* __restrict__ naug,
                                                                  const uint32_t* __restrict__ off, const uint32_t* __restrict__ rot,
                                                                  const uint32_t* __restrict__ ap, const uint32_t* __restrict__ meta,
                                                                  const int32_t* __restrict__ kept, const uint32_t* __restrict__ startp,
                                                                  const uint8_t* __restrict__ flags, const uint32_t* __restrict__ header,
                                                                  int32_t* __restrict__ rings_out, int2* __restrict__ vertices_out,
                                                                  int32_t* __restrict__ left_out, int32_t* __restrict__ info,
                                                                  int max_rings) {
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
    if (f) {
      vertices_out[(int64_t)at + __popcll(below)] = p;
      left_out[(int64_t)at + __popcll(below)] = (int32_t)(meta[o + src] & ~NODE_BIT);
    }
    const uint32_t area2 = wave_sum32(f ? (uint32_t)(px * p.y - p.x * py) : 0u);   // modular: exact if the total fits i32
    const int x0 = __shfl(p.x, 0), y0 = __shfl(p.y, 0);   // vertex 0 of the rotated ring is always kept
    if (lane == 0) {
      write_row(rings_out, r, r0, r1, (int)at, count, (int)area2, x0, y0);
      if (count < 3 || area2 == 0) atomicAdd(info + INFO_COLLAPSED, 1);
    }
  }
}

__global__ __launch_bounds__(256) void shared_scatter_block_kernel(const int32_t* __restrict__ rings, const int32_t* __restrict__ naug,
                                                                   const uint32_t* __restrict__ off, const uint32_t* __restrict__ rot,
                                                                   const uint32_t* __restrict__ ap, const uint32_t* __restrict__ meta,
                                                                   const int32_t* __restrict__ kept, const uint32_t* __restrict__ startp,
                                                                   const uint8_t* __restrict__ flags, const uint32_t* __restrict__ large,
                                                                   const uint32_t* __restrict__ header, int32_t* __restrict__ rings_out,
                                                                   int2* __restrict__ vertices_out, int32_t* __restrict__ left_out,
                                                                   int32_t* __restrict__ info) {
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
    if (threadIdx.x == 0) {
      const int2 first = vertices_out[at];
      write_row(rings_out, r, r0, r1, (int)at, count, (int)sh_area, first.x, first.y);
      if (count < 3 || sh_area == 0) atomicAdd(info + INFO_COLLAPSED, 1);
    }
    __syncthreads();
  }
}

unsigned grid_for(int64_t items, int per_block) {
  int64_t g = (items + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > MAX_GRID ? MAX_GRID : g));
}

}  // namespace

extern "C" void c3d_outlines_simplify_shared_limits(int32_t out[2]) {
  if (!out) return;
  out[0] = WAVE_LIMIT;
  out[1] = LDS_LIMIT;
}

extern "C" int64_t c3d_outlines_simplify_shared_ws_bytes(int32_t Hs, int32_t Ws, int32_t max_rings, int32_t max_vertices) {
  if (Hs < 1 || Ws < 1 || max_rings < 1 || max_vertices < 1 || max_vertices > (1 << 30)) return C3D_E_BADARG;
  if (Hs > COORD_MAX || Ws > COORD_MAX) return C3D_E_UNSUPPORTED;
  return workspace_plan(Hs, Ws, max_rings, max_vertices).bytes;
}

extern "C" int c3d_outlines_simplify_shared(const int32_t* labels, const int32_t* counts_obj, int32_t Hs, int32_t Ws, int32_t max_objects,
                                            const int32_t* rings, const int32_t* vertices, const int32_t* counts, int32_t max_rings,
                                            int32_t max_vertices, int64_t tol2_q, int32_t max_vertices_out, int32_t* rings_out,
                                            int32_t* vertices_out, int32_t* left_out, int32_t* counts_out, int32_t* info, void* ws,
                                            void* stream) {
  if (!labels || !counts_obj || !rings || !vertices || !counts || !rings_out || !vertices_out || !left_out || !counts_out || !info || !ws)
    return C3D_E_BADARG;
  if (Hs < 1 || Ws < 1 || max_objects < 1 || max_objects >= (1 << 30) || max_rings < 1 || max_vertices < 1 || max_vertices > (1 << 30) ||
      max_vertices_out < 1 || tol2_q < 0 || tol2_q > C3D_SIMPLIFY_TOL2_Q_MAX)
    return C3D_E_BADARG;
  if (Hs > COORD_MAX || Ws > COORD_MAX) return C3D_E_UNSUPPORTED;
  const Workspace w = workspace_plan(Hs, Ws, max_rings, max_vertices);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  uint32_t* header = reinterpret_cast<uint32_t*>(base);
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
  const Bits bits{rowbits, colbits, w.WR, w.WC};
  const int2* v_in = reinterpret_cast<const int2*>(vertices);
  int2* v_out = reinterpret_cast<int2*>(vertices_out);

  // only the header: every other word of the workspace is written by the call before the call reads it
  hipError_t e = hipMemsetAsync(base, 0, 256, st);
  if (e != hipSuccess) return (int)e;
  // the ring count is known on the device only: grids are sized by max_rings and surplus waves and workgroups return
  const unsigned g_wave = grid_for(max_rings, 4), g_block = grid_for(max_rings, 1);
  int rc = c3d_launch_lds<shared_nodes_kernel<false>>(dim3(grid_for((int64_t)(Hs + 1) * w.WR * 32, 256)), dim3(256), 0, st, labels, counts_obj,
                                                      (int)Hs, (int)Ws, (int)max_objects, rowbits, w.WR);
  if (rc) return rc;
  rc = c3d_launch_lds<shared_nodes_kernel<true>>(dim3(grid_for((int64_t)(Ws + 1) * w.WC * 32, 256)), dim3(256), 0, st, labels, counts_obj,
                                                 (int)Hs, (int)Ws, (int)max_objects, colbits, w.WC);
  if (rc) return rc;
  rc = c3d_launch_lds<shared_count_kernel>(dim3(g_wave), dim3(256), 0, st, labels, counts_obj, (int)Hs, (int)Ws, (int)max_objects, rings,
                                           v_in, counts, (int)max_rings, (int)max_vertices, naug, bits);
  if (rc) return rc;
  rc = c3d_launch_lds<shared_scan_rows_kernel>(dim3(1), dim3(BLOCK_T), BLOCK_T / 8, st, counts, naug, off, large, header, (int)max_rings,
                                               (int)max_vertices);
  if (rc) return rc;
  rc = c3d_launch_lds<shared_augment_kernel>(dim3(g_wave), dim3(256), 0, st, labels, counts_obj, (int)Hs, (int)Ws, (int)max_objects, rings,
                                             v_in, (const int32_t*)naug, (const uint32_t*)off, rot, ap, meta, header, bits);
  if (rc) return rc;
  rc = c3d_launch_lds<shared_dp_kernel<64, WAVE_LIMIT>>(dim3(g_block), dim3(64), WAVE_LDS_BYTES, st, (const int32_t*)naug,
                                                        (const uint32_t*)off, (const uint32_t*)rot, (const uint32_t*)ap,
                                                        (const uint32_t*)meta, kept, flags, link, arc, idx, best,
                                                        (const uint32_t*)large, header, (u64)tol2_q);
  if (rc) return rc;
  rc = c3d_launch_lds<shared_dp_kernel<BLOCK_T, LDS_LIMIT>>(dim3(g_block), dim3(BLOCK_T), LDS_BYTES, st, (const int32_t*)naug,
                                                            (const uint32_t*)off, (const uint32_t*)rot, (const uint32_t*)ap,
                                                            (const uint32_t*)meta, kept, flags, link, arc, idx, best,
                                                            (const uint32_t*)large, header, (u64)tol2_q);
  if (rc) return rc;
  rc = c3d_launch_lds<shared_scan_kept_kernel>(dim3(1), dim3(BLOCK_T), BLOCK_T / 8 + 8, st, (const int32_t*)kept, startp,
                                               (const uint32_t*)header, counts_out, info, (int)max_vertices_out);
  if (rc) return rc;
  rc = c3d_launch_lds<shared_scatter_wave_kernel>(dim3(g_wave), dim3(256), 0, st, rings, (const int32_t*)naug, (const uint32_t*)off,
                                                  (const uint32_t*)rot, (const uint32_t*)ap, (const uint32_t*)meta, (const int32_t*)kept,
                                                  (const uint32_t*)startp, (const uint8_t*)flags, (const uint32_t*)header, rings_out,
                                                  v_out, left_out, info, (int)max_rings);
  if (rc) return rc;
  return c3d_launch_lds<shared_scatter_block_kernel>(dim3(g_block), dim3(256), 40, st, rings, (const int32_t*)naug, (const uint32_t*)off,
                                                     (const uint32_t*)rot, (const uint32_t*)ap, (const uint32_t*)meta,
                                                     (const int32_t*)kept, (const uint32_t*)startp, (const uint8_t*)flags,
                                                     (const uint32_t*)large, (const uint32_t*)header, rings_out, v_out, left_out, info);
}
