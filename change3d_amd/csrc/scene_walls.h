// The shared-wall passes that csrc/scene_shared.hip and csrc/scene_safe.hip both run: the node bitmaps, the augmented ring,
// the three-tier Douglas-Peucker over the arcs between nodes, the scan of the kept counts and the two scatters.  The rule is the
// header's (include/change3d_hip.h); the stages are described at the top of scene_shared.hip.  Both files include this one and
// neither keeps a copy: their __global__ kernels are thin wrappers around the ..._pass bodies below.
//
// The two callers differ by a compile-time policy P and by nothing at run time.  P::LEVELLED = false is the plain call of
// scene_shared.hip, true the rounds of scene_safe.hip, where every arc has a tolerance level of its own.  P decides
//   - whether augment keeps the direction of the edge that leaves every vertex (dirs);
//   - the arc word of a node in ring_dp (P::arc_word, P::arc_closed, P::arc_level) and the level the chord starts read
//     (P::level through P::Levels; the plain call has none and its level is the constant 0);
//   - where the arcs, closed arcs and arcs with a left label are counted: in ring_dp (plain), or by the caller's key pass;
//   - the gate on the done word at the top of every pass that runs once per round (P::done);
//   - whether the kept-scan leaves the written count in the header (P::written);
//   - what the scatters add for every output edge and defective ring (P::Marks, P::key_at, P::edge_out, P::ring_defective,
//     P::mark, P::out_key, P::bad_ring).
// The hooks of a levelled policy are named only under `if constexpr (P::LEVELLED)`: the plain policy does not define them.
#pragma once
#include <climits>

#include "scene_wave.h"
#include "../../include/change3d_hip.h"

namespace c3d_walls {

using namespace c3d_wave;

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

// words of the workspace header that these passes use (the first 256 bytes, zeroed by the call's memset)
enum { WS_ERR = 0, WS_ROWS = 1, WS_FOUND = 2, WS_STATUS = 3, WS_BADCOUNTS = 4, WS_LARGE = 5, WS_INFO = 8 };
enum { INFO_INSERTED = 0, INFO_NODES = 1, INFO_ARCS = 2, INFO_CLOSED = 3, INFO_SHARED = 4, INFO_COLLAPSED = 5 };

// the arrays of these passes, laid out from the first byte behind the caller's header
struct Space {
  int64_t naug, off, rot, kept, startp, large, ap, meta, flags, link, arc, idx, best, rowbits, colbits, end;   // byte offsets
  int WR, WC;                                              // words per row of the two node bitmaps
};
inline int64_t up256(int64_t b) { return (b + 255) & ~(int64_t)255; }
inline Space space_plan(int64_t first, int64_t Hs, int64_t Ws, int64_t max_rings, int64_t max_vertices) {
  Space w;
  const int64_t A = 2 * max_vertices;
  w.naug = first;
  w.off = w.naug + up256(max_rings * 4);
  w.rot = w.off + up256(max_rings * 4);
  w.kept = w.rot + up256(max_rings * 4);
  w.startp = w.kept + up256(max_rings * 4);
  w.large = w.startp + up256(max_rings * 4);
  w.ap = w.large + up256(max_rings * 4);
  w.meta = w.ap + up256(A * 4);
  w.flags = w.meta + up256(A * 4);
  w.link = w.flags + up256(A);
  w.arc = w.link + up256(A * 4);
  w.idx = w.arc + up256(A * 4);
  w.best = w.idx + up256(A * 8);
  w.WR = (int)((Ws + 1 + 31) / 32);
  w.WC = (int)((Hs + 1 + 31) / 32);
  w.rowbits = w.best + up256(A * 8);
  w.colbits = w.rowbits + up256((Hs + 1) * w.WR * 4);
  w.end = w.colbits + up256((Ws + 1) * w.WC * 4);
  return w;
}
inline unsigned grid_for(int64_t items, int per_block) {
  int64_t g = (items + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > MAX_GRID ? MAX_GRID : g));
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
// 256 threads.  COLS = false: line = vy, position = vx; COLS = true: line = vx, position = vy.  A wave owns 64 consecutive
// positions of one line or of two (a line is a whole number of words), and writes its two words whole: padding bits are 0
template <bool COLS>
__device__ __forceinline__ void nodes_pass(const int32_t* __restrict__ labels, const int32_t* __restrict__ counts_obj, int Hs, int Ws,
                                           int max_objects, uint32_t* __restrict__ bits, int words) {
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
// 256 threads
__device__ __forceinline__ void count_pass(const int32_t* __restrict__ labels, const int32_t* __restrict__ counts_obj, int Hs, int Ws,
                                           int max_objects, const int32_t* __restrict__ rings, const int2* __restrict__ vertices,
                                           const int32_t* __restrict__ counts, int max_rings, int max_vertices,
                                           int32_t* __restrict__ naug, const Bits& bits) {
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
// BLOCK_T threads; part: u64 [BLOCK_T / 64] of LDS
__device__ __forceinline__ void scan_rows_pass(const int32_t* __restrict__ counts, int32_t* __restrict__ naug, uint32_t* __restrict__ off,
                                               uint32_t* __restrict__ large, uint32_t* __restrict__ header, int max_rings,
                                               int max_vertices, u64* part) {
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
// 256 threads.  dirs (levelled only): the direction of the edge that leaves every augmented vertex, as the tracer numbers sides
template <class P>
__device__ __forceinline__ void augment_pass(const int32_t* __restrict__ labels, const int32_t* __restrict__ counts_obj, int Hs, int Ws,
                                             int max_objects, const int32_t* __restrict__ rings, const int2* __restrict__ vertices,
                                             const int32_t* __restrict__ naug, const uint32_t* __restrict__ off,
                                             uint32_t* __restrict__ rot, uint32_t* __restrict__ ap, uint32_t* __restrict__ meta,
                                             uint8_t* __restrict__ dirs, uint32_t* __restrict__ header, const Bits& bits) {
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
        const uint8_t dir = (uint8_t)(e.dx > 0 ? 0 : (e.dy > 0 ? 1 : (e.dx < 0 ? 2 : 3)));
        ap[o + pos] = pack(e.p.x, e.p.y);
        meta[o + pos] = lf | (corner_node ? NODE_BIT : 0u);
        if constexpr (P::LEVELLED) dirs[o + pos] = dir;
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
            if constexpr (P::LEVELLED) dirs[o + at] = dir;
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
// that starts at k.  arc[k] >= 0: k is no node, arc[k] = the node its arc starts at; arc[k] < 0: k is a node and arc[k] is
// P::arc_word of the arc that starts at k: whether it is closed and, levelled, its level getL(k).  The tolerance of a levelled
// arc is tol2_q >> 2 level, read from the arc word at every split test.  best / idx are used at chord starts only.  sh: 18 words
// of LDS.  Returns the kept count; flags_out[k] = kept.  Every thread of the workgroup calls it with the same arguments.
template <class P, int T, class GetP, class GetM, class GetL, class H>
__device__ __forceinline__ int ring_dp(GetP getP, GetM getM, GetL getL, int* link, int* arc, u64* idx, u64* best,
                                       uint8_t* __restrict__ flags_out, int n, u64 tol2_q, int* sh, H* __restrict__ header) {
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
          arc[e] = P::arc_word(closed, getL(e));
          if constexpr (!P::LEVELLED)
            if (closed) atomicAdd(header + WS_INFO + INFO_CLOSED, 1u);
        }
        if constexpr (!P::LEVELLED) {
          atomicAdd(header + WS_INFO + INFO_ARCS, 1u);
          if (m & ~NODE_BIT) atomicAdd(header + WS_INFO + INFO_SHARED, 1u);
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
    arc[last] = P::arc_word(closed, getL(last));
    if constexpr (!P::LEVELLED)
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
      u64 tol = tol2_q;
      if constexpr (P::LEVELLED) {                         // the arc's own tolerance: two LDS reads more
        const int aw = arc[lo];
        tol = tol2_q >> (2 * P::arc_level(aw < 0 ? aw : arc[aw]));
      }
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
    if (a < 0 || link[k] >= -1 || !P::arc_closed(arc[a])) continue;
    atomicAdd(idx + a, 1ull);
    best[a] = (u64)k;
  }
  __syncthreads();
  for (int pass = 0; pass < 2; ++pass) {
    for (int k = tid; k < n; k += T) {
      const int a = arc[k];
      if (a < 0 || link[k] != -1 || !P::arc_closed(arc[a]) || idx[a] != 1ull) continue;
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

// T = 64: the rings of up to WAVE_LIMIT augmented vertices, a wave each; T = BLOCK_T: the listed larger ones.
// lds: best, idx u64 [LIMIT]; link, arc, packed positions u32 [LIMIT]; 18 words
template <class P, int T, int LIMIT, class H>
__device__ __forceinline__ void dp_pass(const int32_t* __restrict__ naug, const uint32_t* __restrict__ off, const uint32_t* __restrict__ rot,
                                        const uint32_t* __restrict__ ap, const uint32_t* __restrict__ meta, int32_t* __restrict__ kept,
                                        uint8_t* __restrict__ flags, int32_t* __restrict__ g_link, int32_t* __restrict__ g_arc,
                                        u64* __restrict__ g_idx, u64* __restrict__ g_best, const uint32_t* __restrict__ large,
                                        H* __restrict__ header, const typename P::Levels& lv, u64 tol2_q, u64* lds) {
  if (P::done(header)) return;
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
    auto getL = [&](int k) { return P::level(lv, o + k); };   // of the arc that starts at vertex k of the rotated ring
    int count;
    if (in_lds) {
      count = ring_dp<P, T>([&](int k) { return unpack(s_p[k]); }, getM, getL, s_link, s_arc, s_idx, s_best, flags + o, n, tol2_q, sh,
                            header);
    } else {
      count = ring_dp<P, T>([&](int k) { return unpack(ap[where(k)]); }, getM, getL, g_link + o, g_arc + o, g_idx + o, g_best + o,
                            flags + o, n, tol2_q, sh, header);
    }
    if (threadIdx.x == 0) kept[r] = count;
  }
}

// ------------------------------------------------------------------------------------------------ 5: one workgroup in all
// start'[r] = kept vertices of the rows before r, or NO_ROOM past max_vertices_out; counts_out; info but for its collapsed rings.
// BLOCK_T threads; part: u64 [BLOCK_T / 64] of LDS, then one word for the first start without room
template <class P, class H>
__device__ __forceinline__ void scan_kept_pass(const int32_t* __restrict__ kept, uint32_t* __restrict__ startp, H* __restrict__ header,
                                               int32_t* __restrict__ counts_out, int32_t* __restrict__ info, int max_vertices_out,
                                               u64* part) {
  if (P::done(header)) return;
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
      P::written(header, 0u);
    } else {
      const u64 written = *sh_cut == ~0ull ? running : *sh_cut;
      counts_out[0] = (int32_t)header[WS_FOUND];
      counts_out[1] = rows;
      counts_out[2] = (int32_t)(running > (u64)INT_MAX ? (u64)INT_MAX : running);
      counts_out[3] = (int32_t)written;
      P::written(header, (uint32_t)written);
      counts_out[4] = (int32_t)(header[WS_STATUS] | (header[WS_ERR] ? (uint32_t)C3D_SIMPLIFY_ST_BAD_INPUT : 0u) |
                                (written < running ? (uint32_t)C3D_OUTLINE_ST_TRUNCATED : 0u));
      for (int j = 0; j < 5; ++j) info[j] = (int32_t)header[WS_INFO + j];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ 6: scatter
__device__ __forceinline__ void write_row(int32_t* __restrict__ rings_out, int r, const int4 r0, const int4 r1, int start, int n,
                                          int area2, int x, int y) {
  int4* dst = reinterpret_cast<int4*>(rings_out + (int64_t)r * 8);
  dst[0] = make_int4(r0.x, start, n, area2);
  dst[1] = make_int4(r1.x, x, y, r0.z);
}

// rows of rings of up to WAVE_LIMIT augmented vertices, rows that are not simplified, and the zero rows past the table.
// 256 threads, a wave per row
template <class P>
__device__ __forceinline__ void scatter_wave_pass(const int32_t* __restrict__ rings, const int32_t* __restrict__ naug,
                                                  const uint32_t* __restrict__ off, const uint32_t* __restrict__ rot,
                                                  const uint32_t* __restrict__ ap, const uint32_t* __restrict__ meta,
                                                  const int32_t* __restrict__ kept, const uint32_t* __restrict__ startp,
                                                  const uint8_t* __restrict__ flags, const uint32_t* __restrict__ header,
                                                  int32_t* __restrict__ rings_out, int2* __restrict__ vertices_out,
                                                  int32_t* __restrict__ left_out, int32_t* __restrict__ info, int max_rings,
                                                  const typename P::Marks& mk) {
  if (P::done(header)) return;
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
    uint32_t key = 0u;
    if constexpr (P::LEVELLED) key = f ? P::key_at(mk, o + lane) : 0u;   // the keys and flags are kept in rotated order
    if (f) {
      const int64_t to = (int64_t)at + __popcll(below);
      vertices_out[to] = p;
      left_out[to] = (int32_t)(meta[o + src] & ~NODE_BIT);
      if constexpr (P::LEVELLED) P::edge_out(mk, to, key, r0.x, r, __popcll(below), count);
    }
    const uint32_t area2 = wave_sum32(f ? (uint32_t)(px * p.y - p.x * py) : 0u);   // modular: exact if the total fits i32
    const int x0 = __shfl(p.x, 0), y0 = __shfl(p.y, 0);   // vertex 0 of the rotated ring is always kept
    bool bad = false;
    if constexpr (P::LEVELLED) {
      bad = P::ring_defective(count, (int)area2, r0.w);
      if (bad && f) P::mark(mk, key);                      // the first vertex of every arc is kept: all its arcs
    }
    if (lane == 0) {
      write_row(rings_out, r, r0, r1, (int)at, count, (int)area2, x0, y0);
      if (count < 3 || area2 == 0) atomicAdd(info + INFO_COLLAPSED, 1);
      if constexpr (P::LEVELLED)
        if (bad) P::bad_ring(mk);
    }
  }
}

// the listed larger rings, a workgroup of 256 each.  part: u64 [4] of LDS, then one word for the area
template <class P>
__device__ __forceinline__ void scatter_block_pass(const int32_t* __restrict__ rings, const int32_t* __restrict__ naug,
                                                   const uint32_t* __restrict__ off, const uint32_t* __restrict__ rot,
                                                   const uint32_t* __restrict__ ap, const uint32_t* __restrict__ meta,
                                                   const int32_t* __restrict__ kept, const uint32_t* __restrict__ startp,
                                                   const uint8_t* __restrict__ flags, const uint32_t* __restrict__ large,
                                                   const uint32_t* __restrict__ header, int32_t* __restrict__ rings_out,
                                                   int2* __restrict__ vertices_out, int32_t* __restrict__ left_out,
                                                   int32_t* __restrict__ info, const typename P::Marks& mk, u64* part) {
  if (P::done(header)) return;
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
        if constexpr (P::LEVELLED) P::edge_out(mk, at + (int64_t)pos, P::key_at(mk, o + k), r0.x, r, (int)pos, count);
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
    bool bad = false;
    if constexpr (P::LEVELLED) {
      bad = P::ring_defective(count, (int)sh_area, r0.w);
      if (bad)
        for (int j = threadIdx.x; j < count; j += 256) P::mark(mk, P::out_key(mk, at + j));
    }
    if (threadIdx.x == 0) {
      const int2 first = vertices_out[at];
      write_row(rings_out, r, r0, r1, (int)at, count, (int)sh_area, first.x, first.y);
      if (count < 3 || sh_area == 0) atomicAdd(info + INFO_COLLAPSED, 1);
      if constexpr (P::LEVELLED)
        if (bad) P::bad_ring(mk);
    }
    __syncthreads();
  }
}

}  // namespace c3d_walls
