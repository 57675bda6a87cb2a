// Polygon rings back to pixels: the ring table and vertex list of c3d_scene_outlines / c3d_outlines_simplify (or any table of
// that shape, with coordinates in units of 2^-f pixel) filled into a label map and an object table.  The rule -- centre
// sampling, half-open rows, the strict left test, even-odd per id, the largest id wins -- is the header's
// (include/change3d_hip.h); this file is one way to compute it.  Integer arithmetic and integer atomics decide everything; the
// one float division below only proposes a column, which the integer predicate then confirms or moves.
//
// Edge-flag fill: every (edge, active row) toggles the first column whose centre lies right of the edge, a prefix XOR along
// the row fills.  No workgroup waits for another, nothing is read back.
//
//   1 init      per-id state in the workspace (box, ring count, cursor) and the table rows
//   2 group     validates the ring rows (a lane per small ring, the wave together on a larger one), takes the pixel box of
//               each id (atomicMin / atomicMax, clipped to the scene) and the rows of each ring, counts the rings of every
//               id, K = the largest used id; one atomic per wave and word where its rows share the id
//   3 scan      one workgroup: off[id] = exclusive scan of the ring counts
//   4 scatter   ring indices grouped by id.  The slot inside a group is claimed by an atomic, so the order varies from run to
//               run; XOR commutes, the result does not
//   5 wave      boxes of up to 64 x 64: one wave per id, lane = row, one u64 per lane = the 64 columns.  Vertices are loaded
//               64 at a time and broadcast; every lane toggles its own bit (no atomics); six shift-XOR steps fill.  It also
//               lists the larger ids for 6
//   6 block     larger boxes: one workgroup per (id, band of 64 rows).  The band's bits live in LDS as u64 [64][ceil(w / 64)]
//               by the box's width w; rings whose rows miss the band are skipped by the row range that 2 left, small rings
//               take a lane each and larger ones a wave, atomicXor on the LDS word; then a wave per row fills inside the
//               words and carries the parity across them; then a wave per word paints
//   5/6 paint   atomicMax of the id into `labels` (zeroed by the call's memset): the only interaction between ids, order-free
//   7 table     one pass over `labels`: area, box, first by integer atomics, kept in registers while a wave's steps share the
//               id; mask and cls_map on the way
//   8 finish    rows without a pixel, cls, the rows past K, counts_obj, info
#include <climits>

#include "scene_groups.h"
#include "scene_host.h"

namespace {

using namespace c3d_groups;                                // the group, scan and scatter passes (steps 2-4)
using c3d_host::grid_for;

typedef unsigned long long u64;

constexpr int BOX_LIMIT = 64;                              // rows and columns of a box that one wave fills in registers
constexpr int BAND_ROWS = 64;                              // rows of a band of the workgroup tier
constexpr int EXTENT_MAX = 16384;                          // scene rows / columns
constexpr int COORD_UNITS = 32768;                         // |coordinate| <= COORD_UNITS << frac_bits
constexpr int FRAC_MAX = 8;
constexpr int BLOCK_T = 512;                               // threads of a band's workgroup
constexpr int TABLE_STEPS = 16;                            // steps of 64 pixels that a wave of the table pass walks
constexpr int MAX_GRID = 8192;
constexpr int LIST_GRID = 128;                             // workgroups that share the list of large ids, per band

// words of the workspace header (256 bytes, zeroed by the call's memset)
enum { WS_STATUS = 0, WS_USED = 1, WS_K = 2, WS_LARGE = 3 };

struct Plan {
  Groups g;
  int4* box;                                               // [max_objects] the pixels the id's rings can reach
  uint32_t* large;                                         // [max_objects] the ids whose box exceeds BOX_LIMIT, in any order
  int2* yrange;                                            // [max_rings] the rows a ring can toggle a bit on
  int64_t bytes;
};

// ws: the workspace, or nullptr where only the sizes are asked for
Plan plan_of(void* ws, int64_t max_rings, int64_t max_vertices, int64_t max_objects) {
  Plan pl{};
  c3d_host::Layout l{static_cast<char*>(ws), 256};
  l.take(pl.box, max_objects * 16);
  l.take(pl.g.cnt, max_objects * 4);
  l.take(pl.g.off, max_objects * 4);
  l.take(pl.g.cursor, max_objects * 4);
  l.take(pl.large, max_objects * 4);
  l.take(pl.g.grouped, max_rings * 4);
  l.take(pl.yrange, max_rings * 8);
  l.take(pl.g.valid, max_rings);
  pl.bytes = l.at;
  pl.g.max_rings = (int)max_rings; pl.g.max_vertices = (int)max_vertices; pl.g.max_objects = (int)max_objects;
  if (ws) pl.g.top = static_cast<uint32_t*>(ws) + WS_K;
  return pl;
}

// The smallest column x in [lo, hi] whose centre lies right of the edge on this row, hi + 1 if none does.  The predicate is
// P(x): (2x + 1) * sdy > A with sdy = 2^f * (Y1 - Y0) > 0 and A = X0 * dy + dx * (Cy - Y0); it is false below the answer and
// true from it on.  |A| < 2^51 and (2x + 1) * sdy < 2^15 * 2^34, so every product fits i64.  The float quotient is an
// estimate: the answer is whatever the integer predicate confirms, by a few steps from the estimate or, should the estimate
// ever be further off, by bisection.
__device__ __forceinline__ int toggle_column(int64_t A, int64_t sdy, int lo, int hi) {
  auto P = [&](int x) { return (int64_t)(2 * x + 1) * sdy > A; };
  if (P(lo)) return lo;
  if (!P(hi)) return hi + 1;
  // lo < answer <= hi: the quotient is a column of the scene, where a float quotient is off by far less than one
  int c = (int)floorf(((float)A + (float)sdy) / (2.0f * (float)sdy));
  c = clampi(c, lo + 1, hi);
  for (int k = 0; k < 2 && !P(c) && c < hi; ++k) ++c;
  for (int k = 0; k < 2 && c - 1 > lo && P(c - 1); ++k) --c;
  if (P(c) && !P(c - 1)) return c;
  int a = lo, b = hi;                                      // P(a) false, P(b) true
  for (int k = 0; k < 16 && b - a > 1; ++k) {
    const int m = a + ((b - a) >> 1);
    if (P(m)) b = m; else a = m;
  }
  return b;
}

// an edge in doubled coordinates, ordered so that Y0 < Y1; dy == 0 for a horizontal one
struct Edge {
  int X0, Y0, dx, dy;
};
__device__ __forceinline__ Edge make_edge(int2 a, int2 b) {
  if (a.y > b.y) { const int2 t = a; a = b; b = t; }
  Edge e;
  e.X0 = 2 * a.x;
  e.Y0 = 2 * a.y;
  e.dx = 2 * (b.x - a.x);
  e.dy = 2 * (b.y - a.y);
  return e;
}
// rows y with Y0 <= (2y + 1) s < Y1: the first and the last (>> floors, also below zero)
__device__ __forceinline__ int first_row(int Y0, int f) { return (Y0 + (1 << f) - 1) >> (f + 1); }
__device__ __forceinline__ int last_row(int Y1, int f) { return (Y1 - 1 - (1 << f)) >> (f + 1); }
__device__ __forceinline__ int edge_column(const Edge& e, int y, int f, int lo, int hi) {
  const int Cy = (2 * y + 1) << f;
  const int64_t A = (int64_t)e.X0 * e.dy + (int64_t)e.dx * (Cy - e.Y0);
  return toggle_column(A, (int64_t)e.dy << f, lo, hi);
}

__global__ __launch_bounds__(256) void fill_init_kernel(int4* __restrict__ box, uint32_t* __restrict__ cnt, uint32_t* __restrict__ cursor,
                                                        int32_t* __restrict__ table, int max_objects) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < max_objects; i += gridDim.x * 256) {
    box[i] = make_int4(INT_MAX, INT_MAX, INT_MIN, INT_MIN);
    cnt[i] = 0;
    cursor[i] = 0;
    int4* row = reinterpret_cast<int4*>(table + (int64_t)i * 8);
    row[0] = make_int4(0, INT_MAX, INT_MAX, INT_MIN);      // area, x0, y0, x1
    row[1] = make_int4(INT_MIN, 0, INT_MAX, 0);            // y1, cls, first, score_q
  }
}

// the box of the pixels whose centre can lie inside a ring with these coordinate extremes, clipped to the scene: Xmin < Cx <=
// Xmax and Ymin <= Cy < Ymax in doubled coordinates.  False: none (a ring wholly left or right of the scene changes no parity)
__device__ __forceinline__ bool pixel_box(int xmin, int ymin, int xmax, int ymax, int f, int Hs, int Ws, int4* out) {
  const int s = 1 << f;
  const int x0 = clampi((2 * xmin + s) >> (f + 1), 0, Ws), x1 = clampi((2 * xmax - s) >> (f + 1), -1, Ws - 1);
  const int y0 = clampi(first_row(2 * ymin, f), 0, Hs), y1 = clampi(last_row(2 * ymax, f), -1, Hs - 1);
  *out = make_int4(x0, y0, x1, y1);
  return x0 <= x1 && y0 <= y1;
}
// the four columns of a box only ever move one way, so a value read earlier that already beats ours still does
__device__ __forceinline__ void box_atomics(int* b, int4 v) {
  if (v.x < b[0]) atomicMin(b + 0, v.x);
  if (v.y < b[1]) atomicMin(b + 1, v.y);
  if (v.z > b[2]) atomicMax(b + 2, v.z);
  if (v.w > b[3]) atomicMax(b + 3, v.w);
}

// what the group pass checks and adds up here: coordinates inside +-(COORD_UNITS << f), the coordinate box of every ring,
// the pixel box of every id; the used rows are counted on the way
struct GroupPolicy {
  int f, Hs, Ws;
  int* box;
  int2* yrange;
  uint32_t* header;
  struct Ring {
    int xmin, ymin, xmax, ymax;
  };
  struct Sum {
    bool has_box;
    int4 pb;
  };
  __device__ __forceinline__ Ring empty() const { return Ring{INT_MAX, INT_MAX, INT_MIN, INT_MIN}; }
  __device__ __forceinline__ bool vertex(Ring& r, int2 p) const {
    const int cmax = COORD_UNITS << f;
    r.xmin = p.x < r.xmin ? p.x : r.xmin;
    r.xmax = p.x > r.xmax ? p.x : r.xmax;
    r.ymin = p.y < r.ymin ? p.y : r.ymin;
    r.ymax = p.y > r.ymax ? p.y : r.ymax;
    return p.x >= -cmax && p.x <= cmax && p.y >= -cmax && p.y <= cmax;
  }
  __device__ __forceinline__ void merge(Ring& r) const {
    r.xmin = wave_min32(r.xmin);
    r.ymin = wave_min32(r.ymin);
    r.xmax = wave_max32(r.xmax);
    r.ymax = wave_max32(r.ymax);
  }
  __device__ __forceinline__ void status(bool look, bool id_ok, bool ring_ok, bool used) const {
    const bool no_id = __any(look && !id_ok) != 0, no_ring = __any(look && !ring_ok) != 0;
    const int n_used = __popcll(__ballot(used));
    if ((threadIdx.x & 63) == 0) {
      if (no_id || no_ring) atomicOr(header + WS_STATUS, (uint32_t)((no_id ? C3D_FILL_ST_BAD_ID : 0) | (no_ring ? C3D_FILL_ST_BAD_RING : 0)));
      if (n_used) atomicAdd(header + WS_USED, (uint32_t)n_used);
    }
  }
  __device__ __forceinline__ Sum ring(int r, int n, bool used, const Ring& c) const {
    Sum v{false, make_int4(0, 0, -1, -1)};
    v.has_box = used && n >= 3 && pixel_box(c.xmin, c.ymin, c.xmax, c.ymax, f, Hs, Ws, &v.pb);
    if (used) yrange[r] = v.has_box ? make_int2(v.pb.y, v.pb.w) : make_int2(1, 0);   // the rows this ring can toggle a bit on
    return v;
  }
  __device__ __forceinline__ Sum fold(bool same, const Sum& v) const {
    const bool sb = same && v.has_box;
    const int4 u = make_int4(wave_min32(sb ? v.pb.x : INT_MAX), wave_min32(sb ? v.pb.y : INT_MAX), wave_max32(sb ? v.pb.z : INT_MIN),
                             wave_max32(sb ? v.pb.w : INT_MIN));
    return Sum{u.x <= u.z, u};
  }
  __device__ __forceinline__ void add(int id, const Sum& v) const {
    if (v.has_box) box_atomics(box + (int64_t)(id - 1) * 4, v.pb);
  }
};
__global__ __launch_bounds__(256) void fill_group_kernel(Groups g, int f, int Hs, int Ws, int* __restrict__ box, int2* __restrict__ yrange,
                                                         uint32_t* __restrict__ header) {
  group_pass(g, GroupPolicy{f, Hs, Ws, box, yrange, header});
}
__global__ __launch_bounds__(SCAN_T) void fill_scan_kernel(Groups g) {
  extern __shared__ uint32_t part[];                       // [SCAN_T / 64]
  scan_pass(g, part);
}
__global__ __launch_bounds__(256) void fill_scatter_kernel(Groups g) { scatter_pass(g); }

// ------------------------------------------------------------------------------------------------- one wave per id
__global__ __launch_bounds__(256) void fill_wave_kernel(const int32_t* __restrict__ rings, const int2* __restrict__ vertices,
                                                        const int4* __restrict__ box, const uint32_t* __restrict__ cnt,
                                                        const uint32_t* __restrict__ off, const uint32_t* __restrict__ grouped,
                                                        uint32_t* __restrict__ large, uint32_t* __restrict__ header, int f, int Ws,
                                                        int32_t* __restrict__ labels) {
  const int lane = threadIdx.x & 63, K = (int)header[WS_K];
  for (int id = 1 + blockIdx.x * 4 + (threadIdx.x >> 6); id <= K; id += gridDim.x * 4) {   // id is uniform over the wave
    const int4 b = box[id - 1];
    if (b.x > b.z || b.y > b.w) continue;                  // no ring of this id reaches a pixel centre of the scene
    const int w = b.z - b.x + 1, h = b.w - b.y + 1;
    if (w > BOX_LIMIT || h > BOX_LIMIT) {                  // for the workgroup tier; the order of the list is of no consequence
      if (lane == 0) large[atomicAdd(header + WS_LARGE, 1u)] = (uint32_t)id;
      continue;
    }
    const int y = b.y + lane;                              // rows past the box toggle bits that are never painted
    u64 bits = 0;
    const uint32_t nr = cnt[id - 1], at = off[id - 1];
    for (uint32_t i = 0; i < nr; ++i) {
      const int r = (int)grouped[at + i];
      const int64_t start = rings[(int64_t)r * 8 + 1];
      const int n = rings[(int64_t)r * 8 + 2];
      if (n < 3) continue;
      for (int base = 0; base < n; base += 64) {
        const int k = base + lane, m = n - base < 64 ? n - base : 64;
        int2 p = make_int2(0, 0), q = make_int2(0, 0);
        if (k < n) {
          p = vertices[start + k];
          q = vertices[start + (k ? k - 1 : n - 1)];
        }
        for (int j = 0; j < m; ++j) {                      // edge (v[base + j - 1], v[base + j]), the same for every lane
          const Edge e = make_edge(make_int2(__shfl(q.x, j), __shfl(q.y, j)), make_int2(__shfl(p.x, j), __shfl(p.y, j)));
          if (e.dy != 0 && y >= first_row(e.Y0, f) && y <= last_row(e.Y0 + e.dy, f)) {   // no lane leaves the loop: the shuffles need all
            const int c = edge_column(e, y, f, b.x, b.z);
            if (c <= b.z) bits ^= 1ull << (c - b.x);
          }
        }
      }
    }
    bits ^= bits << 1;
    bits ^= bits << 2;
    bits ^= bits << 4;
    bits ^= bits << 8;
    bits ^= bits << 16;
    bits ^= bits << 32;
    for (int row = 0; row < h; ++row) {                    // lane = column: neighbouring lanes paint neighbouring pixels
      const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)bits, row), hi = (uint32_t)__shfl((int)(uint32_t)(bits >> 32), row);
      const u64 line = ((u64)hi << 32) | lo;
      if (lane < w && ((line >> lane) & 1ull)) atomicMax(labels + (int64_t)(b.y + row) * Ws + b.x + lane, id);
    }
  }
}

// -------------------------------------------------------------------------------- one workgroup per (id, band of rows)
__global__ __launch_bounds__(BLOCK_T) void fill_block_kernel(const int32_t* __restrict__ rings, const int2* __restrict__ vertices,
                                                            const int4* __restrict__ box, const uint32_t* __restrict__ cnt,
                                                            const uint32_t* __restrict__ off, const uint32_t* __restrict__ grouped,
                                                            const int2* __restrict__ yrange, const uint32_t* __restrict__ large,
                                                            const uint32_t* __restrict__ header, int f, int Ws,
                                                            int32_t* __restrict__ labels) {
  extern __shared__ u64 band[];                            // [BAND_ROWS][wpr]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = BLOCK_T / 64;
  const uint32_t n_large = header[WS_LARGE];
  for (uint32_t li = blockIdx.x; li < n_large; li += gridDim.x) {
    const int id = (int)large[li];
    const int4 b = box[id - 1];
    const int ya = b.y + (int)blockIdx.y * BAND_ROWS;      // the band's rows ya .. yb of the scene
    if (ya > b.w) continue;
    const int yb = ya + BAND_ROWS - 1 < b.w ? ya + BAND_ROWS - 1 : b.w;
    const int w = b.z - b.x + 1, wpr = (w + 63) >> 6, h = yb - ya + 1;
    __syncthreads();                                       // the id before is done with the LDS
    for (int i = threadIdx.x; i < h * wpr; i += BLOCK_T) band[i] = 0;
    __syncthreads();
    const uint32_t nr = cnt[id - 1], at = off[id - 1];
    auto toggle = [&](int2 p, int2 q) {                    // the bits of the edge (p, q) on the rows of this band
      const Edge e = make_edge(p, q);
      if (e.dy == 0) return;
      int y_lo = first_row(e.Y0, f), y_hi = last_row(e.Y0 + e.dy, f);
      y_lo = y_lo < ya ? ya : y_lo;
      y_hi = y_hi > yb ? yb : y_hi;
      for (int y = y_lo; y <= y_hi; ++y) {                 // at most BAND_ROWS rows
        const int c = edge_column(e, y, f, b.x, b.z);
        if (c <= b.z) atomicXor(band + (y - ya) * wpr + ((c - b.x) >> 6), 1ull << ((c - b.x) & 63));
      }
    };
    // 64 rings per wave and step.  A ring whose rows miss the band costs its lane one load; a small ring is walked by its
    // lane (an object with half a million one-pixel holes is half a million such rings); a larger one by the whole wave
    for (uint32_t base = (uint32_t)wave * 64; base < nr; base += (uint32_t)waves * 64) {
      int start = 0, n = 0;
      if (base + lane < nr) {
        const int r = (int)grouped[at + base + lane];
        const int2 yr = yrange[r];
        if (yr.x <= yb && yr.y >= ya) {                    // not empty: the ring has at least 3 vertices
          start = rings[(int64_t)r * 8 + 1];
          n = rings[(int64_t)r * 8 + 2];
        }
      }
      if (n > 0 && n <= SMALL_RING) {
        int2 p = vertices[(int64_t)start + n - 1];
        for (int k = 0; k < n; ++k) {
          const int2 q = vertices[(int64_t)start + k];
          toggle(p, q);
          p = q;
        }
      }
      u64 big = __ballot(n > SMALL_RING);
      for (int step = 0; step < 64 && big; ++step) {       // uniform: the shuffles see every lane
        const int src = __ffsll((long long)big) - 1;
        big &= big - 1;
        const int64_t s0 = __shfl(start, src);
        const int n0 = __shfl(n, src);
        for (int k = lane; k < n0; k += 64) toggle(vertices[s0 + (k ? k - 1 : n0 - 1)], vertices[s0 + k]);
      }
    }
    __syncthreads();
    for (int row = wave; row < h; row += waves) {          // a wave per row: fill inside the words, carry the parity across
      u64* line = band + row * wpr;
      uint32_t carry = 0;
      for (int base = 0; base < wpr; base += 64) {
        const int j = base + lane;
        u64 v = j < wpr ? line[j] : 0ull;
        uint32_t all;                                      // the parity of a sum of parities is their xor
        const uint32_t before = wave_excl_scan32((uint32_t)__popcll(v) & 1u, &all);
        v ^= v << 1;
        v ^= v << 2;
        v ^= v << 4;
        v ^= v << 8;
        v ^= v << 16;
        v ^= v << 32;
        if (carry ^ (before & 1u)) v = ~v;
        if (j < wpr) line[j] = v;
        carry ^= all & 1u;
      }
    }
    __syncthreads();
    for (int i = wave; i < h * wpr; i += waves) {          // a wave per word, a lane per pixel
      const u64 v = band[i];
      if (!v) continue;
      const int row = i / wpr, x = b.x + ((i - row * wpr) << 6) + lane;
      if (x <= b.z && ((v >> lane) & 1ull)) atomicMax(labels + (int64_t)(ya + row) * Ws + x, id);
    }
  }
}

// ------------------------------------------------------------------------------------------------------- the table
struct RowAcc {                                            // what some pixels of one id add to its table row
  int cnt, x0, y0, x1, y1, first;
};
__device__ __forceinline__ void row_atomics(int32_t* table, int id, const RowAcc& a) {   // min / max columns: see box_atomics
  int32_t* row = table + (int64_t)(id - 1) * 8;
  atomicAdd(row, a.cnt);
  if (a.x0 < row[1]) atomicMin(row + 1, a.x0);
  if (a.y0 < row[2]) atomicMin(row + 2, a.y0);
  if (a.x1 > row[3]) atomicMax(row + 3, a.x1);
  if (a.y1 > row[4]) atomicMax(row + 4, a.y1);
  if (a.first < row[6]) atomicMin(row + 6, a.first);
}
__device__ __forceinline__ RowAcc wave_row(bool same, int x, int y, int p) {
  RowAcc a;
  a.cnt = __popcll(__ballot(same));
  a.x0 = wave_min32(same ? x : INT_MAX);
  a.x1 = wave_max32(same ? x : INT_MIN);
  a.y0 = wave_min32(same ? y : INT_MAX);
  a.y1 = wave_max32(same ? y : INT_MIN);
  a.first = wave_min32(same ? p : INT_MAX);
  return a;
}

// A wave walks TABLE_STEPS x 64 consecutive pixels.  The most frequent id of a step is kept in (wave-uniform) registers while
// it stays the same from step to step and goes out as one set of atomics when it changes: inside a large object that is one
// set per 1024 pixels.  The second most frequent id of a step goes out per step, what is left per lane.
__global__ __launch_bounds__(256) void fill_table_kernel(const int32_t* __restrict__ labels, int Hs, int Ws, int max_objects,
                                                         const uint8_t* __restrict__ id_cls, int32_t* __restrict__ table,
                                                         uint8_t* __restrict__ mask, uint8_t* __restrict__ cls_map) {
  const int N = Hs * Ws, lane = threadIdx.x & 63;          // < 2^31: both extents are at most 16384
  constexpr int CHUNK = 64 * TABLE_STEPS;
  for (int64_t cb = (int64_t)(blockIdx.x * 4 + (threadIdx.x >> 6)) * CHUNK; cb < N; cb += (int64_t)gridDim.x * 4 * CHUNK) {   // uniform over the wave
    int cur = 0;
    RowAcc acc = {0, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MAX};
    for (int step = 0; step < TABLE_STEPS && cb + step * 64 < N; ++step) {
      const int p = (int)cb + step * 64 + lane;
      int id = p < N ? labels[p] : 0;
      if (id < 0 || id > max_objects) id = 0;              // cannot happen: the fill paints used ids only
      if (p < N) {
        if (mask) mask[p] = id > 0;
        if (cls_map) cls_map[p] = id > 0 && id_cls ? id_cls[id - 1] : (uint8_t)0;
      }
      const int y = p / Ws, x = p - y * Ws;
      bool open = id > 0;
      u64 m = __ballot(open);
      if (!m) continue;                                    // uniform
      int leader = __ffsll((long long)m) - 1, id0 = __shfl(id, leader);
      bool same = open && id == id0;
      const RowAcc a = wave_row(same, x, y, p);
      if (id0 != cur) {
        if (cur > 0 && lane == 0) row_atomics(table, cur, acc);
        cur = id0;
        acc = a;
      } else {
        acc.cnt += a.cnt;
        acc.x0 = a.x0 < acc.x0 ? a.x0 : acc.x0;
        acc.y0 = a.y0 < acc.y0 ? a.y0 : acc.y0;
        acc.x1 = a.x1 > acc.x1 ? a.x1 : acc.x1;
        acc.y1 = a.y1 > acc.y1 ? a.y1 : acc.y1;
        acc.first = a.first < acc.first ? a.first : acc.first;
      }
      if (same) open = false;
      m = __ballot(open);
      if (!m) continue;                                    // uniform
      leader = __ffsll((long long)m) - 1;
      id0 = __shfl(id, leader);
      same = open && id == id0;
      const RowAcc a2 = wave_row(same, x, y, p);
      if (lane == leader) row_atomics(table, id0, a2);
      if (same) open = false;
      if (open) {
        const RowAcc a1 = {1, x, y, x, y, p};
        row_atomics(table, id, a1);
      }
    }
    if (cur > 0 && lane == 0) row_atomics(table, cur, acc);
  }
}

__global__ __launch_bounds__(256) void fill_finish_kernel(const int32_t* __restrict__ counts, const uint32_t* __restrict__ header,
                                                          const uint8_t* __restrict__ id_cls, int max_objects,
                                                          int32_t* __restrict__ table, int32_t* __restrict__ counts_obj,
                                                          int32_t* __restrict__ info) {
  const int K = (int)header[WS_K];
  const bool bad_counts = (counts[4] & C3D_OUTLINE_ST_BAD_COUNTS) != 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < max_objects; i += gridDim.x * 256) {
    int4* row = reinterpret_cast<int4*>(table + (int64_t)i * 8);
    if (i >= K) {
      row[0] = row[1] = make_int4(0, 0, 0, 0);
      continue;
    }
    const int cls = id_cls ? id_cls[i] : 0;
    const int4 r0 = row[0], r1 = row[1];
    if (r0.x == 0) {                                       // an id that owns no pixel
      row[0] = make_int4(0, 0, 0, 0);
      row[1] = make_int4(0, cls, 0, 0);
    } else {
      row[1] = make_int4(r1.x, cls, r1.z, 0);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    counts_obj[0] = bad_counts ? -1 : K;
    counts_obj[1] = K;
    info[0] = (int32_t)((uint32_t)counts[4] | header[WS_STATUS]);
    info[1] = (int32_t)header[WS_USED];
    info[2] = K;
    info[3] = 0;
  }
}

int refuse(int32_t max_rings, int32_t max_vertices, int32_t max_objects, int32_t Hs, int32_t Ws) {
  if (max_rings < 1 || max_vertices < 1 || max_objects < 1 || Hs < 1 || Ws < 1) return C3D_E_BADARG;
  if (Hs > EXTENT_MAX || Ws > EXTENT_MAX) return C3D_E_UNSUPPORTED;
  return 0;
}

}  // namespace

extern "C" void c3d_rings_fill_limits(int32_t out[2]) {
  if (!out) return;
  out[0] = BOX_LIMIT;
  out[1] = BAND_ROWS;
}

extern "C" int64_t c3d_rings_fill_ws_bytes(int32_t max_rings, int32_t max_vertices, int32_t max_objects, int32_t Hs, int32_t Ws) {
  const int rc = refuse(max_rings, max_vertices, max_objects, Hs, Ws);
  if (rc) return rc;
  return plan_of(nullptr, max_rings, max_vertices, max_objects).bytes;
}

extern "C" int c3d_rings_fill(const int32_t* rings, const int32_t* vertices, const int32_t* counts, int32_t max_rings,
                              int32_t max_vertices, int32_t frac_bits, const uint8_t* id_cls, int32_t max_objects, int32_t Hs,
                              int32_t Ws, int32_t* labels, int32_t* table, int32_t* counts_obj, uint8_t* mask, uint8_t* cls_map,
                              int32_t* info, void* ws, void* stream) {
  if (!rings || !vertices || !counts || !labels || !table || !counts_obj || !info || !ws) return C3D_E_BADARG;
  if (frac_bits < 0 || frac_bits > FRAC_MAX) return C3D_E_BADARG;
  int rc = refuse(max_rings, max_vertices, max_objects, Hs, Ws);
  if (rc) return rc;
  const Plan pl = plan_of(ws, max_rings, max_vertices, max_objects);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint32_t* header = static_cast<uint32_t*>(ws);
  Groups g = pl.g;
  g.rings = rings; g.vertices = reinterpret_cast<const int2*>(vertices); g.counts = counts;
  int4* box = pl.box;
  uint32_t *cnt = g.cnt, *off = g.off, *large = pl.large, *grouped = g.grouped;
  int2* yrange = pl.yrange;
  const int2* v_in = g.vertices;
  const int f = frac_bits;

  // the header and the labels; every other word of the workspace is written by the call before the call reads it
  hipError_t e = hipMemsetAsync(ws, 0, 256, st);
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(labels, 0, (size_t)Hs * (size_t)Ws * 4, st);
  if (e != hipSuccess) return (int)e;
  // ring and id counts are known on the device only: grids are sized by the limits and surplus waves and workgroups return
  const unsigned g_ids = grid_for(max_objects, 256, MAX_GRID), g_idw = grid_for(max_objects, 4, MAX_GRID);
  const unsigned g_rows = grid_for(max_rings, 256, MAX_GRID);
  rc = c3d_launch_lds<fill_init_kernel>(dim3(g_ids), dim3(256), 0, st, box, cnt, g.cursor, table, (int)max_objects);
  if (rc) return rc;
  rc = c3d_launch_lds<fill_group_kernel>(dim3(g_rows), dim3(256), 0, st, g, f, (int)Hs, (int)Ws, reinterpret_cast<int*>(box), yrange, header);
  if (rc) return rc;
  rc = c3d_launch_lds<fill_scan_kernel>(dim3(1), dim3(SCAN_T), SCAN_T / 64 * 4, st, g);
  if (rc) return rc;
  rc = c3d_launch_lds<fill_scatter_kernel>(dim3(g_rows), dim3(256), 0, st, g);
  if (rc) return rc;
  rc = c3d_launch_lds<fill_wave_kernel>(dim3(g_idw), dim3(256), 0, st, rings, v_in, (const int4*)box, (const uint32_t*)cnt,
                                        (const uint32_t*)off, (const uint32_t*)grouped, large, header, f, (int)Ws, labels);
  if (rc) return rc;
  const unsigned bands = (unsigned)((Hs + BAND_ROWS - 1) / BAND_ROWS);
  const unsigned g_list = (unsigned)(max_objects < LIST_GRID ? max_objects : LIST_GRID);
  const size_t lds = (size_t)BAND_ROWS * (size_t)((Ws + 63) / 64) * 8;   // at most 128 KiB; a band uses it by its box's width
  rc = c3d_launch_lds<fill_block_kernel>(dim3(g_list, bands), dim3(BLOCK_T), lds, st, rings, v_in, (const int4*)box,
                                         (const uint32_t*)cnt, (const uint32_t*)off, (const uint32_t*)grouped, (const int2*)yrange,
                                         (const uint32_t*)large, (const uint32_t*)header, f, (int)Ws, labels);
  if (rc) return rc;
  rc = c3d_launch_lds<fill_table_kernel>(dim3(grid_for((int64_t)Hs * Ws, 256 * TABLE_STEPS, MAX_GRID)), dim3(256), 0, st, (const int32_t*)labels, (int)Hs,
                                         (int)Ws, (int)max_objects, id_cls, table, mask, cls_map);
  if (rc) return rc;
  return c3d_launch_lds<fill_finish_kernel>(dim3(g_ids), dim3(256), 0, st, counts, (const uint32_t*)header, id_cls, (int)max_objects,
                                            table, counts_obj, info);
}
