// Regularised footprints of a scene map: the rings of c3d_outlines_simplify (or any table of that shape with integer pixel
// corners) squared to the axes of their object's minimum-area rectangle while they stay in HBM.  The rule -- the direction of
// an id from the chosen hull edge, the frame (T, C), the edge classes, the runs between the junctions, one level per run as a
// length-weighted mean rounded half up, the vertices where two runs meet, the mapping back -- is the header's
// (include/change3d_hip.h); this file is one way to compute it.  Integer arithmetic only in every decision: the one place a
// double appears is the first guess of a quotient, which integer multiplication then confirms or moves.  No workgroup waits
// for another, nothing is read back, every loop is capped.
//
//   1 count_wave   a wave per ring row: classifies the row (pass-through, bad, copied, regularised), looks up the direction
//                  of its id, and for a ring of up to WAVE_LIMIT edges, a lane per edge, takes n' from one ballot.  Lists the
//                  larger rings for 2
//   2 count_block  a larger ring, one workgroup: coordinates, zero-length edges and junctions counted from HBM
//   3 scan         one workgroup: start' = exclusive scan of n'; rows whose vertices would not fit (only tables whose rows
//                  share vertices get there) become bad rows; counts_out
//   4 write_wave   rings of up to WAVE_LIMIT edges, the rows that are not regularised, the zero rows past the table.  The ring
//                  is rotated so that lane 0 holds the first junction: runs are then contiguous lanes, their sums one
//                  segmented scan by shuffles, and the lane at the end of a run divides
//   5 write_block  larger rings, one workgroup each: the junction list by a scan, then a thread per run walks its edges and
//                  divides, then a thread per junction writes.  Vertices, junction list and levels live in LDS up to
//                  LDS_LIMIT edges; beyond that the vertices are read from HBM and the two lists live in the workspace, at
//                  the ring's own place start' (the same code, other pointers)
#include <climits>

#include "scene_host.h"
#include "scene_wave.h"
#include "../../include/change3d_hip.h"

namespace {

using namespace c3d_wave;

typedef unsigned long long u64;
typedef __int128 i128;
typedef unsigned __int128 u128;

constexpr int WAVE_LIMIT = 64;                             // one lane per edge
// 16 bytes per edge (the packed vertex, a junction index, a level): 64 KiB, so that two workgroups share a CU
constexpr int LDS_LIMIT = 4096;
constexpr int BLOCK_T = 256;
constexpr int WAVES = BLOCK_T / 64;
constexpr int COORD_MAX = 16384;
constexpr int MAX_GRID = 4096;
constexpr int SCAN_T = 1024, SCAN_ROWS = 8;
constexpr int LDS_BYTES = LDS_LIMIT * 16 + 64;
enum : uint8_t { ROW_PASS = 0, ROW_BAD = 1, ROW_COPY = 2, ROW_REGULAR = 3, ROW_LARGE = 4 };   // ROW_LARGE: for count_block to decide

// words of the workspace header (256 bytes, zeroed by the call's memset)
enum { WS_STATUS = 0, WS_LARGE = 1 };

struct Workspace {
  int64_t np, startp, large, kind, junc, level, bytes;     // byte offsets
};

Workspace workspace_plan(int64_t max_rings, int64_t max_vertices) {
  Workspace w;
  auto up = c3d_host::up256;
  w.np = 256;
  w.startp = w.np + up(max_rings * 4);
  w.large = w.startp + up(max_rings * 4);
  w.kind = w.large + up(max_rings * 4);
  w.junc = w.kind + up(max_rings);
  w.level = w.junc + up(max_vertices * 4);
  w.bytes = w.level + up(max_vertices * 8);
  return w;
}

__device__ __forceinline__ int64_t absl(int64_t v) { return v < 0 ? -v : v; }
__device__ __forceinline__ bool coord_ok(int2 p) { return p.x >= 0 && p.x <= COORD_MAX && p.y >= 0 && p.y <= COORD_MAX; }

// what the call reads of its two count vectors
struct Limits {
  int rows, k_hull;
  int64_t vlimit, hvlimit;
  bool bad_counts;
  int status;
};
__device__ __forceinline__ Limits limits_of(const int32_t* counts, const int32_t* counts_hull, int max_rings, int max_vertices,
                                            int max_objects, int max_hull_vertices) {
  Limits l;
  l.status = counts[4] | counts_hull[4];
  l.bad_counts = (l.status & C3D_OUTLINE_ST_BAD_COUNTS) != 0;
  l.rows = l.bad_counts ? 0 : clampi(counts[1], 0, max_rings);
  l.vlimit = clampi(counts[3], 0, max_vertices);
  l.k_hull = clampi(counts_hull[1], 0, max_objects);
  l.hvlimit = clampi(counts_hull[3], 0, max_hull_vertices);
  return l;
}

// the direction u of an id, 1 <= id <= max_objects; false: the id has none and its rings are copied
__device__ __forceinline__ bool direction(int id, const int32_t* __restrict__ hulls, const int2* __restrict__ hull_vertices,
                                          const int64_t* __restrict__ rects, const Limits& l, int2* u) {
  if (id > l.k_hull) return false;
  const int64_t k = rects[(int64_t)(id - 1) * 8];
  const int hs = hulls[(int64_t)(id - 1) * 8 + 1], m = hulls[(int64_t)(id - 1) * 8 + 2];
  if (k < 0 || hs < 0 || m < 3 || k >= m || (int64_t)hs + m > l.hvlimit) return false;
  const int2 a = hull_vertices[(int64_t)hs + k], b = hull_vertices[(int64_t)hs + (k + 1 == m ? 0 : k + 1)];
  if (!coord_ok(a) || !coord_ok(b)) return false;
  const int dx = b.x - a.x, dy = b.y - a.y;
  if (dx == 0 && dy == 0) return false;
  int g = dx < 0 ? -dx : dx, h = dy < 0 ? -dy : dy;
  for (int step = 0; step < 32 && h; ++step) {             // Euclid on two numbers of up to 15 bits: at most 22 steps
    const int t = g % h;
    g = h;
    h = t;
  }
  *u = make_int2(dx / g, dy / g);
  return true;
}

// floor(num / den), den > 0, for quotients below 2^40: a guess from doubles, within 2 of the truth (the dividend's magnitude
// carries a relative error of 2^-52, the quotient then one of 2^-50 plus the truncation), confirmed or moved by the
// remainder, which is integer arithmetic
__device__ __forceinline__ int64_t fdiv(i128 num, u64 den) {
  const bool neg = num < 0;
  const u128 mag = neg ? (u128)0 - (u128)num : (u128)num;
  const double d = (double)(u64)(mag >> 64) * 18446744073709551616.0 + (double)(u64)mag;
  int64_t q = (int64_t)(d / (double)den);
  if (neg) q = -q;
  i128 r = num - (i128)q * (i128)den;
  for (int step = 0; step < 4 && r < 0; ++step) { --q; r += (i128)den; }
  for (int step = 0; step < 4 && r >= (i128)den; ++step) { ++q; r -= (i128)den; }
  return q;
}

struct Frame {
  int64_t T, C;
};
__device__ __forceinline__ Frame frame(int2 p, int2 u) {
  Frame f;
  f.T = (int64_t)p.x * u.x + (int64_t)p.y * u.y;
  f.C = (int64_t)p.y * u.x - (int64_t)p.x * u.y;
  return f;
}
// the class of the edge (p, q): true = H
__device__ __forceinline__ bool edge_h(int2 p, int2 q, int2 u) {
  const Frame a = frame(p, u), b = frame(q, u);
  return absl(b.T - a.T) >= absl(b.C - a.C);
}
// what the edge (p, q) of class h adds to its run: the weight and weight * (sum of the other coordinate of its ends)
__device__ __forceinline__ void edge_terms(int2 p, int2 q, int2 u, bool h, u64* w, int64_t* a) {
  const Frame f0 = frame(p, u), f1 = frame(q, u);
  const int64_t wt = h ? absl(f1.T - f0.T) : absl(f1.C - f0.C);   // at most 2^30
  *w = (u64)wt;
  *a = wt * (h ? f0.C + f1.C : f0.T + f1.T);               // below 2^60
}
__device__ __forceinline__ int64_t level_of(u64 W, i128 A, int frac_bits) {
  return fdiv((i128)((u128)A << frac_bits) + (i128)W, 2 * W);   // the shift of a two's complement number is the product by S
}
// the output vertex of a junction from the levels of the two runs that meet there
__device__ __forceinline__ int2 corner(int64_t Tq, int64_t Cq, int2 u) {
  const int64_t N = (int64_t)u.x * u.x + (int64_t)u.y * u.y;
  const int64_t X = 2 * (Tq * u.x - Cq * u.y) + N, Y = 2 * (Tq * u.y + Cq * u.x) + N;
  return make_int2((int)fdiv((i128)X, (u64)(2 * N)), (int)fdiv((i128)Y, (u64)(2 * N)));
}

// -------------------------------------------------------------------------------------------------- 1, 2: n' per ring
__global__ __launch_bounds__(256) void regular_count_wave_kernel(const int32_t* __restrict__ rings, const int2* __restrict__ vertices,
                                                                 const int32_t* __restrict__ counts, int max_rings, int max_vertices,
                                                                 const int32_t* __restrict__ hulls, const int2* __restrict__ hull_vertices,
                                                                 const int64_t* __restrict__ rects, const int32_t* __restrict__ counts_hull,
                                                                 int max_objects, int max_hull_vertices, int32_t* __restrict__ np,
                                                                 uint8_t* __restrict__ kind, uint32_t* __restrict__ large,
                                                                 uint32_t* __restrict__ header) {
  const Limits l = limits_of(counts, counts_hull, max_rings, max_vertices, max_objects, max_hull_vertices);
  const int lane = threadIdx.x & 63;
  for (int r = blockIdx.x * 4 + (int)(threadIdx.x >> 6); r < l.rows; r += gridDim.x * 4) {   // r is uniform over the wave
    const int id = rings[(int64_t)r * 8], start = rings[(int64_t)r * 8 + 1], n = rings[(int64_t)r * 8 + 2];
    if (start < 0) {
      if (lane == 0) { kind[r] = ROW_PASS; np[r] = 0; }
      continue;
    }
    if (n < 0 || (int64_t)start + n > l.vlimit || id < 1 || id > max_objects) {
      if (lane == 0) { kind[r] = ROW_BAD; np[r] = 0; atomicOr(header + WS_STATUS, (uint32_t)C3D_REGULAR_ST_BAD_ROW); }
      continue;
    }
    if (n > WAVE_LIMIT) {                                  // the order of the list is of no consequence
      if (lane == 0) { kind[r] = ROW_LARGE; np[r] = 0; large[atomicAdd(header + WS_LARGE, 1u)] = (uint32_t)r; }
      continue;
    }
    const bool in = lane < n;
    const int2 p = in ? vertices[(int64_t)start + lane] : make_int2(0, 0);
    if (__any(in && !coord_ok(p))) {
      if (lane == 0) { kind[r] = ROW_BAD; np[r] = 0; atomicOr(header + WS_STATUS, (uint32_t)C3D_REGULAR_ST_BAD_ROW); }
      continue;
    }
    int2 u = make_int2(1, 0);
    bool regular = n >= 4 && direction(id, hulls, hull_vertices, rects, l, &u);
    int R = 0;
    if (regular) {                                         // uniform
      const int nx = lane + 1 < n ? lane + 1 : 0;
      const int2 q = make_int2(__shfl(p.x, nx), __shfl(p.y, nx));
      const bool h = in && edge_h(p, q, u);
      const u64 hm = __ballot(h);
      const int pv = lane ? lane - 1 : n - 1;
      R = __popcll(__ballot(in && (((hm >> pv) & 1ull) != (h ? 1ull : 0ull))));
      regular = R >= 4 && !__any(in && p.x == q.x && p.y == q.y);
    }
    if (lane == 0) { kind[r] = regular ? ROW_REGULAR : ROW_COPY; np[r] = regular ? R : n; }
  }
}

__global__ __launch_bounds__(BLOCK_T) void regular_count_block_kernel(const int32_t* __restrict__ rings, const int2* __restrict__ vertices,
                                                                      const int32_t* __restrict__ counts, int max_rings, int max_vertices,
                                                                      const int32_t* __restrict__ hulls, const int2* __restrict__ hull_vertices,
                                                                      const int64_t* __restrict__ rects, const int32_t* __restrict__ counts_hull,
                                                                      int max_objects, int max_hull_vertices, int32_t* __restrict__ np,
                                                                      uint8_t* __restrict__ kind, const uint32_t* __restrict__ large,
                                                                      uint32_t* __restrict__ header) {
  extern __shared__ int s_words[];                         // [3]: dynamic, as the launcher raises the kernel's LDS limit to the CU's
  int &s_bad = s_words[0], &s_zero = s_words[1], &s_R = s_words[2];
  const Limits l = limits_of(counts, counts_hull, max_rings, max_vertices, max_objects, max_hull_vertices);
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t n_large = header[WS_LARGE];
  for (uint32_t li = blockIdx.x; li < n_large; li += gridDim.x) {
    const int r = (int)large[li];
    const int id = rings[(int64_t)r * 8], n = rings[(int64_t)r * 8 + 2];
    const int64_t start = rings[(int64_t)r * 8 + 1];
    __syncthreads();                                       // the ring before is done with the three words
    if (tid == 0) s_bad = s_zero = s_R = 0;
    __syncthreads();
    int2 u = make_int2(1, 0);
    const bool dir = direction(id, hulls, hull_vertices, rects, l, &u);
    int bad = 0, zero = 0, R = 0;
    for (int k = tid; k < n; k += BLOCK_T) {
      const int2 p = vertices[start + k];
      bad |= !coord_ok(p);
    }
    if (bad) s_bad = 1;                                    // every writer stores the same value
    __syncthreads();
    if (s_bad) {
      if (tid == 0) { kind[r] = ROW_BAD; np[r] = 0; atomicOr(header + WS_STATUS, (uint32_t)C3D_REGULAR_ST_BAD_ROW); }
      continue;
    }
    if (dir) {                                             // uniform; the coordinates are in range: the frame cannot overflow
      for (int k = tid; k < n; k += BLOCK_T) {
        const int2 a = vertices[start + (k ? k - 1 : n - 1)], p = vertices[start + k], q = vertices[start + (k + 1 < n ? k + 1 : 0)];
        zero |= p.x == q.x && p.y == q.y;
        R += edge_h(a, p, u) != edge_h(p, q, u);
      }
      for (int d = 32; d; d >>= 1) R += __shfl_xor(R, d);
      if (lane == 0 && R) atomicAdd(&s_R, R);
      if (zero) s_zero = 1;
    }
    __syncthreads();
    const bool regular = dir && !s_zero && s_R >= 4;
    if (tid == 0) { kind[r] = regular ? ROW_REGULAR : ROW_COPY; np[r] = regular ? s_R : n; }
  }
}

// ---------------------------------------------------------------------------------------------------- 3: start', counts
__global__ __launch_bounds__(SCAN_T) void regular_scan_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ counts_hull,
                                                              int max_rings, int max_vertices, int max_objects, int max_hull_vertices,
                                                              int32_t* __restrict__ np, uint8_t* __restrict__ kind,
                                                              uint32_t* __restrict__ startp, const uint32_t* __restrict__ header,
                                                              int32_t* __restrict__ counts_out) {
  extern __shared__ u64 part[];                            // [SCAN_T / 64], then where the first row that does not fit
  u64& s_cut = part[SCAN_T / 64];                          // would have started
  const Limits l = limits_of(counts, counts_hull, max_rings, max_vertices, max_objects, max_hull_vertices);
  if (threadIdx.x == 0) s_cut = ~0ull;
  __syncthreads();
  u64 running = 0;
  for (int base = 0; base < l.rows; base += SCAN_T * SCAN_ROWS) {
    int n[SCAN_ROWS];
    u64 mine = 0;
    for (int j = 0; j < SCAN_ROWS; ++j) {
      const int r = base + (int)threadIdx.x * SCAN_ROWS + j;
      n[j] = r < l.rows ? np[r] : 0;
      mine += (u64)n[j];
    }
    u64 all;
    u64 at = running + block_excl_scan64(mine, part, &all);
    for (int j = 0; j < SCAN_ROWS; ++j) {
      const int r = base + (int)threadIdx.x * SCAN_ROWS + j;
      if (r < l.rows) {
        // `at` only grows: once a row does not fit, no later row with a vertex does
        const bool fits = at + (u64)n[j] <= (u64)max_vertices;
        if (!fits && kind[r] >= ROW_COPY) {
          kind[r] = ROW_BAD;
          np[r] = 0;
          atomicMin(&s_cut, at);
        }
        startp[r] = fits ? (uint32_t)at : 0u;
      }
      at += (u64)n[j];
    }
    running += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (l.bad_counts) {
      counts_out[0] = counts_out[1] = counts_out[2] = counts_out[3] = 0;
      counts_out[4] = l.status;
    } else {
      const bool cut = s_cut != ~0ull;
      const u64 out = cut ? s_cut : running;               // at most max_vertices
      counts_out[0] = counts[0];
      counts_out[1] = l.rows;
      counts_out[2] = counts_out[3] = (int32_t)out;
      counts_out[4] = (int32_t)((uint32_t)l.status | header[WS_STATUS] | (cut ? (uint32_t)C3D_REGULAR_ST_BAD_ROW : 0u));
    }
  }
}

// ------------------------------------------------------------------------------------------------------- 4, 5: writing
__device__ __forceinline__ void write_row(int32_t* __restrict__ rings_out, int r, const int4 r0, const int4 r1, int start, int n,
                                          int flag) {
  int4* dst = reinterpret_cast<int4*>(rings_out + (int64_t)r * 8);
  dst[0] = make_int4(r0.x, start, n, flag);
  dst[1] = make_int4(r1.x, r1.y, r1.z, r0.z);
}

__global__ __launch_bounds__(256) void regular_write_wave_kernel(const int32_t* __restrict__ rings, const int2* __restrict__ vertices,
                                                                 const int32_t* __restrict__ counts, int max_rings, int max_vertices,
                                                                 const int32_t* __restrict__ hulls, const int2* __restrict__ hull_vertices,
                                                                 const int64_t* __restrict__ rects, const int32_t* __restrict__ counts_hull,
                                                                 int max_objects, int max_hull_vertices, int frac_bits,
                                                                 const int32_t* __restrict__ np, const uint8_t* __restrict__ kind,
                                                                 const uint32_t* __restrict__ startp, int32_t* __restrict__ rings_out,
                                                                 int2* __restrict__ vertices_out) {
  const Limits l = limits_of(counts, counts_hull, max_rings, max_vertices, max_objects, max_hull_vertices);
  const int lane = threadIdx.x & 63;
  for (int r = blockIdx.x * 4 + (int)(threadIdx.x >> 6); r < max_rings; r += gridDim.x * 4) {   // r is uniform over the wave
    if (r >= l.rows) {
      if (lane < 2) reinterpret_cast<int4*>(rings_out + (int64_t)r * 8)[lane] = make_int4(0, 0, 0, 0);
      continue;
    }
    const int4 r0 = reinterpret_cast<const int4*>(rings + (int64_t)r * 8)[0], r1 = reinterpret_cast<const int4*>(rings + (int64_t)r * 8)[1];
    const int what = kind[r];
    if (what == ROW_PASS || what == ROW_BAD) {
      if (lane == 0) write_row(rings_out, r, r0, r1, -1, 0, 0);
      continue;
    }
    const int n = r0.z;
    if (n > WAVE_LIMIT) continue;                          // the workgroup kernel's
    const int64_t at = startp[r];
    if (lane == 0) write_row(rings_out, r, r0, r1, (int)at, np[r], what == ROW_REGULAR ? 1 : 0);
    const bool in = lane < n;
    const int2 p0 = in ? vertices[(int64_t)r0.y + lane] : make_int2(0, 0);
    if (what == ROW_COPY) {
      if (in) vertices_out[at + lane] = make_int2(p0.x << frac_bits, p0.y << frac_bits);
      continue;
    }
    int2 u = make_int2(1, 0);
    direction(r0.x, hulls, hull_vertices, rects, l, &u);   // the count kernel found one
    int first;                                             // the smallest junction
    {
      const int nx = lane + 1 < n ? lane + 1 : 0;
      const bool h = in && edge_h(p0, make_int2(__shfl(p0.x, nx), __shfl(p0.y, nx)), u);
      const u64 hm = __ballot(h);
      const int pv = lane ? lane - 1 : n - 1;
      first = __ffsll((long long)__ballot(in && (((hm >> pv) & 1ull) != (h ? 1ull : 0ull)))) - 1;
    }
    // lane i now owns edge first + i, cyclic: the runs are contiguous lanes and lane 0 starts one
    const int src = lane + first < n ? lane + first : lane + first - n;
    const int2 p = make_int2(__shfl(p0.x, in ? src : 0), __shfl(p0.y, in ? src : 0));
    const int nx = lane + 1 < n ? lane + 1 : 0;
    const int2 q = make_int2(__shfl(p.x, nx), __shfl(p.y, nx));
    const bool h = in && edge_h(p, q, u);
    const u64 hm = __ballot(h);
    const int pv = lane ? lane - 1 : n - 1;
    const bool junction = in && (((hm >> pv) & 1ull) != (h ? 1ull : 0ull));
    const u64 jm = __ballot(junction);                     // bit 0 is set
    u64 W = 0, Alo = 0, Ahi = 0;                           // A as two words of a two's complement number
    if (in) {
      int64_t a;
      edge_terms(p, q, u, h, &W, &a);
      Alo = (u64)a;
      Ahi = a < 0 ? ~0ull : 0ull;
    }
    bool closed = junction;                                // the sum already reaches back to the start of its run
    for (int d = 1; d < 64; d <<= 1) {                     // inclusive segmented sum
      const int from = lane >= d ? lane - d : lane;
      const u64 oW = shfl64(W, from), oAlo = shfl64(Alo, from), oAhi = shfl64(Ahi, from);
      const int oclosed = __shfl((int)closed, from);
      if (lane >= d && !closed) {
        W += oW;
        const u64 lo = Alo + oAlo;
        Ahi += oAhi + (lo < Alo ? 1ull : 0ull);
        Alo = lo;
        closed = oclosed != 0;
      }
    }
    const u64 above = (jm >> lane) >> 1;                   // the junctions after this lane
    const int last = above ? lane + __ffsll((long long)above) - 1 : n - 1;   // the last lane of this lane's run
    int64_t level = 0;
    if (in && lane == last) level = level_of(W, (i128)(((u128)Ahi << 64) | (u128)Alo), frac_bits);
    const int64_t ahead = (int64_t)shfl64((u64)level, in ? last : 0);                // of the run that starts here
    const int64_t behind = (int64_t)shfl64((u64)level, lane ? lane - 1 : n - 1);     // of the run that ends here
    if (junction) {
      const int j = __popcll(jm & ((1ull << lane) - 1ull));
      vertices_out[at + j] = h ? corner(behind, ahead, u) : corner(ahead, behind, u);
    }
  }
}

// One ring of a workgroup; every thread calls it.  getP(k) = vertex k; junc and level have room for the ring's n' entries
template <class GetP>
__device__ __forceinline__ void block_ring(GetP getP, int* junc, int64_t* level, int n, int R, int2 u, int frac_bits,
                                           int2* __restrict__ out, int* s_part) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int running = 0;
  for (int base = 0; base < n; base += BLOCK_T) {          // the junctions in ascending order
    const int k = base + tid;
    bool f = false;
    if (k < n) f = edge_h(getP(k ? k - 1 : n - 1), getP(k), u) != edge_h(getP(k), getP(k + 1 < n ? k + 1 : 0), u);
    const u64 m = __ballot(f);
    if (lane == 0) s_part[wave] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < WAVES; ++w) {
      before += w < wave ? s_part[w] : 0;
      all += s_part[w];
    }
    const int j = running + before + __popcll(m & ((1ull << lane) - 1ull));
    if (f && j < R) junc[j] = k;                           // R is what the count kernel found by the same test
    running += all;
    __syncthreads();
  }
  for (int j = tid; j < R; j += BLOCK_T) {                 // the run that ends at junction j
    const int k1 = junc[j];
    int k = junc[j ? j - 1 : R - 1];
    const bool h = edge_h(getP(k), getP(k + 1 < n ? k + 1 : 0), u);
    u64 W = 0;
    i128 A = 0;
    for (int step = 0; step < n && k != k1; ++step) {
      const int nx = k + 1 < n ? k + 1 : 0;
      u64 w;
      int64_t a;
      edge_terms(getP(k), getP(nx), u, h, &w, &a);
      W += w;
      A += (i128)a;
      k = nx;
    }
    level[j] = level_of(W, A, frac_bits);
  }
  __syncthreads();
  for (int j = tid; j < R; j += BLOCK_T) {
    const int k = junc[j];
    const bool h = edge_h(getP(k), getP(k + 1 < n ? k + 1 : 0), u);   // of the run that starts here
    const int64_t behind = level[j], ahead = level[j + 1 < R ? j + 1 : 0];
    out[j] = h ? corner(behind, ahead, u) : corner(ahead, behind, u);
  }
}

__global__ __launch_bounds__(BLOCK_T) void regular_write_block_kernel(const int32_t* __restrict__ rings, const int2* __restrict__ vertices,
                                                                      const int32_t* __restrict__ counts, int max_rings, int max_vertices,
                                                                      const int32_t* __restrict__ hulls, const int2* __restrict__ hull_vertices,
                                                                      const int64_t* __restrict__ rects, const int32_t* __restrict__ counts_hull,
                                                                      int max_objects, int max_hull_vertices, int frac_bits,
                                                                      const int32_t* __restrict__ np, const uint8_t* __restrict__ kind,
                                                                      const uint32_t* __restrict__ startp, const uint32_t* __restrict__ large,
                                                                      const uint32_t* __restrict__ header, int32_t* __restrict__ g_junc,
                                                                      int64_t* __restrict__ g_level, int32_t* __restrict__ rings_out,
                                                                      int2* __restrict__ vertices_out) {
  extern __shared__ int64_t lds[];                         // level i64 [LDS_LIMIT], junc i32 [LDS_LIMIT], vertices u32 [LDS_LIMIT],
  int64_t* s_level = lds;                                  // then a word per wave
  int* s_junc = reinterpret_cast<int*>(s_level + LDS_LIMIT);
  uint32_t* s_p = reinterpret_cast<uint32_t*>(s_junc + LDS_LIMIT);
  int* s_part = reinterpret_cast<int*>(s_p + LDS_LIMIT);
  const Limits l = limits_of(counts, counts_hull, max_rings, max_vertices, max_objects, max_hull_vertices);
  const int tid = threadIdx.x;
  const uint32_t n_large = header[WS_LARGE];
  for (uint32_t li = blockIdx.x; li < n_large; li += gridDim.x) {
    const int r = (int)large[li];
    const int what = kind[r];
    if (what != ROW_COPY && what != ROW_REGULAR) continue;   // a bad row: the wave kernel writes it
    const int4 r0 = reinterpret_cast<const int4*>(rings + (int64_t)r * 8)[0], r1 = reinterpret_cast<const int4*>(rings + (int64_t)r * 8)[1];
    const int n = r0.z, R = np[r];
    const int64_t start = r0.y, at = startp[r];
    if (tid == 0) write_row(rings_out, r, r0, r1, (int)at, R, what == ROW_REGULAR ? 1 : 0);
    if (what == ROW_COPY) {
      for (int k = tid; k < n; k += BLOCK_T) {
        const int2 p = vertices[start + k];
        vertices_out[at + k] = make_int2(p.x << frac_bits, p.y << frac_bits);
      }
      continue;
    }
    int2 u = make_int2(1, 0);
    direction(r0.x, hulls, hull_vertices, rects, l, &u);   // the count kernel found one
    __syncthreads();                                       // the ring before is done with the LDS
    if (n <= LDS_LIMIT) {
      for (int k = tid; k < n; k += BLOCK_T) {
        const int2 p = vertices[start + k];
        s_p[k] = (uint32_t)p.x | ((uint32_t)p.y << 16);
      }
      __syncthreads();
      block_ring([&](int k) { const uint32_t v = s_p[k]; return make_int2((int)(v & 0xFFFFu), (int)(v >> 16)); }, s_junc, s_level, n, R,
                 u, frac_bits, vertices_out + at, s_part);
    } else {
      block_ring([&](int k) { return vertices[start + k]; }, g_junc + at, g_level + at, n, R, u, frac_bits, vertices_out + at, s_part);
    }
  }
}

int refuse(int32_t max_rings, int32_t max_vertices, int32_t max_objects) {
  if (max_rings < 1 || max_vertices < 1 || max_objects < 1) return C3D_E_BADARG;
  return 0;
}

}  // namespace

extern "C" void c3d_rings_regularize_limits(int32_t out[2]) {
  if (!out) return;
  out[0] = WAVE_LIMIT;
  out[1] = LDS_LIMIT;
}

extern "C" int64_t c3d_rings_regularize_ws_bytes(int32_t max_rings, int32_t max_vertices, int32_t max_objects) {
  const int rc = refuse(max_rings, max_vertices, max_objects);
  if (rc) return rc;
  return workspace_plan(max_rings, max_vertices).bytes;
}

extern "C" int c3d_rings_regularize(const int32_t* rings, const int32_t* vertices, const int32_t* counts, int32_t max_rings,
                                    int32_t max_vertices, const int32_t* hulls, const int32_t* hull_vertices, const int64_t* rects,
                                    const int32_t* counts_hull, int32_t max_objects, int32_t max_hull_vertices, int32_t frac_bits,
                                    int32_t* rings_out, int32_t* vertices_out, int32_t* counts_out, void* ws, void* stream) {
  if (!rings || !vertices || !counts || !hulls || !hull_vertices || !rects || !counts_hull || !rings_out || !vertices_out ||
      !counts_out || !ws)
    return C3D_E_BADARG;
  if (max_hull_vertices < 1 || frac_bits < 0 || frac_bits > 8) return C3D_E_BADARG;
  int rc = refuse(max_rings, max_vertices, max_objects);
  if (rc) return rc;
  const Workspace w = workspace_plan(max_rings, max_vertices);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  uint32_t* header = reinterpret_cast<uint32_t*>(base);
  int32_t* np = reinterpret_cast<int32_t*>(base + w.np);
  uint32_t* startp = reinterpret_cast<uint32_t*>(base + w.startp);
  uint32_t* large = reinterpret_cast<uint32_t*>(base + w.large);
  uint8_t* kind = reinterpret_cast<uint8_t*>(base + w.kind);
  int32_t* junc = reinterpret_cast<int32_t*>(base + w.junc);
  int64_t* level = reinterpret_cast<int64_t*>(base + w.level);
  const int2* v_in = reinterpret_cast<const int2*>(vertices);
  const int2* hv = reinterpret_cast<const int2*>(hull_vertices);
  int2* v_out = reinterpret_cast<int2*>(vertices_out);

  // only the header: every other word of the workspace is written by the call before the call reads it
  hipError_t e = hipMemsetAsync(base, 0, 256, st);
  if (e != hipSuccess) return (int)e;
  // the ring count is known on the device only: grids are sized by max_rings and surplus waves and workgroups return
  const unsigned g_wave = c3d_host::grid_for(max_rings, 4, MAX_GRID), g_block = c3d_host::grid_for(max_rings, 1, MAX_GRID);
  rc = c3d_launch_lds<regular_count_wave_kernel>(dim3(g_wave), dim3(256), 0, st, rings, v_in, counts, (int)max_rings, (int)max_vertices,
                                                 hulls, hv, rects, counts_hull, (int)max_objects, (int)max_hull_vertices, np, kind, large,
                                                 header);
  if (rc) return rc;
  rc = c3d_launch_lds<regular_count_block_kernel>(dim3(g_block), dim3(BLOCK_T), 16, st, rings, v_in, counts, (int)max_rings,
                                                  (int)max_vertices, hulls, hv, rects, counts_hull, (int)max_objects,
                                                  (int)max_hull_vertices, np, kind, (const uint32_t*)large, header);
  if (rc) return rc;
  rc = c3d_launch_lds<regular_scan_kernel>(dim3(1), dim3(SCAN_T), SCAN_T / 8 + 8, st, counts, counts_hull, (int)max_rings, (int)max_vertices,
                                           (int)max_objects, (int)max_hull_vertices, np, kind, startp, (const uint32_t*)header,
                                           counts_out);
  if (rc) return rc;
  rc = c3d_launch_lds<regular_write_wave_kernel>(dim3(g_wave), dim3(256), 0, st, rings, v_in, counts, (int)max_rings, (int)max_vertices,
                                                 hulls, hv, rects, counts_hull, (int)max_objects, (int)max_hull_vertices, (int)frac_bits,
                                                 (const int32_t*)np, (const uint8_t*)kind, (const uint32_t*)startp, rings_out, v_out);
  if (rc) return rc;
  return c3d_launch_lds<regular_write_block_kernel>(dim3(g_block), dim3(BLOCK_T), LDS_BYTES, st, rings, v_in, counts, (int)max_rings,
                                                    (int)max_vertices, hulls, hv, rects, counts_hull, (int)max_objects,
                                                    (int)max_hull_vertices, (int)frac_bits, (const int32_t*)np, (const uint8_t*)kind,
                                                    (const uint32_t*)startp, (const uint32_t*)large, (const uint32_t*)header, junc,
                                                    level, rings_out, v_out);
}
