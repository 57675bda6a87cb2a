// Polygon scores of a scene map: PoLiS, the vertex-to-boundary Hausdorff distance and the vertex counts of every matched pair
// (predicted object, ground-truth object) from two ring tables and the match_p of c3d_objects_match while all of them stay in
// HBM.  The rule -- the rows used, the geometry of an id, the distance of a point to an edge, which pairs are scored -- is the
// header's (include/change3d_hip.h); this file is one way to compute it.  Integers decide everything but the distances; every
// integer quantity of a distance is exact in a double.  No workgroup waits for another, nothing is read back, every loop is
// capped, and no floating-point sum depends on scheduling.
//
//   1 rows     a wave per ring row of either side: classifies the row and adds it to its id (ring count, vertex count, the
//              incomplete mark: integer atomics, whose result does not depend on their order)
//     check    the coordinates of the rings above BIG_RING vertices, which kernel 1 only lists: many workgroups, a chunk each
//   2 ids      one workgroup per side: exclusive scans over the ids up to the largest one seen: where an id's rings are listed,
//              where its vertices go
//   3 place    a thread per row: claims a slot in the ring list of its id (the order of the list varies and is never used);
//              also zeroes the output rows past the last predicted object
//   4 gather   a wave per row: the row's place among the vertices of its id = the n of the listed rings with a smaller row
//              index (an integer sum); then writes its edges (a, b), shifted to the common unit, to that place
//     gather   the same for the rings above BIG_RING: their place from kernel 4, many workgroups, a chunk each
//   5 pairs    one workgroup: every predicted id's partner, counts and flag; the pairs of the job tier get their jobs by a scan
//   6 jobs     a workgroup per (pair, direction, CHUNK vertices): the other id's edges pass through LDS in tiles of TILE, a
//              thread per vertex; writes the chunk's sum (a fixed tree) and maximum
//   7 score    a wave per pair: the wave tier (both sides <= WAVE_LIMIT vertices: a lane per vertex and edge of each side, the
//              other side's edges by shuffle, both directions in one walk) or the reduction of the pair's jobs in job order
//   8 totals   one workgroup: counts and sums in ascending p (256 interleaved partial sums, then a fixed tree), totals
#include <climits>

#include "scene_wave.h"
#include "../../include/change3d_hip.h"

namespace {

using namespace c3d_wave;

typedef unsigned long long u64;

constexpr int WAVE_LIMIT = 64;                             // vertices of either side in the wave tier: a lane each
constexpr int CHUNK = 256;                                 // vertices of a job: a thread each
constexpr int TILE = 512;                                  // edges of an LDS tile: 40 bytes each
constexpr int RING_LIMIT = 16384;                          // rings of an id whose order the gather step restores: a scene-filling
                                                           // object of a noisy map has thousands of holes
constexpr int BIG_RING = 4096;                             // a longer ring is checked and copied by many workgroups, a chunk each
constexpr int BLOCK_T = 256;
constexpr int MAX_GRID = 4096;
constexpr int SCAN_T = 1024;
constexpr int COORD_UNIT = 32768;
constexpr double GUARD = 1.0 + 0x1p-50;                    // see edge_update

enum : uint8_t { ROW_SKIP = 0, ROW_USED = 1 };             // ROW_USED: valid, n >= 3, listed under its id
enum : uint8_t { TIER_NONE = 0, TIER_WAVE = 1, TIER_JOB = 2 };
enum { ID_INCOMPLETE = 1 };

// words of the workspace header (256 bytes, zeroed by the call's memset)
enum { WS_STATUS = 0, WS_KP = 1, WS_KG = 2, WS_JOBS = 3, WS_BIG_P = 4, WS_BIG_G = 5 };   // WS_KP + side = the largest id of a row of
                                                                                      // that side, WS_BIG_P + side = its long rings

struct Side {
  const int32_t* rings;
  const int2* vertices;
  const int32_t* counts;
  int max_rings, max_vertices, max_ids, shift;             // shift = F - frac_bits
  int64_t coord_max;                                       // 32768 << frac_bits
  // workspace
  uint8_t* kind;                                           // [max_rings]
  uint2* list;                                             // [max_rings] (ring row, its n) grouped by id
  uint32_t* big;                                           // [max_rings] the rows of the rings above BIG_RING, in any order
  uint32_t* row_at;                                        // [max_rings] where such a ring's vertices go within its id
  uint32_t* id_rings;                                      // [max_ids] used rings with n >= 3
  u64* id_verts;                                           // [max_ids] their vertices
  uint32_t* id_flags;                                      // [max_ids]
  uint32_t* id_claim;                                      // [max_ids]
  uint32_t* id_list;                                       // [max_ids] start in list
  uint32_t* id_start;                                      // [max_ids] start in edges
  int4* edges;                                             // [max_vertices] (a.x, a.y, b.x, b.y) grouped by id
};

struct Plan {
  Side s[2];
  int64_t zero_bytes;                                      // the header and the per-id words the memset clears
  int64_t tier, job_start, partial, job_cap, bytes;
};

Plan plan_of(int64_t max_rings_p, int64_t max_vertices_p, int64_t max_p, int64_t max_rings_g, int64_t max_vertices_g,
             int64_t max_g) {
  Plan pl{};
  auto up = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  int64_t at = 256;
  const int64_t rings[2] = {max_rings_p, max_rings_g}, verts[2] = {max_vertices_p, max_vertices_g}, ids[2] = {max_p, max_g};
  int64_t off[2][11];
  for (int k = 0; k < 2; ++k) {                            // zeroed part first
    off[k][2] = at; at += up(ids[k] * 4);
    off[k][3] = at; at += up(ids[k] * 8);
    off[k][4] = at; at += up(ids[k] * 4);
    off[k][5] = at; at += up(ids[k] * 4);
  }
  pl.zero_bytes = at;
  for (int k = 0; k < 2; ++k) {
    off[k][0] = at; at += up(rings[k]);
    off[k][1] = at; at += up(rings[k] * 8);
    off[k][6] = at; at += up(ids[k] * 4);
    off[k][7] = at; at += up(ids[k] * 4);
    off[k][8] = at; at += up(verts[k] * 16);
    off[k][9] = at; at += up(rings[k] * 4);
    off[k][10] = at; at += up(rings[k] * 4);
  }
  pl.tier = at; at += up(max_p);
  pl.job_start = at; at += up(max_p * 8);
  // enough for every pair of a match that names no ground-truth id twice
  pl.job_cap = (max_vertices_p + CHUNK - 1) / CHUNK + (max_vertices_g + CHUNK - 1) / CHUNK + 2 * max_p;
  pl.partial = at; at += up(pl.job_cap * 16);
  pl.bytes = at;
  for (int k = 0; k < 2; ++k) {
    Side& s = pl.s[k];
    s.max_rings = (int)rings[k]; s.max_vertices = (int)verts[k]; s.max_ids = (int)ids[k];
    s.kind = reinterpret_cast<uint8_t*>(off[k][0]);        // offsets for now: bind() adds the base
    s.list = reinterpret_cast<uint2*>(off[k][1]);
    s.id_rings = reinterpret_cast<uint32_t*>(off[k][2]);
    s.id_verts = reinterpret_cast<u64*>(off[k][3]);
    s.id_flags = reinterpret_cast<uint32_t*>(off[k][4]);
    s.id_claim = reinterpret_cast<uint32_t*>(off[k][5]);
    s.id_list = reinterpret_cast<uint32_t*>(off[k][6]);
    s.id_start = reinterpret_cast<uint32_t*>(off[k][7]);
    s.edges = reinterpret_cast<int4*>(off[k][8]);
    s.big = reinterpret_cast<uint32_t*>(off[k][9]);
    s.row_at = reinterpret_cast<uint32_t*>(off[k][10]);
  }
  return pl;
}

template <class T> void rebase(T*& p, char* base) { p = reinterpret_cast<T*>(base + reinterpret_cast<intptr_t>(p)); }
void bind(Side& s, char* base) {
  rebase(s.kind, base); rebase(s.list, base); rebase(s.id_rings, base); rebase(s.id_verts, base); rebase(s.id_flags, base);
  rebase(s.id_claim, base); rebase(s.id_list, base); rebase(s.id_start, base); rebase(s.edges, base);
  rebase(s.big, base); rebase(s.row_at, base);
}

struct Sides {
  Side s[2];
};

__device__ __forceinline__ int rows_of(const Side& s) {
  return (s.counts[4] & C3D_OUTLINE_ST_BAD_COUNTS) ? 0 : clampi(s.counts[1], 0, s.max_rings);
}
__device__ __forceinline__ bool coord_ok(const Side& s, int2 p) {
  return p.x >= -s.coord_max && p.x <= s.coord_max && p.y >= -s.coord_max && p.y <= s.coord_max;
}
__device__ __forceinline__ double shfl_d(double v, int src) {
  return __longlong_as_double((long long)shfl64((u64)__double_as_longlong(v), src));
}
__device__ __forceinline__ double wave_sum_fixed(double v) {   // the same tree in every run
  for (int o = 32; o > 0; o >>= 1) v += shfl_d(v, (int)(threadIdx.x & 63) ^ o);
  return v;
}
__device__ __forceinline__ double wave_max_fixed(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, shfl_d(v, (int)(threadIdx.x & 63) ^ o));
  return v;
}

// The squared distance of p to the edge (a, a + e), L = e.e, folded into the running minimum `cur`.  Every operand is an
// integer below 2^25 held in a double, every product and sum below 2^53: t, c, w.w and L are exact.  The quotient is the
// header's ((double)c * (double)c) / (double)L.  It is only formed where it can lower the minimum: `guard` is at least
// cur * (1 + 2^-50) (1 - 2^-53), so fl(guard * L) > cur * L, and cc > fl(guard * L) gives cc / L > cur, whose rounding is no
// smaller than cur: the minimum would not move.  The result is the same double as without the test.
__device__ __forceinline__ void edge_update(double px, double py, double ax, double ay, double ex, double ey, double L, double& cur,
                                            double& guard) {
  const double wx = px - ax, wy = py - ay;
  const double t = wx * ex + wy * ey;
  double v;
  if (L == 0.0 || t <= 0.0) {
    v = wx * wx + wy * wy;
  } else if (t >= L) {
    const double ux = wx - ex, uy = wy - ey;
    v = ux * ux + uy * uy;
  } else {
    const double c = wx * ey - wy * ex;
    const double cc = c * c;
    if (cc > guard * L) return;
    v = cc / L;
  }
  if (v < cur) {
    cur = v;
    guard = v * GUARD;
  }
}

// --------------------------------------------------------------------------------------------------------------- 1: rows
__global__ __launch_bounds__(256) void polis_rows_kernel(Sides sd, uint32_t* __restrict__ header) {
  const Side& s = sd.s[blockIdx.y];
  const int rows = rows_of(s), lane = threadIdx.x & 63;
  const int64_t vlimit = clampi(s.counts[3], 0, s.max_vertices);
  // The holes of a scene-filling object are tens of thousands of rows of one id: what a wave adds to an id is kept in
  // registers while the id stays the same, and the largest id is one atomic per wave.  Integer sums: the grouping changes nothing
  int top = 0, held = 0;
  uint32_t held_rings = 0;
  u64 held_verts = 0;
  for (int r = blockIdx.x * 4 + (int)(threadIdx.x >> 6); r < rows; r += gridDim.x * 4) {   // r is uniform over the wave
    const int id = s.rings[(int64_t)r * 8], start = s.rings[(int64_t)r * 8 + 1], n = s.rings[(int64_t)r * 8 + 2];
    uint8_t kind = ROW_SKIP;
    if (id >= 1 && id <= s.max_ids) {
      bool bad = start < 0 || n < 0 || (int64_t)start + n > vlimit;
      if (!bad && n <= BIG_RING) {
        bool out = false;
        for (int k = lane; k < n; k += 64) out |= !coord_ok(s, s.vertices[(int64_t)start + k]);
        bad = __any(out);
      }
      // a longer ring is counted now and checked by the next kernel: a bad coordinate there makes the id incomplete, and the
      // counts of an incomplete id are dropped
      if (!bad && n > BIG_RING && lane == 0) s.big[atomicAdd(header + WS_BIG_P + blockIdx.y, 1u)] = (uint32_t)r;
      top = id > top ? id : top;
      if (bad) {
        if (lane == 0) atomicOr(s.id_flags + (id - 1), (uint32_t)ID_INCOMPLETE);
      } else if (n >= 3) {
        if (id != held) {
          if (held_rings && lane == 0) {
            atomicAdd(s.id_rings + (held - 1), held_rings);
            atomicAdd(s.id_verts + (held - 1), held_verts);
          }
          held = id;
          held_rings = 0;
          held_verts = 0;
        }
        held_rings += 1;
        held_verts += (u64)n;
        kind = ROW_USED;
      }
    }
    if (lane == 0) s.kind[r] = kind;
  }
  if (lane == 0) {
    if (held_rings) {
      atomicAdd(s.id_rings + (held - 1), held_rings);
      atomicAdd(s.id_verts + (held - 1), held_verts);
    }
    if (top) atomicMax(header + WS_KP + blockIdx.y, (uint32_t)top);
  }
}

// The coordinates of the long rings: every workgroup walks the list and takes the chunks blockIdx.x, blockIdx.x + gridDim.x, ...
__global__ __launch_bounds__(256) void polis_check_big_kernel(Sides sd, const uint32_t* __restrict__ header) {
  const Side& s = sd.s[blockIdx.y];
  const uint32_t n_big = min(header[WS_BIG_P + blockIdx.y], (uint32_t)s.max_rings);
  for (uint32_t li = 0; li < n_big; ++li) {
    const int r = (int)s.big[li];
    const int id = s.rings[(int64_t)r * 8], n = s.rings[(int64_t)r * 8 + 2];
    const int64_t start = s.rings[(int64_t)r * 8 + 1];
    bool out = false;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) out |= !coord_ok(s, s.vertices[start + k]);
    if (out) atomicOr(s.id_flags + (id - 1), (uint32_t)ID_INCOMPLETE);
  }
}

// ---------------------------------------------------------------------------------------------------------------- 2: ids
// An id with more than RING_LIMIT rings, or whose vertices no longer fit below max_vertices (only tables whose rows share
// vertices get there), becomes incomplete and takes no room.
__global__ __launch_bounds__(SCAN_T) void polis_ids_kernel(Sides sd, const uint32_t* __restrict__ header) {
  extern __shared__ u64 part_ids[];                        // [2][SCAN_T / 64]: dynamic, as the launcher raises the kernel's LDS
  u64(*part)[SCAN_T / 64] = reinterpret_cast<u64(*)[SCAN_T / 64]>(part_ids);   // limit to the CU's
  const Side& s = sd.s[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int top = clampi((int)header[WS_KP + blockIdx.x], 0, s.max_ids);   // the ids above it have no row: their words stay 0
  u64 run_r = 0, run_v = 0;
  for (int base = 0; base < top; base += SCAN_T) {
    const int i = base + (int)threadIdx.x;
    u64 nr = 0, nv = 0;
    uint32_t fl = 0;
    if (i < top) {
      nr = s.id_rings[i];
      nv = s.id_verts[i];
      fl = s.id_flags[i];
      if (nr > (u64)RING_LIMIT) fl |= ID_INCOMPLETE;
      if (fl & ID_INCOMPLETE) nr = nv = 0;
    }
    u64 ir = nr, iv = nv;
    for (int d = 1; d < 64; d <<= 1) {
      const int from = lane >= d ? lane - d : lane;
      const u64 tr = shfl64(ir, from), tv = shfl64(iv, from);
      if (lane >= d) { ir += tr; iv += tv; }
    }
    if (lane == 63) { part[0][wave] = ir; part[1][wave] = iv; }
    __syncthreads();
    u64 br = 0, bv = 0, ar = 0, av = 0;
    for (int w = 0; w < SCAN_T / 64; ++w) {
      br += w < wave ? part[0][w] : 0ull;
      bv += w < wave ? part[1][w] : 0ull;
      ar += part[0][w];
      av += part[1][w];
    }
    if (i < top) {
      const u64 at_r = run_r + br + ir - nr, at_v = run_v + bv + iv - nv;
      // at_v only grows: an id that does not fit takes its place in the sum all the same, so that no later id fits either
      const bool fits = at_v + nv <= (u64)s.max_vertices;
      if (!fits) fl |= ID_INCOMPLETE;
      s.id_flags[i] = fl;
      s.id_list[i] = (uint32_t)at_r;                       // at most max_rings
      s.id_start[i] = fits ? (uint32_t)at_v : 0u;
      if (fl & ID_INCOMPLETE) { s.id_rings[i] = 0; s.id_verts[i] = 0; }
    }
    run_r += ar;
    run_v += av;
    __syncthreads();
  }
}

// -------------------------------------------------------------------------------------------------------------- 3: place
__global__ __launch_bounds__(256) void polis_place_kernel(Sides sd, const uint32_t* __restrict__ header, int max_p, double* __restrict__ pair,
                                                          int32_t* __restrict__ pair_n) {
  const Side& s = sd.s[blockIdx.y];
  const int rows = rows_of(s);
  if (blockIdx.y == 0) {                                   // the rows past the last predicted object
    for (int p = clampi((int)header[WS_KP], 0, max_p) + blockIdx.x * 256 + (int)threadIdx.x; p < max_p; p += gridDim.x * 256) {
      reinterpret_cast<int4*>(pair_n)[p] = make_int4(0, 0, 0, 0);
      double2* row = reinterpret_cast<double2*>(pair + (int64_t)p * 4);
      row[0] = make_double2(0.0, 0.0);
      row[1] = make_double2(0.0, 0.0);
    }
  }
  for (int r = blockIdx.x * 256 + (int)threadIdx.x; r < rows; r += gridDim.x * 256) {
    if (s.kind[r] != ROW_USED) continue;
    const int id = s.rings[(int64_t)r * 8];
    const uint32_t k = s.id_rings[id - 1];                 // 0: the id became incomplete
    if (!k) continue;
    const uint32_t slot = atomicAdd(s.id_claim + (id - 1), 1u);
    if (slot < k) s.list[(u64)s.id_list[id - 1] + slot] = make_uint2((uint32_t)r, (uint32_t)s.rings[(int64_t)r * 8 + 2]);
  }
}

// ------------------------------------------------------------------------------------------------------------- 4: gather
__global__ __launch_bounds__(256) void polis_gather_kernel(Sides sd) {
  const Side& s = sd.s[blockIdx.y];
  const int rows = rows_of(s), lane = threadIdx.x & 63;
  for (int r = blockIdx.x * 4 + (int)(threadIdx.x >> 6); r < rows; r += gridDim.x * 4) {   // r is uniform over the wave
    if (s.kind[r] != ROW_USED) continue;
    const int id = s.rings[(int64_t)r * 8], n = s.rings[(int64_t)r * 8 + 2];
    const int64_t start = s.rings[(int64_t)r * 8 + 1];
    const int k = (int)s.id_rings[id - 1];                 // at most RING_LIMIT
    if (!k) continue;
    const uint2* list = s.list + s.id_list[id - 1];
    u64 before = 0;                                        // vertices of the id's rings with a smaller row index
    for (int j = lane; j < k; j += 64) {
      const uint2 q = list[j];
      if (q.x < (uint32_t)r) before += (u64)q.y;
    }
    for (int o = 32; o > 0; o >>= 1) before += shfl64(before, lane ^ o);
    const u64 total = s.id_verts[id - 1];
    if (before + (u64)n > total) continue;                 // cannot happen: the sums are those of kernel 1
    if (n > BIG_RING) {                                    // copied by the next kernel
      if (lane == 0) s.row_at[r] = (uint32_t)before;
      continue;
    }
    int4* dst = s.edges + s.id_start[id - 1] + before;     // id_start + total <= max_vertices
    const int scale = 1 << s.shift;                        // |coordinate| * scale <= 2^23
    for (int j = lane; j < n; j += 64) {
      const int2 a = s.vertices[start + j], b = s.vertices[start + (j + 1 < n ? j + 1 : 0)];
      dst[j] = make_int4(a.x * scale, a.y * scale, b.x * scale, b.y * scale);
    }
  }
}

__global__ __launch_bounds__(256) void polis_gather_big_kernel(Sides sd, const uint32_t* __restrict__ header) {
  const Side& s = sd.s[blockIdx.y];
  const uint32_t n_big = min(header[WS_BIG_P + blockIdx.y], (uint32_t)s.max_rings);
  const int scale = 1 << s.shift;
  for (uint32_t li = 0; li < n_big; ++li) {
    const int r = (int)s.big[li];
    if (s.kind[r] != ROW_USED) continue;
    const int id = s.rings[(int64_t)r * 8], n = s.rings[(int64_t)r * 8 + 2];
    const int64_t start = s.rings[(int64_t)r * 8 + 1];
    if (!s.id_rings[id - 1]) continue;                     // the id became incomplete
    const u64 before = s.row_at[r];
    if (before + (u64)n > s.id_verts[id - 1]) continue;    // cannot happen
    int4* dst = s.edges + s.id_start[id - 1] + before;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
      const int2 a = s.vertices[start + j], b = s.vertices[start + (j + 1 < n ? j + 1 : 0)];
      dst[j] = make_int4(a.x * scale, a.y * scale, b.x * scale, b.y * scale);
    }
  }
}

// -------------------------------------------------------------------------------------------------------------- 5: pairs
struct Out {
  double* pair;
  int32_t* pair_n;
  int64_t* counts;
  double* sums;
  int64_t* totals;
  double* total_sums;
};

__global__ __launch_bounds__(SCAN_T) void polis_pairs_kernel(Sides sd, const int32_t* __restrict__ match_p, int max_p, int max_g,
                                                             int64_t max_pair_work, int64_t job_cap, uint8_t* __restrict__ tier,
                                                             u64* __restrict__ job_start, uint32_t* __restrict__ header, Out out) {
  extern __shared__ u64 part[];                            // [SCAN_T / 64]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kp = clampi((int)header[WS_KP], 0, max_p);
  u64 running = 0;
  uint32_t status = 0;
  for (int base = 0; base < kp; base += SCAN_T) {
    const int i = base + (int)threadIdx.x;
    u64 jobs = 0;
    int flag = 0, g = 0;
    u64 np = 0, ng = 0;
    if (i < kp) {
      g = match_p[(int64_t)i * 4];
      if (g < 0 || g > max_g) {
        status |= C3D_POLIS_ST_BAD_PARTNER;
        g = 0;
      }
      const bool p_whole = !(sd.s[0].id_flags[i] & ID_INCOMPLETE);
      np = sd.s[0].id_verts[i];
      const bool g_whole = g >= 1 && !(sd.s[1].id_flags[g - 1] & ID_INCOMPLETE);
      ng = g >= 1 ? sd.s[1].id_verts[g - 1] : 0ull;
      if (g == 0) flag = 1;
      else if (!p_whole || !g_whole || np == 0 || ng == 0) flag = 2;
      else if (2 * np * ng > (u64)max_pair_work) flag = 3; // np, ng < 2^31
      else if (np > (u64)WAVE_LIMIT || ng > (u64)WAVE_LIMIT) jobs = (np + CHUNK - 1) / CHUNK + (ng + CHUNK - 1) / CHUNK;
    }
    u64 inc = jobs;
    for (int d = 1; d < 64; d <<= 1) {
      const u64 t = shfl64(inc, lane >= d ? lane - d : lane);
      if (lane >= d) inc += t;
    }
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    u64 before = 0, all = 0;
    for (int w = 0; w < SCAN_T / 64; ++w) {
      before += w < wave ? part[w] : 0ull;
      all += part[w];
    }
    if (i < kp) {
      const u64 at = running + before + inc - jobs;
      // `at` only grows: once a pair's jobs do not fit, no later pair of the job tier fits (only a match that names a
      // ground-truth id several times gets there)
      if (jobs && at + jobs > (u64)job_cap) flag = 3;
      job_start[i] = at;
      tier[i] = flag ? TIER_NONE : (jobs ? TIER_JOB : TIER_WAVE);
      reinterpret_cast<int4*>(out.pair_n)[i] = make_int4(g, (int)np, (int)ng, flag);
      if (flag) {
        double2* row = reinterpret_cast<double2*>(out.pair + (int64_t)i * 4);
        row[0] = make_double2(0.0, 0.0);
        row[1] = make_double2(0.0, 0.0);
      }
    }
    running += all;
    __syncthreads();
  }
  if (status) atomicOr(header + WS_STATUS, status);
  if (threadIdx.x == 0) {
    const u64 fit = running < (u64)job_cap ? running : (u64)job_cap;   // jobs past the first pair that does not fit are not run
    header[WS_JOBS] = (uint32_t)fit;
  }
}

// --------------------------------------------------------------------------------------------------------------- 6: jobs
__global__ __launch_bounds__(BLOCK_T) void polis_jobs_kernel(Sides sd, int max_p, const uint8_t* __restrict__ tier,
                                                             const u64* __restrict__ job_start, const int32_t* __restrict__ pair_n,
                                                             const uint32_t* __restrict__ header, double2* __restrict__ partial) {
  extern __shared__ double s_tile[];                       // [TILE][5] = (a.x, a.y, e.x, e.y, L), then two doubles per wave
  double* s_red = s_tile + TILE * 5;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t n_jobs = header[WS_JOBS];
  const int kp = clampi((int)header[WS_KP], 0, max_p);
  for (uint32_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
    int lo = 0, hi = kp;                                   // the last pair whose first job is <= job: at most 32 steps
    for (int step = 0; step < 32 && hi - lo > 1; ++step) {
      const int mid = (lo + hi) >> 1;
      if (job_start[mid] <= (u64)job) lo = mid; else hi = mid;
    }
    const int p = lo;
    if (p >= kp || tier[p] != TIER_JOB) continue;          // a pair that did not fit
    const int4 row = reinterpret_cast<const int4*>(pair_n)[p];
    const int g = row.x, np = row.y, ng = row.z;
    const u64 rel = (u64)job - job_start[p];
    const u64 jobs_p = ((u64)np + CHUNK - 1) / CHUNK, jobs_g = ((u64)ng + CHUNK - 1) / CHUNK;
    if (rel >= jobs_p + jobs_g) continue;
    const bool rev = rel >= jobs_p;                        // the direction G -> P
    const int64_t chunk = (int64_t)(rev ? rel - jobs_p : rel);
    const int4* pts = rev ? sd.s[1].edges + sd.s[1].id_start[g - 1] : sd.s[0].edges + sd.s[0].id_start[p];
    const int4* edges = rev ? sd.s[0].edges + sd.s[0].id_start[p] : sd.s[1].edges + sd.s[1].id_start[g - 1];
    const int n_pts = rev ? ng : np, n_edges = rev ? np : ng;
    const int64_t k = chunk * CHUNK + tid;
    const bool in = k < n_pts;
    double px = 0.0, py = 0.0;
    if (in) {
      const int4 v = pts[k];
      px = (double)v.x;
      py = (double)v.y;
    }
    double cur = HUGE_VAL, guard = HUGE_VAL;
    for (int base = 0; base < n_edges; base += TILE) {
      const int m = n_edges - base < TILE ? n_edges - base : TILE;
      __syncthreads();                                     // the tile before has been read
      for (int j = tid; j < m; j += BLOCK_T) {
        const int4 e = edges[(int64_t)base + j];
        const double ax = (double)e.x, ay = (double)e.y, ex = (double)e.z - ax, ey = (double)e.w - ay;
        double* d = s_tile + j * 5;
        d[0] = ax; d[1] = ay; d[2] = ex; d[3] = ey; d[4] = ex * ex + ey * ey;
      }
      __syncthreads();
      if (in) {
        for (int j = 0; j < m; ++j) {
          const double* d = s_tile + j * 5;                // the same address in every lane: a broadcast
          edge_update(px, py, d[0], d[1], d[2], d[3], d[4], cur, guard);
        }
      }
    }
    const double dist = in ? sqrt(cur) : 0.0;
    const double ws = wave_sum_fixed(dist), wm = wave_max_fixed(dist);
    __syncthreads();                                       // the job before has read s_red
    if (lane == 0) { s_red[wave * 2] = ws; s_red[wave * 2 + 1] = wm; }
    __syncthreads();
    if (tid == 0) {
      double sum = 0.0, mx = 0.0;
      for (int w = 0; w < BLOCK_T / 64; ++w) {             // in wave order
        sum += s_red[w * 2];
        mx = fmax(mx, s_red[w * 2 + 1]);
      }
      partial[job] = make_double2(sum, mx);
    }
  }
}

// -------------------------------------------------------------------------------------------------------------- 7: score
__global__ __launch_bounds__(256) void polis_score_kernel(Sides sd, int max_p, int frac_bits, const uint8_t* __restrict__ tier,
                                                          const u64* __restrict__ job_start, const uint32_t* __restrict__ header,
                                                          const double2* __restrict__ partial, Out out) {
  const int lane = threadIdx.x & 63;
  const int kp = clampi((int)header[WS_KP], 0, max_p);
  const double unit = 1.0 / (double)(1 << frac_bits);      // a power of two: the products below are exact
  for (int p = blockIdx.x * 4 + (int)(threadIdx.x >> 6); p < kp; p += gridDim.x * 4) {   // p is uniform over the wave
    const int what = tier[p];
    if (what == TIER_NONE) continue;
    const int4 row = reinterpret_cast<const int4*>(out.pair_n)[p];
    const int g = row.x, np = row.y, ng = row.z;
    double sum_pg = 0.0, sum_gp = 0.0, mx = 0.0;
    if (what == TIER_WAVE) {
      const int4* ep = sd.s[0].edges + sd.s[0].id_start[p];
      const int4* eg = sd.s[1].edges + sd.s[1].id_start[g - 1];
      const int4 a = lane < np ? ep[lane] : make_int4(0, 0, 0, 0), b = lane < ng ? eg[lane] : make_int4(0, 0, 0, 0);
      const double pax = (double)a.x, pay = (double)a.y, gax = (double)b.x, gay = (double)b.y;
      double cur_p = HUGE_VAL, guard_p = HUGE_VAL, cur_g = HUGE_VAL, guard_g = HUGE_VAL;
      const int steps = np > ng ? np : ng;                 // at most WAVE_LIMIT
      for (int k = 0; k < steps; ++k) {
        if (k < ng) {                                      // uniform: edge k of g against the vertices of p
          const double ax = (double)__shfl(b.x, k), ay = (double)__shfl(b.y, k);
          const double ex = (double)__shfl(b.z, k) - ax, ey = (double)__shfl(b.w, k) - ay;
          edge_update(pax, pay, ax, ay, ex, ey, ex * ex + ey * ey, cur_p, guard_p);
        }
        if (k < np) {
          const double ax = (double)__shfl(a.x, k), ay = (double)__shfl(a.y, k);
          const double ex = (double)__shfl(a.z, k) - ax, ey = (double)__shfl(a.w, k) - ay;
          edge_update(gax, gay, ax, ay, ex, ey, ex * ex + ey * ey, cur_g, guard_g);
        }
      }
      const double dp = lane < np ? sqrt(cur_p) : 0.0, dg = lane < ng ? sqrt(cur_g) : 0.0;
      sum_pg = wave_sum_fixed(dp);
      sum_gp = wave_sum_fixed(dg);
      mx = wave_max_fixed(fmax(dp, dg));
    } else {
      const u64 js = job_start[p];
      const int jobs_p = (np + CHUNK - 1) / CHUNK, jobs_g = (ng + CHUNK - 1) / CHUNK;
      for (int j = lane; j < jobs_p; j += 64) {            // lane l adds the jobs l, l + 64, ... in that order, then the tree
        const double2 v = partial[js + j];
        sum_pg += v.x;
        mx = fmax(mx, v.y);
      }
      for (int j = lane; j < jobs_g; j += 64) {
        const double2 v = partial[js + jobs_p + j];
        sum_gp += v.x;
        mx = fmax(mx, v.y);
      }
      sum_pg = wave_sum_fixed(sum_pg);
      sum_gp = wave_sum_fixed(sum_gp);
      mx = wave_max_fixed(mx);
    }
    if (lane == 0) {
      const double mean_pg = sum_pg / (double)np * unit, mean_gp = sum_gp / (double)ng * unit;
      double2* dst = reinterpret_cast<double2*>(out.pair + (int64_t)p * 4);
      dst[0] = make_double2((mean_pg + mean_gp) * 0.5, mx * unit);
      dst[1] = make_double2(mean_pg, mean_gp);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- 8: totals
__global__ __launch_bounds__(256) void polis_totals_kernel(Sides sd, int max_p, const uint32_t* __restrict__ header, Out out) {
  extern __shared__ double s_all[];                        // f64 [4][256], then i64 [6][256]
  double(*s_d)[256] = reinterpret_cast<double(*)[256]>(s_all);
  long long(*s_i)[256] = reinterpret_cast<long long(*)[256]>(s_all + 4 * 256);
  const int tid = threadIdx.x;
  const int kp = clampi((int)header[WS_KP], 0, max_p);
  double polis = 0.0, haus = 0.0, hmax = 0.0, ratio = 0.0;
  long long c[6] = {0, 0, 0, 0, 0, 0};
  for (int p = tid; p < kp; p += 256) {                    // 256 interleaved partial sums, each in ascending p
    const int4 row = reinterpret_cast<const int4*>(out.pair_n)[p];
    c[row.w & 3] += 1;
    if (row.w == 0) {
      const double2 v = reinterpret_cast<const double2*>(out.pair + (int64_t)p * 4)[0];
      polis += v.x;
      haus += v.y;
      hmax = fmax(hmax, v.y);
      ratio += (double)row.y / (double)row.z;
      c[4] += row.y;
      c[5] += row.z;
    }
  }
  s_d[0][tid] = polis; s_d[1][tid] = haus; s_d[2][tid] = hmax; s_d[3][tid] = ratio;
  for (int k = 0; k < 6; ++k) s_i[k][tid] = c[k];
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {                      // a fixed tree
    if (tid < d) {
      s_d[0][tid] += s_d[0][tid + d];
      s_d[1][tid] += s_d[1][tid + d];
      s_d[2][tid] = fmax(s_d[2][tid], s_d[2][tid + d]);
      s_d[3][tid] += s_d[3][tid + d];
      for (int k = 0; k < 6; ++k) s_i[k][tid] += s_i[k][tid + d];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int64_t status = (int64_t)(uint32_t)(sd.s[0].counts[4] | sd.s[1].counts[4]) | (int64_t)header[WS_STATUS];
    for (int k = 0; k < 6; ++k) out.counts[k] = s_i[k][0];
    out.counts[6] = status;
    out.counts[7] = 0;
    for (int k = 0; k < 4; ++k) out.sums[k] = s_d[k][0];
    if (out.totals) {
      for (int k = 0; k < 6; ++k) out.totals[k] += s_i[k][0];
      out.totals[6] |= status;
    }
    if (out.total_sums) {
      out.total_sums[0] += s_d[0][0];
      out.total_sums[1] += s_d[1][0];
      out.total_sums[2] = fmax(out.total_sums[2], s_d[2][0]);
      out.total_sums[3] += s_d[3][0];
    }
  }
}

unsigned grid_for(int64_t items, int per_block) {
  int64_t g = (items + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > MAX_GRID ? MAX_GRID : g));
}

int refuse(int32_t max_rings_p, int32_t max_vertices_p, int32_t max_p, int32_t max_rings_g, int32_t max_vertices_g, int32_t max_g) {
  if (max_rings_p < 1 || max_vertices_p < 1 || max_p < 1 || max_rings_g < 1 || max_vertices_g < 1 || max_g < 1) return C3D_E_BADARG;
  return 0;
}

}  // namespace

extern "C" void c3d_rings_polis_limits(int32_t out[5]) {
  if (!out) return;
  out[0] = WAVE_LIMIT;
  out[1] = CHUNK;
  out[2] = TILE;
  out[3] = RING_LIMIT;
  out[4] = BIG_RING;
}

extern "C" int64_t c3d_rings_polis_ws_bytes(int32_t max_rings_p, int32_t max_vertices_p, int32_t max_p, int32_t max_rings_g,
                                            int32_t max_vertices_g, int32_t max_g) {
  const int rc = refuse(max_rings_p, max_vertices_p, max_p, max_rings_g, max_vertices_g, max_g);
  if (rc) return rc;
  return plan_of(max_rings_p, max_vertices_p, max_p, max_rings_g, max_vertices_g, max_g).bytes;
}

extern "C" int c3d_rings_polis(const int32_t* rings_p, const int32_t* vertices_p, const int32_t* counts_p, int32_t max_rings_p,
                               int32_t max_vertices_p, int32_t frac_bits_p, const int32_t* rings_g, const int32_t* vertices_g,
                               const int32_t* counts_g, int32_t max_rings_g, int32_t max_vertices_g, int32_t frac_bits_g,
                               const int32_t* match_p, int32_t max_p, int32_t max_g, int64_t max_pair_work, double* pair,
                               int32_t* pair_n, int64_t* counts, double* sums, int64_t* totals, double* total_sums, void* ws,
                               void* stream) {
  if (!rings_p || !vertices_p || !counts_p || !rings_g || !vertices_g || !counts_g || !match_p || !pair || !pair_n || !counts ||
      !sums || !ws)
    return C3D_E_BADARG;
  if (frac_bits_p < 0 || frac_bits_p > 8 || frac_bits_g < 0 || frac_bits_g > 8 || max_pair_work < 0) return C3D_E_BADARG;
  int rc = refuse(max_rings_p, max_vertices_p, max_p, max_rings_g, max_vertices_g, max_g);
  if (rc) return rc;
  Plan pl = plan_of(max_rings_p, max_vertices_p, max_p, max_rings_g, max_vertices_g, max_g);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  const int F = frac_bits_p > frac_bits_g ? frac_bits_p : frac_bits_g;
  Sides sd;
  for (int k = 0; k < 2; ++k) {
    sd.s[k] = pl.s[k];
    bind(sd.s[k], base);
  }
  sd.s[0].rings = rings_p; sd.s[0].vertices = reinterpret_cast<const int2*>(vertices_p); sd.s[0].counts = counts_p;
  sd.s[0].shift = F - frac_bits_p; sd.s[0].coord_max = (int64_t)COORD_UNIT << frac_bits_p;
  sd.s[1].rings = rings_g; sd.s[1].vertices = reinterpret_cast<const int2*>(vertices_g); sd.s[1].counts = counts_g;
  sd.s[1].shift = F - frac_bits_g; sd.s[1].coord_max = (int64_t)COORD_UNIT << frac_bits_g;
  uint32_t* header = reinterpret_cast<uint32_t*>(base);
  uint8_t* tier = reinterpret_cast<uint8_t*>(base + pl.tier);
  u64* job_start = reinterpret_cast<u64*>(base + pl.job_start);
  double2* partial = reinterpret_cast<double2*>(base + pl.partial);
  Out out{pair, pair_n, counts, sums, totals, total_sums};

  // the header and the per-id sums: every other word of the workspace is written by the call before the call reads it
  hipError_t e = hipMemsetAsync(base, 0, (size_t)pl.zero_bytes, st);
  if (e != hipSuccess) return (int)e;
  // the ring and pair counts are known on the device only: grids are sized by the maxima and surplus workgroups return
  const int more_rings = max_rings_p > max_rings_g ? max_rings_p : max_rings_g;
  rc = c3d_launch_lds<polis_rows_kernel>(dim3(grid_for(more_rings, 4), 2), dim3(256), 0, st, sd, header);
  if (rc) return rc;
  const int more_vertices = max_vertices_p > max_vertices_g ? max_vertices_p : max_vertices_g;
  const unsigned g_big = grid_for(more_vertices, 4 * 256) < 1024u ? grid_for(more_vertices, 4 * 256) : 1024u;
  rc = c3d_launch_lds<polis_check_big_kernel>(dim3(g_big, 2), dim3(256), 0, st, sd, (const uint32_t*)header);
  if (rc) return rc;
  rc = c3d_launch_lds<polis_ids_kernel>(dim3(2), dim3(SCAN_T), 2 * (SCAN_T / 64) * 8, st, sd, (const uint32_t*)header);
  if (rc) return rc;
  const int more_rows = more_rings > max_p ? more_rings : max_p;
  rc = c3d_launch_lds<polis_place_kernel>(dim3(grid_for(more_rows, 256), 2), dim3(256), 0, st, sd, (const uint32_t*)header, (int)max_p, pair,
                                          pair_n);
  if (rc) return rc;
  rc = c3d_launch_lds<polis_gather_kernel>(dim3(grid_for(more_rings, 4), 2), dim3(256), 0, st, sd);
  if (rc) return rc;
  rc = c3d_launch_lds<polis_gather_big_kernel>(dim3(g_big, 2), dim3(256), 0, st, sd, (const uint32_t*)header);
  if (rc) return rc;
  rc = c3d_launch_lds<polis_pairs_kernel>(dim3(1), dim3(SCAN_T), (SCAN_T / 64) * 8, st, sd, match_p, (int)max_p, (int)max_g, max_pair_work, pl.job_cap,
                                          tier, job_start, header, out);
  if (rc) return rc;
  rc = c3d_launch_lds<polis_jobs_kernel>(dim3(grid_for(pl.job_cap, 1)), dim3(BLOCK_T), (size_t)(TILE * 5 + 2 * BLOCK_T / 64) * 8, st, sd,
                                         (int)max_p, (const uint8_t*)tier, (const u64*)job_start, (const int32_t*)pair_n,
                                         (const uint32_t*)header, partial);
  if (rc) return rc;
  rc = c3d_launch_lds<polis_score_kernel>(dim3(grid_for(max_p, 4)), dim3(256), 0, st, sd, (int)max_p, F, (const uint8_t*)tier,
                                          (const u64*)job_start, (const uint32_t*)header, (const double2*)partial, out);
  if (rc) return rc;
  return c3d_launch_lds<polis_totals_kernel>(dim3(1), dim3(256), 10 * 256 * 8, st, sd, (int)max_p, (const uint32_t*)header, out);
}
