// Polygon scores of a scene map: PoLiS, the vertex-to-boundary Hausdorff distance and the vertex counts of every matched pair
// (predicted object, ground-truth object) from two ring tables and the match_p of c3d_objects_match while all of them stay in
// HBM.  The rule -- the rows used, the geometry of an id, the distance of a point to an edge, which pairs are scored -- is the
// header's (include/change3d_hip.h); this file is one way to compute it.  Integers decide everything but the distances; every
// integer quantity of a distance is exact in a double.  No workgroup waits for another, nothing is read back, every loop is
// capped, and no floating-point sum depends on scheduling.
//
// Steps 1-4 regroup the rows of either side into per-id edge lists; their bodies are csrc/scene_rings.h's, shared by every
// consumer of a ring table, and run here once for both sides (blockIdx.y, or blockIdx.x of the ids scan, is the side):
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

#include "scene_host.h"
#include "scene_rings.h"

namespace {

using namespace c3d_rings;
using c3d_host::grid_for;

constexpr int WAVE_LIMIT = 64;                             // vertices of either side in the wave tier: a lane each
constexpr int CHUNK = 256;                                 // vertices of a job: a thread each
constexpr int TILE = 512;                                  // edges of an LDS tile: 40 bytes each
constexpr int BLOCK_T = 256;
constexpr int MAX_GRID = 4096;
constexpr double GUARD = 1.0 + 0x1p-50;                    // see edge_update

enum : uint8_t { TIER_NONE = 0, TIER_WAVE = 1, TIER_JOB = 2 };

// words of the workspace header (256 bytes, zeroed by the call's memset)
enum { WS_STATUS = 0, WS_KP = 1, WS_KG = 2, WS_JOBS = 3, WS_BIG_P = 4, WS_BIG_G = 5 };   // WS_KP + side = the largest id of a row of
                                                                                      // that side, WS_BIG_P + side = its long rings

struct Side : Lists {
  int shift;                                               // F - frac_bits
  int4* edges;                                             // [max_vertices] (a.x, a.y, b.x, b.y) grouped by id
};

struct Sides {
  Side s[2];
};

struct Plan {
  Sides sd;
  int64_t zero_bytes;                                      // the header and the per-id words the memset clears
  uint8_t* tier;                                           // [max_p]
  u64* job_start;                                          // [max_p]
  double2* partial;                                        // [job_cap]
  int64_t job_cap, bytes;
};

// ws: the workspace, or nullptr where only the sizes are asked for
Plan plan_of(void* ws, int64_t max_rings_p, int64_t max_vertices_p, int64_t max_p, int64_t max_rings_g, int64_t max_vertices_g,
             int64_t max_g) {
  Plan pl{};
  c3d_host::Layout l{static_cast<char*>(ws), 256};
  const int64_t rings[2] = {max_rings_p, max_rings_g}, verts[2] = {max_vertices_p, max_vertices_g}, ids[2] = {max_p, max_g};
  for (int k = 0; k < 2; ++k) {                            // zeroed part first
    Side& s = pl.sd.s[k];
    l.take(s.id_rings, ids[k] * 4);
    l.take(s.id_verts, ids[k] * 8);
    l.take(s.id_flags, ids[k] * 4);
    l.take(s.id_claim, ids[k] * 4);
  }
  pl.zero_bytes = l.at;
  for (int k = 0; k < 2; ++k) {
    Side& s = pl.sd.s[k];
    l.take(s.kind, rings[k]);
    l.take(s.list, rings[k] * 8);
    l.take(s.id_list, ids[k] * 4);
    l.take(s.id_start, ids[k] * 4);
    l.take(s.edges, verts[k] * 16);
    l.take(s.big, rings[k] * 4);
    l.take(s.row_at, rings[k] * 4);
    s.max_rings = (int)rings[k]; s.max_vertices = (int)verts[k]; s.max_ids = (int)ids[k];
    if (ws) {
      s.top = static_cast<uint32_t*>(ws) + WS_KP + k;
      s.n_big = static_cast<uint32_t*>(ws) + WS_BIG_P + k;
    }
  }
  l.take(pl.tier, max_p);
  l.take(pl.job_start, max_p * 8);
  // enough for every pair of a match that names no ground-truth id twice
  pl.job_cap = (max_vertices_p + CHUNK - 1) / CHUNK + (max_vertices_g + CHUNK - 1) / CHUNK + 2 * max_p;
  l.take(pl.partial, pl.job_cap * 16);
  pl.bytes = l.at;
  return pl;
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

// ------------------------------------------------------------------------------------------- 1 - 4: scene_rings.h's passes
__global__ __launch_bounds__(256) void polis_rows_kernel(Sides sd) { rows_pass(sd.s[blockIdx.y]); }
__global__ __launch_bounds__(256) void polis_check_big_kernel(Sides sd) { check_big_pass(sd.s[blockIdx.y]); }
__global__ __launch_bounds__(SCAN_T) void polis_ids_kernel(Sides sd) {
  extern __shared__ u64 part_ids[];                        // [2][SCAN_T / 64]: dynamic, as the launcher raises the kernel's LDS
  ids_pass(sd.s[blockIdx.x], reinterpret_cast<u64(*)[SCAN_T / 64]>(part_ids));   // limit to the CU's
}

__global__ __launch_bounds__(256) void polis_place_kernel(Sides sd, int max_p, double* __restrict__ pair, int32_t* __restrict__ pair_n) {
  if (blockIdx.y == 0) {                                   // the rows past the last predicted object
    for (int p = clampi((int)*sd.s[0].top, 0, max_p) + blockIdx.x * 256 + (int)threadIdx.x; p < max_p; p += gridDim.x * 256) {
      reinterpret_cast<int4*>(pair_n)[p] = make_int4(0, 0, 0, 0);
      double2* row = reinterpret_cast<double2*>(pair + (int64_t)p * 4);
      row[0] = make_double2(0.0, 0.0);
      row[1] = make_double2(0.0, 0.0);
    }
  }
  place_pass(sd.s[blockIdx.y]);
}

// an edge shifted to the common unit of the two sides
struct EdgeWriter {
  static constexpr bool COUNTS = false;
  int4* edges;
  int scale;                                               // |coordinate| * scale <= 2^23
  __device__ __forceinline__ bool edge(u64 at, u64, int, int2 a, int2 b) const {
    edges[at] = make_int4(a.x * scale, a.y * scale, b.x * scale, b.y * scale);
    return false;
  }
};
__global__ __launch_bounds__(256) void polis_gather_kernel(Sides sd) {
  const Side& s = sd.s[blockIdx.y];
  gather_pass(s, EdgeWriter{s.edges, 1 << s.shift});
}
__global__ __launch_bounds__(256) void polis_gather_big_kernel(Sides sd) {
  const Side& s = sd.s[blockIdx.y];
  gather_big_pass(s, EdgeWriter{s.edges, 1 << s.shift});
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
    u64 all;
    const u64 before = block_excl_scan64(jobs, part, &all);
    if (i < kp) {
      const u64 at = running + before;
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
  return plan_of(nullptr, max_rings_p, max_vertices_p, max_p, max_rings_g, max_vertices_g, max_g).bytes;
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
  const Plan pl = plan_of(ws, max_rings_p, max_vertices_p, max_p, max_rings_g, max_vertices_g, max_g);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int F = frac_bits_p > frac_bits_g ? frac_bits_p : frac_bits_g;
  Sides sd = pl.sd;
  sd.s[0].rings = rings_p; sd.s[0].vertices = reinterpret_cast<const int2*>(vertices_p); sd.s[0].counts = counts_p;
  sd.s[0].shift = F - frac_bits_p; sd.s[0].coord_max = (int64_t)COORD_UNIT << frac_bits_p;
  sd.s[1].rings = rings_g; sd.s[1].vertices = reinterpret_cast<const int2*>(vertices_g); sd.s[1].counts = counts_g;
  sd.s[1].shift = F - frac_bits_g; sd.s[1].coord_max = (int64_t)COORD_UNIT << frac_bits_g;
  uint32_t* header = static_cast<uint32_t*>(ws);
  const uint32_t* hdr = header;
  Out out{pair, pair_n, counts, sums, totals, total_sums};

  // the header and the per-id sums: every other word of the workspace is written by the call before the call reads it
  hipError_t e = hipMemsetAsync(ws, 0, (size_t)pl.zero_bytes, st);
  if (e != hipSuccess) return (int)e;
  // the ring and pair counts are known on the device only: grids are sized by the maxima and surplus workgroups return
  const int more_rings = max_rings_p > max_rings_g ? max_rings_p : max_rings_g;
  const int more_vertices = max_vertices_p > max_vertices_g ? max_vertices_p : max_vertices_g;
  const int more_rows = more_rings > max_p ? more_rings : max_p;
  const unsigned g_rows = grid_for(more_rings, 4, MAX_GRID), g_big = grid_for(more_vertices, 4 * 256, 1024);
  rc = c3d_launch_lds<polis_rows_kernel>(dim3(g_rows, 2), dim3(256), 0, st, sd);
  if (rc) return rc;
  rc = c3d_launch_lds<polis_check_big_kernel>(dim3(g_big, 2), dim3(256), 0, st, sd);
  if (rc) return rc;
  rc = c3d_launch_lds<polis_ids_kernel>(dim3(2), dim3(SCAN_T), 2 * (SCAN_T / 64) * 8, st, sd);
  if (rc) return rc;
  rc = c3d_launch_lds<polis_place_kernel>(dim3(grid_for(more_rows, 256, MAX_GRID), 2), dim3(256), 0, st, sd, (int)max_p, pair, pair_n);
  if (rc) return rc;
  rc = c3d_launch_lds<polis_gather_kernel>(dim3(g_rows, 2), dim3(256), 0, st, sd);
  if (rc) return rc;
  rc = c3d_launch_lds<polis_gather_big_kernel>(dim3(g_big, 2), dim3(256), 0, st, sd);
  if (rc) return rc;
  rc = c3d_launch_lds<polis_pairs_kernel>(dim3(1), dim3(SCAN_T), (SCAN_T / 64) * 8, st, sd, match_p, (int)max_p, (int)max_g, max_pair_work, pl.job_cap,
                                          pl.tier, pl.job_start, header, out);
  if (rc) return rc;
  rc = c3d_launch_lds<polis_jobs_kernel>(dim3(grid_for(pl.job_cap, 1, MAX_GRID)), dim3(BLOCK_T), (size_t)(TILE * 5 + 2 * BLOCK_T / 64) * 8, st, sd,
                                         (int)max_p, (const uint8_t*)pl.tier, (const u64*)pl.job_start, (const int32_t*)pair_n, hdr,
                                         pl.partial);
  if (rc) return rc;
  rc = c3d_launch_lds<polis_score_kernel>(dim3(grid_for(max_p, 4, MAX_GRID)), dim3(256), 0, st, sd, (int)max_p, F, (const uint8_t*)pl.tier,
                                          (const u64*)pl.job_start, hdr, (const double2*)pl.partial, out);
  if (rc) return rc;
  return c3d_launch_lds<polis_totals_kernel>(dim3(1), dim3(256), 10 * 256 * 8, st, sd, (int)max_p, hdr, out);
}
