// Polygon validity of a ring table: for every object id the proper crossings, collinear overlaps and touches among its own
// edges, while the table stays in HBM.  The rule -- the rows used, the edges of an id, which pairs are adjacent, the class of a
// pair, which ids are checked -- is the header's (include/change3d_hip.h); this file is one way to compute it.  Everything is
// an integer: coordinate differences stay below 2^25 and every cross or dot product below 2^51, so the doubles that carry them
// are exact and only their signs and orders are used.  No workgroup waits for another, nothing is read back, every loop is
// capped, and every sum is an integer atomic or a ballot count, whose result does not depend on their order.
//
// Steps 1-4 regroup the rows into per-id edge lists; their bodies are csrc/scene_rings.h's, shared by every consumer of a
// ring table:
//
//   1 rows     a wave per ring row: classifies the row and adds it to its id (ring count, vertex count, the incomplete mark)
//     check    the coordinates of the rings above BIG_RING vertices, which kernel 1 only lists: many workgroups, a chunk each
//   2 ids      one workgroup: exclusive scans over the ids up to the largest one seen: where an id's rings are listed, where
//              its edges go
//   3 place    a thread per row: claims a slot in the ring list of its id; also zeroes the output rows past the last id
//   4 gather   a wave per row: the row's place among the edges of its id = the n of the listed rings with a smaller row index;
//              then writes its edges (a, b) to that place, next to each a packed (place of the ring, n) that adjacency needs,
//              and counts the degenerate ones
//     gather   the same for the rings above BIG_RING: many workgroups, a chunk each
//   5 plan     one workgroup: every id's flag, m and tier, the first four columns of its output row; the ids of the job tier
//              get their jobs by a scan
//   6 jobs     a workgroup per (id, chunk i of CHUNK edges): a thread per edge, the chunks i, i+1, .., i + floor(c/2) (mod c)
//              pass through LDS a TILE at a time; four counters per thread, a wave sum, one integer atomic per wave and counter
//   7 score    a wave per id: the wave tier (at most WAVE_LIMIT edges: a lane per edge, the other edge by shuffle, counts by
//              ballot) or the sums of the id's jobs; writes the last four columns of the row
//   8 tail     one workgroup: counts and totals
#include <climits>

#include "scene_host.h"
#include "scene_rings.h"

namespace {

using namespace c3d_rings;
using c3d_host::grid_for;

constexpr int WAVE_LIMIT = 64;                             // edges of an id in the wave tier: a lane each
constexpr int CHUNK = 256;                                 // edges of a chunk: a thread each
constexpr int TILE = 256;                                  // edges of an LDS tile: 24 bytes each; a chunk is one tile
constexpr int BLOCK_T = 256;
constexpr int MAX_GRID = 4096;

enum : uint8_t { TIER_NONE = 0, TIER_WAVE = 1, TIER_JOB = 2 };

// words of the workspace header (256 bytes, zeroed by the call's memset)
enum { WS_K = 1, WS_JOBS = 2, WS_BIG = 3 };                // the largest id of a row, the jobs, the long rings

struct Tab : Lists {
  uint32_t* id_degen;                                      // [max_ids] edges with a == b
  u64* acc;                                                // [max_ids][4] what the jobs add up: cross, overlap, vv, ve
  int4* edges;                                             // [max_vertices] (a.x, a.y, b.x, b.y) grouped by id
  u64* meta;                                               // [max_vertices] place of the edge's ring in the id's list | n << 32
  uint8_t* tier;                                           // [max_ids]
  u64* job_start;                                          // [max_ids]
};

struct Plan {
  Tab t;
  int64_t zero_bytes, job_cap, bytes;
};

// ws: the workspace, or nullptr where only the sizes are asked for
Plan plan_of(void* ws, int64_t max_rings, int64_t max_vertices, int64_t max_ids) {
  Plan pl{};
  c3d_host::Layout l{static_cast<char*>(ws), 256};
  Tab& t = pl.t;
  l.take(t.id_rings, max_ids * 4);                         // zeroed part first
  l.take(t.id_verts, max_ids * 8);
  l.take(t.id_flags, max_ids * 4);
  l.take(t.id_claim, max_ids * 4);
  l.take(t.id_degen, max_ids * 4);
  l.take(t.acc, max_ids * 32);
  pl.zero_bytes = l.at;
  l.take(t.kind, max_rings);
  l.take(t.list, max_rings * 8);
  l.take(t.big, max_rings * 4);
  l.take(t.row_at, max_rings * 4);
  l.take(t.id_list, max_ids * 4);
  l.take(t.id_start, max_ids * 4);
  l.take(t.edges, max_vertices * 16);
  l.take(t.meta, max_vertices * 8);
  l.take(t.tier, max_ids);
  l.take(t.job_start, max_ids * 8);
  // the chunks of the ids add up to at most this whatever the table holds: the edges of all ids fit in max_vertices
  pl.job_cap = (max_vertices + CHUNK - 1) / CHUNK + max_ids;
  pl.bytes = l.at;
  t.max_rings = (int)max_rings; t.max_vertices = (int)max_vertices; t.max_ids = (int)max_ids;
  if (ws) {
    t.top = static_cast<uint32_t*>(ws) + WS_K;
    t.n_big = static_cast<uint32_t*>(ws) + WS_BIG;
  }
  return pl;
}

// edges at the places i and j of an id's list, with the packed (place of the ring, n) of each
__device__ __forceinline__ bool adjacent_of(uint32_t i, u64 mi, uint32_t j, u64 mj) {
  if ((uint32_t)mi != (uint32_t)mj) return false;          // another ring
  const uint32_t d = i > j ? i - j : j - i, n = (uint32_t)(mi >> 32);
  return d == 1u || d == n - 1u;
}

// ------------------------------------------------------------------------------------------- 1 - 4: scene_rings.h's passes
__global__ __launch_bounds__(256) void valid_rows_kernel(Tab s) { rows_pass(s); }
__global__ __launch_bounds__(256) void valid_check_big_kernel(Tab s) { check_big_pass(s); }
__global__ __launch_bounds__(SCAN_T) void valid_ids_kernel(Tab s) {
  extern __shared__ u64 part_ids[];                        // [2][SCAN_T / 64]
  ids_pass(s, reinterpret_cast<u64(*)[SCAN_T / 64]>(part_ids));
}

__global__ __launch_bounds__(256) void valid_place_kernel(Tab s, int64_t* __restrict__ valid) {
  // the rows past the last id: 8 words each, a thread per word
  const int64_t words = (int64_t)s.max_ids * 8;
  for (int64_t w = (int64_t)top_of(s) * 8 + (int64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (int64_t)gridDim.x * 256)
    valid[w] = 0;
  place_pass(s);
}

// an edge as it is, next to it the packed (place of the ring, n) that adjacency needs; the degenerate ones are counted
struct EdgeWriter {
  static constexpr bool COUNTS = true;
  int4* edges;
  u64* meta;
  uint32_t* id_degen;
  __device__ __forceinline__ bool edge(u64 at, u64 before, int n, int2 a, int2 b) const {
    edges[at] = make_int4(a.x, a.y, b.x, b.y);
    meta[at] = before | ((u64)(uint32_t)n << 32);
    return a.x == b.x && a.y == b.y;
  }
  __device__ __forceinline__ void counted(int id, uint32_t c) const { atomicAdd(id_degen + (id - 1), c); }
};
__global__ __launch_bounds__(256) void valid_gather_kernel(Tab s) { gather_pass(s, EdgeWriter{s.edges, s.meta, s.id_degen}); }
__global__ __launch_bounds__(256) void valid_gather_big_kernel(Tab s) { gather_big_pass(s, EdgeWriter{s.edges, s.meta, s.id_degen}); }

// --------------------------------------------------------------------------------------------------------------- 5: plan
__global__ __launch_bounds__(SCAN_T) void valid_plan_kernel(Tab s, int64_t max_id_work, int64_t job_cap, uint32_t* __restrict__ header,
                                                            int64_t* __restrict__ valid) {
  extern __shared__ u64 part[];                            // [SCAN_T / 64]
  const int top = clampi((int)header[WS_K], 0, s.max_ids);
  u64 running = 0;
  for (int base = 0; base < top; base += SCAN_T) {
    const int i = base + (int)threadIdx.x;
    u64 jobs = 0, nv = 0, m = 0;
    uint32_t degen = 0, rings = 0;
    int flag = 0;
    if (i < top) {
      nv = s.id_verts[i];
      rings = s.id_rings[i];
      degen = s.id_degen[i];
      m = nv - (u64)degen;                                 // degen <= nv < 2^31
      if (s.id_flags[i] & ID_INCOMPLETE) flag = 2;
      else if (m == 0) flag = 1;
      else if (m * (m - 1) / 2 > (u64)max_id_work) flag = 3;
      else if (nv > (u64)WAVE_LIMIT) jobs = (nv + CHUNK - 1) / CHUNK;
    }
    u64 all;
    const u64 before = block_excl_scan64(jobs, part, &all);
    if (i < top) {
      s.job_start[i] = running + before;                   // the chunks of all ids stay below job_cap: see plan_of
      s.tier[i] = flag ? TIER_NONE : (jobs ? TIER_JOB : TIER_WAVE);
      int64_t* row = valid + (int64_t)i * 8;
      row[0] = flag; row[1] = rings; row[2] = (int64_t)m; row[3] = degen;
      row[4] = 0; row[5] = 0; row[6] = 0; row[7] = 0;
    }
    running += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) header[WS_JOBS] = (uint32_t)(running < (u64)job_cap ? running : (u64)job_cap);
}

// --------------------------------------------------------------------------------------------------------------- 6: jobs
// The job (id, chunk i) of an id of c chunks compares chunk i with the chunks i, i + 1, .., i + floor(c / 2) (mod c): every
// unordered pair of chunks belongs to exactly one job.  For even c the offset c / 2 joins i and i + c / 2 from both ends, so
// only i < c / 2 takes it; inside chunk i itself a thread takes the partners with a larger index.
__global__ __launch_bounds__(BLOCK_T) void valid_jobs_kernel(Tab s, const uint32_t* __restrict__ header) {
  extern __shared__ int4 t_edge[];                         // [TILE], then u64 [TILE]: dynamic, as the launcher raises the kernel's
  u64* t_meta = reinterpret_cast<u64*>(t_edge + TILE);     // LDS limit to the CU's
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t n_jobs = header[WS_JOBS];
  const int top = clampi((int)header[WS_K], 0, s.max_ids);
  for (uint32_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
    int lo = 0, hi = top;                                  // the last id whose first job is <= job: at most 32 steps
    for (int step = 0; step < 32 && hi - lo > 1; ++step) {
      const int mid = (lo + hi) >> 1;
      if (s.job_start[mid] <= (u64)job) lo = mid; else hi = mid;
    }
    const int id0 = lo;
    if (id0 >= top || s.tier[id0] != TIER_JOB) continue;
    const u64 nv = s.id_verts[id0];
    const u64 c = (nv + CHUNK - 1) / CHUNK, i = (u64)job - s.job_start[id0];
    if (i >= c) continue;
    const int4* edges = s.edges + s.id_start[id0];
    const u64* meta = s.meta + s.id_start[id0];
    const u64 k = i * CHUNK + (u64)tid;
    int4 own = make_int4(0, 0, 0, 0);
    u64 own_meta = 0;
    if (k < nv) { own = edges[k]; own_meta = meta[k]; }
    const bool live = live_of(own);                        // false past the end
    uint32_t n_cross = 0, n_over = 0, n_vv = 0, n_ve = 0;
    const u64 half = c / 2;
    for (u64 kk = 0; kk <= half; ++kk) {                   // at most max_vertices / (2 CHUNK) + 1 steps
      if (kk * 2 == c && i >= half) break;
      const u64 base = ((i + kk) % c) * CHUNK;
      const int cnt = nv - base < (u64)TILE ? (int)(nv - base) : TILE;
      __syncthreads();                                     // the tile before has been read
      if (tid < cnt) { t_edge[tid] = edges[base + tid]; t_meta[tid] = meta[base + tid]; }
      else t_edge[tid] = make_int4(0, 0, 0, 0);            // past the end: a degenerate edge, which takes part in no pair
      __syncthreads();
      const int first = !live ? TILE : (kk == 0 ? tid + 1 : 0);   // the diagonal chunk: partners with a larger index only
      for (int t0 = 0; t0 < cnt; t0 += 4) {                // four partners at a time: the same addresses in every lane, four
        int4 q[4];                                         // LDS reads in flight, one wave-uniform branch for the four
        bool near[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          q[u] = t_edge[t0 + u];                           // TILE is a multiple of 4 and the tile is padded
          near[u] = t0 + u >= first && live_of(q[u]) && boxes_meet(own, q[u]);
        }
        if (!__any(near[0] || near[1] || near[2] || near[3])) continue;   // most partners are far away
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (near[u]) {
            const int t = t0 + u;
            const int cls = pair_class(own, q[u], adjacent_of((uint32_t)k, own_meta, (uint32_t)(base + t), t_meta[t]));
            n_cross += cls == PAIR_CROSS;
            n_over += cls == PAIR_OVERLAP;
            n_vv += cls == PAIR_VV;
            n_ve += cls == PAIR_VE;
          }
        }
      }
    }
    u64 sum[4] = {n_cross, n_over, n_vv, n_ve};
    for (int q = 0; q < 4; ++q) {
      for (int o = 32; o > 0; o >>= 1) sum[q] += shfl64(sum[q], lane ^ o);
      if (lane == 0 && sum[q]) atomicAdd(s.acc + (int64_t)id0 * 4 + q, sum[q]);
    }
  }
}

// -------------------------------------------------------------------------------------------------------------- 7: score
__global__ __launch_bounds__(256) void valid_score_kernel(Tab s, const uint32_t* __restrict__ header, int64_t* __restrict__ valid) {
  const int lane = threadIdx.x & 63;
  const int top = clampi((int)header[WS_K], 0, s.max_ids);
  for (int i = blockIdx.x * 4 + (int)(threadIdx.x >> 6); i < top; i += gridDim.x * 4) {   // i is uniform over the wave
    const int what = s.tier[i];
    if (what == TIER_NONE) continue;
    u64 out[4] = {0, 0, 0, 0};
    if (what == TIER_WAVE) {
      const int nv = (int)s.id_verts[i];                   // at most WAVE_LIMIT
      int4 own = make_int4(0, 0, 0, 0);
      u64 own_meta = 0;
      if (lane < nv) { own = s.edges[(u64)s.id_start[i] + lane]; own_meta = s.meta[(u64)s.id_start[i] + lane]; }
      const bool live = live_of(own);
      // rotation r pairs lane l with lane (l + r) mod 64; the pair counts where l is the smaller one, so each unordered pair
      // is visited once over r = 1 .. 63.  Partners at nv and beyond hold no edge: r < nv reaches every pair that does
      for (int r = 1; r < nv; ++r) {
        const int other = (lane + r) & 63;
        const int4 q = make_int4(__shfl(own.x, other), __shfl(own.y, other), __shfl(own.z, other), __shfl(own.w, other));
        const u64 q_meta = shfl64(own_meta, other);
        int cls = PAIR_NONE;
        const bool near = live && lane < other && live_of(q) && boxes_meet(own, q);
        if (__any(near)) {                                 // uniform over the wave
          if (near) cls = pair_class(own, q, adjacent_of((uint32_t)lane, own_meta, (uint32_t)other, q_meta));
        }
        out[0] += (u64)__popcll(__ballot(cls == PAIR_CROSS));
        out[1] += (u64)__popcll(__ballot(cls == PAIR_OVERLAP));
        out[2] += (u64)__popcll(__ballot(cls == PAIR_VV));
        out[3] += (u64)__popcll(__ballot(cls == PAIR_VE));
      }
    } else {
      for (int q = 0; q < 4; ++q) out[q] = s.acc[(int64_t)i * 4 + q];
    }
    if (lane < 4) valid[(int64_t)i * 8 + 4 + lane] = (int64_t)(lane == 0 ? out[0] : lane == 1 ? out[1] : lane == 2 ? out[2] : out[3]);
  }
}

// --------------------------------------------------------------------------------------------------------------- 8: tail
__global__ __launch_bounds__(256) void valid_tail_kernel(Tab s, const uint32_t* __restrict__ header, const int64_t* __restrict__ valid,
                                                          int64_t* __restrict__ counts, int64_t* __restrict__ totals) {
  extern __shared__ long long s_tail[];                    // [7][256]
  long long(*s_i)[256] = reinterpret_cast<long long(*)[256]>(s_tail);
  const int tid = threadIdx.x;
  const int top = clampi((int)header[WS_K], 0, s.max_ids);
  long long c[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int i = tid; i < top; i += 256) {
    const int64_t* row = valid + (int64_t)i * 8;
    const int flag = (int)row[0];
    if (flag == 0) {
      c[0] += 1;
      c[1] += (row[4] != 0 || row[5] != 0) ? 1 : 0;
      c[5] += row[4];
      c[6] += row[5];
    } else {
      c[1 + flag] += 1;                                    // 1 empty, 2 incomplete, 3 over work
    }
  }
  for (int k = 0; k < 7; ++k) s_i[k][tid] = c[k];
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d)
      for (int k = 0; k < 7; ++k) s_i[k][tid] += s_i[k][tid + d];
    __syncthreads();
  }
  if (tid == 0) {
    const int64_t status = (int64_t)(uint32_t)s.counts[4];
    for (int k = 0; k < 7; ++k) counts[k] = s_i[k][0];
    counts[7] = status;
    if (totals) {
      for (int k = 0; k < 7; ++k) totals[k] += s_i[k][0];
      totals[7] |= status;
    }
  }
}

int refuse(int32_t max_rings, int32_t max_vertices, int32_t max_ids) {
  if (max_rings < 1 || max_vertices < 1 || max_ids < 1) return C3D_E_BADARG;
  return 0;
}

}  // namespace

extern "C" void c3d_rings_valid_limits(int32_t out[5]) {
  if (!out) return;
  out[0] = WAVE_LIMIT;
  out[1] = CHUNK;
  out[2] = TILE;
  out[3] = RING_LIMIT;
  out[4] = BIG_RING;
}

extern "C" int64_t c3d_rings_valid_ws_bytes(int32_t max_rings, int32_t max_vertices, int32_t max_ids) {
  const int rc = refuse(max_rings, max_vertices, max_ids);
  if (rc) return rc;
  return plan_of(nullptr, max_rings, max_vertices, max_ids).bytes;
}

extern "C" int c3d_rings_valid(const int32_t* rings, const int32_t* vertices, const int32_t* counts_in, int32_t max_rings,
                               int32_t max_vertices, int32_t frac_bits, int32_t max_ids, int64_t max_id_work, int64_t* valid,
                               int64_t* counts, int64_t* totals, void* ws, void* stream) {
  if (!rings || !vertices || !counts_in || !valid || !counts || !ws) return C3D_E_BADARG;
  if (frac_bits < 0 || frac_bits > 8 || max_id_work < 0) return C3D_E_BADARG;
  int rc = refuse(max_rings, max_vertices, max_ids);
  if (rc) return rc;
  const Plan pl = plan_of(ws, max_rings, max_vertices, max_ids);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Tab s = pl.t;
  s.rings = rings; s.vertices = reinterpret_cast<const int2*>(vertices); s.counts = counts_in;
  s.coord_max = (int64_t)COORD_UNIT << frac_bits;
  uint32_t* header = static_cast<uint32_t*>(ws);
  const uint32_t* hdr = header;

  // the header, the per-id sums and what the jobs add into: every other word of the workspace is written by the call before
  // the call reads it
  hipError_t e = hipMemsetAsync(ws, 0, (size_t)pl.zero_bytes, st);
  if (e != hipSuccess) return (int)e;
  // the ring and id counts are known on the device only: grids are sized by the maxima and surplus workgroups return
  const unsigned g_rows = grid_for(max_rings, 4, MAX_GRID), g_big = grid_for(max_vertices, 4 * 256, 1024);
  rc = c3d_launch_lds<valid_rows_kernel>(dim3(g_rows), dim3(256), 0, st, s);
  if (rc) return rc;
  rc = c3d_launch_lds<valid_check_big_kernel>(dim3(g_big), dim3(256), 0, st, s);
  if (rc) return rc;
  rc = c3d_launch_lds<valid_ids_kernel>(dim3(1), dim3(SCAN_T), 2 * (SCAN_T / 64) * 8, st, s);
  if (rc) return rc;
  const int64_t more_rows = (int64_t)max_ids * 8 > max_rings ? (int64_t)max_ids * 8 : max_rings;
  rc = c3d_launch_lds<valid_place_kernel>(dim3(grid_for(more_rows, 256, MAX_GRID)), dim3(256), 0, st, s, valid);
  if (rc) return rc;
  rc = c3d_launch_lds<valid_gather_kernel>(dim3(g_rows), dim3(256), 0, st, s);
  if (rc) return rc;
  rc = c3d_launch_lds<valid_gather_big_kernel>(dim3(g_big), dim3(256), 0, st, s);
  if (rc) return rc;
  rc = c3d_launch_lds<valid_plan_kernel>(dim3(1), dim3(SCAN_T), (SCAN_T / 64) * 8, st, s, max_id_work, pl.job_cap, header, valid);
  if (rc) return rc;
  rc = c3d_launch_lds<valid_jobs_kernel>(dim3(grid_for(pl.job_cap, 1, MAX_GRID)), dim3(BLOCK_T), (size_t)TILE * 24, st, s, hdr);
  if (rc) return rc;
  rc = c3d_launch_lds<valid_score_kernel>(dim3(grid_for(max_ids, 4, MAX_GRID)), dim3(256), 0, st, s, hdr, valid);
  if (rc) return rc;
  return c3d_launch_lds<valid_tail_kernel>(dim3(1), dim3(256), 7 * 256 * 8, st, s, hdr, (const int64_t*)valid, counts, totals);
}
