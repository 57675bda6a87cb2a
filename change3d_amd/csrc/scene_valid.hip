// Polygon validity of a ring table: for every object id the proper crossings, collinear overlaps and touches among its own
// edges, while the table stays in HBM.  The rule -- the rows used, the edges of an id, which pairs are adjacent, the class of a
// pair, which ids are checked -- is the header's (include/change3d_hip.h); this file is one way to compute it.  Everything is
// an integer: coordinate differences stay below 2^25 and every cross or dot product below 2^51, so the doubles that carry them
// are exact and only their signs and orders are used.  No workgroup waits for another, nothing is read back, every loop is
// capped, and every sum is an integer atomic or a ballot count, whose result does not depend on their order.
//
// Steps 1-4 regroup the rows into per-id edge lists as csrc/scene_polis.hip does for each of its two sides (one side here, no
// common unit; DESIGN.md says why the steps are repeated and not shared):
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
#include <type_traits>

#include "scene_rings.h"

namespace {

using namespace c3d_rings;                                 // the rows pass, the ids scan and pair_class: shared with
                                                           // csrc/scene_conflicts.hip

constexpr int WAVE_LIMIT = 64;                             // edges of an id in the wave tier: a lane each
constexpr int CHUNK = 256;                                 // edges of a chunk: a thread each
constexpr int TILE = 256;                                  // edges of an LDS tile: 24 bytes each; a chunk is one tile
constexpr int BLOCK_T = 256;
constexpr int MAX_GRID = 4096;

enum : uint8_t { TIER_NONE = 0, TIER_WAVE = 1, TIER_JOB = 2 };

// the workspace header is 256 bytes, zeroed by the call's memset; its words are those of scene_rings.h
struct Tab : Rows {
  uint2* list;                                             // [max_rings] (ring row, its n) grouped by id
  uint32_t* row_at;                                        // [max_rings] where such a ring's edges go within its id
  uint32_t* id_claim;                                      // [max_ids]
  uint32_t* id_degen;                                      // [max_ids] edges with a == b
  u64* acc;                                                // [max_ids][4] what the jobs add up: cross, overlap, vv, ve
  int4* edges;                                             // [max_vertices] (a.x, a.y, b.x, b.y) grouped by id
  u64* meta;                                               // [max_vertices] place of the edge's ring in the id's list | n << 32
  uint8_t* tier;                                           // [max_ids]
  u64* job_start;                                          // [max_ids]
};

struct Plan {
  Tab t;                                                   // offsets until bind() adds the base
  int64_t zero_bytes, job_cap, bytes;
};

Plan plan_of(int64_t max_rings, int64_t max_vertices, int64_t max_ids) {
  Plan pl{};
  auto up = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  int64_t at = 256;
  auto take = [&](auto*& p, int64_t bytes) {
    p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(at);
    at += up(bytes);
  };
  Tab& t = pl.t;
  take(t.id_rings, max_ids * 4);                           // zeroed part first
  take(t.id_verts, max_ids * 8);
  take(t.id_flags, max_ids * 4);
  take(t.id_claim, max_ids * 4);
  take(t.id_degen, max_ids * 4);
  take(t.acc, max_ids * 32);
  pl.zero_bytes = at;
  take(t.kind, max_rings);
  take(t.list, max_rings * 8);
  take(t.big, max_rings * 4);
  take(t.row_at, max_rings * 4);
  take(t.id_list, max_ids * 4);
  take(t.id_start, max_ids * 4);
  take(t.edges, max_vertices * 16);
  take(t.meta, max_vertices * 8);
  take(t.tier, max_ids);
  take(t.job_start, max_ids * 8);
  // the chunks of the ids add up to at most this whatever the table holds: the edges of all ids fit in max_vertices
  pl.job_cap = (max_vertices + CHUNK - 1) / CHUNK + max_ids;
  pl.bytes = at;
  t.max_rings = (int)max_rings; t.max_vertices = (int)max_vertices; t.max_ids = (int)max_ids;
  return pl;
}

template <class T> void rebase(T*& p, char* base) { p = reinterpret_cast<T*>(base + reinterpret_cast<intptr_t>(p)); }
void bind(Tab& t, char* base) {
  rebase(t.kind, base); rebase(t.list, base); rebase(t.big, base); rebase(t.row_at, base); rebase(t.id_rings, base);
  rebase(t.id_verts, base); rebase(t.id_flags, base); rebase(t.id_claim, base); rebase(t.id_degen, base); rebase(t.acc, base);
  rebase(t.id_list, base); rebase(t.id_start, base); rebase(t.edges, base); rebase(t.meta, base); rebase(t.tier, base);
  rebase(t.job_start, base);
}

// edges at the places i and j of an id's list, with the packed (place of the ring, n) of each
__device__ __forceinline__ bool adjacent_of(uint32_t i, u64 mi, uint32_t j, u64 mj) {
  if ((uint32_t)mi != (uint32_t)mj) return false;          // another ring
  const uint32_t d = i > j ? i - j : j - i, n = (uint32_t)(mi >> 32);
  return d == 1u || d == n - 1u;
}

// --------------------------------------------------------------------------------------------------------------- 1: rows
__global__ __launch_bounds__(256) void valid_rows_kernel(Tab s, uint32_t* __restrict__ header) {
  rows_pass(s, header);
}

__global__ __launch_bounds__(256) void valid_check_big_kernel(Tab s, const uint32_t* __restrict__ header) {
  check_big_pass(s, header);
}

// ---------------------------------------------------------------------------------------------------------------- 2: ids
// An id with more than RING_LIMIT rings, or whose edges no longer fit below max_vertices (only tables whose rows share
// vertices get there), becomes incomplete and takes no room.
__global__ __launch_bounds__(SCAN_T) void valid_ids_kernel(Tab s, const uint32_t* __restrict__ header) {
  extern __shared__ u64 part_ids[];                        // [2][SCAN_T / 64]
  ids_pass(s, header, reinterpret_cast<u64(*)[SCAN_T / 64]>(part_ids));
}

// -------------------------------------------------------------------------------------------------------------- 3: place
__global__ __launch_bounds__(256) void valid_place_kernel(Tab s, const uint32_t* __restrict__ header, int64_t* __restrict__ valid) {
  const int rows = rows_of(s);
  // the rows past the last id: 8 words each, a thread per word
  const int64_t words = (int64_t)s.max_ids * 8;
  for (int64_t w = (int64_t)clampi((int)header[WS_K], 0, s.max_ids) * 8 + (int64_t)blockIdx.x * 256 + threadIdx.x; w < words;
       w += (int64_t)gridDim.x * 256)
    valid[w] = 0;
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
__global__ __launch_bounds__(256) void valid_gather_kernel(Tab s) {
  const int rows = rows_of(s), lane = threadIdx.x & 63;
  for (int r = blockIdx.x * 4 + (int)(threadIdx.x >> 6); r < rows; r += gridDim.x * 4) {   // r is uniform over the wave
    if (s.kind[r] != ROW_USED) continue;
    const int id = s.rings[(int64_t)r * 8], n = s.rings[(int64_t)r * 8 + 2];
    const int64_t start = s.rings[(int64_t)r * 8 + 1];
    const int k = (int)s.id_rings[id - 1];                 // at most RING_LIMIT
    if (!k) continue;
    const uint2* list = s.list + s.id_list[id - 1];
    u64 before = 0;                                        // edges of the id's rings with a smaller row index
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
    const u64 at = (u64)s.id_start[id - 1] + before;       // id_start + total <= max_vertices
    const u64 meta = before | ((u64)(uint32_t)n << 32);
    uint32_t degen = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {                   // uniform trip count: the ballot sees every lane
      const int j = j0 + lane;
      bool dead = false;
      if (j < n) {
        const int2 a = s.vertices[start + j], b = s.vertices[start + (j + 1 < n ? j + 1 : 0)];
        s.edges[at + j] = make_int4(a.x, a.y, b.x, b.y);
        s.meta[at + j] = meta;
        dead = a.x == b.x && a.y == b.y;
      }
      degen += (uint32_t)__popcll(__ballot(dead));
    }
    if (degen && lane == 0) atomicAdd(s.id_degen + (id - 1), degen);
  }
}

__global__ __launch_bounds__(256) void valid_gather_big_kernel(Tab s, const uint32_t* __restrict__ header) {
  const uint32_t n_big = min(header[WS_BIG], (uint32_t)s.max_rings);
  const int lane = threadIdx.x & 63;
  for (uint32_t li = 0; li < n_big; ++li) {
    const int r = (int)s.big[li];
    if (s.kind[r] != ROW_USED) continue;
    const int id = s.rings[(int64_t)r * 8], n = s.rings[(int64_t)r * 8 + 2];
    const int64_t start = s.rings[(int64_t)r * 8 + 1];
    if (!s.id_rings[id - 1]) continue;                     // the id became incomplete
    const u64 before = s.row_at[r];
    if (before + (u64)n > s.id_verts[id - 1]) continue;    // cannot happen
    const u64 at = (u64)s.id_start[id - 1] + before;
    const u64 meta = before | ((u64)(uint32_t)n << 32);
    uint32_t degen = 0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
      const int2 a = s.vertices[start + j], b = s.vertices[start + (j + 1 < n ? j + 1 : 0)];
      s.edges[at + j] = make_int4(a.x, a.y, b.x, b.y);
      s.meta[at + j] = meta;
      degen += (a.x == b.x && a.y == b.y) ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) degen += (uint32_t)__shfl((int)degen, lane ^ o);
    if (degen && lane == 0) atomicAdd(s.id_degen + (id - 1), degen);
  }
}

// --------------------------------------------------------------------------------------------------------------- 5: plan
__global__ __launch_bounds__(SCAN_T) void valid_plan_kernel(Tab s, int64_t max_id_work, int64_t job_cap, uint32_t* __restrict__ header,
                                                            int64_t* __restrict__ valid) {
  extern __shared__ u64 part[];                            // [SCAN_T / 64]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
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
    if (i < top) {
      s.job_start[i] = running + before + inc - jobs;      // the chunks of all ids stay below job_cap: see plan_of
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

unsigned grid_for(int64_t items, int per_block) {
  int64_t g = (items + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > MAX_GRID ? MAX_GRID : g));
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
  return plan_of(max_rings, max_vertices, max_ids).bytes;
}

extern "C" int c3d_rings_valid(const int32_t* rings, const int32_t* vertices, const int32_t* counts_in, int32_t max_rings,
                               int32_t max_vertices, int32_t frac_bits, int32_t max_ids, int64_t max_id_work, int64_t* valid,
                               int64_t* counts, int64_t* totals, void* ws, void* stream) {
  if (!rings || !vertices || !counts_in || !valid || !counts || !ws) return C3D_E_BADARG;
  if (frac_bits < 0 || frac_bits > 8 || max_id_work < 0) return C3D_E_BADARG;
  int rc = refuse(max_rings, max_vertices, max_ids);
  if (rc) return rc;
  Plan pl = plan_of(max_rings, max_vertices, max_ids);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  Tab s = pl.t;
  bind(s, base);
  s.rings = rings; s.vertices = reinterpret_cast<const int2*>(vertices); s.counts = counts_in;
  s.coord_max = (int64_t)COORD_UNIT << frac_bits;
  uint32_t* header = reinterpret_cast<uint32_t*>(base);

  // the header, the per-id sums and what the jobs add into: every other word of the workspace is written by the call before
  // the call reads it
  hipError_t e = hipMemsetAsync(base, 0, (size_t)pl.zero_bytes, st);
  if (e != hipSuccess) return (int)e;
  // the ring and id counts are known on the device only: grids are sized by the maxima and surplus workgroups return
  rc = c3d_launch_lds<valid_rows_kernel>(dim3(grid_for(max_rings, 4)), dim3(256), 0, st, s, header);
  if (rc) return rc;
  const unsigned g_big = grid_for(max_vertices, 4 * 256) < 1024u ? grid_for(max_vertices, 4 * 256) : 1024u;
  rc = c3d_launch_lds<valid_check_big_kernel>(dim3(g_big), dim3(256), 0, st, s, (const uint32_t*)header);
  if (rc) return rc;
  rc = c3d_launch_lds<valid_ids_kernel>(dim3(1), dim3(SCAN_T), 2 * (SCAN_T / 64) * 8, st, s, (const uint32_t*)header);
  if (rc) return rc;
  const int64_t more_rows = (int64_t)max_ids * 8 > max_rings ? (int64_t)max_ids * 8 : max_rings;
  rc = c3d_launch_lds<valid_place_kernel>(dim3(grid_for(more_rows, 256)), dim3(256), 0, st, s, (const uint32_t*)header, valid);
  if (rc) return rc;
  rc = c3d_launch_lds<valid_gather_kernel>(dim3(grid_for(max_rings, 4)), dim3(256), 0, st, s);
  if (rc) return rc;
  rc = c3d_launch_lds<valid_gather_big_kernel>(dim3(g_big), dim3(256), 0, st, s, (const uint32_t*)header);
  if (rc) return rc;
  rc = c3d_launch_lds<valid_plan_kernel>(dim3(1), dim3(SCAN_T), (SCAN_T / 64) * 8, st, s, max_id_work, pl.job_cap, header, valid);
  if (rc) return rc;
  rc = c3d_launch_lds<valid_jobs_kernel>(dim3(grid_for(pl.job_cap, 1)), dim3(BLOCK_T), (size_t)TILE * 24, st, s, (const uint32_t*)header);
  if (rc) return rc;
  rc = c3d_launch_lds<valid_score_kernel>(dim3(grid_for(max_ids, 4)), dim3(256), 0, st, s, (const uint32_t*)header, valid);
  if (rc) return rc;
  return c3d_launch_lds<valid_tail_kernel>(dim3(1), dim3(256), 7 * 256 * 8, st, s, (const uint32_t*)header, (const int64_t*)valid, counts, totals);
}
