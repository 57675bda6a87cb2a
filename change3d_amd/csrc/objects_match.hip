// Object-level scores of a scene map (change3d_amd/object_metrics.py): the join of two labelings of c3d_scene_objects over the
// same Hs x Ws, a prediction `p` and a ground truth `g`.  Every pixel inside an object of both sides adds 1 to the count of
// its exact 64-bit key (p << 32) | g; a pair matches iff inter > iou_thr * union, strictly, with iou_thr >= 0.5, which makes a
// match unique on both sides: the result is a set of plain stores, with no assignment problem and no arrival order.  The
// reference has no counterpart.  Integers everywhere but the one float64 sum of the matched IoUs, which one workgroup adds in
// a fixed order: two runs agree bit for bit.
//
//   1 match_init     zeroes the rows of match_p / match_g (the covered column is added into by launch 3).
//   2 pair_count     the hot pass over 2 x 4 B per pixel.  A lane holds 4 consecutive pixels (one 16-byte load per map where
//                    the pointers allow), a wave 256.  Equal neighbouring keys are one run: inside a lane by compares, across
//                    lanes by the ballot of "all four of my keys equal my left neighbour's last one"; a run issues ONE insert
//                    with its length, a wave of one key issues one insert.  Inserts go first to a small per-workgroup table
//                    in LDS (64 slots, two probes, first come first served: the key of a scene-filling object is seen by
//                    every wave and claims its slot at once) which is flushed once per workgroup, so the one address that a
//                    big object funnels every atomic to takes one add per workgroup instead of one per wave.  What finds no
//                    LDS slot goes straight to the global open-addressing table (u64 key by atomicCAS, u32 count by atomicAdd;
//                    a lost CAS is compared and moves on, it never spins; probes are capped at min(capacity, 4096); nothing is
//                    decided by the hash, which only picks where a probe starts).
//   3 match_slots    one thread per slot: union from the two tables, the strict float64 comparison, the stores of a match,
//                    `covered` of both objects by u32 atomics (one add per wave for the wave's first object of each side).
//   4 match_finalise one workgroup: TP / FP / FN, the object confusion matrix, the IoU sum (thread t adds the ids t + 1, t + 257,
//                    .. in ascending order, then a fixed tree over the 256 partial sums), and the addition into `totals`.
//
// One memset (the workspace) and four launches on one stream, no host read, no grid barrier, no loop that waits for another
// workgroup, every loop bounded, no float atomics.  A label outside the rows of its table is counted nowhere.
#include "scene_wave.h"
#include "../../include/change3d_hip.h"

#pragma clang fp contract(off)   // inter > thr * union and inter / union are the two float64 operations, as written

namespace {

using namespace c3d_wave;

typedef unsigned long long u64;

constexpr int WS_HEADER = 256;                             // bytes in front of the table
enum { WS_STATUS = 0, WS_PAIRS = 1 };                      // u32 words of the header
constexpr int LDS_SLOTS = 64, LDS_PROBES = 2;              // the per-workgroup stage of pair_count
constexpr int WAVE_PIXELS = 256;                           // 64 lanes x 4 pixels
constexpr int MAX_GRID = 256 * 8;
constexpr int64_t MAX_PROBES = 4096;                       // of one insert: an overflowing table costs each failing run this, not `cap`

__device__ __forceinline__ uint32_t slot_of(u64 x, uint32_t mask) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return (uint32_t)x & mask;
}

// rows of a table that hold an object: counts[1], kept inside [0, max_rows] whatever the word holds
__device__ __forceinline__ int rows_of(const int32_t* counts, int max_rows) {
  const int r = counts[1];
  return r < 0 ? 0 : (r > max_rows ? max_rows : r);
}

struct Table {
  u64* keys;
  uint32_t* counts;
  uint32_t* header;
  int64_t cap;                                             // a power of two <= 2^32
};

// never waits: a slot is empty, ours, or someone else's for good.  At most min(cap, MAX_PROBES) slots are looked at: a table
// at most half full (the capacity that cannot overflow) has no probe sequence anywhere near that long, and a smaller one that
// overflows spends a bounded time on every run it has to drop.
__device__ __forceinline__ void global_insert(const Table& t, u64 key, uint32_t n) {
  const uint32_t mask = (uint32_t)(t.cap - 1);
  const int limit = (int)(t.cap < MAX_PROBES ? t.cap : MAX_PROBES);
  uint32_t slot = slot_of(key, mask);
  for (int probe = 0; probe < limit; ++probe) {
    u64 cur = __hip_atomic_load(t.keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0) cur = atomicCAS(t.keys + slot, 0ull, key);   // a lost race returns the winner's key: compare again
    if (cur == 0 || cur == key) {
      atomicAdd(t.counts + slot, n);
      return;
    }
    slot = (slot + 1u) & mask;
  }
  atomicOr(t.header + WS_STATUS, (uint32_t)C3D_MATCH_ST_TABLE_FULL);
}

template <bool STAGE>
__device__ __forceinline__ void insert(const Table& t, u64* s_key, uint32_t* s_cnt, u64 key, uint32_t n) {
  if (STAGE) {
    uint32_t s = ((uint32_t)key * 0x9E3779B1u + (uint32_t)(key >> 32) * 0x85EBCA6Bu) >> 26;   // 6 bits
    for (int q = 0; q < LDS_PROBES; ++q) {
      u64 cur = __hip_atomic_load(s_key + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (cur == 0) cur = atomicCAS(s_key + s, 0ull, key);
      if (cur == 0 || cur == key) {
        atomicAdd(s_cnt + s, n);
        return;
      }
      s = (s + 1u) & (LDS_SLOTS - 1);
    }
  }
  global_insert(t, key, n);
}

__global__ __launch_bounds__(256) void match_init_kernel(int32_t* __restrict__ match_p, int32_t* __restrict__ match_g,
                                                         int64_t words_p, int64_t words_g) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words_p + words_g; i += (int64_t)gridDim.x * 256) {
    if (i < words_p) match_p[i] = 0;
    else match_g[i - words_p] = 0;
  }
}

template <bool STAGE>
__global__ __launch_bounds__(256) void pair_count_kernel(const int32_t* __restrict__ labels_p, const int32_t* __restrict__ labels_g,
                                                         const int32_t* __restrict__ counts_p, const int32_t* __restrict__ counts_g,
                                                         const Table t, int64_t N, int64_t n_chunks, int max_p, int max_g,
                                                         int vec) {
  extern __shared__ char lds[];
  u64* s_key = reinterpret_cast<u64*>(lds);                              // [LDS_SLOTS]
  uint32_t* s_cnt = reinterpret_cast<uint32_t*>(lds + LDS_SLOTS * 8);    // [LDS_SLOTS]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (STAGE) {
    if (threadIdx.x < LDS_SLOTS) { s_key[threadIdx.x] = 0ull; s_cnt[threadIdx.x] = 0u; }
    __syncthreads();
  }
  const int np = rows_of(counts_p, max_p), ng = rows_of(counts_g, max_g);
  for (int64_t chunk = (int64_t)blockIdx.x * 4 + wave; chunk < n_chunks; chunk += (int64_t)gridDim.x * 4) {   // wave-uniform
    const int64_t i0 = chunk * WAVE_PIXELS + lane * 4;
    int p[4], g[4];
    if (vec && i0 + 3 < N) {
      const int4 a = *reinterpret_cast<const int4*>(labels_p + i0), b = *reinterpret_cast<const int4*>(labels_g + i0);
      p[0] = a.x; p[1] = a.y; p[2] = a.z; p[3] = a.w;
      g[0] = b.x; g[1] = b.y; g[2] = b.z; g[3] = b.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = i0 + j < N;
        p[j] = in ? labels_p[i0 + j] : 0;
        g[j] = in ? labels_g[i0 + j] : 0;
      }
    }
    u64 k[4];
    uint32_t c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool both = p[j] >= 1 && p[j] <= np && g[j] >= 1 && g[j] <= ng;
      k[j] = both ? ((u64)(uint32_t)p[j] << 32) | (uint32_t)g[j] : 0ull;
    }
    c[0] = 1u;                                             // the last pixel of a run inside the lane carries its length
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      const bool same = k[j] == k[j - 1];
      c[j] = same ? c[j - 1] + 1u : 1u;
      if (same) c[j - 1] = 0u;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (c[j] && k[j]) insert<STAGE>(t, s_key, s_cnt, k[j], c[j]);
    // the lane's last run goes on in the lanes to the right whose four keys all equal it
    const u64 kt = k[3];
    const uint32_t lo = __shfl_up((uint32_t)kt, 1), hi = __shfl_up((uint32_t)(kt >> 32), 1);
    const bool join = lane > 0 && kt != 0 && c[3] == 4u && kt == (((u64)hi << 32) | lo);
    const u64 joined = __ballot(join);
    if (kt != 0 && !join) {
      const u64 rest = lane == 63 ? 0ull : joined >> (lane + 1);       // bit 63 - lane and above are clear
      const int followers = __ffsll((long long)~rest) - 1;
      insert<STAGE>(t, s_key, s_cnt, kt, c[3] + 4u * (uint32_t)followers);
    }
  }
  if (STAGE) {
    __syncthreads();
    if (threadIdx.x < LDS_SLOTS && s_key[threadIdx.x] != 0ull) global_insert(t, s_key[threadIdx.x], s_cnt[threadIdx.x]);
  }
}


// covered[id - 1][3] += inter over the lanes of a wave: one add for the object of the first lane, one per lane for the rest
__device__ __forceinline__ void add_covered(int32_t* match, bool valid, int id, uint32_t inter, int lane) {
  const u64 m = __ballot(valid);
  if (!m) return;
  const int leader = __ffsll((long long)m) - 1;
  const int id0 = __shfl(id, leader);
  const bool same = valid && id == id0;
  const uint32_t sum = wave_sum32(same ? inter : 0u);                  // <= Hs * Ws < 2^31
  if (lane == leader) atomicAdd(reinterpret_cast<uint32_t*>(match + (int64_t)(id0 - 1) * 4 + 3), sum);
  else if (valid && !same) atomicAdd(reinterpret_cast<uint32_t*>(match + (int64_t)(id - 1) * 4 + 3), inter);
}

__global__ __launch_bounds__(256) void match_slots_kernel(const Table t, const int32_t* __restrict__ table_p,
                                                          const int32_t* __restrict__ table_g, const int32_t* __restrict__ counts_p,
                                                          const int32_t* __restrict__ counts_g, int max_p, int max_g, double iou_thr,
                                                          int32_t* __restrict__ match_p, int32_t* __restrict__ match_g) {
  const int lane = threadIdx.x & 63;
  const int np = rows_of(counts_p, max_p), ng = rows_of(counts_g, max_g);
  for (int64_t base = (int64_t)blockIdx.x * 256; base < t.cap; base += (int64_t)gridDim.x * 256) {   // workgroup-uniform
    const int64_t s = base + threadIdx.x;
    const u64 key = s < t.cap ? t.keys[s] : 0ull;
    const int p = (int)(key >> 32), g = (int)(uint32_t)key;
    const bool valid = key != 0ull && p >= 1 && p <= np && g >= 1 && g <= ng;   // pair_count inserts nothing else
    const u64 m = __ballot(valid);
    if (!m) continue;
    const uint32_t inter = valid ? t.counts[s] : 0u;
    if (valid) {
      const int64_t uni = (int64_t)table_p[(int64_t)(p - 1) * 8] + (int64_t)table_g[(int64_t)(g - 1) * 8] - (int64_t)inter;
      if ((double)inter > iou_thr * (double)uni) {         // strict, and iou_thr >= 0.5: no other pair of p or of g passes
        int32_t* rp = match_p + (int64_t)(p - 1) * 4;
        int32_t* rg = match_g + (int64_t)(g - 1) * 4;
        rp[0] = g; rp[1] = (int32_t)inter; rp[2] = (int32_t)uni;
        rg[0] = p; rg[1] = (int32_t)inter; rg[2] = (int32_t)uni;
      }
    }
    add_covered(match_p, valid, p, inter, lane);
    add_covered(match_g, valid, g, inter, lane);
    if (lane == 0) atomicAdd(t.header + WS_PAIRS, (uint32_t)__popcll(m));
  }
}

// class of a table row as an index of conf: a value outside [0, n_cls) counts as 0, "no class"
__device__ __forceinline__ int cls_of(const int32_t* table, int id, int n_cls) {
  const int c = table[(int64_t)(id - 1) * 8 + 5];
  return c >= 0 && c < n_cls ? c : 0;
}

__global__ __launch_bounds__(256) void match_finalise_kernel(const int32_t* __restrict__ table_p, const int32_t* __restrict__ table_g,
                                                             const int32_t* __restrict__ counts_p, const int32_t* __restrict__ counts_g,
                                                             const int32_t* __restrict__ match_p, const int32_t* __restrict__ match_g,
                                                             const uint32_t* __restrict__ header, int max_p, int max_g, int n_cls,
                                                             int64_t* __restrict__ conf, int64_t* __restrict__ counts,
                                                             double* __restrict__ sum_iou, int64_t* __restrict__ totals,
                                                             double* __restrict__ total_iou) {
  extern __shared__ char lds[];
  double* s_sum = reinterpret_cast<double*>(lds);                        // [256]
  uint32_t* s_conf = reinterpret_cast<uint32_t*>(lds + 256 * 8);         // [16 * 16]
  uint32_t* s_tp = s_conf + 256;                                         // [1]
  const int tid = threadIdx.x;
  const int np = rows_of(counts_p, max_p), ng = rows_of(counts_g, max_g);
  s_conf[tid] = 0u;
  if (tid == 0) *s_tp = 0u;
  __syncthreads();
  double sum = 0.0;
  uint32_t tp = 0;
  for (int id = tid + 1; id <= np; id += 256) {            // ascending predicted id
    const int32_t* row = match_p + (int64_t)(id - 1) * 4;
    const int partner = row[0], cp = cls_of(table_p, id, n_cls);
    if (partner >= 1 && partner <= ng) {
      sum += (double)row[1] / (double)row[2];
      ++tp;
      atomicAdd(s_conf + cls_of(table_g, partner, n_cls) * 16 + cp, 1u);
    } else {
      atomicAdd(s_conf + cp, 1u);                          // a false alarm: row 0
    }
  }
  for (int id = tid + 1; id <= ng; id += 256)
    if (match_g[(int64_t)(id - 1) * 4] == 0) atomicAdd(s_conf + cls_of(table_g, id, n_cls) * 16, 1u);   // missed: column 0
  if (tp) atomicAdd(s_tp, tp);
  s_sum[tid] = sum;
  __syncthreads();
  for (int d = 128; d; d >>= 1) {                          // the same tree every run
    if (tid < d) s_sum[tid] += s_sum[tid + d];
    __syncthreads();
  }
  if (tid < n_cls * n_cls) conf[tid] = (int64_t)s_conf[(tid / n_cls) * 16 + tid % n_cls];
  if (tid == 0) {
    const int64_t TP = *s_tp, FP = np - TP, FN = ng - TP, pairs = header[WS_PAIRS];
    int64_t status = header[WS_STATUS];
    if (counts_p[0] > counts_p[1] || counts_g[0] > counts_g[1] || counts_p[1] > max_p || counts_g[1] > max_g)
      status |= C3D_MATCH_ST_TRUNCATED;
    if (counts_p[0] < 0 || counts_g[0] < 0) status |= C3D_MATCH_ST_BAD_COUNTS;
    counts[0] = pairs; counts[1] = TP; counts[2] = FP; counts[3] = FN; counts[4] = status; counts[5] = 0;
    sum_iou[0] = s_sum[0];
    if (totals) {
      totals[0] += TP; totals[1] += FP; totals[2] += FN; totals[3] += pairs; totals[4] |= status;
      for (int k = 0; k < n_cls * n_cls; ++k) totals[5 + k] += (int64_t)s_conf[(k / n_cls) * 16 + k % n_cls];
    }
    if (total_iou) total_iou[0] += s_sum[0];
  }
}

unsigned grid_for(int64_t items, int64_t per_block) {
  int64_t g = (items + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > MAX_GRID ? MAX_GRID : g));
}

// the capacity that cannot overflow: every pair owns at least one pixel, and the table is at most half full
int64_t safe_capacity(int64_t N) {
  int64_t cap = 1;
  while (cap < 2 * N) cap <<= 1;
  return cap;
}

bool power_of_two(int64_t v) { return v >= 1 && v <= (1ll << 32) && (v & (v - 1)) == 0; }

}  // namespace

extern "C" int64_t c3d_objects_match_ws_bytes(int32_t Hs, int32_t Ws, int64_t* table_capacity) {
  if (Hs <= 0 || Ws <= 0 || !table_capacity) return C3D_E_BADARG;
  if ((int64_t)Hs * Ws >= (1ll << 31)) return C3D_E_UNSUPPORTED;
  if (*table_capacity == 0) *table_capacity = safe_capacity((int64_t)Hs * Ws);
  if (!power_of_two(*table_capacity)) return C3D_E_BADARG;
  return WS_HEADER + 12 * *table_capacity;
}

extern "C" int c3d_objects_match(const int32_t* labels_p, const int32_t* table_p, const int32_t* counts_p, const int32_t* labels_g,
                                 const int32_t* table_g, const int32_t* counts_g, int32_t Hs, int32_t Ws, int32_t max_p,
                                 int32_t max_g, int32_t n_cls, double iou_thr, int64_t table_capacity, int32_t* match_p,
                                 int32_t* match_g, int64_t* conf, int64_t* counts, double* sum_iou, int64_t* totals,
                                 double* total_iou, void* ws, void* stream) {
  if (!labels_p || !table_p || !counts_p || !labels_g || !table_g || !counts_g || !match_p || !match_g || !conf || !counts ||
      !sum_iou || !ws)
    return C3D_E_BADARG;
  if (Hs <= 0 || Ws <= 0 || max_p < 1 || max_g < 1 || n_cls < 1 || n_cls > 16) return C3D_E_BADARG;
  if (!(iou_thr >= 0.5 && iou_thr < 1.0)) return C3D_E_BADARG;             // NaN fails both comparisons
  if (!power_of_two(table_capacity)) return C3D_E_BADARG;
  if ((int64_t)Hs * Ws >= (1ll << 31)) return C3D_E_UNSUPPORTED;
  const int64_t N = (int64_t)Hs * Ws, n_chunks = (N + WAVE_PIXELS - 1) / WAVE_PIXELS;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  Table t;
  t.header = reinterpret_cast<uint32_t*>(base);
  t.keys = reinterpret_cast<u64*>(base + WS_HEADER);
  t.counts = reinterpret_cast<uint32_t*>(base + WS_HEADER + 8 * table_capacity);
  t.cap = table_capacity;

  // instrumented build only (common.h c3d_knob): tools/objects_match_step.py times prefixes of the call, the pixel pass with
  // and without its LDS stage, and other spans of a workgroup.  The product library compiles these to 4, 1 and 4.
  const int phases = c3d_knob("C3D_MATCH_PHASES", 4);     // 0: the memset alone
  const int stage = c3d_knob("C3D_MATCH_LDS", 1);
  int span = c3d_knob("C3D_MATCH_SPAN", 4);               // chunks of 256 pixels per wave
  if (span < 1) span = 1;

  hipError_t e = hipMemsetAsync(base, 0, (size_t)(WS_HEADER + 12 * table_capacity), st);
  if (e != hipSuccess) return (int)e;
  if (phases == 0) return 0;
  const int64_t words_p = (int64_t)max_p * 4, words_g = (int64_t)max_g * 4;
  int rc = c3d_launch_lds<match_init_kernel>(dim3(grid_for(words_p + words_g, 256)), dim3(256), 0, st, match_p, match_g, words_p,
                                             words_g);
  if (rc || phases == 1) return rc;
  const int vec = (reinterpret_cast<uintptr_t>(labels_p) | reinterpret_cast<uintptr_t>(labels_g)) % 16 == 0 ? 1 : 0;
  const dim3 grid(grid_for(n_chunks, 4 * (int64_t)span));
  rc = stage ? c3d_launch_lds<pair_count_kernel<true>>(grid, dim3(256), LDS_SLOTS * 12, st, labels_p, labels_g, counts_p, counts_g, t,
                                                       N, n_chunks, (int)max_p, (int)max_g, vec)
             : c3d_launch_lds<pair_count_kernel<false>>(grid, dim3(256), 0, st, labels_p, labels_g, counts_p, counts_g, t, N,
                                                        n_chunks, (int)max_p, (int)max_g, vec);
  if (rc || phases == 2) return rc;
  rc = c3d_launch_lds<match_slots_kernel>(dim3(grid_for(table_capacity, 256)), dim3(256), 0, st, t, table_p, table_g, counts_p,
                                          counts_g, (int)max_p, (int)max_g, iou_thr, match_p, match_g);
  if (rc || phases == 3) return rc;
  return c3d_launch_lds<match_finalise_kernel>(dim3(1), dim3(256), 256 * 8 + 256 * 4 + 16, st, table_p, table_g, counts_p, counts_g,
                                               (const int32_t*)match_p, (const int32_t*)match_g, (const uint32_t*)t.header,
                                               (int)max_p, (int)max_g, (int)n_cls, conf, counts, sum_iou, totals, total_iou);
}
