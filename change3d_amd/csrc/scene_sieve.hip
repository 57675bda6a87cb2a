// The sieve of a class map (change3d_amd/infer.py, predict(regions=.., sieve=N)): regions below min_area are absorbed by the
// neighbour they share the longest border with, in rounds, on the device; the rule is in include/change3d_hip.h and restated
// in tests/sieve_reference.py.  What gdal_sieve does on the host after a download.  Integers everywhere, every decision is a
// maximum or a plain store: no result depends on arrival order and two runs agree bit for bit.
//
// The map is sieved in place in key_out (a copy of key), the root map of a round lives in `labels`, the areas at the roots
// in the workspace of c3d_scene_regions.  max_rounds + 1 rounds are launched ahead; every kernel of a round returns at once
// when the stop word of the header is set.  One round:
//
//   1..3 region roots   c3d_detail_region_roots (csrc/scene_regions.hip), gated
//   4 border_count      one thread per pixel: background pixels, roots and small roots are counted; a pixel of a small region
//                       r adds 1 to the pair (r, n) for each of its four sides with a pixel of another region n or of the
//                       background.  Pairs live in an open-addressing table as in csrc/objects_match.hip: the exact u64 key
//                       ((root_r + 1) << 32) | (root_n + 1), background = 0 in the low word, claimed by atomicCAS -- the
//                       claimer appends the slot to a list, so the later passes walk the entries and not the capacity --,
//                       the u32 count by atomicAdd; a lost CAS compares and moves on; probes are capped.
//   5 border_max        per entry: atomicMax of the border at r.
//   6 border_best       per entry at that maximum: atomicMax of (area(n) << 32) | (0xffffffff - (root_n + 1)) at r: the larger
//                       area, then the smaller root, the background (low word 0) first of all.  Clears the slot.
//   7 decide            per root: the target of a small root and whether it moves (rule 4).
//   8 round_end         one thread: table full / nothing moves / max_rounds rounds have moved -> stop, else the counters of the
//                       next round.
//   9 paint             per pixel of a moving region: walks r -> t(r) -> .. to the first region that stays (capped, error
//                       word) and takes its key; zeroes the per-root words of the next round.
//
// After the rounds the root map and the areas are those of the final map (the stopping round labelled it and painted
// nothing), so the tail of c3d_scene_objects, region_keys and info follow directly.
#include "common.h"
#include "scene_detail.h"
#include "../../include/change3d_hip.h"

namespace {

typedef unsigned long long u64;

constexpr int MIN_AREA_MAX = 1 << 20, ROUNDS_MAX = 65536;
constexpr int64_t MAX_PROBES = 4096;
constexpr int64_t CAP_MIN = 16, CAP_MAX = 1ll << 31;

enum {                                                     // words of the header, from C3D_DETAIL_HEADER_FREE on
  H_STOP = C3D_DETAIL_HEADER_FREE, H_STATUS, H_ROUNDS, H_MOVED, H_PIXELS, H_SMALL_LEFT, H_REGIONS_IN, H_MAX_ENTRIES,
  H_ROUND, H_NBG, H_NROOTS, H_NSMALL, H_NMOVING, H_NENTRIES, H_FULL, H_END
};
static_assert(H_END <= C3D_DETAIL_HEADER_WORDS, "the header of the label workspace has 64 words");

constexpr int T_STAYS = -2, T_BG = -1;                     // tgt[root]: the root it moves to, the background, or it stays

struct Plan {
  int64_t maxb, best, tgt, keys, cnts, list, bytes, cap;
};

int64_t safe_capacity(int64_t Hs, int64_t Ws) {            // a side between two regions holds at most two ordered pairs
  const int64_t pairs = 2 * (Hs * (Ws - 1) + Ws * (Hs - 1));
  int64_t cap = CAP_MIN;
  while (cap < 2 * pairs) cap <<= 1;                       // at most half full
  return cap;
}

Plan plan_for(int64_t N, int64_t cap) {
  auto up = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  Plan p;
  p.cap = cap;
  p.maxb = up(c3d_detail_region_ws_bytes(N));
  p.best = p.maxb + up(N * 4);
  p.tgt = p.best + up(N * 8);
  p.keys = p.tgt + up(N * 4);
  p.cnts = p.keys + up(cap * 8);
  p.list = p.cnts + up(cap * 4);
  p.bytes = p.list + up(cap * 4);
  return p;
}

struct Table {
  u64* keys;
  uint32_t* cnts;
  uint32_t* list;
  int64_t cap;                                             // a power of two <= 2^31
};

__device__ __forceinline__ uint32_t slot_of(u64 x, uint32_t mask) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return (uint32_t)x & mask;
}

// never waits: a slot is empty, ours, or someone else's for good.  The thread whose CAS claims a slot appends it to the list;
// at most `cap` slots are ever claimed, so the list cannot overflow.
__device__ __forceinline__ void pair_add(const Table& t, uint32_t* header, u64 key) {
  const uint32_t mask = (uint32_t)(t.cap - 1);
  const int limit = (int)(t.cap < MAX_PROBES ? t.cap : MAX_PROBES);
  uint32_t slot = slot_of(key, mask);
  for (int probe = 0; probe < limit; ++probe) {
    u64 cur = __hip_atomic_load(t.keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0) {
      cur = atomicCAS(t.keys + slot, 0ull, key);           // a lost race returns the winner's key: compare again
      if (cur == 0) t.list[atomicAdd(header + H_NENTRIES, 1u)] = slot;
    }
    if (cur == 0 || cur == key) {
      atomicAdd(t.cnts + slot, 1u);
      return;
    }
    slot = (slot + 1u) & mask;
  }
  atomicOr(header + H_FULL, 1u);
}

__device__ __forceinline__ void wave_count(uint32_t* word, bool flag) {
  const unsigned long long m = __ballot(flag);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(word, (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(256) void border_count_kernel(const int32_t* __restrict__ L, const uint32_t* __restrict__ area,
                                                           const Table t, uint32_t* __restrict__ header, int Hs, int Ws,
                                                           uint32_t min_area) {
  if (header[H_STOP]) return;
  const int N = Hs * Ws;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < N; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    const bool in = i < N;
    const int r = in ? L[i] : 0;
    const bool small = in && r >= 0 && area[r] < min_area;
    wave_count(header + H_NBG, in && r < 0);
    wave_count(header + H_NROOTS, in && r == (int)i);
    wave_count(header + H_NSMALL, small && r == (int)i);
    if (!small) continue;
    const int y = (int)(i / Ws), x = (int)(i % Ws);
    const u64 hi = (u64)(uint32_t)(r + 1) << 32;
    if (y > 0) { const int n = L[i - Ws]; if (n != r) pair_add(t, header, hi | (uint32_t)(n + 1)); }
    if (x > 0) { const int n = L[i - 1]; if (n != r) pair_add(t, header, hi | (uint32_t)(n + 1)); }
    if (x < Ws - 1) { const int n = L[i + 1]; if (n != r) pair_add(t, header, hi | (uint32_t)(n + 1)); }
    if (y < Hs - 1) { const int n = L[i + Ws]; if (n != r) pair_add(t, header, hi | (uint32_t)(n + 1)); }
  }
}

__global__ __launch_bounds__(256) void border_max_kernel(const Table t, const uint32_t* __restrict__ header,
                                                         uint32_t* __restrict__ maxb) {
  if (header[H_STOP]) return;
  const uint32_t n = header[H_NENTRIES];
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const uint32_t slot = t.list[e];
    atomicMax(maxb + ((uint32_t)(t.keys[slot] >> 32) - 1u), t.cnts[slot]);
  }
}

__global__ __launch_bounds__(256) void border_best_kernel(const Table t, const uint32_t* __restrict__ header,
                                                          const uint32_t* __restrict__ area, const uint32_t* __restrict__ maxb,
                                                          u64* __restrict__ best) {
  if (header[H_STOP]) return;
  const uint32_t n = header[H_NENTRIES];
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const uint32_t slot = t.list[e];
    const u64 k = t.keys[slot];
    const uint32_t r = (uint32_t)(k >> 32) - 1u, lo = (uint32_t)k;
    if (t.cnts[slot] == maxb[r]) {
      const u64 a = lo ? area[lo - 1u] : header[H_NBG];    // >= 1 either way: the neighbour exists
      atomicMax(best + r, (a << 32) | (0xffffffffu - lo));
    }
    t.keys[slot] = 0ull;                                   // the table is empty again for the next round
    t.cnts[slot] = 0u;
  }
}

__global__ __launch_bounds__(256) void decide_kernel(const int32_t* __restrict__ L, const uint32_t* __restrict__ area,
                                                     const u64* __restrict__ best, int32_t* __restrict__ tgt,
                                                     uint32_t* __restrict__ header, int N, uint32_t min_area) {
  if (header[H_STOP]) return;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < N; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    bool moves = false;
    if (i < N && L[i] == (int)i) {
      const uint32_t a = area[i];
      const u64 b = best[i];
      int to = T_STAYS;
      if (a < min_area && b) {
        const uint32_t lo = 0xffffffffu - (uint32_t)b, an = (uint32_t)(b >> 32);
        const int n = (int)lo - 1;                         // -1: the background
        if (n < 0 || an >= min_area || an > a || (an == a && n > (int)i)) to = n;
      }
      tgt[i] = to;
      moves = to != T_STAYS;
    }
    wave_count(header + H_NMOVING, moves);
  }
}

__global__ void round_end_kernel(uint32_t* __restrict__ header, int max_rounds) {
  if (threadIdx.x || blockIdx.x || header[H_STOP]) return;
  const uint32_t round = header[H_ROUND], moving = header[H_NMOVING];
  if (round == 0) header[H_REGIONS_IN] = header[H_NROOTS];
  if (header[H_NENTRIES] > header[H_MAX_ENTRIES]) header[H_MAX_ENTRIES] = header[H_NENTRIES];
  uint32_t status = 0;
  bool stop = false;
  if (header[H_FULL]) { status = C3D_SIEVE_ST_TABLE_FULL; stop = true; }
  else if (moving == 0) stop = true;
  else if (round == (uint32_t)max_rounds) { status = C3D_SIEVE_ST_NOT_CONVERGED; stop = true; }
  if (stop) {
    header[H_STATUS] = status;
    header[H_SMALL_LEFT] = header[H_NSMALL];
    header[H_STOP] = 1u;
    return;
  }
  header[H_ROUNDS] += 1u;
  header[H_MOVED] += moving;
  header[H_ROUND] = round + 1u;
  header[H_NBG] = header[H_NROOTS] = header[H_NSMALL] = header[H_NMOVING] = header[H_NENTRIES] = 0u;
}

__global__ __launch_bounds__(256) void sieve_paint_kernel(uint8_t* __restrict__ K, const int32_t* __restrict__ L,
                                                          const int32_t* __restrict__ tgt, uint32_t* __restrict__ area,
                                                          uint32_t* __restrict__ maxb, u64* __restrict__ best,
                                                          uint32_t* __restrict__ header, int N) {
  if (header[H_STOP]) return;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < N; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    bool changed = false;
    if (i < N) {
      const int r = L[i];
      int cur = r >= 0 ? tgt[r] : T_STAYS;
      if (cur != T_STAYS) {
        // the chain ends at the first region that stays; K there is not written by this launch.  A chain rises in (area,
        // root) among the small regions, so it is shorter than their number; the cap only guards a corrupted workspace.
        int nk = K[i], step = 0;
        for (; step <= N; ++step) {
          if (cur == T_BG) { nk = 0; break; }
          const int next = tgt[cur];
          if (next == T_STAYS) { nk = K[cur]; break; }
          cur = next;
        }
        if (step > N) atomicOr(header + C3D_DETAIL_WS_ERR, 1u);
        if (nk != K[i]) { K[i] = (uint8_t)nk; changed = true; }
      }
      area[i] = 0u;
      maxb[i] = 0u;
      best[i] = 0ull;
    }
    wave_count(header + H_PIXELS, changed);
  }
}

__global__ void sieve_info_kernel(const uint32_t* __restrict__ header, int32_t* __restrict__ info) {
  if (threadIdx.x || blockIdx.x) return;
  info[0] = (int32_t)header[H_STATUS] | (header[C3D_DETAIL_WS_ERR] ? C3D_SIEVE_ST_BAD_LABELS : 0);
  info[1] = (int32_t)header[H_ROUNDS];
  info[2] = (int32_t)header[H_MOVED];
  info[3] = (int32_t)header[H_PIXELS];
  info[4] = (int32_t)header[H_SMALL_LEFT];
  info[5] = (int32_t)header[H_REGIONS_IN];
  info[6] = (int32_t)header[H_MAX_ENTRIES];
  info[7] = 0;
}

unsigned grid_cus(int64_t items) {
  static const int cus = c3d_device_cus();
  const int64_t most = (int64_t)(cus > 0 ? cus : 256) * 8;
  const int64_t g = (items + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > most ? most : g));
}

bool power_of_two(int64_t v) { return v >= CAP_MIN && v <= CAP_MAX && (v & (v - 1)) == 0; }

}  // namespace

extern "C" int64_t c3d_regions_sieve_ws_bytes(int32_t Hs, int32_t Ws, int64_t* table_capacity) {
  if (Hs <= 0 || Ws <= 0 || !table_capacity) return C3D_E_BADARG;
  if ((int64_t)Hs * Ws >= (1ll << 31)) return C3D_E_UNSUPPORTED;
  if (*table_capacity == 0) {
    const int64_t cap = safe_capacity(Hs, Ws);
    if (cap > CAP_MAX) return C3D_E_UNSUPPORTED;
    *table_capacity = cap;
  }
  if (!power_of_two(*table_capacity)) return C3D_E_BADARG;
  return plan_for((int64_t)Hs * Ws, *table_capacity).bytes;
}

extern "C" int c3d_regions_sieve(const uint8_t* key, const float* score, int32_t Hs, int32_t Ws, int32_t connectivity,
                                 int32_t min_area, int32_t max_rounds, int32_t max_objects, int64_t table_capacity, uint8_t* key_out,
                                 int32_t* labels, int32_t* table, int32_t* counts, int32_t* info, void* ws, void* stream) {
  if (!key || !key_out || key == key_out || !labels || !table || !counts || !info || !ws || Hs <= 0 || Ws <= 0 || max_objects < 1)
    return C3D_E_BADARG;
  if (connectivity != 4 && connectivity != 8) return C3D_E_BADARG;
  if (min_area < 1 || min_area > MIN_AREA_MAX || max_rounds < 1 || max_rounds > ROUNDS_MAX) return C3D_E_BADARG;
  if (!power_of_two(table_capacity)) return C3D_E_BADARG;
  if ((int64_t)Hs * Ws >= (1ll << 31)) return C3D_E_UNSUPPORTED;
  const int N = Hs * Ws;
  const int conn8 = connectivity == 8;
  const Plan p = plan_for(N, table_capacity);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  uint32_t* header = reinterpret_cast<uint32_t*>(base);
  uint32_t* area = reinterpret_cast<uint32_t*>(base + c3d_detail_area_offset());
  uint32_t* maxb = reinterpret_cast<uint32_t*>(base + p.maxb);
  u64* best = reinterpret_cast<u64*>(base + p.best);
  int32_t* tgt = reinterpret_cast<int32_t*>(base + p.tgt);
  const Table t = {reinterpret_cast<u64*>(base + p.keys), reinterpret_cast<uint32_t*>(base + p.cnts),
                   reinterpret_cast<uint32_t*>(base + p.list), p.cap};
  const uint32_t* stop = header + H_STOP;

  int rc = c3d_detail_region_clear(ws, N, score, max_objects, st);   // header, areas, score sums
  if (rc) return rc;
  hipError_t e = hipMemsetAsync(base + p.maxb, 0, (size_t)(p.tgt - p.maxb), st);           // maxb, best
  if (e == hipSuccess) e = hipMemsetAsync(base + p.keys, 0, (size_t)(p.list - p.keys), st);   // keys, counts
  if (e == hipSuccess) e = hipMemcpyAsync(key_out, key, (size_t)N, hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) return (int)e;

  const dim3 gp(grid_cus(N)), ge(grid_cus(p.cap < 2ll * N ? p.cap : 2ll * N)), blk(256);
  for (int round = 0; round <= max_rounds; ++round) {      // the last one only finds out whether something would still move
    rc = c3d_detail_region_roots(key_out, labels, header + C3D_DETAIL_WS_ERR, area, Hs, Ws, conn8, stop, st);
    if (rc) return rc;
    rc = c3d_launch_lds<border_count_kernel>(gp, blk, 0, st, (const int32_t*)labels, (const uint32_t*)area, t, header, (int)Hs,
                                             (int)Ws, (uint32_t)min_area);
    if (rc) return rc;
    rc = c3d_launch_lds<border_max_kernel>(ge, blk, 0, st, t, (const uint32_t*)header, maxb);
    if (rc) return rc;
    rc = c3d_launch_lds<border_best_kernel>(ge, blk, 0, st, t, (const uint32_t*)header, (const uint32_t*)area, (const uint32_t*)maxb,
                                            best);
    if (rc) return rc;
    rc = c3d_launch_lds<decide_kernel>(gp, blk, 0, st, (const int32_t*)labels, (const uint32_t*)area, (const u64*)best, tgt, header, N,
                                       (uint32_t)min_area);
    if (rc) return rc;
    rc = c3d_launch_lds<round_end_kernel>(dim3(1), dim3(64), 0, st, header, (int)max_rounds);
    if (rc) return rc;
    rc = c3d_launch_lds<sieve_paint_kernel>(gp, blk, 0, st, key_out, (const int32_t*)labels, (const int32_t*)tgt, area, maxb, best,
                                            header, N);
    if (rc) return rc;
  }
  rc = c3d_detail_objects_tail(nullptr, score, Hs, Ws, 1, 1, 0, max_objects, labels, table, nullptr, nullptr, counts, ws, 9, st);
  if (rc) return rc;
  rc = c3d_detail_region_keys(key_out, labels, table, counts, nullptr, Hs, Ws, max_objects, st);
  if (rc) return rc;
  return c3d_launch_lds<sieve_info_kernel>(dim3(1), dim3(64), 0, st, (const uint32_t*)header, info);
}
