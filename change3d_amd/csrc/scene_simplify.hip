// Simplified polygons of a scene map: Douglas-Peucker with a pixel tolerance on the ring table and vertex list that
// c3d_scene_outlines leaves in HBM (or on any table of that shape).  The rule -- integer segment distance, strict
// comparison, ties to the smallest index, the two anchors, the third vertex of a collapsed ring -- is the header's
// (include/change3d_hip.h); this file is one way to compute it.  Integer arithmetic and integer atomics only.
//
// Douglas-Peucker is as deep as its input is awkward (about n / 4 levels on a serpentine), so the rounds live inside the
// kernels: whoever owns a ring loops until no chord of it splits.  No workgroup waits for another, nothing is read back.
//
//   1 scan_rows   one workgroup of 1024: classifies the rows (pass-through, bad, valid) and scans the vertex counts of the valid
//                 ones: off[r] = where ring r keeps its per-vertex state in the workspace
//   2 wave        rings of up to WAVE_LIMIT vertices, one wave each: a lane per vertex, chord ends in registers, the
//                 segmented arg-max of a round is a segmented suffix scan by shuffles.  It also lists the larger rings, so
//                 that the workgroup kernels need not stride over all rows to find theirs
//   3 block       larger rings, one workgroup of 1024 threads each (a round is latency, not arithmetic): state in LDS up to LDS_LIMIT vertices, in the workspace beyond; the
//                 same loop body for both.  A round is four passes over the still open vertices:
//                   max    atomicMax of num into best[lo], lo = the chord's first vertex (one atomic per wave where a
//                          wave's vertices share the chord, which is every wave of a long chord)
//                   arg    atomicMin of the index into idx[lo] by the vertices whose num is that maximum
//                   split  every vertex reads its chord's verdict: dropped, or it moves to the left or right half; the
//                          split vertex m becomes a chord start and parks `lo` in its own best slot
//                   link   m hands the old chord start its new end and resets both slots
//                 Both 2 and 3 leave one keep flag per vertex and the ring's kept count
//   4 scan_kept   one workgroup: start' = exclusive scan of the kept counts; counts_out
//   5 scatter     wave and block variants: ordered compaction of the kept vertices into vertices_out, the shoelace sum of
//                 the kept ring, the ring row; rows past the table are zeroed
#include <climits>

#include "scene_wave.h"
#include "../../include/change3d_hip.h"

namespace {

using namespace c3d_wave;

typedef unsigned long long u64;

constexpr int WAVE_LIMIT = 64;                             // one lane per vertex
// 20 bytes of state per vertex and 16 for the workgroup: the whole 160 KiB of a CU.  A workgroup of 1024 threads at this
// kernel's register count is alone on its CU anyway (4 waves per SIMD of 7 that fit), so a smaller limit buys no second
// workgroup, and a round in LDS costs about a tenth of a round in the workspace.  Even, so that the 64-bit words stay aligned
constexpr int LDS_LIMIT = 8190;
static_assert(LDS_LIMIT % 2 == 0 && LDS_LIMIT * 20 + 16 <= 160 * 1024, "the ring state of the LDS tier fills at most one CU's LDS");
constexpr int LDS_BYTES = LDS_LIMIT * 20 + 16;
constexpr int BLOCK_T = 1024;                              // threads of a ring's workgroup: a round is latency, not arithmetic
constexpr int COORD_MAX = 16384;
constexpr int MAX_GRID = 2048;
constexpr int SCAN_ROWS = 8;                               // rows per thread and step of the two scans
constexpr int ROW_PASS = -1, ROW_BAD = -2;                 // kept[r] of a row that is not simplified
constexpr int SPLIT_MARK = -2;                             // idx[m] of a vertex that split its chord in this round

// words of the workspace header (256 bytes), written by scan_rows
enum { WS_ERR = 0, WS_ROWS = 1, WS_FOUND = 2, WS_STATUS = 3, WS_BADCOUNTS = 4, WS_LARGE = 5 };

struct Workspace {
  int64_t off, kept, startp, large, flags, link, idx, best, bytes;   // byte offsets
};

Workspace workspace_plan(int64_t max_rings, int64_t max_vertices) {
  Workspace w;
  auto up = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  w.off = 256;
  w.kept = w.off + up(max_rings * 4);
  w.startp = w.kept + up(max_rings * 4);
  w.large = w.startp + up(max_rings * 4);
  w.flags = w.large + up(max_rings * 4);
  w.link = w.flags + up(max_vertices);
  w.idx = w.link + up(max_vertices * 4);
  w.best = w.idx + up(max_vertices * 4);
  w.bytes = w.best + up(max_vertices * 8);
  return w;
}

__device__ __forceinline__ u64 shfl_down64(u64 v, int d) {
  const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)v, d), hi = (uint32_t)__shfl_down((int)(uint32_t)(v >> 32), d);
  return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ bool coord_ok(int2 p) { return p.x >= 0 && p.x <= COORD_MAX && p.y >= 0 && p.y <= COORD_MAX; }

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

// value in the high word, smallest index wins a tie: one 64-bit maximum.  Values stay below 2^30 (squared distances and
// cross products of coordinates in [0, 16384])
__device__ __forceinline__ u64 arg_key(uint32_t value, int k) { return ((u64)value << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)k); }
__device__ __forceinline__ int arg_index(u64 key) { return (int)(0xFFFFFFFFu - (uint32_t)key); }
__device__ __forceinline__ uint32_t dist2(int2 a, int2 p) {
  const int dx = p.x - a.x, dy = p.y - a.y;
  return (uint32_t)(dx * dx + dy * dy);
}
__device__ __forceinline__ uint32_t abs_cross(int2 a, int2 b, int2 p) {
  const int c = (b.x - a.x) * (p.y - a.y) - (b.y - a.y) * (p.x - a.x);
  return (uint32_t)(c < 0 ? -c : c);
}

__global__ __launch_bounds__(BLOCK_T) void scan_rows_kernel(const int32_t* __restrict__ rings, const int32_t* __restrict__ counts,
                                                        uint32_t* __restrict__ off, int32_t* __restrict__ kept,
                                                        uint32_t* __restrict__ header, int max_rings, int max_vertices) {
  extern __shared__ u64 part[];                            // [BLOCK_T / 64]
  const int found = counts[0], rows_in = counts[1], written = counts[3], status = counts[4];
  const bool bad_counts = (status & C3D_OUTLINE_ST_BAD_COUNTS) != 0;
  const int rows = bad_counts ? 0 : (rows_in < 0 ? 0 : (rows_in > max_rings ? max_rings : rows_in));
  const int64_t vlimit = written < 0 ? 0 : (written > max_vertices ? max_vertices : written);
  u64 running = 0;
  bool bad = false;
  for (int base = 0; base < rows; base += BLOCK_T * SCAN_ROWS) {
    int n[SCAN_ROWS], cls[SCAN_ROWS];
    u64 mine = 0;
    for (int j = 0; j < SCAN_ROWS; ++j) {
      const int r = base + (int)threadIdx.x * SCAN_ROWS + j;
      n[j] = 0;
      cls[j] = ROW_PASS;
      if (r < rows) {
        const int start = rings[(int64_t)r * 8 + 1], nv = rings[(int64_t)r * 8 + 2];
        if (start >= 0) {
          if (nv >= 0 && (int64_t)start + nv <= vlimit) { cls[j] = 0; n[j] = nv; }
          else cls[j] = ROW_BAD;
        }
      }
      mine += (u64)n[j];
    }
    u64 all;
    u64 at = running + block_excl_scan64(mine, part, &all);
    for (int j = 0; j < SCAN_ROWS; ++j) {
      const int r = base + (int)threadIdx.x * SCAN_ROWS + j;
      if (r < rows) {
        if (cls[j] == 0 && at + (u64)n[j] > (u64)max_vertices) cls[j] = ROW_BAD;   // the ranges overlap: no room for their state
        bad |= cls[j] == ROW_BAD;
        off[r] = (uint32_t)(at < 0xFFFFFFFFull ? at : 0xFFFFFFFFull);
        kept[r] = cls[j];
      }
      at += (u64)n[j];
    }
    running += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    header[WS_ROWS] = (uint32_t)rows;
    header[WS_FOUND] = (uint32_t)found;
    header[WS_STATUS] = (uint32_t)status;
    header[WS_BADCOUNTS] = bad_counts ? 1u : 0u;
  }
  if (bad) atomicOr(header + WS_ERR, 1u);                  // the header was zeroed by the memset before this launch
}

// ----------------------------------------------------------------------------------------------- one wave per ring
// lane k owns vertex k < n, 4 <= n <= 64.  Returns whether the lane's vertex is kept.
__device__ __forceinline__ bool wave_ring(int lane, int n, int2 p, u64 tol2_q) {
  const bool in = lane < n;
  const int2 v0 = make_int2(__shfl(p.x, 0), __shfl(p.y, 0));
  const int B = arg_index(wave_max64(in ? arg_key(dist2(v0, p), lane) : 0ull));
  bool kept = in && (lane == 0 || lane == B), dropped = false;
  int lo = lane > B ? B : 0, hi = lane > B ? n : B;
  for (int round = 0; round < WAVE_LIMIT; ++round) {       // every round but the last keeps a vertex: fewer than n rounds
    const bool act = in && !kept && !dropped;
    const int hb = hi == n ? 0 : hi;
    const int2 a = make_int2(__shfl(p.x, lo), __shfl(p.y, lo)), b = make_int2(__shfl(p.x, hb), __shfl(p.y, hb));
    u64 den = 1, num = 0;
    if (act) num = seg_num(a, b, p, &den);
    int idx = lane;
    for (int d = 1; d < 64; d <<= 1) {                     // suffix maximum within the chord's interior: lanes lo+1 .. hi-1
      const u64 onum = shfl_down64(num, d);
      const int oidx = __shfl_down(idx, d), olo = __shfl_down(lo, d), oact = __shfl_down((int)act, d);
      if (act && lane + d < 64 && oact && olo == lo && onum > num) { num = onum; idx = oidx; }   // a tie keeps the smaller index
    }
    const int first = act ? lo + 1 : lane;
    const u64 bnum = shfl64(num, first);
    const int m = __shfl(idx, first);
    const bool far = act && 16ull * bnum > tol2_q * den;
    if (act) {
      if (!far) dropped = true;
      else if (lane == m) kept = true;
      else if (lane < m) hi = m;
      else lo = m;
    }
    if (!__any(far)) break;
  }
  if (__popcll(__ballot(kept)) <= 2) {                     // a chain of A and B alone: the vertex farthest from their line
    const int2 vB = make_int2(__shfl(p.x, B), __shfl(p.y, B));
    const int third = arg_index(wave_max64(in ? arg_key(abs_cross(v0, vB, p), lane) : 0ull));
    kept = kept || (in && lane == third);
  }
  return kept;
}

__global__ __launch_bounds__(256) void simplify_wave_kernel(const int32_t* __restrict__ rings, const int2* __restrict__ vertices,
                                                            const uint32_t* __restrict__ off, int32_t* __restrict__ kept,
                                                            uint8_t* __restrict__ flags, uint32_t* __restrict__ large,
                                                            uint32_t* __restrict__ header, u64 tol2_q) {
  const int lane = threadIdx.x & 63, rows = (int)header[WS_ROWS];
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += gridDim.x * 4) {   // r is uniform over the wave
    if (kept[r] < 0) continue;
    const int start = rings[(int64_t)r * 8 + 1], n = rings[(int64_t)r * 8 + 2];
    if (n > WAVE_LIMIT) {                                  // for the workgroup tiers; the order of the list is of no consequence
      if (lane == 0) large[atomicAdd(header + WS_LARGE, 1u)] = (uint32_t)r;
      continue;
    }
    const bool in = lane < n;
    const int2 p = in ? vertices[(int64_t)start + lane] : make_int2(0, 0);
    if (__any(in && !coord_ok(p))) {
      if (lane == 0) { kept[r] = ROW_BAD; atomicOr(header + WS_ERR, 1u); }
      continue;
    }
    const bool keep = n <= 3 ? in : wave_ring(lane, n, p, tol2_q);
    if (in) flags[(int64_t)off[r] + lane] = keep ? 1 : 0;
    const int count = __popcll(__ballot(keep));
    if (lane == 0) kept[r] = count;
  }
}

// ------------------------------------------------------------------------------------------ one workgroup per ring
// link[k] >= 0: vertex k is open, link[k] = its chord's first vertex lo; -1: dropped; < -1: kept, ~link[k] = the end of the
// chord that starts at k (n = the closing repeat of vertex 0).  best / idx are used at chord starts only.  Returns the
// kept count; flags_out[k] = kept.  Every thread of the workgroup calls it with the same arguments.
template <class GetP>
__device__ __forceinline__ int block_ring(GetP getP, int* link, int* idx, u64* best, uint8_t* __restrict__ flags_out, int n,
                                          u64 tol2_q, u64* sh_key, int* sh_cnt) {
  const int tid = threadIdx.x, lane = tid & 63;
  int* sh_far = sh_cnt + 1;
  const int2 v0 = getP(0);
  if (tid == 0) { *sh_key = 0; *sh_cnt = 0; }
  __syncthreads();
  {
    u64 key = 0;
    for (int k = tid; k < n; k += BLOCK_T) {
      const u64 c = arg_key(dist2(v0, getP(k)), k);
      key = c > key ? c : key;
    }
    key = wave_max64(key);
    if (lane == 0) atomicMax(sh_key, key);
  }
  __syncthreads();
  const int B = arg_index(*sh_key);
  const int2 vB = getP(B);
  __syncthreads();
  if (tid == 0) *sh_key = 0;                               // for the third vertex below; many barriers lie between
  for (int k = tid; k < n; k += BLOCK_T) {
    if (k == 0 || k == B) {
      link[k] = (k == 0 && B != 0) ? ~B : ~n;
      best[k] = 0;
      idx[k] = INT_MAX;
    } else {
      link[k] = k > B ? B : 0;
    }
  }
  __syncthreads();

  // the steps t (vertex k = BLOCK_T t + tid) in which this wave still has an open vertex: open vertices only close
  int t0 = 0, t1 = (n + BLOCK_T - 1) / BLOCK_T;
  auto chord = [&](int k, int lo, int2* a, int2* b, int* hi) {
    *hi = ~link[lo];
    *a = getP(lo);
    *b = getP(*hi == n ? 0 : *hi);
    (void)k;
  };
  for (int round = 0; round < n; ++round) {                // every round but the last keeps a vertex: fewer than n rounds
    int nt0 = t1, nt1 = t0;
    for (int t = t0; t < t1; ++t) {                        // max
      const int k = t * BLOCK_T + tid, lo = k < n ? link[k] : -1;
      const bool act = lo >= 0;
      const u64 mk = __ballot(act);
      if (!mk) continue;
      nt0 = t < nt0 ? t : nt0;
      nt1 = t + 1;
      u64 num = 0, den;
      if (act) {
        int2 a, b;
        int hi;
        chord(k, lo, &a, &b, &hi);
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
    for (int t = t0; t < t1; ++t) {                        // arg
      const int k = t * BLOCK_T + tid, lo = k < n ? link[k] : -1;
      const bool act = lo >= 0;
      const u64 mk = __ballot(act);
      if (!mk) continue;
      int cand = INT_MAX;
      if (act) {
        int2 a, b;
        int hi;
        u64 den;
        chord(k, lo, &a, &b, &hi);
        if (seg_num(a, b, getP(k), &den) == best[lo]) cand = k;
      }
      const int leader = __ffsll((long long)mk) - 1, lo0 = __shfl(lo, leader);
      if (__ballot(act && lo != lo0) == 0) {
        const int w = wave_min32(cand);
        if (lane == leader && w != INT_MAX) atomicMin(idx + lo0, w);
      } else if (cand != INT_MAX) {
        atomicMin(idx + lo, cand);
      }
    }
    __syncthreads();
    bool any_far = false;
    for (int t = t0; t < t1; ++t) {                        // split: reads chord starts, writes the vertex's own slots
      const int k = t * BLOCK_T + tid, lo = k < n ? link[k] : -1;
      if (lo < 0) continue;
      int2 a, b;
      int hi;
      chord(k, lo, &a, &b, &hi);
      const int64_t dx = b.x - a.x, dy = b.y - a.y;
      const u64 L2 = (u64)(dx * dx + dy * dy), den = L2 ? L2 : 1ull;
      if (!(16ull * best[lo] > tol2_q * den)) { link[k] = -1; continue; }
      any_far = true;
      const int m = idx[lo];
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
      const int k = t * BLOCK_T + tid;
      if (k >= n || link[k] >= -1 || idx[k] != SPLIT_MARK) continue;
      const int lo = (int)best[k];
      link[lo] = ~k;
      best[lo] = 0;
      idx[lo] = INT_MAX;
      best[k] = 0;
      idx[k] = INT_MAX;
    }
    __syncthreads();
  }

  for (int base = 0; base < n; base += BLOCK_T) {
    const int k = base + tid;
    const bool f = k < n && link[k] < -1;
    if (k < n) flags_out[k] = f ? 1 : 0;
    const int c = __popcll(__ballot(f));
    if (lane == 0 && c) atomicAdd(sh_cnt, c);
  }
  __syncthreads();
  int count = *sh_cnt;
  if (count <= 2) {                                        // uniform: the vertex farthest from the line through A and B
    u64 key = 0;
    for (int k = tid; k < n; k += BLOCK_T) {
      const u64 c = arg_key(abs_cross(v0, vB, getP(k)), k);
      key = c > key ? c : key;
    }
    key = wave_max64(key);
    if (lane == 0) atomicMax(sh_key, key);
    __syncthreads();
    const int third = arg_index(*sh_key);
    if (third != 0 && third != B) {
      if (tid == 0) flags_out[third] = 1;
      ++count;
    }
  }
  return count;
}

__global__ __launch_bounds__(BLOCK_T) void simplify_block_kernel(const int32_t* __restrict__ rings, const int2* __restrict__ vertices,
                                                             const uint32_t* __restrict__ off, int32_t* __restrict__ kept,
                                                             uint8_t* __restrict__ flags, int32_t* __restrict__ g_link,
                                                             int32_t* __restrict__ g_idx, u64* __restrict__ g_best,
                                                             const uint32_t* __restrict__ large, uint32_t* __restrict__ header,
                                                             u64 tol2_q) {
  extern __shared__ u64 lds[];                             // best u64 [LDS_LIMIT], link, idx, packed coordinates u32 [LDS_LIMIT],
  u64* s_best = lds;                                       // then the key, the counter and the flag of block_ring
  int* s_link = reinterpret_cast<int*>(lds + LDS_LIMIT);
  int* s_idx = s_link + LDS_LIMIT;
  uint32_t* s_p = reinterpret_cast<uint32_t*>(s_idx + LDS_LIMIT);
  u64* sh_key = reinterpret_cast<u64*>(s_p + LDS_LIMIT);
  int* sh_cnt = reinterpret_cast<int*>(sh_key + 1);
  const uint32_t n_large = header[WS_LARGE];               // the wave kernel listed the valid rows above its limit
  for (uint32_t at = blockIdx.x; at < n_large; at += gridDim.x) {
    const int r = (int)large[at];
    const int64_t start = rings[(int64_t)r * 8 + 1];
    const int n = rings[(int64_t)r * 8 + 2];
    const bool in_lds = n <= LDS_LIMIT;
    __syncthreads();                                       // the ring before is done with the LDS and the flag
    if (threadIdx.x == 0) sh_cnt[1] = 0;
    __syncthreads();
    int bad = 0;
    for (int k = threadIdx.x; k < n; k += BLOCK_T) {
      const int2 p = vertices[start + k];
      bad |= !coord_ok(p);
      if (in_lds) s_p[k] = (uint32_t)p.x | ((uint32_t)p.y << 16);
    }
    if (bad) sh_cnt[1] = 1;                                // every writer stores the same value
    __syncthreads();
    if (sh_cnt[1]) {                                       // the next writer of the flag waits at a barrier first
      if (threadIdx.x == 0) { kept[r] = ROW_BAD; atomicOr(header + WS_ERR, 1u); }
      continue;
    }
    const int64_t o = off[r];
    int count;
    if (in_lds) {
      count = block_ring([&](int k) { const uint32_t v = s_p[k]; return make_int2((int)(v & 0xFFFFu), (int)(v >> 16)); }, s_link,
                         s_idx, s_best, flags + o, n, tol2_q, sh_key, sh_cnt);
    } else {
      count = block_ring([&](int k) { return vertices[start + k]; }, g_link + o, g_idx + o, g_best + o, flags + o, n, tol2_q,
                         sh_key, sh_cnt);
    }
    if (threadIdx.x == 0) kept[r] = count;
  }
}

// start'[r] = kept vertices of the rows before r; counts_out.  One workgroup.
__global__ __launch_bounds__(BLOCK_T) void scan_kept_kernel(const int32_t* __restrict__ kept, uint32_t* __restrict__ startp,
                                                        const uint32_t* __restrict__ header, int32_t* __restrict__ counts_out) {
  extern __shared__ u64 part[];                            // [BLOCK_T / 64]
  const int rows = (int)header[WS_ROWS];
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
      if (r < rows) startp[r] = (uint32_t)at;              // at most the vertices of the valid rows, which scan_rows bounded
      at += (u64)n[j];
    }
    running += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (header[WS_BADCOUNTS]) {
      counts_out[0] = counts_out[1] = counts_out[2] = counts_out[3] = 0;
      counts_out[4] = C3D_OUTLINE_ST_BAD_COUNTS;
    } else {
      counts_out[0] = (int32_t)header[WS_FOUND];
      counts_out[1] = rows;
      counts_out[2] = counts_out[3] = (int32_t)running;
      counts_out[4] = (int32_t)(header[WS_STATUS] | (header[WS_ERR] ? (uint32_t)C3D_SIMPLIFY_ST_BAD_INPUT : 0u));
    }
  }
}

__device__ __forceinline__ void write_row(int32_t* __restrict__ rings_out, int r, const int4 r0, const int4 r1, int start, int n,
                                          int area2) {
  int4* dst = reinterpret_cast<int4*>(rings_out + (int64_t)r * 8);
  dst[0] = make_int4(r0.x, start, n, area2);
  dst[1] = make_int4(r1.x, r1.y, r1.z, r0.z);
}

// rows of rings of up to WAVE_LIMIT vertices, rows that are not simplified, and the zero rows past the table
__global__ __launch_bounds__(256) void scatter_wave_kernel(const int32_t* __restrict__ rings, const int2* __restrict__ vertices,
                                                           const uint32_t* __restrict__ off, const int32_t* __restrict__ kept,
                                                           const uint32_t* __restrict__ startp, const uint8_t* __restrict__ flags,
                                                           const uint32_t* __restrict__ header, int32_t* __restrict__ rings_out,
                                                           int2* __restrict__ vertices_out, int max_rings) {
  const int lane = threadIdx.x & 63, rows = (int)header[WS_ROWS];
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < max_rings; r += gridDim.x * 4) {
    int4* dst = reinterpret_cast<int4*>(rings_out + (int64_t)r * 8);
    if (r >= rows) {
      if (lane < 2) dst[lane] = make_int4(0, 0, 0, 0);
      continue;
    }
    const int4 r0 = reinterpret_cast<const int4*>(rings + (int64_t)r * 8)[0], r1 = reinterpret_cast<const int4*>(rings + (int64_t)r * 8)[1];
    const int count = kept[r];
    if (count < 0) {
      if (lane == 0) write_row(rings_out, r, r0, r1, -1, 0, 0);
      continue;
    }
    const int n = r0.z;
    if (n > WAVE_LIMIT) continue;
    const bool f = lane < n && flags[(int64_t)off[r] + lane];
    const int2 p = f ? vertices[(int64_t)r0.y + lane] : make_int2(0, 0);
    const u64 mask = __ballot(f), below = mask & ((1ull << lane) - 1ull);
    const u64 from = below ? below : mask;                 // the kept vertex before this one, cyclically
    const int prev = from ? 63 - __clzll((long long)from) : lane;
    const int px = __shfl(p.x, prev), py = __shfl(p.y, prev);
    const int64_t at = (int64_t)startp[r];
    if (f) vertices_out[at + __popcll(below)] = p;
    const uint32_t area2 = wave_sum32(f ? (uint32_t)(px * p.y - p.x * py) : 0u);   // modular: exact if the total fits i32
    if (lane == 0) write_row(rings_out, r, r0, r1, (int)at, count, (int)area2);
  }
}

__global__ __launch_bounds__(256) void scatter_block_kernel(const int32_t* __restrict__ rings, const int2* __restrict__ vertices,
                                                            const uint32_t* __restrict__ off, const int32_t* __restrict__ kept,
                                                            const uint32_t* __restrict__ startp, const uint8_t* __restrict__ flags,
                                                            const uint32_t* __restrict__ large, const uint32_t* __restrict__ header,
                                                            int32_t* __restrict__ rings_out, int2* __restrict__ vertices_out) {
  extern __shared__ u64 part[];                            // [4], then the area
  uint32_t& sh_area = *reinterpret_cast<uint32_t*>(part + 4);
  const uint32_t n_large = header[WS_LARGE];
  for (uint32_t li = blockIdx.x; li < n_large; li += gridDim.x) {
    const int r = (int)large[li];
    const int count = kept[r];
    if (count < 0) continue;                               // a coordinate out of range: the wave kernel writes this row
    const int4 r0 = reinterpret_cast<const int4*>(rings + (int64_t)r * 8)[0], r1 = reinterpret_cast<const int4*>(rings + (int64_t)r * 8)[1];
    const int n = r0.z;
    const int64_t o = off[r], at = startp[r];
    if (threadIdx.x == 0) sh_area = 0;
    u64 run = 0;
    for (int base = 0; base < n; base += 256) {
      const int k = base + (int)threadIdx.x;
      const bool f = k < n && flags[o + k];
      u64 all;
      const u64 pos = run + block_excl_scan64(f ? 1ull : 0ull, part, &all);
      if (f) vertices_out[at + (int64_t)pos] = vertices[(int64_t)r0.y + k];
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
    if (threadIdx.x == 0) write_row(rings_out, r, r0, r1, (int)at, count, (int)sh_area);
    __syncthreads();
  }
}

unsigned grid_for(int64_t items, int per_block) {
  int64_t g = (items + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > MAX_GRID ? MAX_GRID : g));
}

}  // namespace

extern "C" void c3d_outlines_simplify_limits(int32_t out[2]) {
  if (!out) return;
  out[0] = WAVE_LIMIT;
  out[1] = LDS_LIMIT;
}

extern "C" int64_t c3d_outlines_simplify_ws_bytes(int32_t max_rings, int32_t max_vertices) {
  if (max_rings < 1 || max_vertices < 1) return C3D_E_BADARG;
  return workspace_plan(max_rings, max_vertices).bytes;
}

extern "C" int c3d_outlines_simplify(const int32_t* rings, const int32_t* vertices, const int32_t* counts, int32_t max_rings,
                                     int32_t max_vertices, int64_t tol2_q, int32_t* rings_out, int32_t* vertices_out,
                                     int32_t* counts_out, void* ws, void* stream) {
  if (!rings || !vertices || !counts || !rings_out || !vertices_out || !counts_out || !ws) return C3D_E_BADARG;
  if (max_rings < 1 || max_vertices < 1 || tol2_q < 0 || tol2_q > C3D_SIMPLIFY_TOL2_Q_MAX) return C3D_E_BADARG;
  const Workspace w = workspace_plan(max_rings, max_vertices);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  uint32_t* header = reinterpret_cast<uint32_t*>(base);
  uint32_t* off = reinterpret_cast<uint32_t*>(base + w.off);
  int32_t* kept = reinterpret_cast<int32_t*>(base + w.kept);
  uint32_t* startp = reinterpret_cast<uint32_t*>(base + w.startp);
  uint32_t* large = reinterpret_cast<uint32_t*>(base + w.large);
  uint8_t* flags = reinterpret_cast<uint8_t*>(base + w.flags);
  int32_t* link = reinterpret_cast<int32_t*>(base + w.link);
  int32_t* idx = reinterpret_cast<int32_t*>(base + w.idx);
  u64* best = reinterpret_cast<u64*>(base + w.best);
  const int2* v_in = reinterpret_cast<const int2*>(vertices);
  int2* v_out = reinterpret_cast<int2*>(vertices_out);

  // only the header: every other word of the workspace is written by the call before the call reads it
  hipError_t e = hipMemsetAsync(base, 0, 256, st);
  if (e != hipSuccess) return (int)e;
  // the ring count is known on the device only: grids are sized by max_rings and surplus waves and workgroups return
  const unsigned g_wave = grid_for(max_rings, 4), g_block = grid_for(max_rings, 1);
  int rc = c3d_launch_lds<scan_rows_kernel>(dim3(1), dim3(BLOCK_T), BLOCK_T / 8, st, rings, counts, off, kept, header, (int)max_rings,
                                            (int)max_vertices);
  if (rc) return rc;
  rc = c3d_launch_lds<simplify_wave_kernel>(dim3(g_wave), dim3(256), 0, st, rings, v_in, (const uint32_t*)off, kept, flags, large,
                                            header, (u64)tol2_q);
  if (rc) return rc;
  rc = c3d_launch_lds<simplify_block_kernel>(dim3(g_block), dim3(BLOCK_T), LDS_BYTES, st, rings, v_in, (const uint32_t*)off, kept, flags,
                                             link, idx, best, (const uint32_t*)large, header, (u64)tol2_q);
  if (rc) return rc;
  rc = c3d_launch_lds<scan_kept_kernel>(dim3(1), dim3(BLOCK_T), BLOCK_T / 8, st, (const int32_t*)kept, startp, (const uint32_t*)header, counts_out);
  if (rc) return rc;
  rc = c3d_launch_lds<scatter_wave_kernel>(dim3(g_wave), dim3(256), 0, st, rings, v_in, (const uint32_t*)off, (const int32_t*)kept,
                                           (const uint32_t*)startp, (const uint8_t*)flags, (const uint32_t*)header, rings_out, v_out,
                                           (int)max_rings);
  if (rc) return rc;
  return c3d_launch_lds<scatter_block_kernel>(dim3(g_block), dim3(256), 40, st, rings, v_in, (const uint32_t*)off, (const int32_t*)kept,
                                              (const uint32_t*)startp, (const uint8_t*)flags, (const uint32_t*)large, (const uint32_t*)header, rings_out,
                                              v_out);
}
