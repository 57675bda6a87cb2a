// Exact squared Euclidean distance transform of a u8 mask in HBM, and the boundary counts of two masks built on it
// (change3d_amd/boundary_metrics.py).  The contract is in include/change3d_hip.h; the reference has no counterpart.  Integers
// everywhere, nothing read back by the host, no workgroup waits for another, every loop bounded, every workspace word is
// written before it is read: two runs agree bit for bit on any workspace.
//
// c3d_scene_edt is three launches.  The transform separates: g[y][x], the distance along column x to the nearest site, then
// dist2[y][x] = min over x' of (x - x')^2 + g[y][x']^2.
//
//   1 edt_bits   a column is cut into chunks of CHUNK = 64 rows; a lane reads the 64 mask bytes of one (chunk, column) -- a wave
//                reads 64 consecutive bytes of a row at a time -- and stores which of them are sites as ONE u64.
//   2 edt_cols   a lane owns one (chunk, column) again.  The carries of the two scans are the nearest site row above and below
//                the chunk: the lane walks the u64s of the neighbouring chunks until one is not zero (clz / ctz give the row),
//                at most `reach` chunks with a cap, at most all Hs / 64 <= 256 of them without; BORDER puts a site at rows -1
//                and Hs.  Inside the chunk the nearest site above and below a row are a clz and a ctz of the lane's own u64.
//                g goes out as u16 (0xffff: no site in reach), coalesced along x.
//   3 edt_rows   one workgroup per row and segment of SEG = 1024 pixels.  The g^2 of the window the segment can see -- the
//                whole row without a cap, the segment +- isqrt(cap2) with one -- sits in LDS as i32 (at most 64 KiB).  A lane
//                takes the pixels tid, tid + 256, ..: neighbouring lanes read neighbouring banks at every step.  It searches
//                outward, k = 1, 2, .., both sides per step, while k^2 is below its best so far and k <= isqrt(cap2).  BORDER adds
//                the sites (y, -1) and (y, Ws) as two candidates.
//
// The uncapped worst case is a scene with (nearly) no site: every lane walks to the end of its row, O(Ws) LDS reads per
// pixel.  That form is kept, as scene_simplify keeps its serpentine: measured in profiles/scene_edt.txt (one site in a corner).
//
// c3d_boundary_counts is one memset (the eight accumulators) and eight launches: the three above on both masks at once
// (blockIdx.z picks the mask; capped at d2), boundary_band (the band counts, the contour maps Pc / Gc as u8), the three again
// on the two contour maps with INVERT and a cap of tau2 -- the row pass then counts the hits over the OTHER contour map in place
// of storing distances -- and boundary_finalise, one thread, which writes `counts` and adds them into `totals`.
#include "scene_wave.h"
#include "../../include/change3d_hip.h"

namespace {

using namespace c3d_wave;

typedef unsigned long long u64;

constexpr int CHUNK = 64;                                  // rows per column-pass chunk: one bit each in a u64
constexpr int SEG = 1024;                                  // pixels per row-pass workgroup: 256 lanes x 4
constexpr int MAX_SIDE = 16384;
constexpr int G_NONE = 0xffff;                             // g: no site within reach in this column
constexpr int ROW_NONE = 1 << 20;                          // a carry that holds no site: farther than any row
constexpr int BAND_GRID = 256;                             // workgroups of boundary_band: one per CU, four atomics each
constexpr int WS_HEADER = 256;                             // c3d_boundary_counts: u64 accumulators in front
enum { ACC_INTER = 0, ACC_UNION, ACC_PC, ACC_GC, ACC_HIT_P, ACC_HIT_G };   // the order of the accumulators, not of `counts`

struct Job {
  const uint8_t* mask;                                     // [Hs][Ws]
  int32_t* dist2;                                          // [Hs][Ws]; unused where `sel` is set
  const uint8_t* sel;                                      // [Hs][Ws] or NULL: count the pixels of `sel` within the cap instead
  u64* acc;                                                // where that count is added
  u64* bits;                                               // [n_chunks][Ws]
  uint16_t* g;                                             // [Hs][Ws]
  int32_t flags;
};
struct Jobs { Job j[2]; };

__global__ __launch_bounds__(256) void edt_bits_kernel(const Jobs jobs, int Hs, int Ws) {
  const Job J = jobs.j[blockIdx.z];
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= Ws) return;
  const int c = blockIdx.y, y0 = c * CHUNK;
  const int rows = Hs - y0 < CHUNK ? Hs - y0 : CHUNK;
  const bool invert = (J.flags & C3D_EDT_INVERT) != 0;
  const uint8_t* p = J.mask + (int64_t)y0 * Ws + x;
  u64 m = 0;
#pragma unroll 8
  for (int r = 0; r < rows; ++r) {
    const bool site = (p[(int64_t)r * Ws] != 0) == invert;
    m |= (u64)site << r;
  }
  J.bits[(int64_t)c * Ws + x] = m;                         // rows past Hs are no sites
}

__global__ __launch_bounds__(256) void edt_cols_kernel(const Jobs jobs, int Hs, int Ws, int n_chunks, int reach) {
  const Job J = jobs.j[blockIdx.z];
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= Ws) return;
  const int c = blockIdx.y, y0 = c * CHUNK;
  const int rows = Hs - y0 < CHUNK ? Hs - y0 : CHUNK;
  const bool border = (J.flags & C3D_EDT_BORDER) != 0;
  const u64 m = J.bits[(int64_t)c * Ws + x];
  int up = border ? -1 : -ROW_NONE, dn = border ? Hs : ROW_NONE;       // the nearest site row above / below the chunk
  for (int k = c - 1, n = 0; k >= 0 && n < reach; --k, ++n) {
    const u64 b = J.bits[(int64_t)k * Ws + x];
    if (b) { up = k * CHUNK + 63 - __builtin_clzll(b); break; }
  }
  for (int k = c + 1, n = 0; k < n_chunks && n < reach; ++k, ++n) {
    const u64 b = J.bits[(int64_t)k * Ws + x];
    if (b) { dn = k * CHUNK + __builtin_ctzll(b); break; }
  }
  uint16_t* out = J.g + (int64_t)y0 * Ws + x;
  for (int r = 0; r < rows; ++r) {
    const int y = y0 + r;
    const u64 lo = m & (~0ull >> (63 - r)), hi = m >> r;                // the sites at rows <= r, >= r of the chunk
    const int d_up = lo ? r - (63 - __builtin_clzll(lo)) : y - up;
    const int d_dn = hi ? __builtin_ctzll(hi) : dn - y;
    int g = d_up < d_dn ? d_up : d_dn;
    if (g > G_NONE) g = G_NONE;                                          // a true distance is at most 16384
    out[(int64_t)r * Ws] = (uint16_t)g;
  }
}


// acc[k] += the sum of v[k] over the workgroup of 256, k < K: one atomic per workgroup and count, none where the sum is 0 --
// a few thousand adds to one address cost more than the pass they end.  A workgroup's sum stays below 2^32 (its pixels do).
template <int K>
__device__ __forceinline__ void block_add(u64* acc, const uint32_t (&v)[K], uint32_t* s_part /* [4 * K] */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint32_t sum = wave_sum32(v[k]);
    if (lane == 0) s_part[wave * K + k] = sum;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const uint32_t sum = s_part[threadIdx.x] + s_part[K + threadIdx.x] + s_part[2 * K + threadIdx.x] + s_part[3 * K + threadIdx.x];
    if (sum) atomicAdd(acc + threadIdx.x, (u64)sum);
  }
}

// `reach` = isqrt(cap2) with a cap, Ws without.  Dynamic LDS (c3d_launch_lds leaves no room for static LDS beside it): the four
// partial sums of block_add, then the window of the segment, i32 each.
__global__ __launch_bounds__(256) void edt_rows_kernel(const Jobs jobs, int Hs, int Ws, int cap2, int reach) {
  extern __shared__ int32_t lds_rows[];
  uint32_t* s_part = reinterpret_cast<uint32_t*>(lds_rows);
  int32_t* s_g2 = lds_rows + 4;
  const Job J = jobs.j[blockIdx.z];
  const int tid = threadIdx.x, y = blockIdx.y;
  const int seg0 = blockIdx.x * SEG, seg1 = seg0 + SEG < Ws ? seg0 + SEG : Ws;
  const int w0 = seg0 - reach > 0 ? seg0 - reach : 0, w1 = seg1 + reach < Ws ? seg1 + reach : Ws;
  const uint16_t* grow = J.g + (int64_t)y * Ws;
  for (int i = w0 + tid; i < w1; i += 256) {
    const int v = grow[i];
    s_g2[i - w0] = v == G_NONE ? C3D_EDT_FAR : v * v;
  }
  __syncthreads();
  const bool border = (J.flags & C3D_EDT_BORDER) != 0;
  const int limit = cap2 ? cap2 : C3D_EDT_FAR - 1;          // every true value is below FAR
  uint32_t hits = 0;
  for (int x = seg0 + tid; x < seg1; x += 256) {
    int best = s_g2[x - w0];
    if (border) {                                          // the sites (y, -1) and (y, Ws)
      const int a = (x + 1) * (x + 1), b = (Ws - x) * (Ws - x);
      best = best < a ? best : a;
      best = best < b ? best : b;
    }
    const int left = x - w0, right = w1 - 1 - x;
    int kmax = left > right ? left : right;
    if (kmax > reach) kmax = reach;
    for (int k = 1; k <= kmax && k * k < best; ++k) {
      const int k2 = k * k;
      if (k <= left) { const int v = k2 + s_g2[x - k - w0]; best = best < v ? best : v; }
      if (k <= right) { const int v = k2 + s_g2[x + k - w0]; best = best < v ? best : v; }
    }
    const int out = best > limit ? C3D_EDT_FAR : best;
    if (J.sel) hits += (J.sel[(int64_t)y * Ws + x] != 0 && out != C3D_EDT_FAR) ? 1u : 0u;
    else J.dist2[(int64_t)y * Ws + x] = out;
  }
  if (J.sel) {                                             // uniform over the workgroup
    const uint32_t v[1] = {hits};
    block_add<1>(J.acc, v, s_part);
  }
}

// Pd = P and dP <= d2, Gd likewise; Pc = P and dP == 1, Gc likewise (d2 >= 1, so a transform capped at d2 decides all four)
__global__ __launch_bounds__(256) void boundary_band_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt,
                                                            const int32_t* __restrict__ dP, const int32_t* __restrict__ dG,
                                                            int64_t N, int d2, int vec, uint8_t* __restrict__ Pc,
                                                            uint8_t* __restrict__ Gc, u64* __restrict__ acc) {
  extern __shared__ uint32_t s_part[];                     // [16]
  uint32_t n[4] = {0u, 0u, 0u, 0u};                        // inter, union, |Pc|, |Gc|: ACC_INTER .. ACC_GC but for the hits
  const int64_t quads = (N + 3) / 4;                       // a thread takes 4 consecutive pixels: one load per map where aligned
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
    const int64_t i0 = q * 4;
    uint32_t p4 = 0, g4 = 0;
    int a[4], b[4];
    if (vec && i0 + 3 < N) {
      p4 = *reinterpret_cast<const uint32_t*>(pred + i0);
      g4 = *reinterpret_cast<const uint32_t*>(gt + i0);
      const int4 va = *reinterpret_cast<const int4*>(dP + i0), vb = *reinterpret_cast<const int4*>(dG + i0);
      a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w;
      b[0] = vb.x; b[1] = vb.y; b[2] = vb.z; b[3] = vb.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = i0 + j < N;
        p4 |= (uint32_t)(in ? pred[i0 + j] : 0) << (8 * j);
        g4 |= (uint32_t)(in ? gt[i0 + j] : 0) << (8 * j);
        a[j] = in ? dP[i0 + j] : 0;
        b[j] = in ? dG[i0 + j] : 0;
      }
    }
    uint32_t pc4 = 0, gc4 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool p = ((p4 >> (8 * j)) & 0xffu) != 0, g = ((g4 >> (8 * j)) & 0xffu) != 0;
      const bool pd = p && a[j] <= d2, gd = g && b[j] <= d2, pc = p && a[j] == 1, gc = g && b[j] == 1;
      n[0] += pd && gd;
      n[1] += pd || gd;
      n[2] += pc;
      n[3] += gc;
      pc4 |= (uint32_t)pc << (8 * j);
      gc4 |= (uint32_t)gc << (8 * j);
    }
    if (i0 + 3 < N) {                                      // Pc and Gc are rows of the workspace: 256-byte aligned
      *reinterpret_cast<uint32_t*>(Pc + i0) = pc4;
      *reinterpret_cast<uint32_t*>(Gc + i0) = gc4;
    } else {
      for (int j = 0; i0 + j < N; ++j) {
        Pc[i0 + j] = (uint8_t)(pc4 >> (8 * j));
        Gc[i0 + j] = (uint8_t)(gc4 >> (8 * j));
      }
    }
  }
  block_add<4>(acc, n, s_part);
}

__global__ void boundary_finalise_kernel(const u64* __restrict__ acc, int64_t* __restrict__ counts, int64_t* __restrict__ totals) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int64_t c[8] = {(int64_t)acc[ACC_INTER], (int64_t)acc[ACC_UNION], (int64_t)acc[ACC_PC], (int64_t)acc[ACC_HIT_P],
                        (int64_t)acc[ACC_GC],    (int64_t)acc[ACC_HIT_G], 1, 0};
  for (int k = 0; k < 8; ++k) {
    counts[k] = c[k];
    if (totals) totals[k] += c[k];
  }
}

int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }
int chunks_of(int Hs) { return (Hs + CHUNK - 1) / CHUNK; }
int64_t bits_bytes(int Hs, int Ws) { return align256((int64_t)chunks_of(Hs) * Ws * 8); }
int64_t g_bytes(int Hs, int Ws) { return align256((int64_t)Hs * Ws * 2); }

int isqrt_i(int v) {                                       // floor(sqrt(v)), v >= 0
  int r = 0;
  while ((int64_t)(r + 1) * (r + 1) <= v) ++r;
  return r;
}

int size_code(int Hs, int Ws) {
  if (Hs < 1 || Ws < 1) return C3D_E_BADARG;
  if (Hs > MAX_SIDE || Ws > MAX_SIDE) return C3D_E_UNSUPPORTED;
  return 0;
}

// the three launches on `n` masks of one size
int run_edt(const Jobs& jobs, int n, int Hs, int Ws, int cap2, hipStream_t st) {
  const int n_chunks = chunks_of(Hs), r = cap2 ? isqrt_i(cap2) : 0;
  const int reach_px = cap2 && r < Ws ? r : Ws;
  const int reach_chunks = cap2 ? (r + CHUNK - 1) / CHUNK : n_chunks;
  const dim3 cgrid((Ws + 255) / 256, n_chunks, n);
  int rc = c3d_launch_lds<edt_bits_kernel>(cgrid, dim3(256), 0, st, jobs, Hs, Ws);
  if (rc) return rc;
  rc = c3d_launch_lds<edt_cols_kernel>(cgrid, dim3(256), 0, st, jobs, Hs, Ws, n_chunks, reach_chunks);
  if (rc) return rc;
  const int64_t window = (int64_t)SEG + 2 * (int64_t)reach_px;
  const size_t lds = 16 + (size_t)(window < Ws ? window : Ws) * 4;
  return c3d_launch_lds<edt_rows_kernel>(dim3((Ws + SEG - 1) / SEG, Hs, n), dim3(256), lds, st, jobs, Hs, Ws, cap2, reach_px);
}

}  // namespace

extern "C" int64_t c3d_scene_edt_ws_bytes(int32_t Hs, int32_t Ws) {
  const int code = size_code(Hs, Ws);
  return code ? code : bits_bytes(Hs, Ws) + g_bytes(Hs, Ws);
}

extern "C" int c3d_scene_edt_tile(int32_t out[2]) {
  if (!out) return C3D_E_BADARG;
  out[0] = CHUNK;
  out[1] = SEG;
  return 0;
}

extern "C" int c3d_scene_edt(const uint8_t* mask, int32_t Hs, int32_t Ws, int32_t flags, int32_t cap2, int32_t* dist2, void* ws,
                             void* stream) {
  if (!mask || !dist2 || !ws || (flags & ~(C3D_EDT_INVERT | C3D_EDT_BORDER)) || cap2 < 0) return C3D_E_BADARG;
  const int code = size_code(Hs, Ws);
  if (code) return code;
  char* base = static_cast<char*>(ws);
  Jobs jobs = {};
  jobs.j[0].mask = mask;
  jobs.j[0].dist2 = dist2;
  jobs.j[0].bits = reinterpret_cast<u64*>(base);
  jobs.j[0].g = reinterpret_cast<uint16_t*>(base + bits_bytes(Hs, Ws));
  jobs.j[0].flags = flags;
  return run_edt(jobs, 1, Hs, Ws, cap2, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int64_t c3d_boundary_counts_ws_bytes(int32_t Hs, int32_t Ws) {
  const int code = size_code(Hs, Ws);
  if (code) return code;
  const int64_t N = (int64_t)Hs * Ws;
  return WS_HEADER + 2 * bits_bytes(Hs, Ws) + 2 * g_bytes(Hs, Ws) + 2 * align256(N * 4) + 2 * align256(N);
}

extern "C" int c3d_boundary_counts(const uint8_t* pred, const uint8_t* gt, int32_t Hs, int32_t Ws, int32_t d2, int32_t tau2,
                                   int32_t flags, int64_t* counts, int64_t* totals, void* ws, void* stream) {
  if (!pred || !gt || !counts || !ws || (flags & ~C3D_EDT_BORDER)) return C3D_E_BADARG;
  if (d2 < 1 || d2 > C3D_BOUNDARY_R2_MAX || tau2 < 1 || tau2 > C3D_BOUNDARY_R2_MAX) return C3D_E_BADARG;
  const int code = size_code(Hs, Ws);
  if (code) return code;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t N = (int64_t)Hs * Ws;
  char* at = static_cast<char*>(ws);
  u64* acc = reinterpret_cast<u64*>(at);
  at += WS_HEADER;
  Jobs jobs = {};
  for (int k = 0; k < 2; ++k, at += bits_bytes(Hs, Ws)) jobs.j[k].bits = reinterpret_cast<u64*>(at);
  for (int k = 0; k < 2; ++k, at += g_bytes(Hs, Ws)) jobs.j[k].g = reinterpret_cast<uint16_t*>(at);
  int32_t* dP = reinterpret_cast<int32_t*>(at);
  int32_t* dG = reinterpret_cast<int32_t*>(at + align256(N * 4));
  at += 2 * align256(N * 4);
  uint8_t* Pc = reinterpret_cast<uint8_t*>(at);
  uint8_t* Gc = reinterpret_cast<uint8_t*>(at + align256(N));

  hipError_t e = hipMemsetAsync(acc, 0, WS_HEADER, st);
  if (e != hipSuccess) return (int)e;
  jobs.j[0].mask = pred; jobs.j[0].dist2 = dP; jobs.j[0].flags = flags;
  jobs.j[1].mask = gt;   jobs.j[1].dist2 = dG; jobs.j[1].flags = flags;
  int rc = run_edt(jobs, 2, Hs, Ws, d2, st);
  if (rc) return rc;
  int64_t grid = (N + 4095) / 4096;                        // four quads of pixels per thread and more, up to BAND_GRID workgroups
  grid = grid < 1 ? 1 : (grid > BAND_GRID ? BAND_GRID : grid);
  const int vec = (reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(gt)) % 4 == 0 ? 1 : 0;
  rc = c3d_launch_lds<boundary_band_kernel>(dim3((unsigned)grid), dim3(256), 64, st, pred, gt, (const int32_t*)dP, (const int32_t*)dG,
                                            N, (int)d2, vec, Pc, Gc, acc);
  if (rc) return rc;
  // eG over Pc and eP over Gc: the contour distances never take the BORDER bit
  jobs.j[0].mask = Gc; jobs.j[0].dist2 = nullptr; jobs.j[0].sel = Pc; jobs.j[0].acc = acc + ACC_HIT_P; jobs.j[0].flags = C3D_EDT_INVERT;
  jobs.j[1].mask = Pc; jobs.j[1].dist2 = nullptr; jobs.j[1].sel = Gc; jobs.j[1].acc = acc + ACC_HIT_G; jobs.j[1].flags = C3D_EDT_INVERT;
  rc = run_edt(jobs, 2, Hs, Ws, tau2, st);
  if (rc) return rc;
  return c3d_launch_lds<boundary_finalise_kernel>(dim3(1), dim3(64), 0, st, (const u64*)acc, counts, totals);
}
