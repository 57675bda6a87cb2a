// Touching objects of a scene map split apart (change3d_amd/infer.py, predict(objects=True, split=R)): the mask is eroded by
// the radius -- its exact distance transform, csrc/scene_edt.hip, capped at r2 -- the components of what is left are the seeds,
// and every seed grows back inside the mask by geodesic distance; the pieces then go through the tail of c3d_scene_objects
// unchanged.  The contract is in include/change3d_hip.h; the reference has no counterpart.  Integers and integer atomics only,
// nothing read back by the host, no workgroup waits for another, every loop capped, every workspace word written before it is
// read.
//
//   edt (3 launches), core          dist2 capped at r2; core = mask != 0 and dist2 > r2 as a u8 map.  Not with r2 == 0.
//   label core, label mask          the union-find labelling of scene_objects.hip (c3d_detail_label_roots, 3 launches each):
//                                   S[p] = first pixel of p's seed = its id, Cm[p] = first pixel of p's component.  With r2 == 0
//                                   the two are one map and one labelling.
//   seed_keys                       key[p] = (d << 32) | id as one u64: (0, S[p]) on a seed pixel, UNREACHED on the rest of the
//                                   mask, BG outside it; counts the seeds and marks the components that hold one.
//   grow x max_rounds               below.
//   piece_first, piece_roots        first[id] = the smallest index that seed id reached (atomicMin); root[p] = first[id(p)], or
//                                   Cm[p] in a component without a seed; the areas per root.  That is the map label_flatten
//                                   leaves, so
//   c3d_detail_objects_tail         numbers, measures and paints the pieces (6 launches), and split_info writes `info`.
//
// Growth.  key(p) = min(key(p), min over the neighbours q of p in the mask of key(q) + (1 << 32)) has one fixed point below the
// start, and every order of relaxations that ends reaches it: keys only decrease, and every key ever stored is the length of a
// real path to the seed it names.  One workgroup owns a 64 x 64 tile.  It loads the tile and a one-pixel halo into LDS
// (66 x 66 u64, 34 KiB; 64-bit agent-scope atomic loads, so a key that the neighbouring workgroup is storing is seen whole, old
// or new) and relaxes it to its LOCAL fixed point:
//   * a wave owns a band of 16 rows and a lane a column.  Per iteration the wave walks its band down, relaxing every row from
//     the row above, then up, relaxing from the row below: one pass carries a value through the whole band.
//   * along the row the relaxation is a min-plus scan with slope 1 over each run of mask pixels: log-step shuffles, 6 forward
//     and 6 backward, exact in one go.  A row that took nothing from the row above (ballot) skips its scan: it is still closed
//     from the last time.  That is what makes an iteration cheap once the front has passed: 1 (4-conn.) or 3 (8-conn.)
//     ds_read_b64 of the neighbour row, one of the own row, two compares.
//   * the rows just outside a band belong to other waves.  A wave copies them into rows of its own before the barrier that
//     starts the iteration and reads the copies, so that no wave reads an LDS word while another writes it.
//   * the loop ends when an iteration moved nothing in any wave, or after 64 * 64 iterations (then the tile counts as moved).
// A wave instruction touches one LDS row: 64 consecutive u64, 256 B per 32-lane half = one bank row each, conflict-free for
// ds_read_b64 at offsets 0, 8 and 16 B, and 128 B per 16-lane group for ds_write_b64 likewise (tools/lds_bank_model.py 'r64':
// 2 cycles).  So the pitch is the plain 66 u64 and needs no padding.
// A tile whose interior moved stores it back, raises the round's flag and its own byte of the round's dirty map.  In round k
// a tile runs only if itself or one of its 8 neighbours was dirty in round k-1, and every workgroup of round k returns at
// once when round k-1 raised no flag.  Flags and dirty maps rotate through three slots (k-1 read, k written, k+1 cleared), so no
// launch reads a word that the same launch clears.  A round that moved nothing read a state that nobody changed: the fixed point.
#include <climits>

#include "common.h"
#include "scene_detail.h"
#include "../../include/change3d_hip.h"

namespace {

typedef unsigned long long u64;

constexpr int T = 64;                                      // tile extent, both ways: a lane per column
constexpr int PITCH = T + 2, LROWS = T + 2;                // the tile with its halo
constexpr int BAND = T / 4;                                // rows per wave
constexpr int R2_MAX = 1 << 20, ROUNDS_MAX = 65536, EDT_SIDE_MAX = 16384;
constexpr u64 ONE = 1ull << 32;
constexpr u64 BG = ~0ull;                                  // not in the mask
constexpr u64 UNREACHED = 0x7fffffffffffffffull;           // in the mask, no seed yet; every real key is below (d < 2^31 - 1)
constexpr size_t GROW_LDS = (size_t)(LROWS * PITCH + 4 * 2 * PITCH) * 8 + 16;

// header words of the workspace (after the two of scene_objects.hip)
enum { H_SEEDS = C3D_DETAIL_HEADER_FREE, H_ROUNDS, H_FLAG /* 3 words */ };

struct Plan {
  int64_t S, key, first, core, seeded, dirty, edt, bytes;  // byte offsets; dist2 lives where the keys go later
  int64_t n_tiles;
};

Plan plan_for(int Hs, int Ws, int n_cls) {
  auto up = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  const int64_t N = (int64_t)Hs * Ws;
  Plan p;
  p.n_tiles = (int64_t)((Hs + T - 1) / T) * ((Ws + T - 1) / T);
  p.S = c3d_detail_label_ws_bytes(N, n_cls);
  p.key = p.S + up(N * 4);
  p.first = p.key + up(N * 8);
  p.core = p.first + up(N * 4);
  p.seeded = p.core + up(N);
  p.dirty = p.seeded + up(N);
  p.edt = p.dirty + up(3 * p.n_tiles);
  const int64_t e = c3d_scene_edt_ws_bytes(Hs, Ws);        // < 0 past the transform's limits: r2 > 0 is refused there
  p.bytes = p.edt + (e > 0 ? up(e) : 0);
  return p;
}

__device__ __forceinline__ u64 ld_key(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_key(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u64 min64(u64 a, u64 b) { return a < b ? a : b; }

__global__ __launch_bounds__(256) void core_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ dist2,
                                                   uint8_t* __restrict__ core, int64_t N, int r2) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256)
    core[i] = mask[i] != 0 && dist2[i] > r2 ? 1 : 0;
}

__global__ __launch_bounds__(256) void seed_keys_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ S,
                                                        const int32_t* __restrict__ Cm, u64* __restrict__ key,
                                                        uint8_t* __restrict__ seeded, uint32_t* __restrict__ header, int64_t N) {
  if (blockIdx.x == 0 && threadIdx.x == 0) header[H_FLAG] = 1u;   // "round 0 changed something": round 1 runs
  for (int64_t base = (int64_t)blockIdx.x * 256; base < N; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    bool head = false;
    if (i < N) {
      const int s = S[i];
      key[i] = !mask[i] ? BG : (s >= 0 ? (u64)(uint32_t)s : UNREACHED);
      head = s == (int32_t)i;                              // the first pixel of a seed: the seed's id
      if (head) {
        const int c = Cm[i];
        if (c >= 0 && c < N) seeded[c] = 1;
      }
    }
    const u64 b = __ballot(head);
    if (b && (threadIdx.x & 63) == 0) atomicAdd(header + H_SEEDS, (uint32_t)__popcll(b));
  }
}

// One relaxation of interior row y of the tile from the row `nb` (the row above or below, or the wave's copy of it), then
// along the row.  Wave-uniform control flow.  Returns whether the row changed.
__device__ __forceinline__ bool relax_row(u64* row, const u64* nb, int lane, int conn8, bool force) {
  // the lanes of a wave talk through LDS here (a lane reads what its neighbours stored for the row before): the hardware keeps
  // a wave's LDS instructions in order, the fences keep the compiler from moving them across this point
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const u64 own = row[lane + 1];
  u64 c = nb[lane + 1];
  if (conn8) c = min64(c, min64(nb[lane], nb[lane + 2]));
  if (lane == 0) c = min64(c, row[0]);                     // the halo columns: constant during the launch
  if (lane == T - 1) c = min64(c, row[T + 1]);
  const bool fg = own != BG;
  u64 v = own;
  if (fg && c < UNREACHED) v = min64(own, c + ONE);
  const u64 m = __ballot(fg);
  if (!m || (!force && !__ballot(v != own))) return false;
  const u64 gaps = ~m;
  const u64 gl = gaps & ((1ull << lane) - 1ull), gr = gaps & ~((2ull << lane) - 1ull);   // 2 << 63 wraps to 0: no lane right of 63
  const int s = gl ? 64 - __clzll((long long)gl) : 0;      // the run of mask pixels that holds this lane: [s, e]
  const int e = gr ? __ffsll((long long)gr) - 2 : T - 1;
#pragma unroll
  for (int d = 1; d < T; d <<= 1) {
    const u64 o = __shfl_up(v, (unsigned)d, 64);
    if (fg && lane - d >= s && o < UNREACHED) v = min64(v, o + (u64)d * ONE);
  }
#pragma unroll
  for (int d = 1; d < T; d <<= 1) {
    const u64 o = __shfl_down(v, (unsigned)d, 64);
    if (fg && lane + d <= e && o < UNREACHED) v = min64(v, o + (u64)d * ONE);
  }
  const bool ch = v != own;
  if (ch) row[lane + 1] = v;
  return __ballot(ch) != 0;
}

__global__ __launch_bounds__(256) void grow_kernel(u64* key, uint32_t* header, uint8_t* dirty,
                                                   int Hs, int Ws, int tiles_x, int tiles_y, int round, int conn8) {
  extern __shared__ u64 lds[];
  u64* K = lds;                                            // [LROWS][PITCH]
  u64* snap = K + LROWS * PITCH;                           // [4 waves][above, below][PITCH]
  uint32_t* flag = reinterpret_cast<uint32_t*>(snap + 4 * 2 * PITCH);   // [3] rotating "this iteration moved" + [1] "the tile moved"
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int prev = (round + 2) % 3, cur = round % 3, next = (round + 1) % 3;
  const int tile = blockIdx.x, n_tiles = tiles_x * tiles_y;
  const int tyi = tile / tiles_x, txi = tile % tiles_x;
  if (tile == 0 && threadIdx.x == 0) header[H_FLAG + next] = 0u;
  if (header[H_FLAG + prev] == 0u) return;                 // the round before moved nothing: the fixed point is reached
  if (threadIdx.x == 0) dirty[(int64_t)next * n_tiles + tile] = 0;
  bool active = false;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int yy = tyi + dy, xx = txi + dx;
      if (yy >= 0 && yy < tiles_y && xx >= 0 && xx < tiles_x) active = active || dirty[(int64_t)prev * n_tiles + yy * tiles_x + xx] != 0;
    }
  if (!active) return;                                     // uniform over the workgroup

  const int ty0 = tyi * T, tx0 = txi * T;
  if (threadIdx.x < 4) flag[threadIdx.x] = 0u;
  for (int r = wave; r < LROWS; r += 4) {
    const int gy = ty0 - 1 + r;
    for (int c = lane; c < PITCH; c += 64) {
      const int gx = tx0 - 1 + c;
      const bool in = gy >= 0 && gy < Hs && gx >= 0 && gx < Ws;
      K[r * PITCH + c] = in ? ld_key(key + (int64_t)gy * Ws + gx) : BG;
    }
  }
  __syncthreads();

  const int b0 = wave * BAND;                              // interior rows b0 .. b0 + BAND - 1 = LDS rows b0 + 1 .. b0 + BAND
  u64* above = snap + (wave * 2) * PITCH;
  u64* below = above + PITCH;
  bool moved = false;
  for (int it = 0; it < T * T; ++it) {
    for (int c = lane; c < PITCH; c += 64) {               // the rows just outside the band, as they stand now
      above[c] = K[b0 * PITCH + c];
      below[c] = K[(b0 + BAND + 1) * PITCH + c];
    }
    if (threadIdx.x == 0) flag[(it + 1) % 3] = 0u;
    __syncthreads();
    bool ch = false;
    for (int y = 0; y < BAND; ++y) {
      u64* row = K + (b0 + 1 + y) * PITCH;
      ch = relax_row(row, y ? row - PITCH : above, lane, conn8, it == 0) || ch;
    }
    for (int y = BAND - 1; y >= 0; --y) {
      u64* row = K + (b0 + 1 + y) * PITCH;
      ch = relax_row(row, y < BAND - 1 ? row + PITCH : below, lane, conn8, false) || ch;
    }
    if (ch) {
      moved = true;
      if (lane == 0) flag[it % 3] = 1u;
    }
    __syncthreads();
    if (!flag[it % 3]) break;                              // uniform: every thread reads it after the barrier
  }
  if (moved && lane == 0) flag[3] = 1u;                    // a word of the dynamic LDS: c3d_launch_lds refuses static LDS,
  __syncthreads();                                         // which __syncthreads_or would bring
  if (!flag[3]) return;
  const int gx = tx0 + lane;
  for (int y = 0; y < BAND; ++y) {
    const int gy = ty0 + b0 + y;
    if (gy >= Hs || gx >= Ws) continue;
    const u64 v = K[(b0 + 1 + y) * PITCH + lane + 1];
    if (v < UNREACHED) st_key(key + (int64_t)gy * Ws + gx, v);   // a pixel that no seed reached has nothing new to say
  }
  if (threadIdx.x == 0) {
    atomicOr(header + H_FLAG + cur, 1u);
    atomicMax(header + H_ROUNDS, (uint32_t)round);
    dirty[(int64_t)cur * n_tiles + tile] = 1;
  }
}

// first[id] = the smallest index whose key names seed id.  A wave holds 64 consecutive indices: of a run of lanes with one id
// only the first lane needs the atomic.
__global__ __launch_bounds__(256) void piece_first_kernel(const u64* __restrict__ key, uint32_t* __restrict__ first, int64_t N) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < N; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    const u64 k = i < N ? key[i] : BG;
    const uint32_t id = k < UNREACHED ? (uint32_t)k : 0xffffffffu;
    const uint32_t left = __shfl_up(id, 1u, 64);
    if (id < (uint32_t)N && (lane == 0 || left != id)) atomicMin(first + id, (uint32_t)i);
  }
}

__global__ __launch_bounds__(256) void piece_roots_kernel(const u64* __restrict__ key, const uint32_t* __restrict__ first,
                                                          const uint8_t* __restrict__ seeded, int32_t* __restrict__ L,
                                                          uint32_t* __restrict__ area, int64_t N) {
  for (int64_t base = (int64_t)blockIdx.x * 256; base < N; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    int r = -1;
    if (i < N) {
      const u64 k = key[i];
      if (k < UNREACHED) {
        const uint32_t id = (uint32_t)k;
        const uint32_t f = id < (uint32_t)N ? first[id] : 0xffffffffu;
        r = f < (uint32_t)N ? (int)f : -1;
      } else if (k == UNREACHED) {                         // no seed in this component: one piece; or the rounds ran out: nothing
        const int c = L[i];
        r = c >= 0 && c < N && !seeded[c] ? c : -1;
      }
      L[i] = r;                                            // only this thread touches L[i]
    }
    c3d_detail_wave_area_add(area, r);
  }
}

__global__ void split_info_kernel(const uint32_t* __restrict__ header, int32_t* __restrict__ info, int max_rounds) {
  if (blockIdx.x || threadIdx.x) return;
  info[0] = (header[H_FLAG + max_rounds % 3] ? C3D_SPLIT_ST_NOT_CONVERGED : 0) | (header[C3D_DETAIL_WS_ERR] ? C3D_SPLIT_ST_BAD_LABELS : 0);
  info[1] = (int32_t)header[H_SEEDS];
  info[2] = (int32_t)header[H_ROUNDS];
  info[3] = 0;
}

unsigned grid_for(int64_t items) {
  int64_t g = (items + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

}  // namespace

extern "C" int64_t c3d_scene_split_ws_bytes(int32_t Hs, int32_t Ws, int32_t n_cls) {
  if (Hs <= 0 || Ws <= 0 || n_cls < 1 || n_cls > 16) return C3D_E_BADARG;
  if ((int64_t)Hs * Ws >= (1ll << 31)) return C3D_E_UNSUPPORTED;
  return plan_for(Hs, Ws, n_cls).bytes;
}

extern "C" int c3d_scene_split_tile(int32_t out[2]) {
  if (!out) return C3D_E_BADARG;
  out[0] = T;
  out[1] = T;
  return 0;
}

extern "C" int c3d_scene_split(const uint8_t* mask, const uint8_t* cls_map, const float* score, int32_t Hs, int32_t Ws,
                               int32_t connectivity, int32_t min_area, int32_t n_cls, int32_t first_class, int32_t max_objects,
                               int32_t r2, int32_t max_rounds, int32_t* labels, int32_t* table, uint32_t* hist, uint8_t* object_cls,
                               int32_t* counts, int32_t* info, void* ws, void* stream) {
  if (!mask || !labels || !table || !counts || !info || !ws || Hs <= 0 || Ws <= 0 || max_objects < 1 || first_class < 0) return C3D_E_BADARG;
  if (connectivity != 4 && connectivity != 8) return C3D_E_BADARG;
  if (r2 < 0 || r2 > R2_MAX || max_rounds < 1 || max_rounds > ROUNDS_MAX) return C3D_E_BADARG;
  if ((int64_t)Hs * Ws >= (1ll << 31)) return C3D_E_UNSUPPORTED;
  if (r2 > 0 && (Hs > EDT_SIDE_MAX || Ws > EDT_SIDE_MAX)) return C3D_E_UNSUPPORTED;   // the limits of c3d_scene_edt
  if (cls_map && (n_cls < 1 || n_cls > 16)) return C3D_E_BADARG;
  const int64_t N = (int64_t)Hs * Ws;
  const int conn8 = connectivity == 8;
  const Plan p = plan_for(Hs, Ws, cls_map ? n_cls : 1);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  uint32_t* header = reinterpret_cast<uint32_t*>(base);
  uint32_t* area = reinterpret_cast<uint32_t*>(base + c3d_detail_area_offset());
  u64* key = reinterpret_cast<u64*>(base + p.key);
  uint32_t* first = reinterpret_cast<uint32_t*>(base + p.first);
  uint8_t* seeded = reinterpret_cast<uint8_t*>(base + p.seeded);
  uint8_t* dirty = reinterpret_cast<uint8_t*>(base + p.dirty);

  int rc = c3d_detail_objects_clear(ws, N, cls_map, score, n_cls, hist, max_objects, st);
  if (rc) return rc;
  hipError_t e = hipMemsetAsync(first, 0xff, (size_t)N * 4, st);
  if (e == hipSuccess) e = hipMemsetAsync(seeded, 0, (size_t)N, st);
  if (e == hipSuccess) e = hipMemsetAsync(dirty, 1, (size_t)p.n_tiles, st);          // round 1 runs every tile
  if (e == hipSuccess) e = hipMemsetAsync(dirty + p.n_tiles, 0, (size_t)p.n_tiles, st);
  if (e != hipSuccess) return (int)e;

  // components of the mask into `labels`; seeds into S -- the same map when nothing is eroded
  const int32_t* S = labels;
  rc = c3d_detail_label_roots(mask, labels, header + C3D_DETAIL_WS_ERR, nullptr, Hs, Ws, conn8, 3, st);
  if (rc) return rc;
  if (r2 > 0) {
    int32_t* dist2 = reinterpret_cast<int32_t*>(key);      // dead before the keys are written
    uint8_t* core = reinterpret_cast<uint8_t*>(base + p.core);
    int32_t* seeds = reinterpret_cast<int32_t*>(base + p.S);
    rc = c3d_scene_edt(mask, Hs, Ws, C3D_EDT_BORDER, r2, dist2, base + p.edt, stream);
    if (rc) return rc;
    rc = c3d_launch_lds<core_kernel>(dim3(grid_for(N)), dim3(256), 0, st, mask, (const int32_t*)dist2, core, N, (int)r2);
    if (rc) return rc;
    rc = c3d_detail_label_roots(core, seeds, header + C3D_DETAIL_WS_ERR, nullptr, Hs, Ws, conn8, 3, st);
    if (rc) return rc;
    S = seeds;
  }
  rc = c3d_launch_lds<seed_keys_kernel>(dim3(grid_for(N)), dim3(256), 0, st, mask, S, (const int32_t*)labels, key, seeded, header, N);
  if (rc) return rc;

  const int tiles_x = (Ws + T - 1) / T, tiles_y = (Hs + T - 1) / T;
  for (int round = 1; round <= max_rounds; ++round) {
    rc = c3d_launch_lds<grow_kernel>(dim3((unsigned)p.n_tiles), dim3(256), GROW_LDS, st, key, header, dirty, (int)Hs, (int)Ws, tiles_x,
                                     tiles_y, round, conn8);
    if (rc) return rc;
  }

  rc = c3d_launch_lds<piece_first_kernel>(dim3(grid_for(N)), dim3(256), 0, st, (const u64*)key, first, N);
  if (rc) return rc;
  rc = c3d_launch_lds<piece_roots_kernel>(dim3(grid_for(N)), dim3(256), 0, st, (const u64*)key, (const uint32_t*)first,
                                          (const uint8_t*)seeded, labels, area, N);
  if (rc) return rc;
  rc = c3d_detail_objects_tail(cls_map, score, Hs, Ws, min_area, n_cls, first_class, max_objects, labels, table, hist, object_cls,
                               counts, ws, 9, st);
  if (rc) return rc;
  return c3d_launch_lds<split_info_kernel>(dim3(1), dim3(64), 0, st, (const uint32_t*)header, info, (int)max_rounds);
}
