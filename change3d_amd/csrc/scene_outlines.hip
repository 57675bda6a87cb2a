// Outlines of the objects of a scene map (change3d_amd/infer.py, predict(objects=True, outlines=True)): the i32 label map
// of c3d_scene_objects, still in HBM, is traced into closed rectilinear rings -- one ring of positive area per object, one
// of negative area per hole -- as a ring table and one vertex list.  The definition (edges, direction, successor, corners,
// ring start and order) is the header's (include/change3d_hip.h); this file is one way to compute it.  The reference has
// no counterpart: xBD's polygons are drawn on the host there.  Integer arithmetic and integer atomics only.
//
// Work is parallel over boundary edges; no thread walks a ring.  The only data-dependent structure is the successor
// permutation, and it is resolved by pointer doubling in a number of rounds fixed by the host: no loop follows links, so
// there is nothing to cap; what a cap would catch (a corrupted workspace) is caught by the range checks of emit, which set
// C3D_OUTLINE_ST_STEP_CAP instead of writing.  Phases are launches on one stream; no workgroup waits for another.
//
//   1 mark        one thread per pixel: 4 boundary bits and 4 corner bits from the 3 x 3 neighbourhood; edges per chunk of
//                 1024 pixels
//   2 scan        exclusive scan of the chunk counts by one workgroup; E = all edges
//   3 offsets     off[p] = compact index of pixel p's first edge: the compact list is in key order
//   4 link        tuple (next, best, c, t) per edge: next = compact index of the successor, best = key if corner else
//                 INT_MAX, c = 0, t = corner
//   5 double      R = ceil(log2(4 Hs Ws)) rounds, double-buffered: window A = [e, e + 2^k) joined with window B at next.
//                 best = smallest corner key of the window, c = corners before its FIRST occurrence, t = corners.  A round
//                 in which no `best` changed has every ring agreed on its start (see below): it leaves its flag 0 and the
//                 remaining rounds return at once
//   6 ring_count  ring starts (corner edge whose key is its ring's best) and their vertex counts per chunk
//   7 scan x 2    of both
//   8 ring_rows   ring index = rank of the start in key order, start = exclusive scan of the vertex counts; writes the ring
//                 rows, and (index, n, start) into the idle tuple buffer at the start edge's slot
//   9 emit        every corner edge writes its vertex at start + position; every edge adds to its ring's area and perimeter:
//                 a wave whose edges of one side share a ring adds them up in registers, across sides and iterations, and
//                 reaches memory when its ring changes
//  10 finalise    counts, status, zero rows
//
// Why "no best changed" means done.  After round k, best(e) is the minimum over the 2^(k+1) edges from e.  If round k+1
// changes nothing then best(e) <= best(e + 2^(k+1)) along every ring, so best is constant on each orbit of that step; the
// windows of an orbit tile the ring, so the constant is the ring's minimum.  `c` is then final too: with best = the ring's
// one smallest corner key, its first occurrence in the window is the ring's start edge, and A wins ties.
#include <climits>

#include "scene_wave.h"
#include "../../include/change3d_hip.h"

namespace {

using namespace c3d_wave;

constexpr int CHUNK = 1024;                                // pixels per chunk of the scans
constexpr int MAX_GRID = 256 * 8;
constexpr int MAX_ROUNDS = 32;

// words of the workspace header (256 bytes)
enum { WS_ERR = 0, WS_EDGES = 1, WS_RINGS = 2, WS_VFOUND = 3, WS_VWRITTEN = 4, WS_FINAL = 5, WS_CHG = 16 };

struct Workspace {
  int64_t info, off, chunks_e, chunks_r, chunks_v, tup0, tup1, bytes;   // byte offsets
  int64_t n_chunks, cap;                                   // cap = most edges a label map can own = 4 N
};

Workspace workspace_plan(int64_t N) {
  Workspace w;
  auto up = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  w.n_chunks = (N + CHUNK - 1) / CHUNK;
  w.cap = 4 * N;
  w.info = 256;
  w.off = w.info + up(N);
  w.chunks_e = w.off + up(N * 4);
  w.chunks_r = w.chunks_e + up(w.n_chunks * 4);
  w.chunks_v = w.chunks_r + up(w.n_chunks * 4);
  w.tup0 = w.chunks_v + up(w.n_chunks * 4);
  w.tup1 = w.tup0 + up(w.cap * 16);
  w.bytes = w.tup1 + up(w.cap * 16);
  return w;
}

// travel of side s with the object on the right (y down): top +x, right +y, bottom -x, left -y
__device__ __forceinline__ int trav_dx(int s) { return (s == 0) - (s == 2); }
__device__ __forceinline__ int trav_dy(int s) { return (s == 1) - (s == 3); }
// start vertex of side s of pixel (x, y)
__device__ __forceinline__ int start_dx(int s) { return s == 1 || s == 2; }
__device__ __forceinline__ int start_dy(int s) { return s >= 2; }

__device__ __forceinline__ bool same_id(const int32_t* __restrict__ L, int H, int W, int y, int x, int id) {
  return y >= 0 && y < H && x >= 0 && x < W && L[(int64_t)y * W + x] == id;
}

__device__ __forceinline__ int object_rows(const int32_t* __restrict__ counts_obj, int max_objects) {
  const int found = counts_obj[0], rows = counts_obj[1];
  return found < 0 ? 0 : (rows < 0 ? 0 : (rows > max_objects ? max_objects : rows));
}

// low nibble: side s is a boundary edge; high nibble: it is a corner edge (its predecessor is not the same side of the
// pixel behind it, which it would be iff that pixel has the id and the pixel beside it on the outside has not)
__device__ __forceinline__ uint32_t pixel_info(const int32_t* __restrict__ L, int H, int W, int y, int x, int rows) {
  const int id = L[(int64_t)y * W + x];
  if (id < 1 || id > rows) return 0u;
  uint32_t nb = 0;                                         // bit (dy+1)*3 + dx+1: that neighbour has the id
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx)
      if ((dy || dx) && same_id(L, H, W, y + dy, x + dx, id)) nb |= 1u << ((dy + 1) * 3 + dx + 1);
  uint32_t info = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int oy = trav_dy((s + 3) & 3), ox = trav_dx((s + 3) & 3), ty = trav_dy(s), tx = trav_dx(s);
    if (nb >> ((oy + 1) * 3 + ox + 1) & 1u) continue;
    const bool behind = nb >> ((-ty + 1) * 3 - tx + 1) & 1u, beside = nb >> ((-ty + oy + 1) * 3 - tx + ox + 1) & 1u;
    info |= (1u << s) | ((behind && !beside) ? 0u : (16u << s));
  }
  return info;
}

__device__ __forceinline__ int edge_rank(uint32_t info, int s) { return __popc(info & ((1u << s) - 1u) & 15u); }

// compact index of the successor of side s of pixel (y, x) with label id; -1 if the workspace contradicts the labels
__device__ __forceinline__ int successor(const int32_t* __restrict__ L, const uint8_t* __restrict__ info,
                                         const int32_t* __restrict__ off, int H, int W, int y, int x, int s, int id, int conn8,
                                         uint32_t edges) {
  const int ay = y + trav_dy(s), ax = x + trav_dx(s);      // the pixel ahead, and the diagonal one ahead on the outside
  const int dy = ay + trav_dy((s + 3) & 3), dx = ax + trav_dx((s + 3) & 3);
  const bool a = same_id(L, H, W, ay, ax, id), d = same_id(L, H, W, dy, dx, id);
  int qy = y, qx = x, qs = (s + 1) & 3;                    // right turn
  if (d && (a || conn8)) { qy = dy; qx = dx; qs = (s + 3) & 3; }   // left turn
  else if (a) { qy = ay; qx = ax; qs = s; }               // straight
  const int64_t q = (int64_t)qy * W + qx;
  const uint32_t qi = info[q];
  if (!(qi >> qs & 1u)) return -1;
  const uint32_t e = (uint32_t)off[q] + (uint32_t)edge_rank(qi, qs);
  return e < edges ? (int)e : -1;
}


// exclusive prefix of v over the 256 threads; `all` = the sum.  part: 4 words of LDS; the caller syncs before reusing it
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* part, uint32_t* all) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  if (lane == 63) part[wave] = inc;
  __syncthreads();
  uint32_t before = 0, sum = 0;
  for (int w = 0; w < 4; ++w) {
    before += w < wave ? part[w] : 0u;
    sum += part[w];
  }
  *all = sum;
  return before + inc - v;
}

__global__ __launch_bounds__(256) void mark_kernel(const int32_t* __restrict__ L, const int32_t* __restrict__ counts_obj,
                                                   uint8_t* __restrict__ info, uint32_t* __restrict__ chunks, int H, int W, int N,
                                                   int64_t n_chunks, int max_objects) {
  extern __shared__ uint32_t part[];                       // [4]
  const int rows = object_rows(counts_obj, max_objects);
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    uint32_t n = 0;
    for (int k = 0; k < CHUNK / 256; ++k) {
      const int64_t i = c * CHUNK + k * 256 + threadIdx.x;
      if (i < N) {
        const uint32_t v = pixel_info(L, H, W, (int)(i / W), (int)(i % W), rows);
        info[i] = (uint8_t)v;
        n += (uint32_t)__popc(v & 15u);
      }
    }
    n = wave_sum32(n);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) chunks[c] = part[0] + part[1] + part[2] + part[3];
    __syncthreads();
  }
}

// in place: chunks[c] = sum before chunk c; *total = all of them.  One workgroup.
__global__ __launch_bounds__(256) void scan_chunks_kernel(uint32_t* __restrict__ chunks, uint32_t* __restrict__ total,
                                                          int64_t n_chunks) {
  extern __shared__ uint32_t part[];                       // [4]
  uint32_t running = 0;
  for (int64_t base = 0; base < n_chunks; base += 256) {
    const int64_t c = base + threadIdx.x;
    const uint32_t v = c < n_chunks ? chunks[c] : 0u;
    uint32_t all;
    const uint32_t before = block_excl_scan(v, part, &all);
    if (c < n_chunks) chunks[c] = running + before;
    running += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = running;
}

__global__ __launch_bounds__(256) void offsets_kernel(const uint8_t* __restrict__ info, const uint32_t* __restrict__ chunks,
                                                      int32_t* __restrict__ off, int N, int64_t n_chunks) {
  extern __shared__ uint32_t part[];                       // [4]
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    uint32_t run = chunks[c];
    for (int k = 0; k < CHUNK / 256; ++k) {
      const int64_t i = c * CHUNK + k * 256 + threadIdx.x;
      const uint32_t v = i < N ? (uint32_t)__popc(info[i] & 15u) : 0u;
      uint32_t all;
      const uint32_t before = block_excl_scan(v, part, &all);
      if (i < N) off[i] = (int32_t)(run + before);         // < 4 N < 2^31
      run += all;
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(256) void link_kernel(const int32_t* __restrict__ L, const uint8_t* __restrict__ info,
                                                   const int32_t* __restrict__ off, int4* __restrict__ tup,
                                                   uint32_t* __restrict__ header, int H, int W, int N, int conn8) {
  const uint32_t edges = header[WS_EDGES];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
    const uint32_t v = info[i];
    if (!(v & 15u)) continue;
    const int y = (int)(i / W), x = (int)(i % W), id = L[i];
    uint32_t e = (uint32_t)off[i];
    for (int s = 0; s < 4; ++s) {
      if (!(v >> s & 1u)) continue;
      if (e >= edges) { atomicOr(header + WS_ERR, 1u); break; }
      int nx = successor(L, info, off, H, W, y, x, s, id, conn8, edges);
      if (nx < 0) { atomicOr(header + WS_ERR, 1u); nx = (int)e; }
      const int corner = v >> (4 + s) & 1u;
      tup[e] = make_int4(nx, corner ? (int)(4 * i + s) : INT_MAX, 0, corner);
      ++e;
    }
  }
}

// round k: in = windows of 2^k edges, out = windows of 2^(k+1)
__global__ __launch_bounds__(256) void double_kernel(const int4* __restrict__ in, int4* __restrict__ out,
                                                     uint32_t* __restrict__ header, int k) {
  if (k > 0 && header[WS_CHG + k - 1] == 0u) return;      // the round before changed nothing: every later one would not
  const uint32_t edges = header[WS_EDGES];
  if (blockIdx.x == 0 && threadIdx.x == 0) header[WS_FINAL] = (uint32_t)((k + 1) & 1);
  bool changed = false;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < edges; e += (int64_t)gridDim.x * 256) {
    const int4 a = in[e];
    uint32_t nx = (uint32_t)a.x;
    if (nx >= edges) { atomicOr(header + WS_ERR, 1u); nx = (uint32_t)e; }
    const int4 b = in[nx];
    int4 o;
    o.x = b.x;
    if (a.y <= b.y) { o.y = a.y; o.z = a.z; }             // A wins a tie: c counts up to the FIRST occurrence of the start
    else { o.y = b.y; o.z = (int)((uint32_t)a.w + (uint32_t)b.z); changed = true; }
    o.w = (int)((uint32_t)a.w + (uint32_t)b.w);           // exact while it is used, i.e. until the window wraps the ring
    out[e] = o;
  }
  if (changed) header[WS_CHG + k] = 1u;                    // every writer stores the same value
}

// The ring starts of pixel i: calls f(side, edge, n_vertices) for each in key order.
template <class F>
__device__ __forceinline__ void for_ring_starts(const int32_t* __restrict__ L, const uint8_t* __restrict__ info,
                                                const int32_t* __restrict__ off, const int4* __restrict__ fin, int H, int W,
                                                int64_t i, int conn8, uint32_t edges, uint32_t* err, F f) {
  const uint32_t v = info[i];
  if (!(v >> 4)) return;
  const int y = (int)(i / W), x = (int)(i % W), id = L[i];
  const uint32_t e0 = (uint32_t)off[i];
  for (int s = 0; s < 4; ++s) {
    if (!(v >> (4 + s) & 1u)) continue;
    const uint32_t e = e0 + (uint32_t)edge_rank(v, s);
    if (e >= edges) { atomicOr(err, 1u); return; }
    if (fin[e].y != (int)(4 * i + s)) continue;
    const int nx = successor(L, info, off, H, W, y, x, s, id, conn8, edges);
    const int n = nx < 0 ? 0 : fin[nx].z + 1;              // corners from the start's successor round to the start, and the start
    if (n < 4 || (uint32_t)n > edges) { atomicOr(err, 1u); continue; }
    f(s, e, n);
  }
}

__global__ __launch_bounds__(256) void ring_count_kernel(const int32_t* __restrict__ L, const uint8_t* __restrict__ info,
                                                         const int32_t* __restrict__ off, const int4* __restrict__ tup0,
                                                         const int4* __restrict__ tup1, uint32_t* __restrict__ header,
                                                         uint32_t* __restrict__ chunks_r, uint32_t* __restrict__ chunks_v, int H,
                                                         int W, int N, int64_t n_chunks, int conn8) {
  extern __shared__ uint32_t part[];                       // [8]
  const uint32_t edges = header[WS_EDGES];
  const int4* fin = header[WS_FINAL] ? tup1 : tup0;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    uint32_t nr = 0, nv = 0;
    for (int k = 0; k < CHUNK / 256; ++k) {
      const int64_t i = c * CHUNK + k * 256 + threadIdx.x;
      if (i < N) for_ring_starts(L, info, off, fin, H, W, i, conn8, edges, header + WS_ERR, [&](int, uint32_t, int n) { ++nr; nv += (uint32_t)n; });
    }
    nr = wave_sum32(nr);
    nv = wave_sum32(nv);
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6] = nr; part[4 + (threadIdx.x >> 6)] = nv; }
    __syncthreads();
    if (threadIdx.x == 0) {
      chunks_r[c] = part[0] + part[1] + part[2] + part[3];
      chunks_v[c] = part[4] + part[5] + part[6] + part[7];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void ring_rows_kernel(const int32_t* __restrict__ L, const uint8_t* __restrict__ info,
                                                        const int32_t* __restrict__ off, int4* __restrict__ tup0,
                                                        int4* __restrict__ tup1, uint32_t* __restrict__ header,
                                                        const uint32_t* __restrict__ chunks_r, const uint32_t* __restrict__ chunks_v,
                                                        int32_t* __restrict__ rings, int H, int W, int N, int64_t n_chunks, int conn8,
                                                        int max_rings, int max_vertices) {
  extern __shared__ uint32_t part[];                       // [4]
  const uint32_t edges = header[WS_EDGES];
  const int4* fin = header[WS_FINAL] ? tup1 : tup0;
  int4* idle = header[WS_FINAL] ? tup0 : tup1;
  uint32_t end = 0;                                        // end of the last ring of this thread whose vertices fit
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    uint32_t run_r = chunks_r[c], run_v = chunks_v[c];
    for (int k = 0; k < CHUNK / 256; ++k) {
      const int64_t i = c * CHUNK + k * 256 + threadIdx.x;
      uint32_t nr = 0, nv = 0;
      if (i < N) for_ring_starts(L, info, off, fin, H, W, i, conn8, edges, header + WS_ERR, [&](int, uint32_t, int n) { ++nr; nv += (uint32_t)n; });
      uint32_t all_r, all_v;
      uint32_t r = run_r + block_excl_scan(nr, part, &all_r);
      __syncthreads();
      uint32_t vs = run_v + block_excl_scan(nv, part, &all_v);
      __syncthreads();
      if (nr) {
        const int y = (int)(i / W), x = (int)(i % W), id = L[i];
        for_ring_starts(L, info, off, fin, H, W, i, conn8, edges, header + WS_ERR, [&](int s, uint32_t e, int n) {
          const bool row = r < (uint32_t)max_rings;
          const bool fits = row && (uint64_t)vs + (uint32_t)n <= (uint32_t)max_vertices;
          if (row) {
            int4* dst = reinterpret_cast<int4*>(rings + (int64_t)r * 8);
            dst[0] = make_int4(id, fits ? (int)vs : -1, n, 0);
            dst[1] = make_int4(0, x + start_dx(s), y + start_dy(s), 0);
          }
          if (fits) end = vs + (uint32_t)n;                // starts ascend with the ring index: the last one is the largest
          idle[e] = make_int4(row ? (int)r : -1, n, fits ? (int)vs : -1, 0);
          ++r;
          vs += (uint32_t)n;
        });
      }
      run_r += all_r;
      run_v += all_v;
    }
  }
  for (int d = 32; d; d >>= 1) { const uint32_t o = __shfl_xor(end, d); end = o > end ? o : end; }
  if ((threadIdx.x & 63) == 0 && end) atomicMax(header + WS_VWRITTEN, end);   // one per wave, not one per ring
}

__global__ __launch_bounds__(256) void emit_kernel(const uint8_t* __restrict__ info, const int32_t* __restrict__ off,
                                                   const int4* __restrict__ tup0, const int4* __restrict__ tup1,
                                                   uint32_t* __restrict__ header, int32_t* __restrict__ rings,
                                                   int32_t* __restrict__ vertices, int W, int N, int max_rings, int max_vertices) {
  const int lane = threadIdx.x & 63;
  const uint32_t edges = header[WS_EDGES];
  const int4* fin = header[WS_FINAL] ? tup1 : tup0;
  const int4* ring_of = header[WS_FINAL] ? tup0 : tup1;   // written by ring_rows at the slots of the start edges
  int acc_r = -1;                                          // wave-uniform: the ring the wave is adding up for, and its sums;
  uint32_t acc_a = 0, acc_p = 0;                           // they go to memory when the ring changes and at the end
  auto flush = [&]() {
    if (acc_r >= 0 && lane == 0) {
      if (acc_a) atomicAdd(reinterpret_cast<uint32_t*>(rings) + (int64_t)acc_r * 8 + 3, acc_a);   // modular: the total fits i32
      atomicAdd(reinterpret_cast<uint32_t*>(rings) + (int64_t)acc_r * 8 + 4, acc_p);
    }
  };
  for (int64_t base = (int64_t)blockIdx.x * 256; base < N; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    const uint32_t v = i < N ? info[i] : 0u;
    const int y = (int)(i / W), x = (int)(i % W);
    const uint32_t e0 = (v & 15u) ? (uint32_t)off[i] : 0u;
    for (int s = 0; s < 4; ++s) {                          // uniform over the wave: the ballots below need every lane
      int r = -1, term = 0;
      if (v >> s & 1u) {
        const uint32_t e = e0 + (uint32_t)edge_rank(v, s);
        bool ok = e < edges;
        int4 t = make_int4(0, 0, 0, 0), ring = t;
        uint32_t m = 0;
        if (ok) {
          t = fin[e];
          const int64_t pm = (int64_t)(t.y >> 2);          // the ring's start edge: a corner edge of some pixel
          const int sm = t.y & 3;
          ok = t.y >= 0 && pm < N && (info[pm] >> (4 + sm) & 1u);
          if (ok) {
            m = (uint32_t)off[pm] + (uint32_t)edge_rank(info[pm], sm);
            ok = m < edges;
          }
        }
        if (ok) {
          ring = ring_of[m];
          ok = ring.x >= -1 && ring.x < max_rings && ring.y >= 4;
        }
        if (!ok) {
          atomicOr(header + WS_ERR, 1u);
        } else {
          r = ring.x;
          term = s == 0 ? -y : (s == 2 ? y + 1 : 0);       // the horizontal half of the shoelace sum is the area itself
          if ((v >> (4 + s) & 1u) && ring.z >= 0) {
            const int pos = e == m ? 0 : ring.y - t.z;
            if (pos < 0 || pos >= ring.y || (int64_t)ring.z + pos >= max_vertices) {
              atomicOr(header + WS_ERR, 1u);
            } else {
              int2* dst = reinterpret_cast<int2*>(vertices) + ((int64_t)ring.z + pos);
              *dst = make_int2(x + start_dx(s), y + start_dy(s));
            }
          }
        }
      }
      const bool act = r >= 0;
      const unsigned long long mk = __ballot(act);
      if (!mk) continue;
      const int leader = __ffsll((long long)mk) - 1;
      const int r0 = __shfl(r, leader);
      if (__ballot(act && r != r0) == 0) {                 // one ring on this side of the wave's pixels
        const uint32_t a = wave_sum32(act ? (uint32_t)term : 0u);
        if (r0 != acc_r) {
          flush();
          acc_r = r0;
          acc_a = acc_p = 0;
        }
        acc_a += a;
        acc_p += (uint32_t)__popcll(mk);
      } else if (act) {
        if (term) atomicAdd(reinterpret_cast<uint32_t*>(rings) + (int64_t)r * 8 + 3, (uint32_t)term);
        atomicAdd(reinterpret_cast<uint32_t*>(rings) + (int64_t)r * 8 + 4, 1u);
      }
    }
  }
  flush();
}

__global__ __launch_bounds__(256) void finalise_kernel(int32_t* __restrict__ rings, int32_t* __restrict__ counts,
                                                       const int32_t* __restrict__ counts_obj,
                                                       const uint32_t* __restrict__ header, int max_rings) {
  const uint32_t found = header[WS_RINGS];
  const int rows = found < (uint32_t)max_rings ? (int)found : max_rings;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint32_t vfound = header[WS_VFOUND], vwritten = header[WS_VWRITTEN];
    const int obj_found = counts_obj[0], obj_rows = counts_obj[1];
    int status = header[WS_ERR] ? C3D_OUTLINE_ST_STEP_CAP : 0;
    if (obj_found < 0) status |= C3D_OUTLINE_ST_BAD_COUNTS;
    else if (found > (uint32_t)rows || vfound > vwritten || obj_found > obj_rows) status |= C3D_OUTLINE_ST_TRUNCATED;
    counts[0] = (int32_t)found;
    counts[1] = rows;
    counts[2] = (int32_t)vfound;
    counts[3] = (int32_t)vwritten;
    counts[4] = status;
  }
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < max_rings; k += (int64_t)gridDim.x * 256) {
    if (k < rows) continue;                                // ring_rows wrote it
    int4* row = reinterpret_cast<int4*>(rings + k * 8);
    row[0] = make_int4(0, 0, 0, 0);
    row[1] = make_int4(0, 0, 0, 0);
  }
}

unsigned grid_for(int64_t items, int per_block) {
  int64_t g = (items + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > MAX_GRID ? MAX_GRID : g));
}

}  // namespace

extern "C" int64_t c3d_scene_outlines_ws_bytes(int32_t Hs, int32_t Ws) {
  if (Hs <= 0 || Ws <= 0) return C3D_E_BADARG;
  if ((int64_t)Hs * Ws >= (1ll << 29)) return C3D_E_UNSUPPORTED;
  return workspace_plan((int64_t)Hs * Ws).bytes;
}

extern "C" int c3d_scene_outlines(const int32_t* labels, const int32_t* counts_obj, int32_t Hs, int32_t Ws, int32_t connectivity,
                                  int32_t max_objects, int32_t max_rings, int32_t max_vertices, int32_t* rings, int32_t* vertices,
                                  int32_t* counts, void* ws, void* stream) {
  if (!labels || !counts_obj || !rings || !vertices || !counts || !ws || Hs <= 0 || Ws <= 0) return C3D_E_BADARG;
  if (connectivity != 4 && connectivity != 8) return C3D_E_BADARG;
  if (max_objects < 1 || max_rings < 1 || max_vertices < 1) return C3D_E_BADARG;
  if ((int64_t)Hs * Ws >= (1ll << 29)) return C3D_E_UNSUPPORTED;
  const int N = Hs * Ws, conn8 = connectivity == 8;
  const Workspace w = workspace_plan(N);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  uint32_t* header = reinterpret_cast<uint32_t*>(base);
  uint8_t* info = reinterpret_cast<uint8_t*>(base + w.info);
  int32_t* off = reinterpret_cast<int32_t*>(base + w.off);
  uint32_t* chunks_e = reinterpret_cast<uint32_t*>(base + w.chunks_e);
  uint32_t* chunks_r = reinterpret_cast<uint32_t*>(base + w.chunks_r);
  uint32_t* chunks_v = reinterpret_cast<uint32_t*>(base + w.chunks_v);
  int4* tup0 = reinterpret_cast<int4*>(base + w.tup0);
  int4* tup1 = reinterpret_cast<int4*>(base + w.tup1);
  int rounds = 0;
  while ((1ll << rounds) < w.cap) ++rounds;                // ceil(log2(4 N)) <= 31: a window of 2^rounds edges holds any ring
  static_assert(WS_CHG + MAX_ROUNDS <= 64, "the round flags live in the 256-byte header");

  // instrumented build only (common.h c3d_knob): tools/outlines_step.py times prefixes of the phases.  The product library
  // compiles this to 10, and every `phases == k` below to false.
  const int phases = c3d_knob("C3D_OUTLINES_PHASES", 10);

  // only the header: every other word of the workspace is written by the call before the call reads it
  hipError_t e = hipMemsetAsync(base, 0, 256, st);
  if (e != hipSuccess) return (int)e;
  const unsigned g_chunks = grid_for(w.n_chunks, 1), g_pix = grid_for(N, 256);
  int rc = c3d_launch_lds<mark_kernel>(dim3(g_chunks), dim3(256), 16, st, labels, counts_obj, info, chunks_e, (int)Hs, (int)Ws, N,
                                       w.n_chunks, (int)max_objects);
  if (rc || phases == 1) return rc;
  rc = c3d_launch_lds<scan_chunks_kernel>(dim3(1), dim3(256), 16, st, chunks_e, header + WS_EDGES, w.n_chunks);
  if (rc || phases == 2) return rc;
  rc = c3d_launch_lds<offsets_kernel>(dim3(g_chunks), dim3(256), 16, st, (const uint8_t*)info, (const uint32_t*)chunks_e, off, N,
                                      w.n_chunks);
  if (rc || phases == 3) return rc;
  rc = c3d_launch_lds<link_kernel>(dim3(g_pix), dim3(256), 0, st, labels, (const uint8_t*)info, (const int32_t*)off, tup0, header,
                                   (int)Hs, (int)Ws, N, conn8);
  if (rc || phases == 4) return rc;
  const unsigned g_edges = grid_for(w.cap, 256);
  for (int k = 0; k < rounds; ++k) {
    rc = c3d_launch_lds<double_kernel>(dim3(g_edges), dim3(256), 0, st, (const int4*)(k & 1 ? tup1 : tup0), k & 1 ? tup0 : tup1,
                                       header, k);
    if (rc) return rc;
  }
  if (phases == 5) return 0;
  rc = c3d_launch_lds<ring_count_kernel>(dim3(g_chunks), dim3(256), 32, st, labels, (const uint8_t*)info, (const int32_t*)off,
                                         (const int4*)tup0, (const int4*)tup1, header, chunks_r, chunks_v, (int)Hs, (int)Ws, N,
                                         w.n_chunks, conn8);
  if (rc || phases == 6) return rc;
  rc = c3d_launch_lds<scan_chunks_kernel>(dim3(1), dim3(256), 16, st, chunks_r, header + WS_RINGS, w.n_chunks);
  if (rc) return rc;
  rc = c3d_launch_lds<scan_chunks_kernel>(dim3(1), dim3(256), 16, st, chunks_v, header + WS_VFOUND, w.n_chunks);
  if (rc || phases == 7) return rc;
  rc = c3d_launch_lds<ring_rows_kernel>(dim3(g_chunks), dim3(256), 16, st, labels, (const uint8_t*)info, (const int32_t*)off, tup0,
                                        tup1, header, (const uint32_t*)chunks_r, (const uint32_t*)chunks_v, rings, (int)Hs, (int)Ws,
                                        N, w.n_chunks, conn8, (int)max_rings, (int)max_vertices);
  if (rc || phases == 8) return rc;
  rc = c3d_launch_lds<emit_kernel>(dim3(g_pix), dim3(256), 0, st, (const uint8_t*)info, (const int32_t*)off, (const int4*)tup0,
                                   (const int4*)tup1, header, rings, vertices, (int)Ws, N, (int)max_rings, (int)max_vertices);
  if (rc || phases == 9) return rc;
  return c3d_launch_lds<finalise_kernel>(dim3(grid_for(max_rings, 256)), dim3(256), 0, st, rings, counts, counts_obj,
                                         (const uint32_t*)header, (int)max_rings);
}
