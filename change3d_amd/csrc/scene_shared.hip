// Shared-wall simplification of a scene's traced rings: every boundary is cut at the lattice points where three or more regions
// meet (the nodes, read from the label map), and every arc between two nodes is simplified once by a Douglas-Peucker whose
// result does not depend on the direction of travel, so that both neighbours of a wall get the same chords.  The rule -- the
// four labels of a node, the augmented ring, its start, the tie to the smallest (vy, vx), the guard of a closed arc -- is the
// header's (include/change3d_hip.h); this file is one way to compute it.  Integer arithmetic and integer atomics only.
//
//   0 nodes       two launches over the lattice points: a bitmap of the nodes by rows (a bit per vx) and one by columns (a bit per
//                 vy), written whole words at a time from a wave's ballot.  An edge then finds the nodes inside it by popcount
//                 over a bit range instead of walking its lattice points with four label reads each: one wave owns a ring, and
//                 on the serpentine (2050 edges, half of them 1024 long) the walk took 31 ms beside 2 ms of simplification
//   1 count       one wave per ring row, a lane per stored edge: validates the edge and counts the nodes strictly inside it;
//                 naug[r] = the ring's augmented vertex count, or why the row is not simplified
//   2 scan_rows   one workgroup: off[r] = where ring r keeps its augmented vertices and per-vertex state in the workspace; lists
//                 the rings above WAVE_LIMIT for the workgroup tiers
//   3 augment     one wave per ring: reads the edges' bits again and writes the augmented vertices (packed position; left label and
//                 node flag) in stored order, and the ring's start = its first node, or its smallest (vy, vx) without one.  The
//                 later stages read position k of the rotated ring at (k + start) mod n
//   4 dp          whoever owns a ring loops until no chord of it splits: one wave (a workgroup of 64) with the state in LDS up to
//                 WAVE_LIMIT augmented vertices, one workgroup of 1024 with the state in LDS up to LDS_LIMIT, in the workspace
//                 beyond: the same loop body for all three.  The chord starts of round 0 are the nodes, found by an exclusive
//                 max-scan over the node flags.  A round is the four passes of scene_simplify.hip (max, arg, split, link); arg
//                 takes the minimum of (vy * 16385 + vx) << 32 | k among the vertices at the maximum, which is unique inside an
//                 arc and carries the index with it.  Then the guard of the closed arcs
//   5 scan_kept   one workgroup: start' = exclusive scan of the kept counts, cut prefix-shaped at max_vertices_out; counts, info
//   6 scatter     wave and block variants: ordered compaction into vertices_out and left_out, the shoelace sum, the ring row
// No workgroup waits for another, nothing is read back, every loop is capped by a count that was checked against the workspace.
// The passes themselves are csrc/scene_walls.h's, which csrc/scene_safe.hip runs too; this file holds the plain policy, the
// kernels around the passes and the entries.
#include "scene_walls.h"

namespace {

using namespace c3d_walls;

// the plain call: no levels, no directions, no marks, no done word; ring_dp counts the arcs
struct Plain {
  static constexpr bool LEVELLED = false;
  struct Levels {};
  struct Marks {};
  static __device__ __forceinline__ int level(const Levels&, int64_t) { return 0; }
  static __device__ __forceinline__ int arc_word(bool closed, int) { return ~(closed ? 1 : 0); }
  static __device__ __forceinline__ bool arc_closed(int word) { return word == ~1; }
  static __device__ __forceinline__ bool done(const uint32_t*) { return false; }
  static __device__ __forceinline__ void written(const uint32_t*, uint32_t) {}
};

template <bool COLS>
__global__ __launch_bounds__(256) void shared_nodes_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ counts_obj,
                                                           int Hs, int Ws, int max_objects, uint32_t* __restrict__ bits, int words) {
  nodes_pass<COLS>(labels, counts_obj, Hs, Ws, max_objects, bits, words);
}

__global__ __launch_bounds__(256) void shared_count_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ counts_obj,
                                                           int Hs, int Ws, int max_objects, const int32_t* __restrict__ rings,
                                                           const int2* __restrict__ vertices, const int32_t* __restrict__ counts,
                                                           int max_rings, int max_vertices, int32_t* __restrict__ naug, Bits bits) {
  count_pass(labels, counts_obj, Hs, Ws, max_objects, rings, vertices, counts, max_rings, max_vertices, naug, bits);
}

__global__ __launch_bounds__(BLOCK_T) void shared_scan_rows_kernel(const int32_t* __restrict__ counts, int32_t* __restrict__ naug,
                                                               uint32_t* __restrict__ off, uint32_t* __restrict__ large,
                                                               uint32_t* __restrict__ header, int max_rings, int max_vertices) {
  extern __shared__ u64 part[];                            // [BLOCK_T / 64]
  scan_rows_pass(counts, naug, off, large, header, max_rings, max_vertices, part);
}

__global__ __launch_bounds__(256) void shared_augment_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ counts_obj,
                                                             int Hs, int Ws, int max_objects, const int32_t* __restrict__ rings,
                                                             const int2* __restrict__ vertices, const int32_t* __restrict__ naug,
                                                             const uint32_t* __restrict__ off, uint32_t* __restrict__ rot,
                                                             uint32_t* __restrict__ ap, uint32_t* __restrict__ meta,
                                                             uint32_t* __restrict__ header, Bits bits) {
  augment_pass<Plain>(labels, counts_obj, Hs, Ws, max_objects, rings, vertices, naug, off, rot, ap, meta, nullptr, header, bits);
}

// T = 64: the rings of up to WAVE_LIMIT augmented vertices, a wave each; T = BLOCK_T: the listed larger ones
template <int T, int LIMIT>
__global__ __launch_bounds__(T) void shared_dp_kernel(const int32_t* __restrict__ naug, const uint32_t* __restrict__ off,
                                                      const uint32_t* __restrict__ rot, const uint32_t* __restrict__ ap,
                                                      const uint32_t* __restrict__ meta, int32_t* __restrict__ kept,
                                                      uint8_t* __restrict__ flags, int32_t* __restrict__ g_link,
                                                      int32_t* __restrict__ g_arc, u64* __restrict__ g_idx, u64* __restrict__ g_best,
                                                      const uint32_t* __restrict__ large, uint32_t* __restrict__ header, u64 tol2_q) {
  extern __shared__ u64 lds[];
  dp_pass<Plain, T, LIMIT>(naug, off, rot, ap, meta, kept, flags, g_link, g_arc, g_idx, g_best, large, header, Plain::Levels{}, tol2_q,
                           lds);
}

__global__ __launch_bounds__(BLOCK_T) void shared_scan_kept_kernel(const int32_t* __restrict__ kept, uint32_t* __restrict__ startp,
                                                               const uint32_t* __restrict__ header, int32_t* __restrict__ counts_out,
                                                               int32_t* __restrict__ info, int max_vertices_out) {
  extern __shared__ u64 part[];                            // [BLOCK_T / 64], then the first start without room
  scan_kept_pass<Plain>(kept, startp, header, counts_out, info, max_vertices_out, part);
}

__global__ __launch_bounds__(256) void shared_scatter_wave_kernel(const int32_t* __restrict__ rings, const int32_t* __restrict__ naug,
                                                                  const uint32_t* __restrict__ off, const uint32_t* __restrict__ rot,
                                                                  const uint32_t* __restrict__ ap, const uint32_t* __restrict__ meta,
                                                                  const int32_t* __restrict__ kept, const uint32_t* __restrict__ startp,
                                                                  const uint8_t* __restrict__ flags, const uint32_t* __restrict__ header,
                                                                  int32_t* __restrict__ rings_out, int2* __restrict__ vertices_out,
                                                                  int32_t* __restrict__ left_out, int32_t* __restrict__ info,
                                                                  int max_rings) {
  scatter_wave_pass<Plain>(rings, naug, off, rot, ap, meta, kept, startp, flags, header, rings_out, vertices_out, left_out, info,
                           max_rings, Plain::Marks{});
}

__global__ __launch_bounds__(256) void shared_scatter_block_kernel(const int32_t* __restrict__ rings, const int32_t* __restrict__ naug,
                                                                   const uint32_t* __restrict__ off, const uint32_t* __restrict__ rot,
                                                                   const uint32_t* __restrict__ ap, const uint32_t* __restrict__ meta,
                                                                   const int32_t* __restrict__ kept, const uint32_t* __restrict__ startp,
                                                                   const uint8_t* __restrict__ flags, const uint32_t* __restrict__ large,
                                                                   const uint32_t* __restrict__ header, int32_t* __restrict__ rings_out,
                                                                   int2* __restrict__ vertices_out, int32_t* __restrict__ left_out,
                                                                   int32_t* __restrict__ info) {
  extern __shared__ u64 part[];                            // [4], then the area
  scatter_block_pass<Plain>(rings, naug, off, rot, ap, meta, kept, startp, flags, large, header, rings_out, vertices_out, left_out, info,
                            Plain::Marks{}, part);
}

}  // namespace

extern "C" void c3d_outlines_simplify_shared_limits(int32_t out[2]) {
  if (!out) return;
  out[0] = WAVE_LIMIT;
  out[1] = LDS_LIMIT;
}

extern "C" int64_t c3d_outlines_simplify_shared_ws_bytes(int32_t Hs, int32_t Ws, int32_t max_rings, int32_t max_vertices) {
  if (Hs < 1 || Ws < 1 || max_rings < 1 || max_vertices < 1 || max_vertices > (1 << 30)) return C3D_E_BADARG;
  if (Hs > COORD_MAX || Ws > COORD_MAX) return C3D_E_UNSUPPORTED;
  return space_plan(256, Hs, Ws, max_rings, max_vertices).end;
}

extern "C" int c3d_outlines_simplify_shared(const int32_t* labels, const int32_t* counts_obj, int32_t Hs, int32_t Ws, int32_t max_objects,
                                            const int32_t* rings, const int32_t* vertices, const int32_t* counts, int32_t max_rings,
                                            int32_t max_vertices, int64_t tol2_q, int32_t max_vertices_out, int32_t* rings_out,
                                            int32_t* vertices_out, int32_t* left_out, int32_t* counts_out, int32_t* info, void* ws,
                                            void* stream) {
  if (!labels || !counts_obj || !rings || !vertices || !counts || !rings_out || !vertices_out || !left_out || !counts_out || !info || !ws)
    return C3D_E_BADARG;
  if (Hs < 1 || Ws < 1 || max_objects < 1 || max_objects >= (1 << 30) || max_rings < 1 || max_vertices < 1 || max_vertices > (1 << 30) ||
      max_vertices_out < 1 || tol2_q < 0 || tol2_q > C3D_SIMPLIFY_TOL2_Q_MAX)
    return C3D_E_BADARG;
  if (Hs > COORD_MAX || Ws > COORD_MAX) return C3D_E_UNSUPPORTED;
  const Space w = space_plan(256, Hs, Ws, max_rings, max_vertices);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  uint32_t* header = reinterpret_cast<uint32_t*>(base);
  int32_t* naug = reinterpret_cast<int32_t*>(base + w.naug);
  uint32_t* off = reinterpret_cast<uint32_t*>(base + w.off);
  uint32_t* rot = reinterpret_cast<uint32_t*>(base + w.rot);
  int32_t* kept = reinterpret_cast<int32_t*>(base + w.kept);
  uint32_t* startp = reinterpret_cast<uint32_t*>(base + w.startp);
  uint32_t* large = reinterpret_cast<uint32_t*>(base + w.large);
  uint32_t* ap = reinterpret_cast<uint32_t*>(base + w.ap);
  uint32_t* meta = reinterpret_cast<uint32_t*>(base + w.meta);
  uint8_t* flags = reinterpret_cast<uint8_t*>(base + w.flags);
  int32_t* link = reinterpret_cast<int32_t*>(base + w.link);
  int32_t* arc = reinterpret_cast<int32_t*>(base + w.arc);
  u64* idx = reinterpret_cast<u64*>(base + w.idx);
  u64* best = reinterpret_cast<u64*>(base + w.best);
  uint32_t* rowbits = reinterpret_cast<uint32_t*>(base + w.rowbits);
  uint32_t* colbits = reinterpret_cast<uint32_t*>(base + w.colbits);
  const Bits bits{rowbits, colbits, w.WR, w.WC};
  const int2* v_in = reinterpret_cast<const int2*>(vertices);
  int2* v_out = reinterpret_cast<int2*>(vertices_out);

  // only the header: every other word of the workspace is written by the call before the call reads it
  hipError_t e = hipMemsetAsync(base, 0, 256, st);
  if (e != hipSuccess) return (int)e;
  // the ring count is known on the device only: grids are sized by max_rings and surplus waves and workgroups return
  const unsigned g_wave = grid_for(max_rings, 4), g_block = grid_for(max_rings, 1);
  int rc = c3d_launch_lds<shared_nodes_kernel<false>>(dim3(grid_for((int64_t)(Hs + 1) * w.WR * 32, 256)), dim3(256), 0, st, labels, counts_obj,
                                                      (int)Hs, (int)Ws, (int)max_objects, rowbits, w.WR);
  if (rc) return rc;
  rc = c3d_launch_lds<shared_nodes_kernel<true>>(dim3(grid_for((int64_t)(Ws + 1) * w.WC * 32, 256)), dim3(256), 0, st, labels, counts_obj,
                                                 (int)Hs, (int)Ws, (int)max_objects, colbits, w.WC);
  if (rc) return rc;
  rc = c3d_launch_lds<shared_count_kernel>(dim3(g_wave), dim3(256), 0, st, labels, counts_obj, (int)Hs, (int)Ws, (int)max_objects, rings,
                                           v_in, counts, (int)max_rings, (int)max_vertices, naug, bits);
  if (rc) return rc;
  rc = c3d_launch_lds<shared_scan_rows_kernel>(dim3(1), dim3(BLOCK_T), BLOCK_T / 8, st, counts, naug, off, large, header, (int)max_rings,
                                               (int)max_vertices);
  if (rc) return rc;
  rc = c3d_launch_lds<shared_augment_kernel>(dim3(g_wave), dim3(256), 0, st, labels, counts_obj, (int)Hs, (int)Ws, (int)max_objects, rings,
                                             v_in, (const int32_t*)naug, (const uint32_t*)off, rot, ap, meta, header, bits);
  if (rc) return rc;
  rc = c3d_launch_lds<shared_dp_kernel<64, WAVE_LIMIT>>(dim3(g_block), dim3(64), WAVE_LDS_BYTES, st, (const int32_t*)naug,
                                                        (const uint32_t*)off, (const uint32_t*)rot, (const uint32_t*)ap,
                                                        (const uint32_t*)meta, kept, flags, link, arc, idx, best,
                                                        (const uint32_t*)large, header, (u64)tol2_q);
  if (rc) return rc;
  rc = c3d_launch_lds<shared_dp_kernel<BLOCK_T, LDS_LIMIT>>(dim3(g_block), dim3(BLOCK_T), LDS_BYTES, st, (const int32_t*)naug,
                                                            (const uint32_t*)off, (const uint32_t*)rot, (const uint32_t*)ap,
                                                            (const uint32_t*)meta, kept, flags, link, arc, idx, best,
                                                            (const uint32_t*)large, header, (u64)tol2_q);
  if (rc) return rc;
  rc = c3d_launch_lds<shared_scan_kept_kernel>(dim3(1), dim3(BLOCK_T), BLOCK_T / 8 + 8, st, (const int32_t*)kept, startp,
                                               (const uint32_t*)header, counts_out, info, (int)max_vertices_out);
  if (rc) return rc;
  rc = c3d_launch_lds<shared_scatter_wave_kernel>(dim3(g_wave), dim3(256), 0, st, rings, (const int32_t*)naug, (const uint32_t*)off,
                                                  (const uint32_t*)rot, (const uint32_t*)ap, (const uint32_t*)meta, (const int32_t*)kept,
                                                  (const uint32_t*)startp, (const uint8_t*)flags, (const uint32_t*)header, rings_out,
                                                  v_out, left_out, info, (int)max_rings);
  if (rc) return rc;
  return c3d_launch_lds<shared_scatter_block_kernel>(dim3(g_block), dim3(256), 40, st, rings, (const int32_t*)naug, (const uint32_t*)off,
                                                     (const uint32_t*)rot, (const uint32_t*)ap, (const uint32_t*)meta,
                                                     (const int32_t*)kept, (const uint32_t*)startp, (const uint8_t*)flags,
                                                     (const uint32_t*)large, (const uint32_t*)header, rings_out, v_out, left_out, info);
}
