// Pieces shared by the depthwise 3x3x3 translation units (dw_conv.hip, dw_bwd_fused.hip).
#pragma once
#include "common.h"
#include "../../include/change3d_hip.h"   // c3d_bn_fin
#include "launch_hints.h"   // c3d_option_dw_t4
#include <type_traits>

namespace {

constexpr int DW_CV = 4;    // channel vectors (of 8) per workgroup pass = 32 channels
constexpr int DW_MAXT = 5;

struct DwGeom {
  int B, T, H, W, Ho, Wo, C, Cp, stride;
};

// XCD-aware workgroup order.  A 32-channel chunk reads 64 B of every 112/224/432-byte pixel row, so
// the chunks of one tile share their 128-byte lines: counters showed the depthwise kernels fetching
// ~1.8x their input when sibling chunks ran far apart (3-D grid: chunk = blockIdx.y).  Workgroups are
// dealt round-robin to the 8 XCDs (one L2 each) in flattened-id order, so a 1-D grid decoded as
//   id -> (xcd = id % 8, k = id / 8), chunk = k % chunks, group = (k / chunks) * 8 + xcd
// makes the chunks of a group consecutive arrivals on ONE XCD: the second chunk hits that L2.
constexpr int N_XCD = 8;
struct ChunkOrder {
  int chunk, group;   // group = index over (tile groups x samples); < 0: padding workgroup
};
__device__ __forceinline__ ChunkOrder chunk_order(const int chunks, const int ngroups) {
  const int id = blockIdx.x, xcd = id % N_XCD, k = id / N_XCD;
  ChunkOrder o;
  o.chunk = k % chunks;
  o.group = (k / chunks) * N_XCD + xcd;
  if (o.group >= ngroups) o.group = -1;
  return o;
}
inline unsigned chunk_order_grid(const int chunks, const long ngroups) {
  return (unsigned)(((ngroups + N_XCD - 1) / N_XCD) * N_XCD * chunks);
}
// The workgroup decode of every tile-walking depthwise kernel (kernel arguments `g`, `tiles_per_wg`): tile counts, walk
// groups per sample `gx`, then co / b (sample) / tg (walk group) / c0 (first channel of the chunk); a padding workgroup
// returns.  This and the weight staging are macros over the kernels' own arguments and locals: every forced-inline function
// tried in their place changed the register allocation of all the kernels that used it (profiles/dw_refactor.txt).
#define DW_WG_DECODE(TILES_X, TILES_Y)                                                            \
  const int tiles_x = (TILES_X), tiles_y = (TILES_Y);                                             \
  const int ntiles = tiles_x * tiles_y;                                                           \
  const int gx = (ntiles + tiles_per_wg - 1) / tiles_per_wg;                                      \
  const ChunkOrder co = chunk_order((g.Cp + DW_CV * 8 - 1) / (DW_CV * 8), gx * g.B);              \
  if (co.group < 0) return;                                                                       \
  const int b = co.group / gx, tg = co.group % gx;                                                \
  const int c0 = co.chunk * DW_CV * 8;

// weights of the chunk -> LDS as [tap][32 channels] (zero for channels >= C); kernel locals `wl`, `tid`, argument `w`
#define DW_STAGE_WEIGHTS(NTHR)                                                                    \
  for (int i = tid; i < 27 * 32; i += (NTHR)) {                                                   \
    const int tap = i >> 5, c = c0 + (i & 31);                                                    \
    wl[i] = (c < g.C) ? w[(size_t)c * 27 + tap] : 0.f;                                            \
  }

// raw (unconverted) 8-element vectors: what a register prefetch holds between issue and use
template <typename T> struct Raw8;
template <> struct Raw8<bf16_t> {
  typedef uint4 type;
  static __device__ __forceinline__ type load(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }
  static __device__ __forceinline__ void cvt(const type& v, float (&f)[8]) {
    f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
    f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
    f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
  }
};
template <> struct Raw8<float> {
  struct type { float4 a, b; };
  static __device__ __forceinline__ type load(const float* p) {
    type t; t.a = *reinterpret_cast<const float4*>(p); t.b = *reinterpret_cast<const float4*>(p + 4); return t;
  }
  static __device__ __forceinline__ void cvt(const type& v, float (&f)[8]) {
    f[0] = v.a.x; f[1] = v.a.y; f[2] = v.a.z; f[3] = v.a.w; f[4] = v.b.x; f[5] = v.b.y; f[6] = v.b.z; f[7] = v.b.w;
  }
};

__device__ __forceinline__ void lds8(const float* p, float (&f)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

// Frame-count instantiation of a clip: three frames (BCD, CC), four (BDA: num_perception_frame = 2), five (SCD).  With
// C3D_OPT_DW_T4 = 0 a four-frame clip runs on the five-frame instantiation, its fifth frame staged as zeros.
inline int dw_frames(const int T) { return T <= 3 ? 3 : (T == 4 && c3d_option_dw_t4) ? 4 : 5; }

// f(std::integral_constant<int, N>{}) with N = dw_frames(T): the one frame ladder of the depthwise launchers
template <class F> auto with_frames(const int T, F&& f) {
  switch (dw_frames(T)) {
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, 5>{});
  }
}

// the one place Ho / Wo are computed (a stride that is not positive is left for geom_ok to reject)
inline DwGeom dw_geom(const int B, const int T, const int H, const int W, const int C, const int Cp, const int stride) {
  const int s = stride > 0 ? stride : 1;
  return DwGeom{B, T, H, W, (H - 1) / s + 1, (W - 1) / s + 1, C, Cp, stride};
}
inline int dw_chunks(const DwGeom& g) { return (g.Cp + DW_CV * 8 - 1) / (DW_CV * 8); }   // 32-channel chunks

// Walk length of a tile-walking workgroup and the chunk_order_grid extent that goes with it: from `start` tiles, halved
// while more than `floor` and the grid would hold fewer than `wanted` workgroups; then the tuning knob (when named and
// positive), then the clamp to the tile count.
struct DwWalk {
  int tpw;
  unsigned grid;
};
inline DwWalk dw_walk(const DwGeom& g, const int ntiles, const int start, const int floor, const long wanted, const char* knob) {
  const int chunks = dw_chunks(g);
  int tpw = start;
  while (tpw > floor && (long)((ntiles + tpw - 1) / tpw) * chunks * g.B < wanted) tpw >>= 1;
  if (knob && c3d_knob(knob, 0) > 0) tpw = c3d_knob(knob, 0);
  if (tpw > ntiles) tpw = ntiles;
  return DwWalk{tpw, chunk_order_grid(chunks, (long)((ntiles + tpw - 1) / tpw) * g.B)};
}

// One forward / one fused-backward call, built by the extern "C" entry point and passed down to the launcher.
// fin == nullptr (forward) / a zeroed fin (backward) is the form without the folded BatchNorm finalize.
struct DwFwdCall {
  const void* x;
  const float* ss;
  const float* w;
  void* y;
  double* nc;
  DwGeom g;
  hipStream_t stream;
  const c3d_bn_fin* fin;
};
struct DwBwdCall {
  const void *t1, *b;
  const float *cA, *cB, *cC, *w;
  const void* a;
  const float *ss_a, *mr_a;
  void* t2;
  double* dsums;
  float* dw;
  DwGeom g;
  hipStream_t stream;
  c3d_bn_fin fin;
};

inline bool geom_ok(const DwGeom& g) {
  if (g.B <= 0 || g.T <= 0 || g.T > DW_MAXT || g.H <= 0 || g.W <= 0 || g.C <= 0 || g.Cp < g.C || (g.Cp & 7))
    return false;
  if (g.stride != 1 && g.stride != 2) return false;
  if (g.Ho != (g.H - 1) / g.stride + 1 || g.Wo != (g.W - 1) / g.stride + 1) return false;
  return true;
}

}  // namespace
