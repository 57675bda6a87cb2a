// Shared pieces of the pointwise-convolution kernels: the matrix-core wrappers, and the host-side vocabulary of their launch
// plans (pw_gemm*.hip, pw_cfwd.hip, pw_cdgrad.hip, pw_wgrad.hip, pw_wgrad_v2.hip, make_plan of stage_plan.h).
#pragma once
#include "common.h"
#include "launch_hints.h"

namespace {

template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
  typedef bf16_t lds_t;
  static constexpr int KSTEP = 32;
  static constexpr int KPAD = 8;
  typedef uint4 frag_t;
  static __device__ __forceinline__ frag_t load(const lds_t* base, int row, int ks, int kl, int lane) {
    return *reinterpret_cast<const uint4*>(base + row * kl + ks * 32 + (lane >> 4) * 8);
  }
  // WEIGHT image of the narrow kernel: 8-element k-chunk major, [Kpad / 8][NROWS][8] (NROWS = NT * 16 image rows).  A
  // ds_read_b128 is served in four groups of 16 lanes, each half of one 16-lane row group and half of the next
  // ({0-3, 12-15, 20-27}, ...: /opt/skills/guides/MI355X_MICROARCH.md, LDS table): an A fragment (lane = image row
  // lane % 16, k-chunk lane / 16) of a row-major [n][KL] image makes those halves share bank quads for every KL (8 LDS
  // cycles per read instead of 4); with the chunk index a multiple of 256 B away, the bank quad is the row alone.
  static __host__ __device__ __forceinline__ int widx(int n, int k, int kl, int nrows) { return ((k >> 3) * nrows + n) * 8 + (k & 7); }
  static __device__ __forceinline__ frag_t loadw(const lds_t* base, int n, int ks, int kl, int nrows, int lane) {
    return *reinterpret_cast<const uint4*>(base + ((ks * 4 + (lane >> 4)) * nrows + n) * 8);
  }
  static __device__ __forceinline__ f32x4_t mma(frag_t a, frag_t b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a),
                                                   __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ void store8(lds_t* p, const float (&f)[8]) { Vec8<bf16_t>::store(p, f); }
  static __device__ __forceinline__ lds_t cvt(float f) { return f32_to_bf16(f); }
};
template <> struct Mma<float> {
  typedef float lds_t;
  static constexpr int KSTEP = 4;
  static constexpr int KPAD = 4;
  typedef float frag_t;
  static __device__ __forceinline__ frag_t load(const lds_t* base, int row, int ks, int kl, int lane) {
    return base[row * kl + ks * 4 + (lane >> 4)];
  }
  static __host__ __device__ __forceinline__ int widx(int n, int k, int kl, int nrows) { return n * kl + k; }   // row major
  static __device__ __forceinline__ frag_t loadw(const lds_t* base, int n, int ks, int kl, int nrows, int lane) {
    return load(base, n, ks, kl, lane);
  }
  static __device__ __forceinline__ f32x4_t mma(frag_t a, frag_t b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ void store8(lds_t* p, const float (&f)[8]) { Vec8<float>::store(p, f); }
  static __device__ __forceinline__ lds_t cvt(float f) { return f; }
};


inline int device_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
    cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  return cus;
}

// ------------------------------------------------------------------------------------------ launch plans (host)
// Output tiles (16 channels each) of the packed weight image (c3d_pw_pack_weights: [Kpad / 8][16 * bucket][8]) for Np padded
// output channels.  The buckets ARE the NT instantiations of the wave-private kernel: dispatch_nt (pw_gemm_impl.h) and
// dispatch_wg / plan_wg (pw_gemm_wg.hip) spell them as ladders of template arguments, and every kernel that reads an image
// (pw_cfwd.hip, pw_cdgrad.hip) strides it by this many rows.
inline int pw_nt_bucket(int Np) {
  const int nt = (Np + 15) / 16;
  return nt <= 2 ? 2 : nt <= 4 ? 4 : nt <= 7 ? 7 : 14;
}

// The narrow kernels (channel counts up to 224) address rows with 32-bit byte offsets into bounds-checked buffer resources,
// and offset 2^31 means "nowhere" (a lane without an item still issues its load, so that counted waits stay exact): every
// tensor of a call -- `rows` rows of Kp or Np elements -- must stay under 2 GiB.  The cooperative kernels address one tile
// past the end, and "nowhere" + a tile base must not wrap into the tensor: they pass rows + 512.
inline bool pw_fits_u32(int64_t rows, int Kp, int Np, int elem_bytes) {
  return rows * (int64_t)(Kp > Np ? Kp : Np) * elem_bytes < ((int64_t)1 << 31);
}

// Persistent walk: `tiles` row tiles on at most `cap` workgroups that take at least `min_tpw` tiles each while there is
// enough work; every workgroup walks tiles_per_wg consecutive tiles, and the grid is what that leaves.
struct PwWalk { int64_t blocks; int tiles_per_wg; };
inline PwWalk pw_walk(int64_t tiles, int64_t cap, int min_tpw) {
  int64_t blocks = (tiles + min_tpw - 1) / min_tpw;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  const int tpw = (int)((tiles + blocks - 1) / blocks);
  return {(tiles + tpw - 1) / tpw, tpw};
}

// Workgroups of a pointwise weight gradient (pw_wgrad.hip, pw_wgrad_v2.hip: one partial per workgroup, `max_parts` of them
// fit the workspace): one per CU -- or, launched on the stage driver's side stream (c3d_side_launch), 7/8 of the CUs.  These
// single-round kernels hold a CU for their whole duration: at full width every kernel of the data-gradient chain that becomes
// ready meanwhile, its 1-8 workgroup coefficient kernels included, waits for the weight gradient to end.
// Measured on MI355X, B=32 bf16, ms per step (profiles/r02_side_stream_width_final.json):
//   round 2, 60-step runs: 256 / 208 / 192 / 176 / 160 / 128 workgroups -> 32.52 / 32.08 / 31.84 / 32.11 / 32.48 / 32.87: 3/4;
//   round 5, after the data-gradient kernels' waits became exact (same-call sweeps through the instrumented build): 128 / 144 /
//   160 / 176 / 192 / 256 -> 23.01 / 22.99 / 22.86 / 23.53 / 23.18 / 23.34: 5/8;
//   ...and once c3d_block_out_bwd was folded into the conv_a data gradient (the elementwise pass that used to fill the CUs a
//   narrow weight gradient left): 96 / 128 / 160 / 192 / 208 / 224 / 240 / 256 -> 23.46 / 22.81 / 22.70 / 22.53 / 22.34 / 22.29 /
//   22.33 / 22.34 (SCD and CC: 224 best by 0.5 % too): 7/8.
// Tuning knobs (instrumented build): C3D_WG_BLOCKS = the cap itself, C3D_PWWG_SIDE_WGS = the side-stream cap.
#ifndef W2_SIDE_EIGHTHS
#define W2_SIDE_EIGHTHS 7
#endif
inline int64_t pw_wgrad_cap(int max_parts) {
  static const int cap_env = c3d_knob("C3D_WG_BLOCKS", 0), side_env = c3d_knob("C3D_PWWG_SIDE_WGS", 0);
  int64_t cap = device_cus() < max_parts ? device_cus() : max_parts;
  if (cap_env > 0 && cap_env <= max_parts) return cap_env;
  if (c3d_side_launch) {
    const int64_t side_cap = side_env > 0 ? side_env : (int64_t)device_cus() * W2_SIDE_EIGHTHS / 8;
    if (side_cap < cap) cap = side_cap;
  }
  return cap;
}

// Weight gradient, eight waves as a WN x WK grid over the NT x KT tiles (16 x 16) of dW: per-wave tile grids (TN x TK) are
// instantiated for the table below, a launch runs the smallest that covers its ceil(NT / WN) x ceil(KT / WK), zero-padded --
// and that instantiated grid is what costs: MFMAs dominate, then fragment loads.  WN == 0: no grid holds the shape.
struct PwWgInst { int tn, tk; };
constexpr PwWgInst PW_WG_INSTS[] = {{1, 1}, {2, 2}, {3, 4}, {4, 3}, {4, 4}};
struct PwWaveGrid { int WN, WK, inst; };
inline PwWaveGrid pw_wave_grid(int NT, int KT) {
  PwWaveGrid g = {0, 0, 4};
  const int cand[4][2] = {{8, 1}, {4, 2}, {2, 4}, {1, 8}};
  int best = 1 << 30;
  for (int c = 0; c < 4; ++c) {
    const int tn = (NT + cand[c][0] - 1) / cand[c][0], tk = (KT + cand[c][1] - 1) / cand[c][1];
    if (tn > 4 || tk > 4) continue;
    int inst = 4;
    for (int i = 0; i < 5; ++i)
      if (PW_WG_INSTS[i].tn >= tn && PW_WG_INSTS[i].tk >= tk) { inst = i; break; }
    const int ti = PW_WG_INSTS[inst].tn, tj = PW_WG_INSTS[inst].tk;
    const int cost = ti * tj * 4 + ti + tj;
    if (cost < best) { best = cost; g = {cand[c][0], cand[c][1], inst}; }
  }
  return g;
}

}  // namespace
