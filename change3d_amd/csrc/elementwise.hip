// Elementwise / reduction kernels on channels-last tensors, 8-channel vectors per thread:
//   * res-block output: y = relu(bn_c(c) + shortcut)      (reference model/x3d.py:326-327 and the
//     stem's BN+ReLU, model/x3d.py:94-106) and its backward g = dy*(y>0) with the BN-backward sums
//   * the pieces of Encoder.enhance (reference model/trainer.py:71-108)
//   * the stem's output + enhance without a stored y / dy (stem_enhance_fwd / _mid kernels)
// The backward of the first and the last item is ONE kernel, block_out_bwd_kernel, with two operand policies: the
// stored operands (dy, y, c, optional shortcut) and the stem-enhance operands (y and dy formed on load).
// Threads keep a FIXED channel vector (blockDim is a multiple of Cp/8 and so is the grid stride),
// so per-channel parameters and partial sums stay in registers.
#include "common.h"
#include "bn_fin.h"
#include <cstring>
#include <cstdlib>
#include "../../include/change3d_hip.h"

namespace {

__host__ __device__ inline int ew_block(int G) { return G * (256 / G); }

// shortcut modes
enum { SC_NONE = 0, SC_IDENTITY = 1, SC_BN = 2, SC_RAW = 3 };

// ---- small pieces used from more than one kernel ------------------------------------------------------------------
// one 8-float parameter row as two 16-byte loads (the rows are 32-byte aligned: Cp is a multiple of 8)
__device__ __forceinline__ void load_rows8(const float* p, float (&f)[8]) {
  const float4 x = *reinterpret_cast<const float4*>(p), y = *reinterpret_cast<const float4*>(p + 4);
  f[0] = x.x; f[1] = x.y; f[2] = x.z; f[3] = x.w; f[4] = y.x; f[5] = y.y; f[6] = y.z; f[7] = y.w;
}

// the stem's y = relu(bn(u)), rounded to T exactly as block_out_fwd_kernel stores it (the stem has no shortcut)
template <typename T>
__device__ __forceinline__ void stem_y(const float (&uv)[8], const float (&a)[8], const float (&b)[8], float (&y)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) y[j] = round_as<T>(fmaxf(fmaf(uv[j], a[j], b[j]), 0.f));
}

// enhance's d = |y_pre - y_post|, written over p
__device__ __forceinline__ void absdiff8(float (&p)[8], const float (&q)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) p[j] = fabsf(p[j] - q[j]);
}

// enhance backward, one element of a t_pre (sgn_self = +1) or t_post (-1) row: dy = dout +- sign(y_pre - y_post) * dd in
// f32 (the caller rounds to T once: by storing it, or with round_as where dy is consumed in registers)
__device__ __forceinline__ float enhance_dy(float dout, float y_pre, float y_post, float dd, float sgn_self) {
  const float df = y_pre - y_post;
  const float sg = (df > 0.f) ? 1.f : ((df < 0.f) ? -1.f : 0.f);
  return dout + sgn_self * sg * dd;
}

template <typename T>
__global__ void block_out_fwd_kernel(const T* __restrict__ c, const float* __restrict__ ss_c,
                                     const T* __restrict__ sc, const float* __restrict__ ss_1, int sc_mode,
                                     T* __restrict__ y, int64_t nvec, int G, int C, const c3d_bn_fin fin_c,
                                     const c3d_bn_fin fin_1) {
  __shared__ float lss[4][256];   // scale_c | shift_c | scale_1 | shift_1 (consumer-side BatchNorm finalisation)
  const int v = threadIdx.x % G;
  const int Cp = G * 8;
  float a[8], b[8], a1[8], b1[8];
  if (fin_c.sums) {
    // every workgroup rebuilds the vectors from the producers' completed sums (csrc/bn_fin.h); workgroup 0 owns the
    // global outputs (scale/shift, mean/rstd for backward, running statistics)
    const bool owner = blockIdx.x == 0;
    if (owner && threadIdx.x == 0 && fin_c.nbt) *fin_c.nbt += 1;
    c3dfin::bn_consume(fin_c, C, Cp, 0, Cp, owner, lss[0], lss[1], threadIdx.x, blockDim.x);
    if (sc_mode == SC_BN) {
      if (owner && threadIdx.x == 0 && fin_1.nbt) *fin_1.nbt += 1;
      c3dfin::bn_consume(fin_1, C, Cp, 0, Cp, owner, lss[2], lss[3], threadIdx.x, blockDim.x);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = lss[0][v * 8 + j]; b[j] = lss[1][v * 8 + j];
      a1[j] = (sc_mode == SC_BN) ? lss[2][v * 8 + j] : 1.f;
      b1[j] = (sc_mode == SC_BN) ? lss[3][v * 8 + j] : 0.f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = ss_c[v * 8 + j]; b[j] = ss_c[Cp + v * 8 + j];
      a1[j] = (sc_mode == SC_BN) ? ss_1[v * 8 + j] : 1.f;
      b1[j] = (sc_mode == SC_BN) ? ss_1[Cp + v * 8 + j] : 0.f;
    }
  }
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    float f[8], s[8];
    Vec8<T>::load(c + i * 8, f);
    if (sc_mode != SC_NONE) Vec8<T>::load(sc + i * 8, s);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float r = fmaf(f[j], a[j], b[j]);
      if (sc_mode != SC_NONE) r += fmaf(s[j], a1[j], b1[j]);
      f[j] = fmaxf(r, 0.f);
    }
    Vec8<T>::store(y + i * 8, f);
  }
}

// ---- res-block / stem output backward: one kernel, two operand policies ------------------------------------------
// g = dy * (y > 0); dsums_c += (sum g, sum g*chat); dsums_1 += (sum g, sum g*shat) when the shortcut
// has BN, with chat = (c - mean)*rstd accumulated centred (mr = mean[Cp], rstd[Cp]).
// A policy says where one row's (dy, y, c) come from: `Row` is what load() fetches in the batched load phase (raw
// vectors, nothing converted), finish() turns one Row into f32 values, `Walk` is per-thread state set up by begin().
// The optional shortcut s and the fin.ticket tail are the kernel's own; a policy says whether a launch can have them.
// Policies are static functions over the kernel's arguments (element offset e = 8 * row), not objects holding them, and
// StoredOperands::Row has the member order it has, because either change moves the register allocation of the four
// stored instantiations, which are hot: after an edit here compare them with tools/device_code_diff.sh.
//
// Stored operands: dy, y and c are tensors.
// PRE: `dy` is already dy * (y > 0) (masked by its producer, c3d_pw_args.wg_mask_out): y is not read, g is not written -- the
// pass only produces the BatchNorm-backward sums.  (A compile-time switch: the same test at run time cost the unmasked form
// 12 % -- 1.57 -> 1.76 ms per step.)
template <typename T, bool PRE>
struct StoredOperands {
  typedef T elem_t;
  typedef typename Vec8<T>::raw_t raw_t;
  static constexpr bool MASKED = PRE;
  static constexpr bool SHORTCUT = true;   // the launch may carry a shortcut s
  static constexpr bool FIN = true;        // ... and the fin.ticket tail
  struct Row { raw_t c, y, d; };
  struct Walk {};
  static __device__ __forceinline__ void begin(Walk&, int, int, int64_t) {}
  static __device__ __forceinline__ void load(Row& r, Walk&, const T* dy, const T* y, const T* c, int64_t e, int64_t) {
    r.d = Vec8<T>::load_raw(dy + e);
    if (!PRE) r.y = Vec8<T>::load_raw(y + e);
    r.c = Vec8<T>::load_raw(c + e);
  }
  static __device__ __forceinline__ void finish(const Row& r, const Walk&, float (&d)[8], float (&yv)[8], float (&cv)[8]) {
    Vec8<T>::cvt_raw(r.d, d);
    if (!PRE) Vec8<T>::cvt_raw(r.y, yv);
    Vec8<T>::cvt_raw(r.c, cv);
  }
};

// Stem-enhance operands (no stored y, no stored dy, no shortcut): the kernel's dy argument is dout, its c argument is
// the stem's u, y and s are not passed;
//   y  = relu(bn(u)) rounded to T;   dy = dout, and on frames t_pre / t_post dout +- sign(y_pre - y_post) * dd in f32
//   rounded to T (the value enhance_bwd_apply_kernel stores).
// The row -> (sample, frame, offset) split is carried along the walk (one division per thread, not one per row).
template <typename T>
struct StemEnhanceOperands {
  typedef T elem_t;
  typedef typename Vec8<T>::raw_t raw_t;
  static constexpr bool MASKED = false;
  static constexpr bool SHORTCUT = false;
  static constexpr bool FIN = false;
  struct Extra {
    const float* ss;   // scale | shift
    const T* dd;
    int64_t hwv;
    int Tn, t_pre, t_post;
  };
  struct Row {
    raw_t d, c, o, dd;   // o: the partner row (t_post for a t_pre row and the reverse)
    int side;            // 0: untouched frame, +1: t_pre row, -1: t_post row
  };
  struct Walk {
    float a[8], b[8];   // scale | shift
    int64_t other;      // element distance from a t_pre row to its t_post partner
    int64_t cb, cr;     // cursor of the next row this thread visits: sample cb, frame ct, offset cr inside the frame
    int ct;
  };
  static __device__ __forceinline__ void begin(Walk& w, int v, int Cp, int64_t first, const Extra& x) {
    load_rows8(x.ss + v * 8, w.a);
    load_rows8(x.ss + Cp + v * 8, w.b);
    w.other = (int64_t)(x.t_post - x.t_pre) * x.hwv * 8;
    const int64_t bt = first / x.hwv;
    w.cr = first - bt * x.hwv;
    w.cb = bt / x.Tn;
    w.ct = (int)(bt - w.cb * x.Tn);
  }
  static __device__ __forceinline__ void load(Row& r, Walk& w, const T* dout, const T*, const T* u, int64_t e, int64_t stride,
                                              const Extra& x) {
    r.d = Vec8<T>::load_raw(dout + e);
    r.c = Vec8<T>::load_raw(u + e);
    r.side = (w.ct == x.t_pre) ? 1 : ((w.ct == x.t_post) ? -1 : 0);
    if (r.side) {
      r.o = Vec8<T>::load_raw(u + e + r.side * w.other);
      r.dd = Vec8<T>::load_raw(x.dd + (w.cb * x.hwv + w.cr) * 8);
    }
    w.cr += stride;
    while (w.cr >= x.hwv) {
      w.cr -= x.hwv;
      if (++w.ct == x.Tn) { w.ct = 0; ++w.cb; }
    }
  }
  static __device__ __forceinline__ void finish(const Row& r, const Walk& w, float (&d)[8], float (&yv)[8], float (&cv)[8]) {
    Vec8<T>::cvt_raw(r.d, d);
    Vec8<T>::cvt_raw(r.c, cv);
    stem_y<T>(cv, w.a, w.b, yv);
    if (r.side) {
      float ov[8], yo[8], dv[8];
      Vec8<T>::cvt_raw(r.o, ov);
      Vec8<T>::cvt_raw(r.dd, dv);
      stem_y<T>(ov, w.a, w.b, yo);
      const bool is_pre = r.side > 0;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        d[j] = round_as<T>(enhance_dy(d[j], is_pre ? yv[j] : yo[j], is_pre ? yo[j] : yv[j], dv[j], is_pre ? 1.f : -1.f));
    }
  }
};

template <class Ops, class... Extra>   // Extra: the policy's own kernel argument (none, or one Ops::Extra)
__global__ __launch_bounds__(256) void block_out_bwd_kernel(
    const typename Ops::elem_t* __restrict__ dy, const typename Ops::elem_t* __restrict__ y,
    const typename Ops::elem_t* __restrict__ c, const typename Ops::elem_t* __restrict__ s_,
    typename Ops::elem_t* __restrict__ g, const float* __restrict__ mr_c, const float* __restrict__ mr_1,
    double* __restrict__ dsums_c, double* __restrict__ dsums_1, int64_t nvec, int G, int C, const c3d_bn_fin fin_c,
    const c3d_bn_fin fin_1, const Extra... extra) {
  typedef typename Ops::elem_t T;
  extern __shared__ float red[];  // [blockDim][24]
  const int v = threadIdx.x % G;
  const int Cp = G * 8;
  const T* const s = Ops::SHORTCUT ? s_ : nullptr;
  // per-thread partial sums in f32 (a thread's grid-stride chain is 12-200 terms: its rounding error is ~1e-5 of ONE
  // term and random across the ~1e5 threads), everything across threads in f64 below -- the near-cancellation of
  // (sum g*chat) happens between threads, not inside one.  (Per-element v_cvt_f64_f32 + v_add_f64 triples -- f64 VALU runs
  // at a fraction of the f32 rate -- plus 48 accumulator registers made this elementwise pass run at 3.7 TB/s.)
  float s1[8], s2[8], s3[8];
  float mc[8], rc[8], m1[8], r1[8];
  {
    // eight 16-byte loads in ONE round trip (the rows are 32-byte aligned: Cp is a multiple of 8, the vectors come from the
    // stage workspace).  As 32 scalar loads with `s ? mr_1[..] : 0` selects the compiler put s_waitcnt vmcnt(0) behind every
    // pair: eight dependent memory round trips, ~8 us of a 27 us launch on the 32 x 32 maps (round 5, from the ISA)
    const float* q1 = s ? mr_1 : mr_c;   // a valid address either way: the loads are unconditional
    float vc[8], vd[8];
    load_rows8(mr_c + v * 8, mc);
    load_rows8(mr_c + Cp + v * 8, rc);
    load_rows8(q1 + v * 8, vc);
    load_rows8(q1 + Cp + v * 8, vd);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s1[j] = 0.f; s2[j] = 0.f; s3[j] = 0.f;
      m1[j] = s ? vc[j] : 0.f; r1[j] = s ? vd[j] : 0.f;
    }
  }
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  typename Ops::Walk walk;
  Ops::begin(walk, v, Cp, first, extra...);
  // The grid is capped (the closing same-address atomics): ~1.5 workgroups per CU, so the bytes in flight come from the
  // loop itself -- BOB_U iterations' loads (raw vectors) are issued before the first is consumed; a thread's terms are
  // added in the order of the plain loop (bit-identical sums, whichever policy).
  constexpr int BOB_U = 4;
  for (int64_t i0 = first; i0 < nvec; i0 += BOB_U * stride) {
    struct { typename Ops::Row ops; typename Vec8<T>::raw_t s; } row[BOB_U];
#pragma unroll
    for (int u = 0; u < BOB_U; ++u) {
      const int64_t i = i0 + u * stride;
      if (i < nvec) {
        Ops::load(row[u].ops, walk, dy, y, c, i * 8, stride, extra...);
        if (s) row[u].s = Vec8<T>::load_raw(s + i * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < BOB_U; ++u) {
      const int64_t i = i0 + u * stride;
      if (i < nvec) {
        float d[8], yv[8], cv[8], sv[8];
        Ops::finish(row[u].ops, walk, d, yv, cv);
        if (s) Vec8<T>::cvt_raw(row[u].s, sv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float gg = (Ops::MASKED || yv[j] > 0.f) ? d[j] : 0.f;
          d[j] = gg;
          s1[j] += gg; s2[j] += gg * ((cv[j] - mc[j]) * rc[j]);
          if (s) s3[j] += gg * ((sv[j] - m1[j]) * r1[j]);
        }
        if (!Ops::MASKED) Vec8<T>::store(g + i * 8, d);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[threadIdx.x * 24 + j] = s1[j]; red[threadIdx.x * 24 + 8 + j] = s2[j]; red[threadIdx.x * 24 + 16 + j] = s3[j];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < G * 24; idx += blockDim.x) {
    const int vv = idx / 24, k = idx % 24;
    double acc = 0;
    for (int t = vv; t < (int)blockDim.x; t += G) acc += red[t * 24 + k];
    const int ch = vv * 8 + (k & 7);
    const int which = k >> 3;
    if (ch < C) {
      if (which == 0) { atomicAdd(dsums_c + ch, acc); if (dsums_1) atomicAdd(dsums_1 + ch, acc); }
      else if (which == 1) atomicAdd(dsums_c + C + ch, acc);
      else if (dsums_1) atomicAdd(dsums_1 + C + ch, acc);
    }
  }
  if (Ops::FIN && fin_c.ticket) {   // last workgroup: BatchNorm_c (and shortcut BatchNorm) backward coefficients
    if (c3dfin::last_workgroup(fin_c.ticket, gridDim.x, reinterpret_cast<int*>(red))) {
      c3dfin::bn_backward(fin_c, dsums_c, 1, C, Cp, threadIdx.x, blockDim.x & ~15);
      if (dsums_1 && fin_1.ss) c3dfin::bn_backward(fin_1, dsums_1, 1, C, Cp, threadIdx.x, blockDim.x & ~15);
    }
  }
}

// ---- enhance pieces -----------------------------------------------------------------------
// d[m][c] = | y[b, t_pre, p, c] - y[b, t_post, p, c] |   (dense [B*HW][Cp])
template <typename T>
__global__ void frame_absdiff_kernel(const T* __restrict__ y, T* __restrict__ d, int64_t nvec, int64_t hwv,
                                     int Tn, int t_pre, int t_post) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    const int64_t b = i / hwv, r = i - b * hwv;
    float p[8], q[8];
    Vec8<T>::load(y + ((b * Tn + t_pre) * hwv + r) * 8, p);
    Vec8<T>::load(y + ((b * Tn + t_post) * hwv + r) * 8, q);
    absdiff8(p, q);
    Vec8<T>::store(d + i * 8, p);
  }
}

// out = copy(y); out[:, t_mid] += relu(e)      (e dense [B*HW][Cp])
template <typename T>
__global__ void enhance_apply_kernel(const T* __restrict__ y, const T* __restrict__ e, T* __restrict__ out,
                                     int64_t nvec_all, int64_t hwv, int Tn, int t_mid) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec_all; i += stride) {
    const int64_t bt = i / hwv, r = i - bt * hwv;
    const int64_t b = bt / Tn;
    const int t = (int)(bt - b * Tn);
    float f[8];
    Vec8<T>::load(y + i * 8, f);
    if (t == t_mid) {
      float ev[8];
      Vec8<T>::load(e + (b * hwv + r) * 8, ev);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] += fmaxf(ev[j], 0.f);
    }
    Vec8<T>::store(out + i * 8, f);
  }
}

// de[m][c] = dout[b, t_mid, p, c] * (e[m][c] > 0)
template <typename T>
__global__ void enhance_bwd_mask_kernel(const T* __restrict__ dout, const T* __restrict__ e, T* __restrict__ de,
                                        int64_t nvec, int64_t hwv, int Tn, int t_mid) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    const int64_t b = i / hwv, r = i - b * hwv;
    float g[8], ev[8];
    Vec8<T>::load(dout + ((b * Tn + t_mid) * hwv + r) * 8, g);
    Vec8<T>::load(e + i * 8, ev);
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = ev[j] > 0.f ? g[j] : 0.f;
    Vec8<T>::store(de + i * 8, g);
  }
}

// dy = copy(dout); dy[:, t_pre] += dd*sign(pre-post); dy[:, t_post] -= dd*sign(pre-post)
template <typename T>
__global__ void enhance_bwd_apply_kernel(const T* __restrict__ dout, const T* __restrict__ y,
                                         const T* __restrict__ dd, T* __restrict__ dy, int64_t nvec_all,
                                         int64_t hwv, int Tn, int t_pre, int t_post) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec_all; i += stride) {
    const int64_t bt = i / hwv, r = i - bt * hwv;
    const int64_t b = bt / Tn;
    const int t = (int)(bt - b * Tn);
    float f[8];
    Vec8<T>::load(dout + i * 8, f);
    if (t == t_pre || t == t_post) {
      float p[8], q[8], dv[8];
      Vec8<T>::load(y + ((b * Tn + t_pre) * hwv + r) * 8, p);
      Vec8<T>::load(y + ((b * Tn + t_post) * hwv + r) * 8, q);
      Vec8<T>::load(dd + (b * hwv + r) * 8, dv);
      const float sgn_self = (t == t_pre) ? 1.f : -1.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = enhance_dy(f[j], p[j], q[j], dv[j], sgn_self);
    }
    Vec8<T>::store(dy + i * 8, f);
  }
}

// ---- stem output + enhance without the stem's y ----------------------------------------------------------------
// The stem has no shortcut, so y = relu(bn(u)) is a pure function of u and the 2 x Cp scale|shift vector: the two
// kernels below recompute it on load (stem_y) instead of reading a materialised y; their backward is
// block_out_bwd_kernel<StemEnhanceOperands>.  Threads keep a fixed channel vector (blockDim and hwv are multiples of G),
// as block_out_* do.
// forward, every frame but t_mid: out[:, t] = y[:, t];  d = |y[:, t_pre] - y[:, t_post]|   (d dense [B*HW][Cp])
template <typename T>
__global__ __launch_bounds__(256) void stem_enhance_fwd_kernel(const T* __restrict__ u, const float* __restrict__ ss,
                                                               T* __restrict__ out, T* __restrict__ d, int64_t nvec,
                                                               int64_t hwv, int G, int Tn, int t_pre, int t_post,
                                                               int t_mid) {
  const int v = threadIdx.x % G;
  float a[8], b[8];
  load_rows8(ss + v * 8, a);
  load_rows8(ss + G * 8 + v * 8, b);
  typedef typename Vec8<T>::raw_t raw_t;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    const int64_t bb = i / hwv, r = i - bb * hwv;
    const int64_t base = bb * Tn * hwv + r;
    const raw_t rp = Vec8<T>::load_raw(u + (base + t_pre * hwv) * 8);
    const raw_t rq = Vec8<T>::load_raw(u + (base + t_post * hwv) * 8);
    float f[8], p[8], q[8];
    Vec8<T>::cvt_raw(rp, f);
    stem_y<T>(f, a, b, p);
    Vec8<T>::store(out + (base + t_pre * hwv) * 8, p);
    Vec8<T>::cvt_raw(rq, f);
    stem_y<T>(f, a, b, q);
    Vec8<T>::store(out + (base + t_post * hwv) * 8, q);
    absdiff8(p, q);
    Vec8<T>::store(d + i * 8, p);
    for (int t = 0; t < Tn; ++t) {   // the perception frames other than t_mid (none for T = 3)
      if (t == t_pre || t == t_post || t == t_mid) continue;
      Vec8<T>::load(u + (base + t * hwv) * 8, f);
      stem_y<T>(f, a, b, q);
      Vec8<T>::store(out + (base + t * hwv) * 8, q);
    }
  }
}

// forward, frame t_mid: out[:, t_mid] = y[:, t_mid] + relu(e)      (e dense [B*HW][Cp]; the add in f32 on the rounded y)
template <typename T>
__global__ __launch_bounds__(256) void stem_enhance_mid_kernel(const T* __restrict__ u, const float* __restrict__ ss,
                                                               const T* __restrict__ e, T* __restrict__ out,
                                                               int64_t nvec, int64_t hwv, int G, int Tn, int t_mid) {
  const int v = threadIdx.x % G;
  float a[8], b[8];
  load_rows8(ss + v * 8, a);
  load_rows8(ss + G * 8 + v * 8, b);
  typedef typename Vec8<T>::raw_t raw_t;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    const int64_t bb = i / hwv, r = i - bb * hwv;
    const int64_t row = (bb * Tn + t_mid) * hwv + r;
    const raw_t ru = Vec8<T>::load_raw(u + row * 8);
    const raw_t re = Vec8<T>::load_raw(e + i * 8);
    float f[8], y[8], ev[8];
    Vec8<T>::cvt_raw(ru, f);
    Vec8<T>::cvt_raw(re, ev);
    stem_y<T>(f, a, b, y);
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] += fmaxf(ev[j], 0.f);
    Vec8<T>::store(out + row * 8, y);
  }
}

// Generic helpers ------------------------------------------------------------------------------
// dst[b, t, p, :] (frame of an NDHWC tensor) += / = src dense [B*HW][Cp]
template <typename T>
__global__ void frame_scatter_kernel(const T* __restrict__ src, T* __restrict__ dst, int64_t nvec, int64_t hwv,
                                     int Tn, int t_dst, int accumulate) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    const int64_t b = i / hwv, r = i - b * hwv;
    float f[8];
    Vec8<T>::load(src + i * 8, f);
    T* p = dst + ((b * Tn + t_dst) * hwv + r) * 8;
    if (accumulate) {
      float o[8];
      Vec8<T>::load(p, o);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] += o[j];
    }
    Vec8<T>::store(p, f);
  }
}

inline int ew_grid(int64_t nvec, int block) {
  int64_t g = (nvec + block - 1) / block;
  if (g > 256 * 16) g = 256 * 16;
  if (g < 1) g = 1;
  return (int)g;
}

// block_out_bwd_kernel's grid, whichever operand policy: the walk, and with it every thread's sum, is the same.
// Every workgroup ends with an LDS reduction and G*24 same-address f64 atomics: measured on MI355X
// 128/256/384/512/1024/2048 workgroups -> 2.55/1.70/1.59/1.68/2.22/3.07 ms per step
inline int bob_grid(int64_t nvec, int blk) {
  static const int env_cap = c3d_env("C3D_BOB_GRID") ? atoi(c3d_env("C3D_BOB_GRID")) : 0;   // tuning knob
  const int cap = env_cap > 0 ? env_cap : 384;
  const int grid = ew_grid(nvec, blk);
  return grid > cap ? cap : grid;
}

// launch(T{}, stream) with T = float / bf16_t as `dtype` says; the entry point's return value
template <class Launch>
int ew_typed(int32_t dtype, void* stream, Launch&& launch) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == C3D_DT_F32) launch(float{}, s);
  else if (dtype == C3D_DT_BF16) launch(bf16_t{}, s);
  else return C3D_E_BADARG;
  C3D_CHECK_LAUNCH();
  return 0;
}

// [B][T][HW][Cp] frames as 8-channel vectors: G per pixel, hwv per frame, nvec in one frame of every sample
struct FrameGeom {
  int32_t B, T, Cp;
  int64_t HW;
  int G;
  int64_t hwv, nvec;
  FrameGeom(int32_t B_, int32_t T_, int64_t HW_, int32_t Cp_)
      : B(B_), T(T_), Cp(Cp_), HW(HW_), G(Cp_ / 8), hwv(HW_ * (Cp_ / 8)), nvec((int64_t)B_ * HW_ * (Cp_ / 8)) {}
  int64_t nvec_all() const { return nvec * T; }
  bool ok() const { return B > 0 && T > 0 && HW > 0 && !(Cp & 7); }
  bool ok_fixed_vector() const { return ok() && Cp > 0 && Cp <= 256; }   // for kernels whose threads keep a channel vector
  bool has(int32_t t) const { return t >= 0 && t < T; }
};

}  // namespace

namespace {
int block_out_fwd_launch(const void* c, const float* ss_c, const void* shortcut, const float* ss_1, int32_t sc_mode,
                         void* y, int64_t M, int32_t C, int32_t Cp, int32_t dtype, void* stream, const c3d_bn_fin* fin_c,
                         const c3d_bn_fin* fin_1) {
  const int G = Cp / 8, blk = ew_block(G);
  const int64_t nvec = M * G;
  c3d_bn_fin f0;
  std::memset(&f0, 0, sizeof(f0));
  const c3d_bn_fin fc = fin_c ? *fin_c : f0, f1 = fin_1 ? *fin_1 : f0;
  // grid stride must stay a multiple of G: blk is, so any grid works.  With the finalisation folded in every
  // workgroup starts with a ~1.5 us dependent prologue: ONE round of workgroups (4 per CU), each walking the rows.
  int grid = ew_grid(nvec, blk);
  static const int env_grid = c3d_env("C3D_BOF_GRID") ? atoi(c3d_env("C3D_BOF_GRID")) : 0;   // tuning knob
  if (fin_c && grid > (env_grid > 0 ? env_grid : 1024)) grid = env_grid > 0 ? env_grid : 1024;
  return ew_typed(dtype, stream, [&](auto t, hipStream_t s) {
    typedef decltype(t) E;
    c3d_note_launch(reinterpret_cast<const void*>(&block_out_fwd_kernel<E>));
    block_out_fwd_kernel<E><<<grid, blk, 0, s>>>((const E*)c, ss_c, (const E*)shortcut, ss_1, sc_mode, (E*)y, nvec, G, C, fc,
                                                  f1);
  });
}

// one block_out_bwd_kernel<Ops> launch over `nvec` vectors, G per row
template <class Ops, class... Extra>
void block_out_bwd_launch(const void* dy, const void* y, const void* c, const void* s, void* g, const float* mr_c,
                          const float* mr_1, double* dsums_c, double* dsums_1, int64_t nvec, int G, int32_t C,
                          const c3d_bn_fin& fin_c, const c3d_bn_fin& fin_1, hipStream_t stream, const Extra&... extra) {
  typedef typename Ops::elem_t E;
  const int blk = ew_block(G);
  const size_t lds = (size_t)blk * 24 * sizeof(float);
  c3d_note_launch(reinterpret_cast<const void*>(&block_out_bwd_kernel<Ops, Extra...>));
  block_out_bwd_kernel<Ops, Extra...><<<bob_grid(nvec, blk), blk, lds, stream>>>(
      (const E*)dy, (const E*)y, (const E*)c, (const E*)s, (E*)g, mr_c, mr_1, dsums_c, dsums_1, nvec, G, C, fin_c, fin_1, extra...);
}
}  // namespace

extern "C" int c3d_block_out_fwd(const void* c, const float* ss_c, const void* shortcut, const float* ss_1,
                                 int32_t sc_mode, void* y, int64_t M, int32_t Cp, int32_t dtype, void* stream) {
  if (!c || !ss_c || !y || M <= 0 || (Cp & 7) || Cp > 256) return C3D_E_BADARG;
  if (sc_mode != SC_NONE && !shortcut) return C3D_E_BADARG;
  if (sc_mode == SC_BN && !ss_1) return C3D_E_BADARG;
  return block_out_fwd_launch(c, ss_c, shortcut, ss_1, sc_mode, y, M, Cp, Cp, dtype, stream, nullptr, nullptr);
}

extern "C" int c3d_block_out_fwd_fin(const void* c, const c3d_bn_fin* fin_c, const void* shortcut,
                                     const c3d_bn_fin* fin_1, int32_t sc_mode, void* y, int64_t M, int32_t C,
                                     int32_t Cp, int32_t dtype, void* stream) {
  if (!c || !fin_c || !fin_c->sums || !fin_c->ss || !fin_c->training || !y || M <= 0 || (Cp & 7) || Cp > 256 || C > Cp)
    return C3D_E_BADARG;
  if (sc_mode != SC_NONE && !shortcut) return C3D_E_BADARG;
  if (sc_mode == SC_BN && (!fin_1 || !fin_1->sums || !fin_1->ss)) return C3D_E_BADARG;
  return block_out_fwd_launch(c, fin_c->ss, shortcut, fin_1 ? fin_1->ss : nullptr, sc_mode, y, M, C, Cp, dtype, stream,
                              fin_c, sc_mode == SC_BN ? fin_1 : nullptr);
}

extern "C" int c3d_block_out_bwd(const void* dy, const void* y, const void* c, const void* s_bn, void* g,
                                 const float* mr_c, const float* mr_1, double* dsums_c, double* dsums_1, int64_t M,
                                 int32_t C, int32_t Cp, int32_t dtype, void* stream) {
  return c3d_block_out_bwd_fin(dy, y, c, s_bn, g, mr_c, mr_1, dsums_c, dsums_1, M, C, Cp, dtype, nullptr, nullptr, stream);
}

extern "C" int c3d_block_out_bwd_fin(const void* dy, const void* y, const void* c, const void* s_bn, void* g,
                                     const float* mr_c, const float* mr_1, double* dsums_c, double* dsums_1, int64_t M,
                                     int32_t C, int32_t Cp, int32_t dtype, const c3d_bn_fin* fc, const c3d_bn_fin* f1,
                                     void* stream) {
  if (!dy || !c || !mr_c || !dsums_c || M <= 0 || (Cp & 7) || Cp > 256) return C3D_E_BADARG;
  if (((uintptr_t)mr_c & 15) || (s_bn && ((uintptr_t)mr_1 & 15))) return C3D_E_BADARG;   // mean | rstd rows are read as 16-byte vectors
  if ((y == nullptr) != (g == nullptr)) return C3D_E_BADARG;   // both NULL: dy is already masked, only the sums are produced
  if ((s_bn == nullptr) != (dsums_1 == nullptr) || (s_bn && !mr_1)) return C3D_E_BADARG;
  if (fc && fc->ticket && (!fc->gamma || !fc->ss || !fc->mr || !(fc->count > 0))) return C3D_E_BADARG;
  if (fc && fc->ticket && s_bn && (!f1 || !f1->gamma || !f1->ss || !f1->mr || !(f1->count > 0))) return C3D_E_BADARG;
  const c3d_bn_fin fin_c = fc ? *fc : c3d_bn_fin{};
  const c3d_bn_fin fin_1 = (f1 && s_bn) ? *f1 : c3d_bn_fin{};
  const int G = Cp / 8;
  return ew_typed(dtype, stream, [&](auto t, hipStream_t s) {
    typedef decltype(t) E;
    auto go = [&](auto ops) {
      block_out_bwd_launch<decltype(ops)>(dy, y, c, s_bn, g, mr_c, mr_1, dsums_c, dsums_1, M * G, G, C, fin_c, fin_1, s);
    };
    if (y) go(StoredOperands<E, false>{});
    else go(StoredOperands<E, true>{});
  });
}

extern "C" int c3d_frame_absdiff(const void* y, void* d, int32_t B, int32_t T, int64_t HW, int32_t Cp,
                                 int32_t t_pre, int32_t t_post, int32_t dtype, void* stream) {
  const FrameGeom fg(B, T, HW, Cp);
  if (!y || !d || !fg.ok() || !fg.has(t_pre) || !fg.has(t_post)) return C3D_E_BADARG;
  return ew_typed(dtype, stream, [&](auto t, hipStream_t s) {
    typedef decltype(t) E;
    c3d_note_launch(reinterpret_cast<const void*>(&frame_absdiff_kernel<E>));
    frame_absdiff_kernel<E><<<ew_grid(fg.nvec, 256), 256, 0, s>>>((const E*)y, (E*)d, fg.nvec, fg.hwv, T, t_pre, t_post);
  });
}

extern "C" int c3d_enhance_apply(const void* y, const void* e, void* out, int32_t B, int32_t T, int64_t HW,
                                 int32_t Cp, int32_t t_mid, int32_t dtype, void* stream) {
  const FrameGeom fg(B, T, HW, Cp);
  if (!y || !e || !out || !fg.ok() || !fg.has(t_mid)) return C3D_E_BADARG;
  const int64_t nvec = fg.nvec_all();
  return ew_typed(dtype, stream, [&](auto t, hipStream_t s) {
    typedef decltype(t) E;
    c3d_note_launch(reinterpret_cast<const void*>(&enhance_apply_kernel<E>));
    enhance_apply_kernel<E><<<ew_grid(nvec, 256), 256, 0, s>>>((const E*)y, (const E*)e, (E*)out, nvec, fg.hwv, T, t_mid);
  });
}

extern "C" int c3d_enhance_bwd_mask(const void* dout, const void* e, void* de, int32_t B, int32_t T, int64_t HW,
                                    int32_t Cp, int32_t t_mid, int32_t dtype, void* stream) {
  const FrameGeom fg(B, T, HW, Cp);
  if (!dout || !e || !de || !fg.ok() || !fg.has(t_mid)) return C3D_E_BADARG;
  return ew_typed(dtype, stream, [&](auto t, hipStream_t s) {
    typedef decltype(t) E;
    c3d_note_launch(reinterpret_cast<const void*>(&enhance_bwd_mask_kernel<E>));
    enhance_bwd_mask_kernel<E><<<ew_grid(fg.nvec, 256), 256, 0, s>>>((const E*)dout, (const E*)e, (E*)de, fg.nvec, fg.hwv, T,
                                                                      t_mid);
  });
}

extern "C" int c3d_enhance_bwd_apply(const void* dout, const void* y, const void* dd, void* dy, int32_t B,
                                     int32_t T, int64_t HW, int32_t Cp, int32_t t_pre, int32_t t_post,
                                     int32_t dtype, void* stream) {
  const FrameGeom fg(B, T, HW, Cp);
  // t_pre / t_post outside [0, T) match no frame (the kernel reads y only on a matching frame): dy = dout then
  if (!dout || !y || !dd || !dy || !fg.ok()) return C3D_E_BADARG;
  // ... but BOTH: on a matching frame the kernel reads y on t_pre AND t_post, so one index in range with the other outside
  // would read outside y
  if (fg.has(t_pre) != fg.has(t_post)) return C3D_E_BADARG;
  const int64_t nvec = fg.nvec_all();
  return ew_typed(dtype, stream, [&](auto t, hipStream_t s) {
    typedef decltype(t) E;
    c3d_note_launch(reinterpret_cast<const void*>(&enhance_bwd_apply_kernel<E>));
    enhance_bwd_apply_kernel<E><<<ew_grid(nvec, 256), 256, 0, s>>>((const E*)dout, (const E*)y, (const E*)dd, (E*)dy, nvec,
                                                                    fg.hwv, T, t_pre, t_post);
  });
}

// ---- stem output + enhance (no materialised y / dy): see the kernels above --------------------------------------
extern "C" int c3d_stem_enhance_fwd(const void* u, const float* ss, void* out, void* d, int32_t B, int32_t T, int64_t HW,
                                    int32_t Cp, int32_t t_pre, int32_t t_post, int32_t t_mid, int32_t dtype, void* stream) {
  const FrameGeom fg(B, T, HW, Cp);
  if (!u || !ss || !out || !d || !fg.ok_fixed_vector() || T < 3 || !fg.has(t_pre) || !fg.has(t_post) || !fg.has(t_mid) ||
      t_pre == t_post || t_mid == t_pre || t_mid == t_post)
    return C3D_E_BADARG;
  if ((uintptr_t)ss & 15) return C3D_E_BADARG;   // scale | shift rows are read as 16-byte vectors
  const int blk = ew_block(fg.G);
  return ew_typed(dtype, stream, [&](auto t, hipStream_t s) {
    typedef decltype(t) E;
    c3d_note_launch(reinterpret_cast<const void*>(&stem_enhance_fwd_kernel<E>));
    stem_enhance_fwd_kernel<E><<<ew_grid(fg.nvec, blk), blk, 0, s>>>((const E*)u, ss, (E*)out, (E*)d, fg.nvec, fg.hwv, fg.G, T,
                                                                      t_pre, t_post, t_mid);
  });
}

extern "C" int c3d_stem_enhance_mid(const void* u, const float* ss, const void* e, void* out, int32_t B, int32_t T,
                                    int64_t HW, int32_t Cp, int32_t t_mid, int32_t dtype, void* stream) {
  const FrameGeom fg(B, T, HW, Cp);
  if (!u || !ss || !e || !out || !fg.ok_fixed_vector() || !fg.has(t_mid)) return C3D_E_BADARG;
  if ((uintptr_t)ss & 15) return C3D_E_BADARG;
  const int blk = ew_block(fg.G);
  return ew_typed(dtype, stream, [&](auto t, hipStream_t s) {
    typedef decltype(t) E;
    c3d_note_launch(reinterpret_cast<const void*>(&stem_enhance_mid_kernel<E>));
    stem_enhance_mid_kernel<E><<<ew_grid(fg.nvec, blk), blk, 0, s>>>((const E*)u, ss, (const E*)e, (E*)out, fg.nvec, fg.hwv,
                                                                      fg.G, T, t_mid);
  });
}

extern "C" int c3d_stem_enhance_bwd(const void* dout, const void* u, const float* ss, const void* dd, const float* mr,
                                    void* g, double* dsums, int32_t B, int32_t T, int64_t HW, int32_t C, int32_t Cp,
                                    int32_t t_pre, int32_t t_post, int32_t dtype, void* stream) {
  const FrameGeom fg(B, T, HW, Cp);
  if (!dout || !u || !ss || !dd || !mr || !g || !dsums || C <= 0 || C > Cp) return C3D_E_BADARG;
  if (!fg.ok_fixed_vector() || T < 2 || !fg.has(t_pre) || !fg.has(t_post) || t_pre == t_post) return C3D_E_BADARG;
  if (((uintptr_t)ss & 15) || ((uintptr_t)mr & 15)) return C3D_E_BADARG;
  return ew_typed(dtype, stream, [&](auto t, hipStream_t s) {
    typedef decltype(t) E;
    typedef StemEnhanceOperands<E> Ops;   // dy = dout, c = u; no y, no shortcut, no ticket tail
    block_out_bwd_launch<Ops>(dout, nullptr, u, nullptr, g, mr, nullptr, dsums, nullptr, fg.nvec_all(), fg.G, C, c3d_bn_fin{},
                              c3d_bn_fin{}, s, typename Ops::Extra{ss, (const E*)dd, fg.hwv, T, t_pre, t_post});
  });
}

extern "C" int c3d_frame_scatter(const void* src, void* dst, int32_t B, int32_t T, int64_t HW, int32_t Cp,
                                 int32_t t_dst, int32_t accumulate, int32_t dtype, void* stream) {
  const FrameGeom fg(B, T, HW, Cp);
  if (!src || !dst || !fg.ok() || !fg.has(t_dst)) return C3D_E_BADARG;
  return ew_typed(dtype, stream, [&](auto t, hipStream_t s) {
    typedef decltype(t) E;
    c3d_note_launch(reinterpret_cast<const void*>(&frame_scatter_kernel<E>));
    frame_scatter_kernel<E><<<ew_grid(fg.nvec, 256), 256, 0, s>>>((const E*)src, (E*)dst, fg.nvec, fg.hwv, T, t_dst, accumulate);
  });
}
