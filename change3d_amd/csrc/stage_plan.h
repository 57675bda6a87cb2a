// Workspace plans of the residual-stage driver (stage_driver.hip): the geometry of every block, where each tensor of a
// stage pass lives in the caller's workspaces, and the typed per-block views the passes work on.  Host only, no launches.
// A plan is a pure function of the descriptor -- never of an option value: a c3d_set_option between c3d_stage_ws_bytes and
// c3d_stage_bwd must not move a region under the caller.
#pragma once
#include "../../include/change3d_hip.h"
#include "common.h"
#include "pw_common.h"
#include <algorithm>
#include <cstring>
#include <vector>

bool c3d_detail_pw_gemm_wg_supported(int Kp, int Np, int wg_mode);   // pw_gemm_wg.hip: the fused kernel's own LDS plan
bool c3d_detail_pw_gemm_masksum_supported(int Kp, int Np);           // pw_gemm_wg.hip: C3D_WG_MASKSUM

namespace {

inline int cpad(int c) { return (c + 7) / 8 * 8; }
inline size_t al(size_t v) { return (v + 255) / 256 * 256; }
inline size_t es(int dtype) { return dtype == C3D_DT_F32 ? 4 : 2; }
constexpr int S = C3D_STAT_STRIPES;

// c3d_stage_desc.flags (include/change3d_hip.h): the unfused launch sequences, kept callable so that the fused ones can
// be tested bit for bit against them (tests/test_model_gpu.py) -- the default (flags = 0) is the measured-best sequence
inline bool fin_consumer(const c3d_stage_desc* d) { return !(d->flags & C3D_STAGE_SEPARATE_FINALIZE); }
inline bool fuse_residual(const c3d_stage_desc* d) { return !(d->flags & C3D_STAGE_SEPARATE_RESIDUAL); }
inline bool use_pw_img(const c3d_stage_desc* d) { return !(d->flags & C3D_STAGE_NO_WEIGHT_IMAGES); }

struct BlkGeom {
  int H, W, Ho, Wo;
  int64_t M, Mo;   // rows in / out
  int Cin, Ci, Co, Cinp, Cip, Cop, s, Cr;
  bool se, sc_conv, sc_bn;
};

// A carved region: its offset and the bytes asked for (the carver advances by the 256-byte round-up of that).  A region the
// plan does not have keeps off == SIZE_MAX.
struct Region {
  size_t off = SIZE_MAX, bytes = 0;
};

struct Carver {
  size_t off = 0;
  size_t take(size_t bytes) { const size_t o = off; off += al(bytes); return o; }
  Region region(size_t bytes) { return {take(bytes), bytes}; }
};

struct BlkFwd {   // regions of ws_fwd: the size of each is written once, where make_plan carves it
  Region a, b, c, sc, y;                                        // activations (y: absent for the last block)
  Region ss_a, mr_a, ss_b, mr_b, gate, hid, ss_c, mr_c, ss_1, mr_1;   // f32 vectors
  Region sums_a, nc_b, sums_c, sums_1;                          // f64 accumulators
  Region tick;                                                  // u32 [4] last-workgroup tickets (a, c, shortcut)
  // pointwise weights as LDS images (c3d_pw_pack_weights): forward orientation and transposed (data gradient);
  // absent where the narrow GEMM kernel does not take the shape
  Region img_a, img_at, img_c, img_ct, img_s, img_st;
};

// Ring depth of the backward temporaries: block i shares its slot with block i+R, so the side stream (weight gradients)
// may run up to R-1 blocks behind the data-gradient chain before the main stream has to wait for it.
#ifndef C3D_BWD_RING_DEFAULT
#define C3D_BWD_RING_DEFAULT 3
#endif
constexpr int BWD_RING_MAX = 8;
inline int bwd_ring() {
  static const int r = [] {
    const char* s = c3d_env("C3D_BWD_RING");
    // measured on MI355X (B=32 bf16): 2, 3, 4 slots -> 34.04 / 34.10 / 34.32 ms per step before the weight gradients were
    // forked ahead of their data gradients; 32.62 / 32.45 ms for 2 / 3 slots after (three interleaved repeats each)
    const int v = s ? atoi(s) : C3D_BWD_RING_DEFAULT;
    return v < 2 ? 2 : (v > BWD_RING_MAX ? BWD_RING_MAX : v);
  }();
  return r;
}

struct BlkBwd {   // byte offsets into ws_bwd (ring slot for the big tensors)
  size_t g, t1, t2, dxs, dx;
  size_t coef_c, coef_1, coef_a, cA, cC, cB;                   // f32 vectors
  size_t dsums_c, dsums_1, nc3, dsums_a;                        // f64 accumulators
  size_t tick;                                                  // u32 [4] last-workgroup tickets (c (+shortcut), a)
};

struct Plan {
  std::vector<BlkGeom> g;
  std::vector<BlkFwd> f;
  std::vector<BlkBwd> b;
  size_t fwd_acc_off = 0, fwd_acc_bytes = 0, fwd_total = 0;
  size_t bwd_acc_off = 0, bwd_acc_bytes = 0, bwd_total = 0, wgrad_ws = 0, wgrad_ws2 = 0, wgrad_ws_fused = 0, wgrad_ws_fused_slot = 0;
  size_t y_bytes = 0, dx_bytes = 0;
};

// pointwise weight gradient inside the data-gradient launch (c3d_pw_args.wg_mode; csrc/pw_gemm_impl.h): bf16 layers whose
// accumulator image fits in LDS beside the tiles -- the res2 / res3 shapes (K, N <= 112 padded)
inline bool fuse_wgrad(const c3d_stage_desc* d, int Kp, int Np, int wg_mode) {
  return !(d->flags & C3D_STAGE_SEPARATE_WGRAD) && d->dtype == C3D_DT_BF16 && Kp <= 112 && Np <= 112 && c3d_knob("C3D_PW_WG", 1) &&
         c3d_detail_pw_gemm_wg_supported(Kp, Np, wg_mode);
}

inline int make_plan(const c3d_stage_desc* d, Plan& P) {
  if (!d || d->n_blocks <= 0 || !d->blocks || d->B <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0) return C3D_E_BADARG;
  if (d->dtype != C3D_DT_F32 && d->dtype != C3D_DT_BF16) return C3D_E_BADARG;
  const size_t e = es(d->dtype);
  const int n = d->n_blocks;
  P.g.resize(n); P.f.resize(n); P.b.resize(n);
  int H = d->H, W = d->W;
  for (int i = 0; i < n; ++i) {
    const c3d_block_desc& k = d->blocks[i];
    if (k.cin <= 0 || k.cinner <= 0 || k.cout <= 0 || (k.stride != 1 && k.stride != 2)) return C3D_E_BADARG;
    if (i > 0 && k.cin != d->blocks[i - 1].cout) return C3D_E_BADARG;
    if (!k.has_sc_conv && (k.cin != k.cout || k.stride != 1)) return C3D_E_BADARG;
    if (k.has_sc_bn && !k.has_sc_conv) return C3D_E_BADARG;
    BlkGeom& G = P.g[i];
    G.H = H; G.W = W; G.s = k.stride;
    G.Ho = (H - 1) / k.stride + 1; G.Wo = (W - 1) / k.stride + 1;
    G.M = (int64_t)d->B * d->T * H * W; G.Mo = (int64_t)d->B * d->T * G.Ho * G.Wo;
    G.Cin = k.cin; G.Ci = k.cinner; G.Co = k.cout;
    G.Cinp = cpad(k.cin); G.Cip = cpad(k.cinner); G.Cop = cpad(k.cout);
    G.se = k.se_width > 0; G.Cr = k.se_width; G.sc_conv = k.has_sc_conv != 0; G.sc_bn = k.has_sc_bn != 0;
    // A tensor the narrow pointwise kernels (channel counts up to 224) cannot address (pw_fits_u32) would be refused by the
    // first launch that meets it, in the MIDDLE of a stage pass.  Refuse the stage here instead -- c3d_stage_ws_bytes is the
    // caller's first contact with a geometry.
    // (bf16, 256 x 256, T = 3: B <= 96 per GPU; f32: half of that.  The wide (res5) kernels have no such limit.)
    {
      const int cmax = std::max(std::max(G.Cinp, G.Cip), G.Cop);
      if (cmax <= 224 && !pw_fits_u32(std::max(G.M, G.Mo), cmax, cmax, (int)e)) return C3D_E_UNSUPPORTED;
    }
    H = G.Ho; W = G.Wo;
  }
  // ---- forward workspace: activations, then f32 vectors, then ONE contiguous f64 accumulator region
  Carver cf;
  for (int i = 0; i < n; ++i) {
    const BlkGeom& G = P.g[i];
    BlkFwd& F = P.f[i];
    F.a = cf.region((size_t)G.M * G.Cip * e);
    F.b = cf.region((size_t)G.Mo * G.Cip * e);
    F.c = cf.region((size_t)G.Mo * G.Cop * e);
    if (G.sc_conv) F.sc = cf.region((size_t)G.Mo * G.Cop * e);
    if (i + 1 < n) F.y = cf.region((size_t)G.Mo * G.Cop * e);
  }
  for (int i = 0; i < n; ++i) {
    const BlkGeom& G = P.g[i];
    BlkFwd& F = P.f[i];
    F.ss_a = cf.region(2 * G.Cip * 4); F.mr_a = cf.region(2 * G.Cip * 4);
    F.ss_b = cf.region(2 * G.Cip * 4); F.mr_b = cf.region(2 * G.Cip * 4);
    if (G.se) { F.gate = cf.region((size_t)d->B * G.Cip * 4); F.hid = cf.region((size_t)d->B * G.Cr * 4); }
    F.ss_c = cf.region(2 * G.Cop * 4); F.mr_c = cf.region(2 * G.Cop * 4);
    if (G.sc_bn) { F.ss_1 = cf.region(2 * G.Cop * 4); F.mr_1 = cf.region(2 * G.Cop * 4); }
  }
  P.fwd_acc_off = cf.off;
  for (int i = 0; i < n; ++i) {
    const BlkGeom& G = P.g[i];
    BlkFwd& F = P.f[i];
    F.sums_a = cf.region((size_t)S * 2 * G.Ci * 8);
    F.nc_b = cf.region((size_t)d->B * G.Cip * 2 * 8);
    F.sums_c = cf.region((size_t)S * 2 * G.Co * 8);
    if (G.sc_bn) F.sums_1 = cf.region((size_t)S * 2 * G.Co * 8);
    F.tick = cf.region(16);
  }
  P.fwd_acc_bytes = cf.off - P.fwd_acc_off;
  for (int i = 0; i < n; ++i) {
    const BlkGeom& G = P.g[i];
    BlkFwd& F = P.f[i];
    auto img = [&](int Np, int Kp) -> Region {
      const int64_t b = c3d_pw_weight_image_bytes(Np, Kp, d->dtype);
      return b > 0 ? cf.region((size_t)b) : Region{};
    };
    F.img_a = img(G.Cip, G.Cinp); F.img_at = img(G.Cinp, G.Cip);
    F.img_c = img(G.Cop, G.Cip); F.img_ct = img(G.Cip, G.Cop);
    if (G.sc_conv) { F.img_s = img(G.Cop, G.Cinp); F.img_st = img(G.Cinp, G.Cop); }
  }
  P.fwd_total = cf.off;
  // ---- backward workspace: bwd_ring() ring slots of big temporaries (the side stream may lag the data-gradient chain
  //      by ring-1 blocks), per-block f32 coefficient vectors, one f64 accumulator region, the split-K scratch of
  //      the pointwise weight gradient
  size_t mx_g = 0, mx_t1 = 0, mx_t2 = 0, mx_dxs = 0, mx_dx = 0;
  int64_t wsf = 0, wsf_fused = 0;
  for (int i = 0; i < n; ++i) {
    const BlkGeom& G = P.g[i];
    if (fuse_wgrad(d, G.Cop, G.Cip, C3D_WG_SWISH)) wsf_fused = std::max(wsf_fused, c3d_pw_gemm_wg_ws_floats(G.Co, G.Ci));
    if (fuse_wgrad(d, G.Cip, G.Cinp, C3D_WG_ROWS)) wsf_fused = std::max(wsf_fused, c3d_pw_gemm_wg_ws_floats(G.Ci, G.Cin));
    // (the cooperative conv_a data + weight gradient, csrc/pw_cdgrad.hip: reserved whatever C3D_OPT_PW_CDG says right now)
    if (d->dtype == C3D_DT_BF16 && c3d_detail_pw_cdg_a_shape(G.Cip, G.Cinp, G.M)) wsf_fused = std::max(wsf_fused, c3d_pw_gemm_wg_ws_floats(G.Ci, G.Cin));
    if (d->dtype == C3D_DT_BF16 && c3d_detail_pw_cdg_c_shape(G.Cop, G.Cip, G.Mo, (int64_t)d->T * G.Ho * G.Wo))
      wsf_fused = std::max(wsf_fused, c3d_pw_gemm_wg_ws_floats(G.Co, G.Ci));
    mx_g = std::max(mx_g, (size_t)G.Mo * G.Cop * e);
    mx_t1 = std::max(mx_t1, (size_t)G.Mo * G.Cip * e);
    mx_t2 = std::max(mx_t2, (size_t)G.M * G.Cip * e);
    if (G.sc_conv) mx_dxs = std::max(mx_dxs, (size_t)G.Mo * G.Cinp * e);
    if (i > 0) mx_dx = std::max(mx_dx, (size_t)G.M * G.Cinp * e);
    wsf = std::max(wsf, c3d_pw_wgrad_ws_floats(G.Co, G.Ci));
    wsf = std::max(wsf, c3d_pw_wgrad_ws_floats(G.Ci, G.Cin));
    wsf = std::max(wsf, c3d_pw_wgrad_ws_floats(G.Co, G.Cin));
  }
  Carver cb;
  const int R = bwd_ring();
  size_t ring[BWD_RING_MAX][4];
  for (int r = 0; r < R; ++r) {
    ring[r][0] = cb.take(mx_g); ring[r][1] = cb.take(mx_t1); ring[r][2] = cb.take(mx_t2);
    ring[r][3] = mx_dxs ? cb.take(mx_dxs) : SIZE_MAX;
  }
  // dx of block i is dy of block i - 1 -- and, when the conv_a data gradient masked it (c3d_pw_args.wg_mask_out /
  // C3D_WG_MASKSUM), that block's g as well, which its SIDE-stream weight gradients read: one slot more than the ring, so that
  // block i - R - 1 overwrites it after the side marks of blocks >= i - 1 are joined (c3d_stage_bwd's lag rule)
  size_t ring_dx[BWD_RING_MAX + 1];
  for (int r = 0; r < R + 1; ++r) ring_dx[r] = mx_dx ? cb.take(mx_dx) : SIZE_MAX;
  P.wgrad_ws = cb.take((size_t)wsf * 4);
  P.wgrad_ws2 = cb.take((size_t)wsf * 4);   // chained weight-gradient launches alternate between the two (c3d_pw_wgrad_args.chain)
  // slot 0: the wave-private kernel's fused variant (kernel, then its reducer, on the main stream); slots 1..2n: one per
  // cooperative data + weight gradient launch of a backward pass -- their partials are reduced behind ONE fork at the end of
  // the pass (c3d_stage_bwd), not launch by launch
  P.wgrad_ws_fused = wsf_fused ? cb.take((size_t)wsf_fused * 4 * (1 + 2 * (size_t)n)) : SIZE_MAX;
  P.wgrad_ws_fused_slot = (size_t)wsf_fused * 4;
  for (int i = 0; i < n; ++i) {
    const BlkGeom& G = P.g[i];
    BlkBwd& Bk = P.b[i];
    const int r = i % R;
    Bk.g = ring[r][0]; Bk.t1 = ring[r][1]; Bk.t2 = ring[r][2]; Bk.dxs = ring[r][3];
    Bk.dx = i > 0 ? ring_dx[i % (R + 1)] : SIZE_MAX;
    Bk.coef_c = cb.take(3 * G.Cop * 4);
    Bk.coef_1 = G.sc_bn ? cb.take(3 * G.Cop * 4) : SIZE_MAX;
    Bk.coef_a = cb.take(3 * G.Cip * 4);
    Bk.cA = cb.take(G.Cip * 4); Bk.cC = cb.take(G.Cip * 4); Bk.cB = cb.take((size_t)d->B * G.Cip * 4);
  }
  P.bwd_acc_off = cb.off;
  for (int i = 0; i < n; ++i) {
    const BlkGeom& G = P.g[i];
    BlkBwd& Bk = P.b[i];
    Bk.dsums_c = cb.take(2 * G.Co * 8);
    Bk.dsums_1 = G.sc_bn ? cb.take(2 * G.Co * 8) : SIZE_MAX;
    Bk.nc3 = cb.take((size_t)d->B * G.Cip * 3 * 8);
    Bk.dsums_a = cb.take(2 * G.Ci * 8);
    Bk.tick = cb.take(16);
  }
  P.bwd_acc_bytes = cb.off - P.bwd_acc_off;
  P.bwd_total = cb.off;
  P.y_bytes = (size_t)P.g[n - 1].Mo * P.g[n - 1].Cop * e;
  P.dx_bytes = (size_t)P.g[0].M * P.g[0].Cinp * e;
  return 0;
}

// ---- eval: folded BatchNorm (stage_driver.hip, "eval" section)
struct BlkFold { size_t w_a, w_b, w_c, w_sc, ss_a, ss_b, ss_c, ss_1; };
struct BlkEval { size_t a, b, c, sc, y, gate, hid, nc_b; };
struct FoldPlan {
  std::vector<BlkFold> f;
  std::vector<BlkEval> e;
  size_t fold_total = 0, ws_total = 0, acc_off = 0, acc_bytes = 0;
};

inline int make_fold_plan(const c3d_stage_desc* d, const Plan& P, FoldPlan& Q) {
  const int n = d->n_blocks;
  Q.f.resize(n); Q.e.resize(n);
  // A geometry the eval launches cannot take is refused here, at the caller's first contact with it (c3d_stage_fold_bytes), not
  // by a launch in the middle of the pass: the narrow pointwise kernel (channel counts up to 224) takes one SE gate per 16-row
  // sub-tile, so conv_c of an SE block needs T * Ho * Wo to be a multiple of 16 (c3d_pw_gemm answers C3D_E_BADARG otherwise,
  // after conv_a and conv_b ran)
  for (int i = 0; i < n; ++i) {
    const BlkGeom& G = P.g[i];
    if (G.se && G.Cip <= 224 && G.Cop <= 224 && (((int64_t)d->T * G.Ho * G.Wo) & 15)) return C3D_E_UNSUPPORTED;
  }
  Carver cf;
  for (int i = 0; i < n; ++i) {
    const BlkGeom& G = P.g[i];
    BlkFold& F = Q.f[i];
    F.w_a = cf.take((size_t)G.Ci * G.Cin * 4); F.w_b = cf.take((size_t)G.Ci * 27 * 4);
    F.w_c = cf.take((size_t)G.Co * G.Ci * 4);
    F.w_sc = G.sc_conv ? cf.take((size_t)G.Co * G.Cin * 4) : SIZE_MAX;
    F.ss_a = cf.take(2 * G.Cip * 4); F.ss_b = cf.take(2 * G.Cip * 4); F.ss_c = cf.take(2 * G.Cop * 4);
    F.ss_1 = G.sc_bn ? cf.take(2 * G.Cop * 4) : SIZE_MAX;
  }
  Q.fold_total = cf.off;
  // one set of activations for all blocks: the largest a, b, c (y has c's size) and per-sample sums of the training plan;
  // gate / hid are sized for every block, with or without SE
  size_t mx_a = 0, mx_b = 0, mx_c = 0, mx_gate = 0, mx_hid = 0;
  for (int i = 0; i < n; ++i) {
    const BlkGeom& G = P.g[i];
    const BlkFwd& F = P.f[i];
    mx_a = std::max(mx_a, F.a.bytes); mx_b = std::max(mx_b, F.b.bytes); mx_c = std::max(mx_c, F.c.bytes);
    mx_gate = std::max(mx_gate, (size_t)d->B * G.Cip * 4); mx_hid = std::max(mx_hid, (size_t)d->B * std::max(G.Cr, 1) * 4);
  }
  Carver cw;
  const size_t a = cw.take(mx_a), b = cw.take(mx_b), c = cw.take(mx_c), sc = cw.take(mx_c);
  const size_t y0 = cw.take(mx_c), y1 = cw.take(mx_c), gate = cw.take(mx_gate), hid = cw.take(mx_hid);
  Q.acc_off = cw.off;
  for (int i = 0; i < n; ++i) {
    BlkEval& E = Q.e[i];
    E.a = a; E.b = b; E.c = c; E.sc = sc; E.y = (i & 1) ? y1 : y0; E.gate = gate; E.hid = hid;
    E.nc_b = P.g[i].se ? cw.take(P.f[i].nc_b.bytes) : SIZE_MAX;   // only SE blocks need the per-sample means
  }
  Q.acc_bytes = cw.off - Q.acc_off;
  Q.ws_total = cw.off;
  return 0;
}

// ------------------------------------------------------------------------------------------ per-block views
// Typed pointers of one block for one pass: null where the plan has no region.  The views own the two boundary rules:
// the LAST block writes the caller's y_out instead of a workspace region, and block 0 reads the caller's x and writes the
// caller's dx_out.
inline char* at(void* base, size_t off) { return off == SIZE_MAX ? nullptr : reinterpret_cast<char*>(base) + off; }
template <typename T> inline T* atT(void* base, size_t off) { return reinterpret_cast<T*>(at(base, off)); }

struct BlkFwdView {
  void *a, *b, *c, *sc, *y;
  float *ss_a, *mr_a, *ss_b, *mr_b, *ss_c, *mr_c, *ss_1, *mr_1, *gate, *hid;
  double *sums_a, *nc_b, *sums_c, *sums_1;
  const void *img_a, *img_c, *img_s;   // null under C3D_STAGE_NO_WEIGHT_IMAGES too
};

inline BlkFwdView view(const c3d_stage_desc* d, void* ws, void* y_out, const Plan& P, int i) {
  const BlkFwd& F = P.f[i];
  const bool wimg = use_pw_img(d);
  auto f = [&](const Region& r) { return atT<float>(ws, r.off); };
  auto f64 = [&](const Region& r) { return atT<double>(ws, r.off); };
  BlkFwdView V;
  V.a = at(ws, F.a.off); V.b = at(ws, F.b.off); V.c = at(ws, F.c.off); V.sc = at(ws, F.sc.off);
  V.y = i + 1 == d->n_blocks ? y_out : at(ws, F.y.off);
  V.ss_a = f(F.ss_a); V.mr_a = f(F.mr_a); V.ss_b = f(F.ss_b); V.mr_b = f(F.mr_b); V.ss_c = f(F.ss_c); V.mr_c = f(F.mr_c);
  V.ss_1 = f(F.ss_1); V.mr_1 = f(F.mr_1); V.gate = f(F.gate); V.hid = f(F.hid);
  V.sums_a = f64(F.sums_a); V.nc_b = f64(F.nc_b); V.sums_c = f64(F.sums_c); V.sums_1 = f64(F.sums_1);
  V.img_a = wimg ? at(ws, F.img_a.off) : nullptr; V.img_c = wimg ? at(ws, F.img_c.off) : nullptr;
  V.img_s = wimg ? at(ws, F.img_s.off) : nullptr;
  return V;
}

struct BlkBwdView {
  // what the forward pass left (ws_fwd, and the caller's x / y_out at the two ends of the stage)
  const void *xin, *a, *b, *c, *sc, *y;
  const float *ss_a, *mr_a, *ss_b, *mr_b, *mr_c, *mr_1, *gate, *hid;
  const double* nc_b;
  const void *img_at, *img_ct, *img_st;   // transposed weight images written by this step's c3d_stage_fwd (training mode)
  // of the block BELOW (i - 1; null for block 0), for the conv_a data gradient that takes over its c3d_block_out_bwd
  const void* below_c;
  const float* below_mr_c;
  double* below_dsums_c;
  // ws_bwd
  void *g, *t1, *t2, *dxs, *dx;
  float *coef_c, *coef_1, *coef_a, *cA, *cC, *cB;
  double *dsums_c, *dsums_1, *nc3, *dsums_a;
};

inline BlkBwdView view(const c3d_stage_desc* d, void* ws, void* wb, const void* x, const void* y_out, void* dx_out,
                       const Plan& P, int i) {
  const BlkFwd& F = P.f[i];
  const BlkBwd& Bk = P.b[i];
  const bool wimg = use_pw_img(d);
  auto y_of = [&](int j) -> const void* { return j + 1 == d->n_blocks ? y_out : at(ws, P.f[j].y.off); };
  auto f = [&](const Region& r) -> const float* { return atT<float>(ws, r.off); };
  BlkBwdView V;
  V.xin = i == 0 ? x : y_of(i - 1);
  V.a = at(ws, F.a.off); V.b = at(ws, F.b.off); V.c = at(ws, F.c.off); V.sc = at(ws, F.sc.off); V.y = y_of(i);
  V.ss_a = f(F.ss_a); V.mr_a = f(F.mr_a); V.ss_b = f(F.ss_b); V.mr_b = f(F.mr_b); V.mr_c = f(F.mr_c); V.mr_1 = f(F.mr_1);
  V.gate = f(F.gate); V.hid = f(F.hid);
  V.nc_b = atT<double>(ws, F.nc_b.off);
  V.img_at = wimg ? at(ws, F.img_at.off) : nullptr; V.img_ct = wimg ? at(ws, F.img_ct.off) : nullptr;
  V.img_st = wimg ? at(ws, F.img_st.off) : nullptr;
  V.below_c = i > 0 ? at(ws, P.f[i - 1].c.off) : nullptr;
  V.below_mr_c = i > 0 ? f(P.f[i - 1].mr_c) : nullptr;
  V.below_dsums_c = i > 0 ? atT<double>(wb, P.b[i - 1].dsums_c) : nullptr;
  V.g = at(wb, Bk.g); V.t1 = at(wb, Bk.t1); V.t2 = at(wb, Bk.t2); V.dxs = at(wb, Bk.dxs);
  V.dx = i == 0 ? dx_out : at(wb, Bk.dx);
  V.coef_c = atT<float>(wb, Bk.coef_c); V.coef_1 = atT<float>(wb, Bk.coef_1); V.coef_a = atT<float>(wb, Bk.coef_a);
  V.cA = atT<float>(wb, Bk.cA); V.cC = atT<float>(wb, Bk.cC); V.cB = atT<float>(wb, Bk.cB);
  V.dsums_c = atT<double>(wb, Bk.dsums_c); V.dsums_1 = atT<double>(wb, Bk.dsums_1);
  V.nc3 = atT<double>(wb, Bk.nc3); V.dsums_a = atT<double>(wb, Bk.dsums_a);
  return V;
}

struct BlkEvalView {
  void *a, *b, *c, *sc, *y;
  float *w_a, *w_b, *w_c, *w_sc, *ss_a, *ss_b, *ss_c, *ss_1;   // the folded weights and biases (c3d_stage_fold_bn)
  float *gate, *hid;                                            // gate: null for a block without SE
  double* nc_b;
};

inline BlkEvalView view(const c3d_stage_desc* d, void* fold, void* ws, void* y_out, const Plan& P, const FoldPlan& Q, int i) {
  const BlkFold& F = Q.f[i];
  const BlkEval& E = Q.e[i];
  BlkEvalView V;
  V.a = at(ws, E.a); V.b = at(ws, E.b); V.c = at(ws, E.c); V.sc = at(ws, E.sc);
  V.y = i + 1 == d->n_blocks ? y_out : at(ws, E.y);
  V.w_a = atT<float>(fold, F.w_a); V.w_b = atT<float>(fold, F.w_b); V.w_c = atT<float>(fold, F.w_c); V.w_sc = atT<float>(fold, F.w_sc);
  V.ss_a = atT<float>(fold, F.ss_a); V.ss_b = atT<float>(fold, F.ss_b); V.ss_c = atT<float>(fold, F.ss_c); V.ss_1 = atT<float>(fold, F.ss_1);
  V.gate = P.g[i].se ? atT<float>(ws, E.gate) : nullptr;
  V.hid = atT<float>(ws, E.hid);
  V.nc_b = atT<double>(ws, E.nc_b);
  return V;
}

}  // namespace
