// Residual-stage step driver (host code): enqueues every kernel of one X3D residual stage, forward or backward,
// from ONE C call (reference model/x3d.py:331-412 ResStage / ResBlock / BottleneckBlock, driven by
// `self.x3d.blocks[i](x)` at reference model/trainer.py:126-139).
//
// Why it exists: a B=32 BCD step is ~1000 kernel launches; issued one by one through Python + ctypes they cost
// 19-22 ms of host time per step (round-1 measurement), a floor the kernels had almost reached.  Here the
// per-block launch sequence runs in C++ (sub-microsecond argument marshalling), the activations of a whole stage
// live in ONE workspace carved by a deterministic plan (no allocator calls between kernels), the f64 statistics
// accumulators of the stage are zeroed by one memset, and the leaf gradients (weight gradients) go to an internal
// side stream forked / joined with events.
//
// Where things are: stage_plan.h -- the workspace plans and the per-block pointer views; stage_run.h -- the per-launch
// profiler and the side stream; this file -- which launches a block takes (the predicates below), one function per layer
// and pass, and the C entry points.
#include "../../include/change3d_hip.h"
#include <hip/hip_runtime.h>
#include "stage_plan.h"
#include "stage_run.h"

namespace {

enum { SC_NONE = 0, SC_IDENTITY = 1, SC_BN = 2, SC_RAW = 3 };

// ------------------------------------------------------------------------------------------ launch helpers
struct PwCall {
  c3d_pw_args a;
  PwCall(const void* x, const float* w, void* y, int64_t M, int K, int N, int w_sn, int w_sk, int dtype) {
    std::memset(&a, 0, sizeof(a));
    a.x = x; a.w = w; a.y = y; a.M = M; a.K = K; a.Kp = cpad(K); a.N = N; a.Np = cpad(N);
    a.w_sn = w_sn; a.w_sk = w_sk; a.dtype = dtype;
    a.pro_mode = C3D_PRO_NONE; a.epi_mode = C3D_EPI_STORE; a.row_mode = C3D_ROWS_DENSE;
  }
};

struct WgCall {
  c3d_pw_wgrad_args a;
  WgCall(const void* p, const void* q, float* dw, int64_t M, int K, int N, int dw_sn, int dw_sk, int dtype) {
    std::memset(&a, 0, sizeof(a));
    a.p = p; a.q = q; a.dw = dw; a.M = M; a.K = K; a.Kp = cpad(K); a.N = N; a.Np = cpad(N);
    a.dw_sn = dw_sn; a.dw_sk = dw_sk; a.dtype = dtype; a.q_mode = C3D_PRO_NONE; a.row_mode = C3D_ROWS_DENSE;
  }
};

// c3d_bn_fin (csrc/bn_fin.h): a consumer's prologue finishes the BatchNorm its producer accumulated sums for.
// Forward: the struct is what it says.
inline c3d_bn_fin fin_consume(const double* sums, const c3d_bn_ptrs& bn, double count, float momentum, float eps,
                              float* ss, float* mr) {
  c3d_bn_fin f;
  std::memset(&f, 0, sizeof(f));
  f.gamma = bn.gamma; f.beta = bn.beta; f.running_mean = bn.running_mean; f.running_var = bn.running_var;
  f.nbt = bn.num_batches_tracked; f.ss = ss; f.mr = mr; f.count = count; f.momentum = momentum; f.eps = eps;
  f.training = 1; f.sums = sums;
  return f;
}

// Backward consumer side: the AFFINE2 prologues of the data-gradient GEMM and of the weight-gradient kernel rebuild
// A|B|C from the single-stripe sums.  Two fields are OVERLOADED here, and only here: with `accumulate` (the data-gradient
// GEMM and the depthwise backward, never the weight gradient) running_mean := dgamma and running_var := dbeta, the
// parameter gradients the prologue adds to.  `batch` > 0: the sums are per sample (the depthwise backward's BatchNorm_b).
inline c3d_bn_fin fin_coef_consume(const double* dsums, const c3d_bn_ptrs& bn, double count, const float* mr,
                                   bool accumulate, int batch = 0) {
  c3d_bn_fin f;
  std::memset(&f, 0, sizeof(f));
  f.sums = dsums; f.batch = batch; f.gamma = bn.gamma; f.mr = const_cast<float*>(mr); f.count = count;
  if (accumulate) { f.running_mean = bn.dgamma; f.running_var = bn.dbeta; }
  return f;
}

// BatchNorm backward on operand load, y = A g + B + C x2: the coefficients come from `coef` (a c3d_bn_bwd_coef launch
// wrote them) or, `consb`, the kernel rebuilds them from the sums.  The data-gradient GEMM also accumulates dgamma / dbeta.
struct BnBwd { const void* x2; const float* coef; const double* dsums; const c3d_bn_ptrs& bn; double count; const float* mr; };
inline void bn_bwd_operand(c3d_pw_args& a, bool consb, const BnBwd& o) {
  a.x2 = o.x2; a.pro_mode = C3D_PRO_AFFINE2; a.pro_p = o.coef;
  if (consb) a.fin = fin_coef_consume(o.dsums, o.bn, o.count, o.mr, true);
}
inline void bn_bwd_operand(c3d_pw_wgrad_args& a, bool consb, const BnBwd& o) {
  a.p2 = o.x2; a.p_coef = o.coef;
  if (consb) a.p_fin = fin_coef_consume(o.dsums, o.bn, o.count, o.mr, false);
}

// Zero fill of the accumulator regions with an ordinary kernel launch: hipMemsetAsync goes through the runtime's blit path,
// and the kernel trace shows a ~32 us hole in the main queue in front of every one of them (7 per BCD step = 0.22 ms;
// tools/trace_step.sh).  The regions are carved in 256-byte units, 16-byte aligned.
__global__ __launch_bounds__(256) void zero_fill_kernel(uint4* __restrict__ p, size_t n16) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) p[i] = make_uint4(0, 0, 0, 0);
}
int zero_fill(void* p, size_t bytes, hipStream_t st) {
  if (!bytes) return 0;
  if (((uintptr_t)p & 15) || (bytes & 15)) { HIPRC(hipMemsetAsync(p, 0, bytes, st)); return 0; }
  const size_t n16 = bytes >> 4;
  size_t blocks = (n16 + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  zero_fill_kernel<<<dim3((unsigned)blocks), dim3(256), 0, st>>>(reinterpret_cast<uint4*>(p), n16);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// ------------------------------------------------------------------------------------------ which sequence a block takes
// Functions of (descriptor, geometry, options), one per decision of the two training passes.
// ---- forward
// BatchNorm finalised by the consumer's prologue (training mode; else a c3d_bn_finalize launch: eval mode, C3D_STAGE_SEPARATE_FINALIZE)
inline bool fwd_cons(const c3d_stage_desc* d) { return d->training && fin_consumer(d); }
// BatchNorm_b (+ the SqueezeExcitation gate).  Blocks WITHOUT SE (every odd block) need only the batch statistics:
// conv_c's prologue rebuilds scale / shift from the per-sample sums itself (csrc/bn_fin.h bn_consume_nc; narrow
// kernel) -- one single-workgroup launch less on the forward critical path per such block
// (blocks WITH SE since round 4: every conv_c workgroup also computes the gate of its samples, c3d_pw_args.se_w1)
inline bool fwd_fold_b(const c3d_stage_desc* d, const BlkGeom& G) {
  return fwd_cons(d) && G.Cip <= 224 && G.Cop <= 224 && (!G.se || (c3d_option_fold_se && G.Cr <= 32));
}
// the next block's conv_a can take over this block's residual add when that block reads dense rows of y
// (stride 1 inside a stage), its kernels are the narrow bf16 ones, and the shortcut carries no BatchNorm
inline bool fwd_fuse_next(const c3d_stage_desc* d, const Plan& P, int i, int sc_mode) {
  return fwd_cons(d) && fuse_residual(d) && i + 1 < d->n_blocks && sc_mode != SC_BN && d->dtype == C3D_DT_BF16 &&
         P.g[i].Cop <= 224 && P.g[i + 1].Cip <= 224 && d->blocks[i + 1].stride == 1 && !d->blocks[i + 1].has_sc_conv;
}
// ---- backward
// BatchNorm-backward coefficients rebuilt by their consumers (bf16 kernels, narrow and wide; csrc/bn_fin.h) instead of
// c3d_bn_bwd_coef launches
inline bool bwd_consb(const c3d_stage_desc* d) { return fin_consumer(d) && d->dtype == C3D_DT_BF16; }
// BatchNorm_b / SE backward coefficients.  Blocks without SE (stride 1 always): the fused depthwise backward kernel
// rebuilds A | B | C from the per-sample sums in its prologue -- no coefficient launch on the critical path
inline bool bwd_fold_b(const c3d_stage_desc* d, const BlkGeom& G) { return fin_consumer(d) && !G.se && G.s == 1; }
// The weight gradient of conv_c / conv_a inside its data-gradient launch: the cooperative kernel (csrc/pw_cdgrad.hip) if it
// accepts the call as it will be launched, else the wave-private kernel's variant where that holds the layer
inline bool coop_wc(const c3d_stage_desc* d, const c3d_pw_args& a) {
  return (c3d_option_pw_cdg & 2) && !(d->flags & C3D_STAGE_SEPARATE_WGRAD) && c3d_detail_pw_cdg_c_accepts(&a);
}
inline bool fuse_wc(const c3d_stage_desc* d, const BlkGeom& G, bool coop) {
  return coop || ((c3d_option_fuse_wgrad & 2) && fuse_wgrad(d, G.Cop, G.Cip, C3D_WG_SWISH) && G.Cop <= 48);
}
inline bool coop_wa(const c3d_stage_desc* d, const c3d_pw_args& a) {
  return (c3d_option_pw_cdg & 1) && !(d->flags & C3D_STAGE_SEPARATE_WGRAD) && c3d_detail_pw_cdg_a_accepts(&a);
}
inline bool fuse_wa(const c3d_stage_desc* d, const BlkGeom& G, bool coop) {
  return coop || ((c3d_option_fuse_wgrad & 1) && fuse_wgrad(d, G.Cip, G.Cinp, C3D_WG_ROWS));
}
// xin of conv_a is the previous block's output y: its ReLU mask goes onto dx in the conv_a data gradient -- dx IS that
// block's g then (the dx slots outlive that block's side-stream weight gradients: make_plan) -- and, unless its shortcut has a
// BatchNorm of its own, its BatchNorm_c-backward sums are taken in the same epilogue (add_sums): no c3d_block_out_bwd launch for
// it.  Without the fused weight gradient the same epilogue is the C3D_WG_MASKSUM kernel (res4: the 7-tile bucket).
inline bool masksum(const c3d_stage_desc* d, const BlkGeom& G, bool fuse_wa) {
  return !fuse_wa && d->dtype == C3D_DT_BF16 && c3d_detail_pw_gemm_masksum_supported(G.Cip, G.Cinp);
}
struct MaskNext { bool mask, sums; };   // what the conv_a data gradient of block i does for block i - 1
inline MaskNext mask_next(const c3d_stage_desc* d, const Plan& P, int i, int res_mode, bool fuse_wa) {
  const int opt = c3d_option_mask_in_dgrad;
  const bool ms = masksum(d, P.g[i], fuse_wa);
  bool mask = i > 0 && (opt & 1) && res_mode == 0 && (fuse_wa || (ms && (opt & 2)));
  const bool sums = mask && (opt & 2) && !P.g[i - 1].sc_bn;
  if (mask && !fuse_wa && !sums) mask = false;   // (C3D_WG_MASKSUM always sums)
  return {mask, sums};
}

// ------------------------------------------------------------------------------------------ forward pass
struct FwdPass {
  const c3d_stage_desc* d;
  const Plan& P;
  hipStream_t st;
  int epi;            // epilogue of the GEMMs in front of a BatchNorm: C3D_EPI_STATS in training mode
  const void* cur;    // input of the block being enqueued: x, then the output of the block above
  // Residual add of block i fused into conv_a of block i+1 (c3d_pw_args.pro_out): pending operands of block i
  struct Pending { const void* c; const void* sc; c3d_bn_fin fin; void* y; bool on; } pend;
  // the shortcut operand of the block being enqueued (fwd_shortcut -> fwd_block_out)
  int sc_mode;
  const void* scp;
};

int fwd_bn_finalize(FwdPass& S, const double* sums, double count, const c3d_bn_ptrs& bn, int C, int Cp, float* ss, float* mr) {
  const c3d_stage_desc* d = S.d;
  const int tr = d->training ? 1 : 0;
  return prof_call("c3d_bn_finalize", 0.0, S.st, [&] {
    return c3d_bn_finalize(sums, C3D_STAT_STRIPES, count, bn.gamma, bn.beta, bn.running_mean, bn.running_var,
                           tr ? bn.num_batches_tracked : nullptr, d->momentum, d->eps, C, Cp, tr, ss, mr, S.st); });
}

// Weight images of the whole stage in one launch per 64 images: the f32 master weights change once per optimizer
// step, the four (six with a shortcut convolution) GEMMs of a block read them in ~256 workgroups each.  The backward
// pass of this forward reads the transposed images from the same workspace.
int fwd_pack_weights(FwdPass& S, void* ws) {
  std::vector<c3d_pw_pack_desc> pk;
  auto add = [&](const float* w, const Region& r, int N, int K, int sn, int sk) {
    if (r.off != SIZE_MAX) pk.push_back(c3d_pw_pack_desc{w, at(ws, r.off), N, cpad(N), K, cpad(K), sn, sk});
  };
  for (int i = 0; i < S.d->n_blocks; ++i) {
    const c3d_block_desc& k = S.d->blocks[i];
    const BlkGeom& G = S.P.g[i];
    const BlkFwd& F = S.P.f[i];
    add(k.w_a, F.img_a, G.Ci, G.Cin, G.Cin, 1);
    add(k.w_c, F.img_c, G.Co, G.Ci, G.Ci, 1);
    if (G.sc_conv) add(k.w_sc, F.img_s, G.Co, G.Cin, G.Cin, 1);
    add(k.w_a, F.img_at, G.Cin, G.Ci, 1, G.Cin);
    add(k.w_c, F.img_ct, G.Ci, G.Co, 1, G.Ci);
    if (G.sc_conv) add(k.w_sc, F.img_st, G.Cin, G.Co, 1, G.Cin);
  }
  return prof_call("c3d_pw_pack_weights", 0.0, S.st, [&] { return c3d_pw_pack_weights(pk.data(), (int32_t)pk.size(), S.d->dtype, S.st); });
}

// conv_a (1x1x1) + BN_a statistics
int fwd_conv_a(FwdPass& S, const BlkFwdView& V, int i) {
  const c3d_block_desc& k = S.d->blocks[i];
  const BlkGeom& G = S.P.g[i];
  PwCall p(S.pend.on ? S.pend.c : S.cur, k.w_a, V.a, G.M, G.Cin, G.Ci, G.Cin, 1, S.d->dtype);
  if (S.pend.on) {   // y(i-1) = relu(bn_c(c) + shortcut) computed on load, written out, and fed to the GEMM
    p.a.x2 = S.pend.sc; p.a.pro_mode = C3D_PRO_AFFINE2; p.a.fin = S.pend.fin; p.a.pro_p = S.pend.fin.ss; p.a.pro_out = S.pend.y;
    S.pend.on = false;
  }
  p.a.epi_mode = S.epi; p.a.stats = V.sums_a; p.a.w_img = V.img_a;
  return pw_launch(p.a, S.st);
}

// conv_b (depthwise 3x3x3, BN_a + ReLU on load) + per-sample statistics.  BN_a is finalised by the depthwise kernel's own
// prologue (or by a separate launch: eval mode, C3D_FIN_CONSUMER=0)
int fwd_depthwise(FwdPass& S, const BlkFwdView& V, int i) {
  const c3d_stage_desc* d = S.d;
  const c3d_block_desc& k = d->blocks[i];
  const BlkGeom& G = S.P.g[i];
  const int dt = d->dtype, B = d->B, T = d->T;
  const double dw_bytes = ((double)G.M + (double)G.Mo) * G.Cip * (double)es(dt);
  if (fwd_cons(d)) {
    const c3d_bn_fin fa = fin_consume(V.sums_a, k.bn_a, (double)G.M, d->momentum, d->eps, V.ss_a, V.mr_a);
    return prof_call("c3d_dw333_fwd", dw_bytes, S.st, [&] {
      return c3d_dw333_fwd_fin(V.a, &fa, k.w_b, V.b, V.nc_b, B, T, G.H, G.W, G.Ci, G.Cip, G.s, dt, S.st); });
  }
  RC(fwd_bn_finalize(S, V.sums_a, (double)G.M, k.bn_a, G.Ci, G.Cip, V.ss_a, V.mr_a));
  return prof_call("c3d_dw333_fwd", dw_bytes, S.st, [&] {
    return c3d_dw333_fwd(V.a, V.ss_a, k.w_b, V.b, V.nc_b, B, T, G.H, G.W, G.Ci, G.Cip, G.s, dt, S.st); });
}

// BN_b + SE (a launch of its own unless conv_c folds it: fwd_fold_b), then conv_c (BN_b * SE gate, Swish on load) + BN_c
// statistics
int fwd_conv_c(FwdPass& S, const BlkFwdView& V, int i) {
  const c3d_stage_desc* d = S.d;
  const c3d_block_desc& k = d->blocks[i];
  const BlkGeom& G = S.P.g[i];
  const int tr = d->training ? 1 : 0, B = d->B;
  const int64_t rps = (int64_t)d->T * G.Ho * G.Wo;
  const bool fold_b = fwd_fold_b(d, G);
  if (!fold_b)
    RC(prof_call("c3d_bn_se_finalize", 0.0, S.st, [&] {
      return c3d_bn_se_finalize(V.nc_b, B, (double)rps, k.bn_b.gamma, k.bn_b.beta, k.bn_b.running_mean, k.bn_b.running_var,
                                tr ? k.bn_b.num_batches_tracked : nullptr, d->momentum, d->eps, G.Ci, G.Cip, tr,
                                G.se ? k.se_w1 : nullptr, k.se_b1, k.se_w2, k.se_b2, G.Cr, V.ss_b, V.mr_b, V.gate, V.hid, S.st); }));
  PwCall p(V.b, k.w_c, V.c, G.Mo, G.Ci, G.Co, G.Ci, 1, d->dtype);
  p.a.pro_mode = C3D_PRO_BN_SE_SWISH; p.a.pro_p = V.ss_b; p.a.pro_gate = V.gate; p.a.rows_per_sample = rps;
  if (fold_b) {
    p.a.fin = fin_consume(V.nc_b, k.bn_b, (double)rps * B, d->momentum, d->eps, V.ss_b, V.mr_b);
    p.a.fin.batch = B;
    if (G.se) { p.a.se_w1 = k.se_w1; p.a.se_b1 = k.se_b1; p.a.se_w2 = k.se_w2; p.a.se_b2 = k.se_b2; p.a.se_hid = V.hid; p.a.se_cr = G.Cr; }
  }
  p.a.epi_mode = S.epi; p.a.stats = V.sums_c; p.a.w_img = V.img_c;
  RC(pw_launch(p.a, S.st));
  if (!fwd_cons(d)) RC(fwd_bn_finalize(S, V.sums_c, (double)G.Mo, k.bn_c, G.Co, G.Cop, V.ss_c, V.mr_c));
  return 0;
}

// shortcut: the block's input itself, or a (strided) 1x1x1 convolution of it with or without a BatchNorm
int fwd_shortcut(FwdPass& S, const BlkFwdView& V, int i) {
  const c3d_block_desc& k = S.d->blocks[i];
  const BlkGeom& G = S.P.g[i];
  S.sc_mode = SC_IDENTITY;
  S.scp = S.cur;
  if (!G.sc_conv) return 0;
  PwCall p(S.cur, k.w_sc, V.sc, G.Mo, G.Cin, G.Co, G.Cin, 1, S.d->dtype);
  p.a.row_mode = G.s == 2 ? C3D_ROWS_STRIDE2 : C3D_ROWS_DENSE; p.a.H = G.H; p.a.W = G.W;
  p.a.epi_mode = G.sc_bn ? S.epi : C3D_EPI_STORE; p.a.stats = V.sums_1; p.a.w_img = V.img_s;
  RC(pw_launch(p.a, S.st));
  if (G.sc_bn && !fwd_cons(S.d)) RC(fwd_bn_finalize(S, V.sums_1, (double)G.Mo, k.bn_sc, G.Co, G.Cop, V.ss_1, V.mr_1));
  S.sc_mode = G.sc_bn ? SC_BN : SC_RAW;
  S.scp = V.sc;
  return 0;
}

// y = relu(bn_c(c) + shortcut): left to the next block's conv_a (fwd_fuse_next), or a launch of its own
int fwd_block_out(FwdPass& S, const BlkFwdView& V, int i) {
  const c3d_stage_desc* d = S.d;
  const c3d_block_desc& k = d->blocks[i];
  const BlkGeom& G = S.P.g[i];
  const int dt = d->dtype, mode = S.sc_mode;
  const void* scp = S.scp;
  const double bo_bytes = (double)G.Mo * G.Cop * 3 * (double)es(dt);
  S.cur = V.y;
  if (fwd_fuse_next(d, S.P, i, mode)) {
    S.pend.c = V.c; S.pend.sc = scp; S.pend.y = V.y; S.pend.on = true;
    S.pend.fin = fin_consume(V.sums_c, k.bn_c, (double)G.Mo, d->momentum, d->eps, V.ss_c, V.mr_c);
    return 0;
  }
  if (fwd_cons(d)) {
    const c3d_bn_fin fc = fin_consume(V.sums_c, k.bn_c, (double)G.Mo, d->momentum, d->eps, V.ss_c, V.mr_c);
    c3d_bn_fin f1;
    if (mode == SC_BN) f1 = fin_consume(V.sums_1, k.bn_sc, (double)G.Mo, d->momentum, d->eps, V.ss_1, V.mr_1);
    return prof_call("c3d_block_out_fwd", bo_bytes, S.st, [&] {
      return c3d_block_out_fwd_fin(V.c, &fc, scp, mode == SC_BN ? &f1 : nullptr, mode, V.y, G.Mo, G.Co, G.Cop, dt, S.st); });
  }
  return prof_call("c3d_block_out_fwd", bo_bytes, S.st, [&] {
    return c3d_block_out_fwd(V.c, V.ss_c, scp, V.ss_1, mode, V.y, G.Mo, G.Cop, dt, S.st); });
}

// ------------------------------------------------------------------------------------------ backward pass
struct RedJob { const float* ws; float* dw; int K, N, parts, sk, sn; };

struct BwdPass {
  const c3d_stage_desc* d;
  const Plan& P;
  hipStream_t st;
  // chained separate weight gradients: launch k leaves its partials in workspace k & 1, launch k + 1 reduces them
  float* wg_ws[2];
  int wg_n;
  // cooperative data + weight gradient launches of this call (workspace slot 1 + cdg_n) and their partials: reduced on the
  // side stream behind one fork at the end of the pass
  float* wg_fused;
  int cdg_n;
  std::vector<RedJob> red_jobs;
  // carried from the block above
  const void* cur_dy;
  bool premasked;   // cur_dy is already dy * (y > 0): the conv_a data gradient of the block above stored it that way
  bool sums_done;   // ...and accumulated this block's BatchNorm_c-backward sums too: no c3d_block_out_bwd for it
  std::deque<uint64_t> lag;   // side-stream marks of the blocks whose ring slots are still in flight
  // of the block being enqueued
  void* g;           // the masked gradient at the block's output: the view's g, or cur_dy itself where it arrived masked
  const void* res;   // what conv_a's epilogue adds (bwd_shortcut -> bwd_conv_a): g, or the shortcut convolution's data gradient
  int res_mode;
};

// A cooperative data + weight gradient (csrc/pw_cdgrad.hip; the caller has asked its _accepts).  With the side stream on, the
// kernel leaves its weight-gradient partials in a slot of their own and ALL reducers of the pass are launched behind one
// fork at its end.  (Per launch -- on the side stream, six rotating buffers -- every fork was a barrier packet on the main
// queue: 11 us in front of every conv_c launch with the side queue otherwise idle, profiles/r06_trace_gaps.txt; on the main
// stream each reducer is 5 us of the data-gradient chain.)  Side stream off: slot 0, the reducer right behind the kernel.
int coop_launch(BwdPass& S, c3d_pw_args& a, int (*launch)(const c3d_pw_args*, int*, void*)) {
  const bool defer = side_enabled();
  int parts = 0;
  if (defer) a.wg_ws = S.wg_fused + (size_t)(1 + S.cdg_n) * (S.P.wgrad_ws_fused_slot / 4);
  RC(pw_prof(a, S.st, [&] { return launch(&a, defer ? &parts : nullptr, S.st); }));
  if (defer) { ++S.cdg_n; S.red_jobs.push_back({a.wg_ws, a.wg_dw, a.K, a.N, parts, a.w_sk, a.w_sn}); }
  return 0;
}

// The separate weight gradient of a pointwise layer, on the side stream: the caller has filled the operands, the pass
// supplies the next of the two chained-reduction workspaces.
int side_wgrad(BwdPass& S, WgCall& w) {
  return side_run(S.st, [&](hipStream_t s2) {
    w.a.ws = S.wg_ws[S.wg_n++ & 1];
    w.a.chain = c3d_option_wgrad_chain;
    return wg_launch(w.a, s2);
  });
}

int bwd_coef(BwdPass& S, const double* dsums, double count, const c3d_bn_ptrs& bn, const float* mr, int C, int Cp, float* out) {
  return prof_call("c3d_bn_bwd_coef", 0.0, S.st, [&] {
    return c3d_bn_bwd_coef(dsums, 1, count, bn.gamma, mr, C, Cp, out, bn.dgamma, bn.dbeta, S.st); });
}

// ---- y = relu(bn_c(c) + shortcut)
int bwd_block_out(BwdPass& S, const BlkBwdView& V, int i) {
  const c3d_block_desc& k = S.d->blocks[i];
  const BlkGeom& G = S.P.g[i];
  const int dt = S.d->dtype;
  const double e = (double)es(dt);
  const bool scbn = G.sc_bn;
  const void* cur_dy = S.cur_dy;
  if (S.premasked && S.sums_done) {   // c3d_block_out_bwd of this block ran inside the conv_a data gradient of the block above
    S.g = const_cast<void*>(cur_dy);
  } else if (S.premasked) {   // the mask was applied where dy was produced (c3d_pw_args.wg_mask_out): statistics only, g IS dy
    S.g = const_cast<void*>(cur_dy);
    RC(prof_call("c3d_block_out_bwd", (double)G.Mo * G.Cop * (scbn ? 3 : 2) * e, S.st, [&] {
      return c3d_block_out_bwd(cur_dy, nullptr, V.c, scbn ? V.sc : nullptr, nullptr, V.mr_c, scbn ? V.mr_1 : nullptr, V.dsums_c,
                               scbn ? V.dsums_1 : nullptr, G.Mo, G.Co, G.Cop, dt, S.st); }));
  } else {
    S.g = V.g;
    RC(prof_call("c3d_block_out_bwd", (double)G.Mo * G.Cop * (scbn ? 5 : 4) * e, S.st, [&] {
      return c3d_block_out_bwd(cur_dy, V.y, V.c, scbn ? V.sc : nullptr, V.g, V.mr_c, scbn ? V.mr_1 : nullptr, V.dsums_c,
                               scbn ? V.dsums_1 : nullptr, G.Mo, G.Co, G.Cop, dt, S.st); }));
  }
  if (!bwd_consb(S.d)) RC(bwd_coef(S, V.dsums_c, (double)G.Mo, k.bn_c, V.mr_c, G.Co, G.Cop, V.coef_c));
  return 0;
}

// ---- conv_c data gradient, Swish / SE backward in the epilogue; weight gradient on the side stream (it needs
//      coef_c, not the data gradient: it is forked BEFORE the data-gradient launch)
//      -- or fused into the data-gradient launch (coop_wc / fuse_wc)
int bwd_conv_c(BwdPass& S, const BlkBwdView& V, int i) {
  const c3d_stage_desc* d = S.d;
  const c3d_block_desc& k = d->blocks[i];
  const BlkGeom& G = S.P.g[i];
  const int dt = d->dtype;
  const bool consb = bwd_consb(d);
  const int64_t rps = (int64_t)d->T * G.Ho * G.Wo;
  const BnBwd bn_c{V.c, V.coef_c, V.dsums_c, k.bn_c, (double)G.Mo, V.mr_c};
  PwCall pc(S.g, k.w_c, V.t1, G.Mo, G.Co, G.Ci, 1, G.Ci, dt);
  pc.a.wg_mode = C3D_WG_SWISH; pc.a.wg_dw = k.dw_c; pc.a.wg_ws = S.wg_fused;
  bn_bwd_operand(pc.a, consb, bn_c);
  pc.a.epi_mode = C3D_EPI_SWISH_SE_BWD; pc.a.e1 = V.b; pc.a.epi_p = V.ss_b; pc.a.epi_gate = V.gate; pc.a.epi_q = V.mr_b;
  pc.a.stats = V.nc3; pc.a.rows_per_sample = rps; pc.a.w_img = V.img_ct;
  const bool coop = coop_wc(d, pc.a);
  if (!fuse_wc(d, G, coop)) {
    pc.a.wg_mode = C3D_WG_NONE; pc.a.wg_dw = nullptr; pc.a.wg_ws = nullptr;
    WgCall w(S.g, V.b, k.dw_c, G.Mo, G.Ci, G.Co, G.Ci, 1, dt);
    bn_bwd_operand(w.a, consb, bn_c);
    w.a.q_mode = C3D_PRO_BN_SE_SWISH; w.a.q_ss = V.ss_b; w.a.q_gate = V.gate; w.a.rows_per_sample = rps;
    RC(side_wgrad(S, w));
  }
  return coop ? coop_launch(S, pc.a, c3d_detail_pw_cdg_c) : pw_launch(pc.a, S.st);
}

// ---- BatchNorm_b / SE backward coefficients (a launch of their own unless the depthwise kernel rebuilds them: bwd_fold_b),
//      then depthwise conv_b: data gradient and weight gradient in ONE pass over t1, b, a (csrc/dw_bwd_fused.hip; stride 1
//      and the stride-2 first block of a stage, any extents)
int bwd_depthwise(BwdPass& S, const BlkBwdView& V, int i) {
  const c3d_stage_desc* d = S.d;
  const c3d_block_desc& k = d->blocks[i];
  const BlkGeom& G = S.P.g[i];
  const int dt = d->dtype, B = d->B, T = d->T;
  const int64_t rps = (int64_t)T * G.Ho * G.Wo;
  const double dw_bytes = ((double)G.Mo * 2 + (double)G.M * 2) * G.Cip * (double)es(dt);
  if (bwd_fold_b(d, G)) {
    const c3d_bn_fin fb = fin_coef_consume(V.nc3, k.bn_b, (double)rps * B, V.mr_b, true, B);
    RC(prof_call("c3d_dw333_bwd_fused", dw_bytes, S.st, [&] {
      return c3d_dw333_bwd_fused_fin(V.t1, V.b, &fb, k.w_b, V.a, V.ss_a, V.mr_a, V.t2, V.dsums_a, k.dw_b, B, T, G.H, G.W, G.Ci, G.Cip, 1, dt, S.st); }));
  } else {
    RC(prof_call("c3d_se_bn_bwd_coef", 0.0, S.st, [&] {
      return c3d_se_bn_bwd_coef(V.nc3, V.nc_b, B, (double)rps, k.bn_b.gamma, V.mr_b, V.ss_b, G.Ci, G.Cip, G.se ? k.se_w1 : nullptr,
                                k.se_w2, V.gate, V.hid, G.Cr, V.cA, V.cC, V.cB, k.bn_b.dgamma, k.bn_b.dbeta, k.dse_w1, k.dse_b1,
                                k.dse_w2, k.dse_b2, S.st); }));
    RC(prof_call("c3d_dw333_bwd_fused", dw_bytes, S.st, [&] {
      return c3d_dw333_bwd_fused(V.t1, V.b, V.cA, V.cB, V.cC, k.w_b, V.a, V.ss_a, V.mr_a, V.t2, V.dsums_a, k.dw_b, B, T, G.H, G.W, G.Ci, G.Cip, G.s, dt, S.st); }));
  }
  if (!bwd_consb(d)) RC(bwd_coef(S, V.dsums_a, (double)G.M, k.bn_a, V.mr_a, G.Ci, G.Cip, V.coef_a));
  return 0;
}

// ---- shortcut branch: the data gradient on the main stream, then the weight gradient on the side stream
int bwd_shortcut(BwdPass& S, const BlkBwdView& V, int i) {
  const c3d_stage_desc* d = S.d;
  const c3d_block_desc& k = d->blocks[i];
  const BlkGeom& G = S.P.g[i];
  const int dt = d->dtype;
  const bool consb = bwd_consb(d);
  S.res = S.g;
  S.res_mode = 0;
  if (!G.sc_conv) return 0;
  const BnBwd bn_1{V.sc, V.coef_1, V.dsums_1, k.bn_sc, (double)G.Mo, V.mr_1};
  PwCall p(S.g, k.w_sc, V.dxs, G.Mo, G.Co, G.Cin, 1, G.Cin, dt);
  p.a.w_img = V.img_st;
  if (G.sc_bn) {
    if (!consb) RC(bwd_coef(S, V.dsums_1, (double)G.Mo, k.bn_sc, V.mr_1, G.Co, G.Cop, V.coef_1));
    bn_bwd_operand(p.a, consb, bn_1);
  }
  RC(pw_launch(p.a, S.st));
  WgCall w(S.g, V.xin, k.dw_sc, G.Mo, G.Cin, G.Co, G.Cin, 1, dt);
  if (G.sc_bn) bn_bwd_operand(w.a, consb, bn_1);
  w.a.row_mode = G.s == 2 ? C3D_ROWS_STRIDE2 : C3D_ROWS_DENSE; w.a.H = G.H; w.a.W = G.W;
  RC(side_wgrad(S, w));
  S.res = V.dxs;
  S.res_mode = G.s == 2 ? 1 : 0;
  return 0;
}

// The conv_a data gradient's arguments, with the weight gradient fused into the launch or not, and what the launch does
// for the block below (mask_next)
PwCall conv_a_call(const BwdPass& S, const BlkBwdView& V, int i, bool fuse_wa, MaskNext& mn) {
  const c3d_stage_desc* d = S.d;
  const c3d_block_desc& k = d->blocks[i];
  const BlkGeom& G = S.P.g[i];
  PwCall p(V.t2, k.w_a, V.dx, G.M, G.Ci, G.Cin, 1, G.Cin, d->dtype);
  if (fuse_wa) { p.a.wg_mode = C3D_WG_ROWS; p.a.wg_x3 = V.xin; p.a.wg_dw = k.dw_a; p.a.wg_ws = S.wg_fused; }
  mn = mask_next(d, S.P, i, S.res_mode, fuse_wa);
  p.a.wg_mask_out = mn.mask ? 1 : 0;
  if (mn.mask && !fuse_wa) { p.a.wg_mode = C3D_WG_MASKSUM; p.a.wg_x3 = V.xin; }
  if (mn.sums) { p.a.add_c = V.below_c; p.a.add_mr = V.below_mr_c; p.a.add_sums = V.below_dsums_c; }
  bn_bwd_operand(p.a, bwd_consb(d), BnBwd{V.a, V.coef_a, V.dsums_a, k.bn_a, (double)G.M, V.mr_a});
  p.a.epi_mode = C3D_EPI_ADD; p.a.e1 = S.res; p.a.res_mode = S.res_mode; p.a.H = G.H; p.a.W = G.W;
  p.a.w_img = V.img_at;
  return p;
}

// ---- conv_a data gradient (+ shortcut gradient in the epilogue) and weight gradient (forked first: it needs the
//      coefficients, not the data gradient)
// ... or fused into the data-gradient launch: the wave-private kernel's variant (K, N <= 112) or the cooperative kernel
// (csrc/pw_cdgrad.hip: any of the three stage widths, dense shortcut gradient, packed weight image)
// The arguments are filled for the fused form first, and the cooperative kernel is asked about exactly those.
int bwd_conv_a(BwdPass& S, const BlkBwdView& V, int i) {
  const c3d_stage_desc* d = S.d;
  const c3d_block_desc& k = d->blocks[i];
  const BlkGeom& G = S.P.g[i];
  MaskNext mn;
  PwCall pa = conv_a_call(S, V, i, true, mn);
  const bool coop = coop_wa(d, pa.a);
  if (!fuse_wa(d, G, coop)) {
    pa = conv_a_call(S, V, i, false, mn);
    WgCall w(V.t2, V.xin, k.dw_a, G.M, G.Cin, G.Ci, G.Cin, 1, d->dtype);
    bn_bwd_operand(w.a, bwd_consb(d), BnBwd{V.a, V.coef_a, V.dsums_a, k.bn_a, (double)G.M, V.mr_a});
    RC(side_wgrad(S, w));
  }
  RC(coop ? coop_launch(S, pa.a, c3d_detail_pw_cdg_a) : pw_launch(pa.a, S.st));
  S.cur_dy = V.dx;
  S.premasked = mn.mask;
  S.sums_done = mn.sums;
  return 0;
}

// the last chained weight gradient's partials (its own reducer launch, on the stream it ran on)
int bwd_finish(BwdPass& S) {
  if (!S.wg_n && S.red_jobs.empty()) return 0;
  return side_run(S.st, [&](hipStream_t s2) {
    for (const RedJob& j : S.red_jobs) RC(c3d_detail_pw_wgrad_reduce(j.ws, j.dw, j.K, j.N, j.parts, j.sk, j.sn, s2));
    return S.wg_n ? c3d_pw_wgrad_flush(s2) : 0;
  });
}

// ------------------------------------------------------------------------------------------ eval: folded BatchNorm
// Eval-mode BatchNorm is the per-channel affine map y = x*scale + shift with scale = gamma / sqrt(running_var + eps),
// shift = beta - running_mean*scale (reference scripts/train_BCD.py:92-154 runs the model under model.eval()).
// The scale is folded into the rows of the producing convolution's weight matrix ONCE (c3d_stage_fold_bn); what is
// left of every BatchNorm is a bias that the consumer adds on operand load.  The eval forward then needs no
// statistics, no finalize launches (4-5 kernels per block instead of 7) and no saved activations (ring workspace).
__global__ void fold_bn_kernel(const float* __restrict__ w, float* __restrict__ wf, int N, int K, const float* __restrict__ gamma,
                               const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ var,
                               float eps, float* __restrict__ ss, int Cp) {
  const int n = blockIdx.x;
  if (n >= Cp) return;
  float sc = 0.f, sh = 0.f;
  if (n < N) {
    // same arithmetic as bn_finalize_kernel's eval branch: rstd in f64, rounded once
    const float rstd = (float)(1.0 / sqrt((double)var[n] + (double)eps));
    sc = gamma[n] * rstd;
    sh = beta[n] - mean[n] * sc;
    for (int k = threadIdx.x; k < K; k += blockDim.x) wf[(size_t)n * K + k] = w[(size_t)n * K + k] * sc;
  }
  if (threadIdx.x == 0) { ss[n] = n < N ? 1.f : 0.f; ss[Cp + n] = sh; }
}

}  // namespace

// =================================================================================================== C ABI
extern "C" int c3d_stage_ws_bytes(const c3d_stage_desc* d, int64_t* ws_fwd_bytes, int64_t* ws_bwd_bytes, int64_t* y_bytes,
                                  int64_t* dx_bytes) {
  Plan P;
  RC(make_plan(d, P));
  if (ws_fwd_bytes) *ws_fwd_bytes = (int64_t)P.fwd_total;
  if (ws_bwd_bytes) *ws_bwd_bytes = (int64_t)P.bwd_total;
  if (y_bytes) *y_bytes = (int64_t)P.y_bytes;
  if (dx_bytes) *dx_bytes = (int64_t)P.dx_bytes;
  return 0;
}

extern "C" int c3d_stage_saved(const c3d_stage_desc* d, int32_t blk, const char* name, int64_t* offset, int64_t* bytes) {
  static const struct { const char* name; Region BlkFwd::*region; } saved[] = {
      {"a", &BlkFwd::a},       {"b", &BlkFwd::b},       {"c", &BlkFwd::c},       {"sc", &BlkFwd::sc},
      {"mr_a", &BlkFwd::mr_a}, {"mr_b", &BlkFwd::mr_b}, {"mr_c", &BlkFwd::mr_c}, {"mr_sc", &BlkFwd::mr_1},
      {"ss_a", &BlkFwd::ss_a}, {"ss_b", &BlkFwd::ss_b}, {"ss_c", &BlkFwd::ss_c}, {"ss_sc", &BlkFwd::ss_1},
      {"gate", &BlkFwd::gate}};
  Plan P;
  RC(make_plan(d, P));
  if (blk < 0 || blk >= d->n_blocks || !name || !offset || !bytes) return C3D_E_BADARG;
  for (const auto& s : saved) {
    if (std::strcmp(name, s.name)) continue;
    const Region& r = P.f[blk].*s.region;
    if (r.off == SIZE_MAX) return C3D_E_BADARG;   // the block has no such region
    *offset = (int64_t)r.off; *bytes = (int64_t)r.bytes;   // the bytes asked for, not the carver's 256-byte round-up
    return 0;
  }
  return C3D_E_BADARG;
}

extern "C" int c3d_side_join(void* stream) { return side_join(reinterpret_cast<hipStream_t>(stream), UINT64_MAX); }

extern "C" int c3d_stage_fwd(const c3d_stage_desc* d, const void* x, void* ws, void* y_out, void* stream) {
  Plan P;
  RC(make_plan(d, P));
  if (!x || !ws || !y_out) return C3D_E_BADARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  RC(zero_fill(at(ws, P.fwd_acc_off), P.fwd_acc_bytes, st));
  FwdPass S{d, P, st, d->training ? C3D_EPI_STATS : C3D_EPI_STORE, x, {}, SC_IDENTITY, x};
  if (use_pw_img(d)) RC(fwd_pack_weights(S, ws));
  for (int i = 0; i < d->n_blocks; ++i) {
    const BlkGeom& G = P.g[i];
    prof_tag_block(G.H, G.Ci, G.s, G.se);
    const BlkFwdView V = view(d, ws, y_out, P, i);
    RC(fwd_conv_a(S, V, i));
    RC(fwd_depthwise(S, V, i));
    RC(fwd_conv_c(S, V, i));
    RC(fwd_shortcut(S, V, i));
    RC(fwd_block_out(S, V, i));
  }
  return 0;
}

extern "C" int c3d_stage_bwd(const c3d_stage_desc* d, const void* x, const void* y_out, const void* dy, void* ws,
                             void* wb, void* dx_out, void* stream) {
  Plan P;
  RC(make_plan(d, P));
  if (!x || !y_out || !dy || !ws || !wb || !dx_out) return C3D_E_BADARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  RC(zero_fill(at(wb, P.bwd_acc_off), P.bwd_acc_bytes, st));
  BwdPass S{d, P, st, {atT<float>(wb, P.wgrad_ws), atT<float>(wb, P.wgrad_ws2)}, 0, atT<float>(wb, P.wgrad_ws_fused), 0, {},
            dy, false, false, {}, nullptr, nullptr, 0};
  // chained weight-gradient partials this call leaves pending are this call's to settle: the flush at the end of the pass,
  // or -- returning early with an error -- forgotten (somebody else's pending partials are not touched: c3d_pw_wgrad settles them)
  struct PendingGuard {
    float* const* ws;
    bool armed = true;
    ~PendingGuard() { if (armed) { c3d_detail_pw_wgrad_v2_forget(ws[0]); c3d_detail_pw_wgrad_v2_forget(ws[1]); } }
  } pending_guard{S.wg_ws};
  for (int i = d->n_blocks - 1; i >= 0; --i) {
    const BlkGeom& G = P.g[i];
    prof_tag_block(G.H, G.Ci, G.s, G.se);
    const BlkBwdView V = view(d, ws, wb, x, y_out, dx_out, P, i);
    RC(bwd_block_out(S, V, i));
    RC(bwd_conv_c(S, V, i));
    RC(bwd_depthwise(S, V, i));
    RC(bwd_shortcut(S, V, i));
    RC(bwd_conv_a(S, V, i));
    // the side stream may lag by ring-1 blocks: block i-1 reuses the ring slot of block i-1+ring
    S.lag.push_back(side_mark());
    if ((int)S.lag.size() >= bwd_ring()) { RC(side_join(st, S.lag.front())); S.lag.pop_front(); }
  }
  RC(bwd_finish(S));
  pending_guard.armed = false;
  return 0;
}

// ---- profile -------------------------------------------------------------------------------------------------------
extern "C" int c3d_prof_begin(int32_t flags) {
  for (ProfRec& r : g_prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  g_prof.clear();
  g_prof_flags = flags & 3;
  g_prof_tag[0] = 0;
  return 0;
}

extern "C" int c3d_prof_end(c3d_prof_row* rows, int32_t cap, int32_t* n_rows) {
  g_prof_flags = -1;
  if (!n_rows || (cap > 0 && !rows)) return C3D_E_BADARG;
  HIPRC(hipDeviceSynchronize());
  int n = 0;
  for (ProfRec& r : g_prof) {
    float ms = 0.f;
    HIPRC(hipEventElapsedTime(&ms, r.e0, r.e1));
    (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1);
    int j = 0;
    while (j < n && std::strncmp(rows[j].name, r.name, sizeof(rows[j].name)) != 0) ++j;
    if (j == n) {
      if (n >= cap) continue;   // table full: the row is dropped (callers pass cap >= 256)
      std::memset(&rows[n], 0, sizeof(rows[n]));
      std::snprintf(rows[n].name, sizeof(rows[n].name), "%s", r.name);
      ++n;
    }
    rows[j].launches += 1; rows[j].ms_total += ms; rows[j].bytes_total += r.bytes;
  }
  g_prof.clear();
  *n_rows = n;
  return 0;
}

// ---- eval ----------------------------------------------------------------------------------------------------------
extern "C" int c3d_stage_fold_bytes(const c3d_stage_desc* d, int64_t* fold_bytes, int64_t* ws_eval_bytes) {
  Plan P;
  RC(make_plan(d, P));
  FoldPlan Q;
  RC(make_fold_plan(d, P, Q));
  if (fold_bytes) *fold_bytes = (int64_t)Q.fold_total;
  if (ws_eval_bytes) *ws_eval_bytes = (int64_t)Q.ws_total;
  return 0;
}

extern "C" int c3d_stage_fold_bn(const c3d_stage_desc* d, void* fold, void* stream) {
  Plan P;
  RC(make_plan(d, P));
  FoldPlan Q;
  RC(make_fold_plan(d, P, Q));
  if (!fold) return C3D_E_BADARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for (int i = 0; i < d->n_blocks; ++i) {
    const c3d_block_desc& k = d->blocks[i];
    const BlkGeom& G = P.g[i];
    const BlkFold& F = Q.f[i];
    struct Job { const float* w; size_t wf; int N, K; const c3d_bn_ptrs* bn; size_t ss; int Cp; bool on; };
    const Job jobs[4] = {{k.w_a, F.w_a, G.Ci, G.Cin, &k.bn_a, F.ss_a, G.Cip, true},
                         {k.w_b, F.w_b, G.Ci, 27, &k.bn_b, F.ss_b, G.Cip, true},
                         {k.w_c, F.w_c, G.Co, G.Ci, &k.bn_c, F.ss_c, G.Cop, true},
                         {k.w_sc, F.w_sc, G.Co, G.Cin, &k.bn_sc, F.ss_1, G.Cop, G.sc_bn}};
    for (const Job& j : jobs) {
      if (!j.on) continue;
      if (!j.w || !j.bn->gamma || !j.bn->beta || !j.bn->running_mean || !j.bn->running_var) return C3D_E_BADARG;
      fold_bn_kernel<<<dim3(j.Cp), dim3(64), 0, st>>>(j.w, atT<float>(fold, j.wf), j.N, j.K, j.bn->gamma, j.bn->beta,
                                                     j.bn->running_mean, j.bn->running_var, d->eps, atT<float>(fold, j.ss), j.Cp);
    }
    if (G.sc_conv && !G.sc_bn)   // shortcut convolution without BatchNorm (stage 1 block 0): plain copy of the weights
      HIPRC(hipMemcpyAsync(at(fold, F.w_sc), k.w_sc, (size_t)G.Co * G.Cin * 4, hipMemcpyDeviceToDevice, st));
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// The eval forward shares no step with the training forward: its launches carry no statistics, no weight images and no
// profile rows (c3d_pw_gemm directly, not pw_launch), so none of them is literally a training-pass call.
extern "C" int c3d_stage_fwd_folded(const c3d_stage_desc* d, const void* fold_c, const void* x, void* ws, void* y_out,
                                    void* stream) {
  Plan P;
  RC(make_plan(d, P));
  FoldPlan Q;
  RC(make_fold_plan(d, P, Q));
  if (!fold_c || !x || !ws || !y_out) return C3D_E_BADARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int dt = d->dtype, B = d->B, T = d->T;
  RC(zero_fill(at(ws, Q.acc_off), Q.acc_bytes, st));
  const void* cur = x;
  for (int i = 0; i < d->n_blocks; ++i) {
    const c3d_block_desc& k = d->blocks[i];
    const BlkGeom& G = P.g[i];
    const BlkEvalView V = view(d, const_cast<void*>(fold_c), ws, y_out, P, Q, i);
    const int64_t rps = (int64_t)T * G.Ho * G.Wo;
    {
      PwCall p(cur, V.w_a, V.a, G.M, G.Cin, G.Ci, G.Cin, 1, dt);
      RC(c3d_pw_gemm(&p.a, st));
    }
    RC(c3d_dw333_fwd(V.a, V.ss_a, V.w_b, V.b, V.nc_b, B, T, G.H, G.W, G.Ci, G.Cip, G.s, dt, st));
    if (G.se)   // SE gate from the per-sample means of the (already scaled) conv_b output: training = 2 -> ss is given
      RC(c3d_bn_se_finalize(V.nc_b, B, (double)rps, k.bn_b.gamma, k.bn_b.beta, k.bn_b.running_mean, k.bn_b.running_var, nullptr,
                            d->momentum, d->eps, G.Ci, G.Cip, 2, k.se_w1, k.se_b1, k.se_w2, k.se_b2, G.Cr, V.ss_b, nullptr,
                            V.gate, V.hid, st));
    {
      PwCall p(V.b, V.w_c, V.c, G.Mo, G.Ci, G.Co, G.Ci, 1, dt);
      p.a.pro_mode = C3D_PRO_BN_SE_SWISH; p.a.pro_p = V.ss_b; p.a.pro_gate = V.gate; p.a.rows_per_sample = rps;
      RC(c3d_pw_gemm(&p.a, st));
    }
    int mode = SC_IDENTITY;
    const void* scp = cur;
    if (G.sc_conv) {
      PwCall p(cur, V.w_sc, V.sc, G.Mo, G.Cin, G.Co, G.Cin, 1, dt);
      p.a.row_mode = G.s == 2 ? C3D_ROWS_STRIDE2 : C3D_ROWS_DENSE; p.a.H = G.H; p.a.W = G.W;
      RC(c3d_pw_gemm(&p.a, st));
      mode = G.sc_bn ? SC_BN : SC_RAW;
      scp = V.sc;
    }
    RC(c3d_block_out_fwd(V.c, V.ss_c, scp, V.ss_1, mode, V.y, G.Mo, G.Cop, dt, st));
    cur = V.y;
  }
  return 0;
}
