/* change3d_hip.h — C ABI of libchange3d_hip.so (MI355X / gfx950 kernels for the Change3D
 * BCD hot path).  Plain pointers and sizes only; every pointer is a DEVICE pointer unless
 * noted; `stream` is a hipStream_t passed as void*.  Every function returns 0 on success
 * or a hipError_t / negative C3D_E* code.
 *
 * The reference (zhuduowang/Change3D) has no FFI: its boundary for this path is the Python
 * module surface of model/x3d.py, model/change_decoder.py, model/trainer.py and
 * model/utils.py.  Each entry point below therefore names the reference construct whose
 * device work it replaces (file:line into /root/reference); the Python mirror in
 * change3d_amd/model/ (Python) binds them with ctypes.
 *
 * Tensor layout: activations are channels-last [B][T][H][W][Cp], Cp = round_up(C,8), pad
 * channels zero; `dtype` selects the storage type of activations (C3D_F32 | C3D_BF16).
 * Parameters, BN statistics, gradients of parameters and optimizer state are always f32
 * (reductions accumulate in f64).
 */
#ifndef CHANGE3D_HIP_H
#define CHANGE3D_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define C3D_DT_F32 0
#define C3D_DT_BF16 1

#define C3D_E_BADARG (-1)
#define C3D_E_UNSUPPORTED (-2)

/* library / device identification (host-only; safe to call without a GPU) */
int c3d_abi_version(void);
const char* c3d_build_info(void);
/* number of compute units of the current device (needs a GPU) */
int c3d_device_cus(void);

/* ------------------------------------------------------------------------------------
 * Pointwise (1x1x1 / 1x1) convolution family as a row GEMM on MFMA:
 *     Y[m, n] = epilogue( sum_k prologue(X)[m, k] * Wt[n, k] )
 * Replaces: nn.Conv3d k=1 conv_a / conv_c / branch1_conv (reference model/x3d.py:173-175,
 * 214-216, 302-308) forward and data-gradient, nn.Conv2d k=1 of the decoder
 * (reference model/change_decoder.py:30-45), with the neighbouring BatchNorm3d-apply,
 * SE gate, Swish and BN-backward arithmetic fused on operand load / result store.
 * ------------------------------------------------------------------------------------ */
#define C3D_PRO_NONE 0
#define C3D_PRO_BN_SE_SWISH 1 /* v = x*scale+shift; q = gate*v; out = q*sigmoid(q)            */
#define C3D_PRO_AFFINE2 2     /* out = A*x + B + C*x2   (BatchNorm backward applied on load)  */

#define C3D_EPI_STORE 0
#define C3D_EPI_STATS 1        /* store + per-channel sum / sum-of-squares into one of
                                  C3D_STAT_STRIPES striped f64 accumulator sets               */
#define C3D_STAT_STRIPES 16
#define C3D_EPI_SWISH_SE_BWD 2 /* t1 = result*swish'(gate*bn(e1))*gate; per-(sample,channel)
                                  sums (d gate, t1, t1*e1hat) -> stats [B][Np][3]            */
#define C3D_EPI_ADD 3          /* result + residual e1 (dense, or scattered from half res)    */

#define C3D_ROWS_DENSE 0  /* row m at x + m*Kp                                               */
#define C3D_ROWS_FRAME 1  /* row m at x + (m / rpg)*gstride + (m % rpg)*Kp (one frame of NDHWC) */
#define C3D_ROWS_STRIDE2 2 /* row m=(bt,ho,wo) gathers input pixel (bt,2ho,2wo) of [BT][H][W] */
#define C3D_ROWS_S2SHIFT 3 /* (wgrad only) as STRIDE2 but pixel (2ho+dy, 2wo+dx), zero outside */

/* In-kernel BatchNorm finalisation by the last workgroup of a statistics producer (csrc/bn_fin.h): when `ticket`
 * is non-NULL the producing kernel itself turns the completed sums into scale/shift (+ running statistics), or into
 * the BatchNorm-backward coefficients, instead of a separate c3d_bn_finalize / c3d_bn_bwd_coef launch.
 *   forward  (c3d_pw_gemm C3D_EPI_STATS)          : ss = scale|shift [2][Cp], mr = mean|rstd [2][Cp] (may be NULL)
 *   backward (c3d_block_out_bwd): ss = coefficients A|B|C [3][Cp], mr = saved mean|rstd (input),
 *              running_mean / running_var carry dgamma / dbeta (accumulated), beta / nbt unused
 * `ticket` is a zeroed uint32 (re-zeroed by the caller before every launch that uses it).                        */
typedef struct c3d_bn_fin {
  uint32_t* ticket;
  const float* gamma; const float* beta;
  float* running_mean; float* running_var;
  int64_t* nbt;
  float* ss; float* mr;
  double count;
  float momentum, eps;
  int32_t training, batch;   /* batch > 0: `sums` is the PER-SAMPLE layout of c3d_dw333_fwd / the Swish-SE-backward epilogue   */
  /* consumer side (c3d_dw333_fwd_fin, c3d_block_out_fwd_fin): the completed f64 sums [C3D_STAT_STRIPES][2][C] of an
   * EARLIER launch; every workgroup of the consuming kernel rebuilds scale/shift of the channels it reads, one
   * workgroup also writes ss / mr / the running statistics.  `ticket` is unused (NULL) in this mode.                */
  const double* sums;
  /* batch > 0 (BatchNorm_b of blocks WITHOUT SqueezeExcitation; the SE blocks keep c3d_bn_se_finalize / c3d_se_bn_bwd_coef):
   *   forward  (c3d_pw_gemm C3D_PRO_BN_SE_SWISH): sums = nc f64 [batch][Cp][2] -> scale|shift rebuilt by every workgroup in
   *             the 4-lane order of c3d_bn_se_finalize (bit-identical), workgroup 0 writes ss / mr / running statistics;
   *   backward (c3d_dw333_bwd_fused): sums = nc3 f64 [batch][Cp][3] -> A | B | C of c3d_se_bn_bwd_coef (no-SE branch),
   *             running_mean / running_var carry dgamma / dbeta (accumulated by one workgroup per channel chunk).      */
} c3d_bn_fin;

typedef struct c3d_pw_args {
  const void* x;         /* A-side tensor, storage dtype, rows of Kp elements                */
  const void* x2;        /* second A-side tensor for C3D_PRO_AFFINE2 (same addressing)       */
  void* y;               /* output [M][Np], storage dtype                                    */
  const void* e1;        /* epilogue tensor ([M][Np] dense; or half-res residual)            */
  const float* w;        /* weights, element (n,k) at w[n*w_sn + k*w_sk]                     */
  const float* pro_p;    /* BN_SE_SWISH: scale[Kp],shift[Kp]; AFFINE2: A[Kp],B[Kp],C[Kp]     */
  const float* pro_gate; /* BN_SE_SWISH: gate[B][Kp] or NULL (=1)                            */
  const float* epi_p;    /* SWISH_SE_BWD: scale[Np],shift[Np] of the BN applied to e1        */
  const float* epi_gate; /* SWISH_SE_BWD: gate[B][Np] or NULL (=1)                           */
  const float* epi_q;    /* SWISH_SE_BWD: mean[Np],rstd[Np] of that BN (centred sum t1*bhat)  */
  double* stats;         /* STATS: [C3D_STAT_STRIPES][2][N]; SWISH_SE_BWD: [B][Np][3]         */
                         /* (SWISH_SE_BWD, block-tiled kernel: a workgroup adds its rows in 2^-40 fixed point, so   */
                         /* the three sums over one workgroup's <= 64 rows of a sample must stay within +-8.4e6)    */
  int64_t M;             /* output rows                                                      */
  int64_t gstride;       /* C3D_ROWS_FRAME: elements between consecutive row groups          */
  int64_t rows_per_sample; /* output rows per batch sample (gate / per-sample sums)          */
  int32_t K, Kp, N, Np;
  int32_t w_sn, w_sk;
  int32_t row_mode, rpg;
  int32_t H, W;          /* STRIDE2: input H,W.  EPI_ADD res_mode 1: output H,W              */
  int32_t pro_mode, epi_mode;
  int32_t res_mode;      /* EPI_ADD: 0 dense [M][Np]; 1 e1 is [BT][H/2][W/2][Np], added where h,w even */
  int32_t dtype;
  c3d_bn_fin fin;        /* C3D_EPI_STATS: fin.ticket != NULL -> the last workgroup finalises the BatchNorm.      */
                         /* C3D_PRO_AFFINE2: fin.sums != NULL -> A|B|C are rebuilt from the completed single-   */
                         /* stripe sums f64 [2][K] (fin.gamma, fin.mr = mean|rstd, fin.count; workgroup 0 adds    */
                         /* dgamma / dbeta into fin.running_mean / fin.running_var and writes fin.ss if non-NULL) */
                         /* instead of read from pro_p (narrow kernel only: K, N <= 224, no bias).                */
  const float* bias;     /* optional bias[N] added before the epilogue (linear layers of the caption decoder)  */
  void* pro_out;         /* C3D_PRO_AFFINE2, dense rows, narrow kernel: relu(A*x + B + C*x2) is what enters the GEMM  */
                         /* AND is written here [M][Kp] (the residual add of the previous block fused into conv_a:    */
                         /* x = c, x2 = shortcut, fin.training = 1 + fin.sums = BatchNorm_c's 16-stripe sums, C = 1)  */
  const void* w_img;     /* optional: image of `w` made by c3d_pw_pack_weights for the same (N, Np, K, Kp, w_sn, w_sk,  */
                         /* dtype).  The narrow kernel then copies it into LDS (one 16-byte DMA per lane) instead of     */
                         /* converting and scattering the f32 weights in every workgroup; same results bit for bit.     */
                         /* `w` must still be given (the block-tiled kernel reads it).                                  */
  /* ---- weight gradient fused into the DATA-gradient launch (round 4; reference model/x3d.py:173-175,214-216: autograd's
   * convolution_backward produces both gradients of a 1x1x1 convolution from one read of its operands).  For a data-gradient
   * call (x = dY-side tensor with the C3D_PRO_AFFINE2 prologue, w addressed transposed) the kernel ALSO accumulates
   *     dW[k][n] += sum_m P(m, k) * Q(m, n),   P = prologue(x, x2) (the rows already staged for the GEMM),
   *     wg_mode C3D_WG_SWISH : Q = swish(bn(e1) * gate), the forward operand the C3D_EPI_SWISH_SE_BWD epilogue rebuilds anyway
   *     wg_mode C3D_WG_ROWS  : Q = rows of wg_x3 ([M][Np] dense, storage dtype: the layer's forward input)
   * into dw[n*w_sn + k*w_sk] (the strides of `w`): per-workgroup partial sums go to wg_ws (f32, at least
   * c3d_pw_gemm_wg_ws_floats(K, N) elements) and a fixed-order reducer launched behind the kernel on the same stream adds them
   * to wg_dw.  Narrow bf16 kernel, dense rows, Kp <= 112 and Np <= 112 only (C3D_E_UNSUPPORTED otherwise: callers keep
   * c3d_pw_wgrad for those).  wg_mode 0 (the zero-initialised default): no weight gradient.                            */
  const void* wg_x3;
  float* wg_dw;
  float* wg_ws;
  int32_t wg_mode;
  int32_t wg_mask_out;   /* C3D_WG_ROWS with C3D_EPI_ADD: 1 = the stored output is dx * (wg_x3 > 0) -- the ReLU mask of the PREVIOUS   */
                         /* block's output (wg_x3 is that output), i.e. the g = dy * (y > 0) of c3d_block_out_bwd, which then */
                         /* only has to produce the BatchNorm-backward sums (its y = g = NULL form)                          */
  /* ---- SqueezeExcitation gate computed by the CONSUMER (round 4): with C3D_PRO_BN_SE_SWISH, fin.sums (per-sample sums of
   * c3d_dw333_fwd, fin.batch > 0) and se_w1 != NULL, every workgroup of the narrow kernel rebuilds BatchNorm_b's scale / shift
   * AND the SE gate of the samples its rows belong to (z = bn(mean_n), FC1 + ReLU, FC2 + sigmoid: the arithmetic and summation
   * order of c3d_bn_se_finalize, bit-identical) in its prologue -- no c3d_bn_se_finalize launch between conv_b and conv_c.  The
   * workgroup that holds a sample's first row writes gate[n][Kp] (-> pro_gate, which must be given: the backward pass reads it)
   * and se_hid[n][Cr].  When a workgroup would span more than 4 samples (tiny inputs) the entry point launches
   * c3d_bn_se_finalize itself and runs the unfused form.  Reference: fvcore SqueezeExcitation at model/x3d.py:194-202.      */
  const float* se_w1; const float* se_b1; const float* se_w2; const float* se_b2;
  float* se_hid;
  int32_t se_cr;
  int32_t se_reserved;
  /* ---- c3d_block_out_bwd of the PREVIOUS block fused into this data-gradient launch (round 5; reference model/x3d.py:
   * 229-236: y = relu(bn_c(c) + shortcut), whose backward is one masked pass over dy in autograd).  With C3D_EPI_ADD, dense
   * rows, bf16 and wg_x3 = that block's output y:
   *     wg_mode C3D_WG_ROWS + wg_mask_out, or wg_mode C3D_WG_MASKSUM (no weight gradient; any Kp <= 224, Np <= 112):
   *     the stored output is g = (result + e1) * (wg_x3 > 0), and with add_sums != NULL (required by C3D_WG_MASKSUM) the
   *     kernel also accumulates that block's BatchNorm_c-backward sums  add_sums f64 [2][N] += (sum g, sum g * chat),
   *     chat = (add_c - mean) * rstd, add_c = its conv_c output [M][Np], add_mr = mean[Np] | rstd[Np] -- the sums of
   *     c3d_block_out_bwd (g as stored, i.e. rounded to the storage type), which is then not launched at all.            */
  const void* add_c;
  const float* add_mr;
  double* add_sums;
} c3d_pw_args;
#define C3D_WG_NONE 0
#define C3D_WG_SWISH 1
#define C3D_WG_ROWS 2
#define C3D_WG_MASKSUM 3
int64_t c3d_pw_gemm_wg_ws_floats(int32_t K, int32_t N);

/* K, N <= 224 run the wave-private-tile kernel (pw_gemm_impl.h); wider layers (X3D res5: 432 inner channels; the
 * caption decoder's 192 -> 576 / vocabulary projections) or a non-NULL bias run the block-tiled kernel of
 * pw_wide.hip with the same prologues / epilogues (row modes DENSE and STRIDE2; no in-kernel finalisation).
 * The wave-private-tile kernels address rows through bounds-checked buffer resources with 32-bit byte offsets: a call
 * whose largest operand (M * max(Kp, Np) elements) reaches 2 GiB returns C3D_E_UNSUPPORTED. */
int c3d_pw_gemm(const c3d_pw_args* args, void* stream);

/* Weight images for c3d_pw_args.w_img: the narrow kernel's LDS operand layout (f32: [NT*16][Kpad+pad]; bf16: 8-element
 * k-chunk major [Kpad/8 + 1][NT*16][8], the bank-conflict-free form for ds_read_b128 A fragments; zero padded; opaque to callers) written once per weight VERSION instead of rebuilt by each of the ~256 workgroups of each launch
 * (the f32 master weights change once per optimizer step; a block's four GEMMs per step read two weights, each in two
 * orientations).  c3d_pw_weight_image_bytes returns 0 for shapes the narrow kernel does not take (Kp or Np > 224).
 * One launch packs up to C3D_PW_PACK_MAX images (descriptors travel as kernel arguments). */
typedef struct c3d_pw_pack_desc {
  const float* w;        /* element (n,k) at w[n*w_sn + k*w_sk] */
  void* img;             /* c3d_pw_weight_image_bytes(Np, Kp, dtype) bytes, 16-byte aligned */
  int32_t N, Np, K, Kp, w_sn, w_sk;
} c3d_pw_pack_desc;
#define C3D_PW_PACK_MAX 64
int64_t c3d_pw_weight_image_bytes(int32_t Np, int32_t Kp, int32_t dtype);
int c3d_pw_pack_weights(const c3d_pw_pack_desc* descs, int32_t n, int32_t dtype, void* stream);

/* Weight gradient of the same family:
 *     dW[n, k] += sum_m P(m, n) * Q(m, k),  P = prologue_p(p, p2),  Q = prologue_q(q)
 * (replaces the weight half of aten::convolution_backward for the k=1 convs above).
 * `ws` is an f32 workspace of at least c3d_pw_wgrad_ws_floats(N,K) elements.             */
typedef struct c3d_pw_wgrad_args {
  const void* p;  const void* p2;   /* dY-side operand ([M][Np] dense) + AFFINE2 companion   */
  const void* q;                    /* X-side operand, rows of Kp elements (row_mode applies)*/
  float* dw;                        /* element (n,k) accumulated at dw[n*dw_sn + k*dw_sk]    */
  float* ws;
  const float* p_coef;              /* AFFINE2 A,B,C [Np] each, or NULL (plain p)            */
  const float* q_ss;                /* BN_SE_SWISH scale,shift [Kp] each, or NULL            */
  const float* q_gate;              /* gate[B][Kp] or NULL                                   */
  int64_t M;
  int64_t gstride;
  int64_t rows_per_sample;
  int32_t K, Kp, N, Np;
  int32_t dw_sn, dw_sk;
  int32_t row_mode, rpg, H, W;      /* addressing of q (p is always dense)                   */
  int32_t dy, dx;                   /* C3D_ROWS_S2SHIFT: row m=(b,i,j) reads pixel (2i+dy, 2j+dx) */
  int32_t q_mode;                   /* C3D_PRO_NONE | C3D_PRO_BN_SE_SWISH                    */
  int32_t dtype;
  int32_t taps;                     /* C3D_ROWS_S2SHIFT: 16 = ONE launch covers the 4x4 taps of a ConvTranspose2d   */
  int32_t dw_tap_stride;            /* k4s2p1 weight gradient, (dy,dx) = (tap/4-1, tap%4-1), tap t accumulates at   */
                                    /* dw + t*dw_tap_stride (reference model/change_decoder.py:30-45); 0/1 = dy,dx */
  c3d_bn_fin p_fin;                 /* p_fin.sums != NULL: the AFFINE2 coefficients are rebuilt from the completed   */
                                    /* single-stripe sums (gamma, mr, count as in c3d_bn_bwd_coef) instead of p_coef  */
  int32_t chain;                    /* 1: the per-workgroup partials of this launch may stay PENDING in `ws` -- the next */
  int32_t reserved_;                /* chained launch on the same stream adds them into dw in its prologue (same fixed  */
                                    /* order as the reducer launch it replaces: bit-identical dw), c3d_pw_wgrad_flush    */
                                    /* completes the last one.  The caller alternates between two `ws` buffers and does  */
                                    /* not touch a pending `ws` / read `dw` before the flush.  0 (default): dw is        */
                                    /* complete, in stream order, when c3d_pw_wgrad returns                              */
} c3d_pw_wgrad_args;

int64_t c3d_pw_wgrad_ws_floats(int32_t N, int32_t K);
int c3d_pw_wgrad(const c3d_pw_wgrad_args* args, void* stream);
/* Adds the pending partials of this thread's last chained c3d_pw_wgrad launch (if any) into its dw, on `stream` (the stream of
 * that launch).  The stage driver calls it at the end of c3d_stage_bwd; a no-op when nothing is pending.  c3d_pw_wgrad itself
 * adds them first whenever a launch, chained or not, is about to write the `ws` they sit in.                                 */
int c3d_pw_wgrad_flush(void* stream);

/* ------------------------------------------------------------------------------------
 * Train-mode BatchNorm3d split (reference model/x3d.py:97,179,207,220,298): statistics are
 * accumulated by producer epilogues, finalised here, applied by consumer prologues.
 *   sums : f64 [stripes][2][C] (sum, sumsq), summed over the stripes;   ss : f32 scale[Cp], shift[Cp];   mr : f32 mean[Cp], rstd[Cp]
 * training=0 builds scale/shift from the running statistics (eval mode); c3d_bn_se_finalize also accepts
 * training=2: scale/shift are GIVEN in ss (BatchNorm already folded into the weights), only the SE gate is computed.
 * ------------------------------------------------------------------------------------ */
int c3d_bn_finalize(const double* sums, int32_t stripes, double count, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, int64_t* num_batches_tracked,
                    float momentum, float eps, int32_t C, int32_t Cp, int32_t training, float* ss,
                    float* mr, void* stream);
/* BN_b + SqueezeExcitation (fvcore SqueezeExcitation called at reference model/x3d.py:194-202):
 * nc is f64 [B][Cp][2] per-(sample,channel) sum / sumsq from c3d_dw333_fwd; gate is f32 [B][Cp];
 * hid is f32 [B][Cr] (saved ReLU output of the first FC).  w1 == NULL -> block without SE.  */
int c3d_bn_se_finalize(const double* nc, int32_t B, double cnt_per_sample, const float* gamma,
                       const float* beta, float* running_mean, float* running_var,
                       int64_t* num_batches_tracked, float momentum, float eps, int32_t C, int32_t Cp,
                       int32_t training, const float* w1, const float* b1, const float* w2,
                       const float* b2, int32_t Cr, float* ss, float* mr, float* gate, float* hid,
                       void* stream);
/* BatchNorm backward as an affine map dx = A*g + B + C*x: dsums f64 [stripes][2][C] = (sum g, sum g*xhat),
 * xhat = (x-mean)*rstd accumulated centred by the producer;
 * coef f32 A[Cp],B[Cp],C[Cp]; dgamma/dbeta are accumulated (+=).                            */
int c3d_bn_bwd_coef(const double* dsums, int32_t stripes, double count, const float* gamma, const float* mr, int32_t C,
                    int32_t Cp, float* coef, float* dgamma, float* dbeta, void* stream);
/* SE backward + BN_b backward: nc3 f64 [B][Cp][3] from C3D_EPI_SWISH_SE_BWD, ncf = forward nc.
 * db = coefA[c]*t1 + coefB[n][c] + coefC[c]*b.  FC / BN parameter gradients accumulated (+=). */
int c3d_se_bn_bwd_coef(const double* nc3, const double* ncf, int32_t B, double cnt_per_sample,
                       const float* gamma, const float* mr, const float* ss, int32_t C, int32_t Cp,
                       const float* w1, const float* w2, const float* gate, const float* hid, int32_t Cr,
                       float* coefA, float* coefC, float* coefB, float* dgamma, float* dbeta,
                       float* dw1, float* db1, float* dw2, float* db2, void* stream);

/* ------------------------------------------------------------------------------------
 * Depthwise 3x3x3 Conv3d, stride (1,s,s) (conv_b, reference model/x3d.py:184-193).
 *   fwd      : x = a (raw conv_a output) with BN_a+ReLU applied on load (ss = scale/shift);
 *              y = b raw; nc_sums f64 [B][Cp][2] accumulated (+=).
 *   bwd_data : db = coefA*t1 + coefB[n] + coefC*b on load -> t2 = dconv*(bn_a(a)>0);
 *              dsums f64 [2][C] += (sum t2, sum t2*ahat), ahat = (a-mean_a)*rstd_a (mr_a).
 *   wgrad    : dw f32 [C][27] += sum db * relu(bn_a(a)).
 * ------------------------------------------------------------------------------------ */
int c3d_dw333_fwd(const void* x, const float* ss, const float* w, void* y, double* nc_sums, int32_t B,
                  int32_t T, int32_t H, int32_t W, int32_t C, int32_t Cp, int32_t stride, int32_t dtype,
                  void* stream);
/* Same, with the BatchNorm finalisation of the INPUT statistics folded in (no c3d_bn_finalize launch between the
 * producer of `fin->sums` and this kernel): bit-identical scale/shift, running statistics and saved vectors.  Shapes
 * without a folded kernel (stride 2) run c3d_bn_finalize + c3d_dw333_fwd internally.                              */
int c3d_dw333_fwd_fin(const void* x, const c3d_bn_fin* fin, const float* w, void* y, double* nc_sums, int32_t B,
                      int32_t T, int32_t H, int32_t W, int32_t C, int32_t Cp, int32_t stride, int32_t dtype,
                      void* stream);
/* bwd_data AND wgrad from one staged tile of db (csrc/dw_bwd_fused.hip) -- what autograd's convolution_backward returns
 * for conv_b (reference model/x3d.py:184-193) in one pass over t1, b and a: t2 = d conv * (bn_a(a) > 0), dsums f64 [2][C] =
 * (sum t2, sum t2 * ahat), dw += (f32 atomics).  stride 1 or 2, any extents.                      */
int c3d_dw333_bwd_fused(const void* t1, const void* b, const float* coefA, const float* coefB,
                        const float* coefC, const float* w, const void* a, const float* ss_a,
                        const float* mr_a, void* t2, double* dsums, float* dw, int32_t B, int32_t T,
                        int32_t H, int32_t W, int32_t C, int32_t Cp, int32_t stride, int32_t dtype, void* stream);
/* Same, with the BatchNorm_b backward coefficients of a block WITHOUT SqueezeExcitation rebuilt in the kernel's prologue
 * from the per-sample sums nc3 (fin_b->sums, fin_b->batch = B, fin_b->gamma, fin_b->mr = mean|rstd of BatchNorm_b,
 * fin_b->count = B*T*Ho*Wo; dgamma / dbeta += through fin_b->running_mean / running_var): no c3d_se_bn_bwd_coef launch
 * between the conv_c data gradient and this kernel.                                                                  */
int c3d_dw333_bwd_fused_fin(const void* t1, const void* b, const c3d_bn_fin* fin_b, const float* w, const void* a,
                            const float* ss_a, const float* mr_a, void* t2, double* dsums, float* dw, int32_t B,
                            int32_t T, int32_t H, int32_t W, int32_t C, int32_t Cp, int32_t stride, int32_t dtype,
                            void* stream);

/* ------------------------------------------------------------------------------------
 * Res-block output y = relu(bn_c(c) + shortcut) (reference model/x3d.py:326-327; also the
 * stem's BN+ReLU with sc_mode 0) and its backward g = dy*(y>0) with BN-backward sums.
 * sc_mode: 0 none, 1 identity, 2 shortcut*scale1+shift1 (branch1_norm), 3 raw shortcut.
 * ------------------------------------------------------------------------------------ */
int c3d_block_out_fwd(const void* c, const float* ss_c, const void* shortcut, const float* ss_1,
                      int32_t sc_mode, void* y, int64_t M, int32_t Cp, int32_t dtype, void* stream);
/* Same with BN_c (and, for sc_mode BN, the shortcut BatchNorm) finalised from their sums by the kernel itself;
 * C = real channel count.  fin_1 is NULL unless sc_mode is BN.                                                     */
int c3d_block_out_fwd_fin(const void* c, const c3d_bn_fin* fin_c, const void* shortcut, const c3d_bn_fin* fin_1,
                          int32_t sc_mode, void* y, int64_t M, int32_t C, int32_t Cp, int32_t dtype, void* stream);
/* y == NULL and g == NULL: `dy` already IS dy * (y > 0) (masked by its producer, c3d_pw_args.wg_mask_out): only the sums.
 * mr_c / mr_1 (mean | rstd rows, Cp floats each) must be 16-byte aligned (C3D_E_BADARG otherwise). */
int c3d_block_out_bwd(const void* dy, const void* y, const void* c, const void* s_bn, void* g,
                      const float* mr_c, const float* mr_1, double* dsums_c, double* dsums_1, int64_t M,
                      int32_t C, int32_t Cp, int32_t dtype, void* stream);
/* as c3d_block_out_bwd; with fin_c->ticket != NULL the last workgroup also writes the backward coefficients of
 * BatchNorm_c (fin_c) and, when s_bn is given, of the shortcut BatchNorm (fin_1; shares fin_c's ticket). */
int c3d_block_out_bwd_fin(const void* dy, const void* y, const void* c, const void* s_bn, void* g,
                          const float* mr_c, const float* mr_1, double* dsums_c, double* dsums_1, int64_t M,
                          int32_t C, int32_t Cp, int32_t dtype, const c3d_bn_fin* fin_c, const c3d_bn_fin* fin_1,
                          void* stream);

/* Encoder.enhance pieces (reference model/trainer.py:71-108); HW = H*W pixels per frame.    */
int c3d_frame_absdiff(const void* y, void* d, int32_t B, int32_t T, int64_t HW, int32_t Cp, int32_t t_pre,
                      int32_t t_post, int32_t dtype, void* stream);
int c3d_enhance_apply(const void* y, const void* e, void* out, int32_t B, int32_t T, int64_t HW,
                      int32_t Cp, int32_t t_mid, int32_t dtype, void* stream);
int c3d_enhance_bwd_mask(const void* dout, const void* e, void* de, int32_t B, int32_t T, int64_t HW,
                         int32_t Cp, int32_t t_mid, int32_t dtype, void* stream);
/* t_pre and t_post both outside [0, T): no frame matches, dy = dout.  One inside and one outside: C3D_E_BADARG. */
int c3d_enhance_bwd_apply(const void* dout, const void* y, const void* dd, void* dy, int32_t B, int32_t T,
                          int64_t HW, int32_t Cp, int32_t t_pre, int32_t t_post, int32_t dtype,
                          void* stream);
/* Stem output + enhance without a materialised y = relu(bn(u)) (the stem has no shortcut: y is recomputed on load from
 * u and ss = scale[Cp] | shift[Cp], rounded to the storage type exactly as c3d_block_out_fwd stores it).
 *   c3d_stem_enhance_fwd : out[:, t] = y[:, t] for every t != t_mid;  d = |y[:, t_pre] - y[:, t_post]|  (dense [B*HW][Cp])
 *   c3d_stem_enhance_mid : out[:, t_mid] = y[:, t_mid] + relu(e)                 (after c3d_pw_gemm(d -> e))
 *   c3d_stem_enhance_bwd : c3d_block_out_bwd (no shortcut) on dy = c3d_enhance_bwd_apply(dout, y, dd), neither y nor dy
 *                          stored: g = dy * (y > 0), dsums[2][C] += (sum g, sum g * (u - mean) * rstd); mr = mean | rstd.
 * Results are bit-identical to the c3d_block_out_fwd / c3d_frame_absdiff / c3d_enhance_* / c3d_block_out_bwd sequence. */
int c3d_stem_enhance_fwd(const void* u, const float* ss, void* out, void* d, int32_t B, int32_t T, int64_t HW,
                         int32_t Cp, int32_t t_pre, int32_t t_post, int32_t t_mid, int32_t dtype, void* stream);
int c3d_stem_enhance_mid(const void* u, const float* ss, const void* e, void* out, int32_t B, int32_t T, int64_t HW,
                         int32_t Cp, int32_t t_mid, int32_t dtype, void* stream);
int c3d_stem_enhance_bwd(const void* dout, const void* u, const float* ss, const void* dd, const float* mr, void* g,
                         double* dsums, int32_t B, int32_t T, int64_t HW, int32_t C, int32_t Cp, int32_t t_pre,
                         int32_t t_post, int32_t dtype, void* stream);
int c3d_frame_scatter(const void* src, void* dst, int32_t B, int32_t T, int64_t HW, int32_t Cp,
                      int32_t t_dst, int32_t accumulate, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * Stem (reference model/x3d.py:70-106): x is the logical NCDHW f32 clip [B][3][T][H][W];
 * u is the raw channels-last output [B][T][H][W][24]; sums f64 [2][24] accumulated.
 * Backward: dv = conv_xy^T(du) with du = A*g0+B+C*u on load (coef f32 [3][24]); then
 * d w_t and the batch-summed input gradient of frames t_first..t_first+n_frames-1
 * (dP f32 [3][n_frames][H][W], the learnable perception frames, model/trainer.py:51-54;
 * with per_sample=1 dP is instead a full NCDHW gradient [B][3][T][H][W], written not summed).
 * ------------------------------------------------------------------------------------ */
int c3d_stem_fwd(const float* x, const float* w_t, const float* w_xy, void* u, double* sums, int32_t B,
                 int32_t T, int32_t H, int32_t W, int32_t dtype, void* stream);
int c3d_stem_bwd_dv(const float* x, const float* w_t, const float* w_xy, const void* g0, const void* u,
                    const float* coef, void* dv, float* dw_xy, int32_t B, int32_t T, int32_t H, int32_t W,
                    int32_t dtype, void* stream);
int c3d_stem_bwd_wx(const float* x, const float* w_t, const void* dv, float* dw_t, float* dP, int32_t B,
                    int32_t T, int32_t H, int32_t W, int32_t t_first, int32_t n_frames, int32_t per_sample,
                    int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * ChangeDecoder (reference model/change_decoder.py:30-55, 68-81).
 *   convT4s2_fwd : out[B][2h][2w][C] = bias + skip + ConvTranspose2d(k4,s2,p1)(in[B][h][w][C]);
 *                  skip is one frame of an NDHWC tensor (element batch stride skip_bstride).
 *   head3x3      : Conv2d 3x3 (24 -> NC, no bias) [+ sigmoid]; out / dout / prob are f32
 *                  NCHW [B][NC][H][W]; dw f32 [NC][24][3][3] accumulated.
 * ------------------------------------------------------------------------------------ */
int c3d_convT4s2_fwd(const void* in, const float* w, const float* bias, const void* skip,
                     int64_t skip_bstride, void* out, int32_t B, int32_t h, int32_t wd, int32_t C,
                     int32_t dtype, void* stream);
int c3d_convT4s2_bwd_data(const void* dout, const float* w, void* din, int32_t B, int32_t h, int32_t wd,
                          int32_t C, int32_t dtype, void* stream);
/* weight gradient of the transposed convolution on MFMA (bf16 storage, C = 24 | 48): dw[ci][co][ky][kx] +=
 * sum t[b,i,j,ci] * dout[b,2i-1+ky,2j-1+kx,co]; t is the layer input [B][h][wd][C], dout its output gradient
 * [B][2h][2wd][C]; ws: f32 scratch of c3d_convT4s2_wgrad_ws_floats elements.  (f32 storage uses c3d_pw_wgrad with
 * C3D_ROWS_S2SHIFT / taps = 16; this entry returns C3D_E_UNSUPPORTED for it.)                               */
int64_t c3d_convT4s2_wgrad_ws_floats(int32_t B, int32_t h, int32_t wd, int32_t C);
int c3d_convT4s2_wgrad(const void* t, const void* dout, float* dw, float* ws, int32_t B, int32_t h, int32_t wd,
                       int32_t C, int32_t dtype, void* stream);
int c3d_col_sum(const void* x, float* out, int64_t M, int32_t C, int32_t Cp, int32_t dtype, void* stream);
int c3d_head3x3_fwd(const void* x, const float* w, float* out, int32_t B, int32_t H, int32_t W, int32_t C,
                    int32_t NC, int32_t has_sigmoid, int32_t dtype, void* stream);
/* ws: optional f32 scratch of c3d_head3x3_bwd_ws_floats elements for the bf16 matrix-core kernel (per-workgroup partials of dw +
 * fixed-order reducer); NULL: every workgroup adds its partial with global atomics (~1000 of them queue on the same 216 NC
 * addresses: 3-4 x slower on the full-size heads).                                                                          */
int64_t c3d_head3x3_bwd_ws_floats(int32_t B, int32_t H, int32_t W, int32_t NC);
int c3d_head3x3_bwd(const float* dout, const float* prob, const void* x, const float* w, void* dx,
                    float* dw, float* ws, int32_t B, int32_t H, int32_t W, int32_t C, int32_t NC, int32_t has_sigmoid,
                    int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * Train-step shell: BCEDiceLoss (reference model/utils.py:154-169), Adam
 * (reference scripts/train_BCD.py:284-290), thresholded confusion matrix
 * (reference scripts/train_BCD.py:204-208, utils/metric_tool.py:111-128).
 * sums4 f64 [4] = (sum bce terms, sum p*t, sum p, sum t).  hparams_dev (optional, f32 [3] =
 * lr, bias_correction1, sqrt(bias_correction2)) overrides the by-value scalars so a captured
 * HIP graph can be replayed with a new learning rate.
 * ------------------------------------------------------------------------------------ */
int c3d_bce_dice_fwd(const float* prob, const float* target, int64_t n, double* sums4, float* loss,
                     void* stream);
int c3d_bce_dice_bwd(const float* prob, const float* target, const double* sums4, const float* dloss,
                     int64_t n, float* dprob, void* stream);
int c3d_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  const float* hparams_dev, float lr, float bias_correction1, float bias_correction2_sqrt,
                  float beta1, float beta2, float eps, float weight_decay, void* stream);
int c3d_confusion2(const float* prob, const float* target, int64_t n, unsigned long long* cm4, void* stream);
/* SCD validation (reference scripts/train_SCD.py:104-178, model/utils.py:313-378 fast_hist / get_hist / SCDD_eval_all):
 * hist[a*n + b] += #{i : a[i] == a, b[i] == b} for 0 <= a < n (a = prediction, b = label; int64 device arrays), n <= 16;
 * hist has n*n + 1 u64 slots, the last one counts pairs whose b is outside [0, n) (numpy would raise there).        */
int c3d_hist2d(const int64_t* a, const int64_t* b, int64_t n_elems, int32_t n, unsigned long long* hist, void* stream);
/* BDA validation (reference scripts/train_BDA.py:102-143 `val`: `pred_loc.cpu().numpy() > 0.5`, `torch.argmax(pred_cls,
 * dim=1).cpu().numpy()`, `[label_loc > 0]`, model/utils.py:466-475 Evaluator._generate_matrix / add_batch, twice per
 * iteration): pred_cls f32 [B][n][HW] logits, pred_loc f32 [B][1][HW] probabilities, label_loc f32 [B][HW], label_cls int64
 * [B][HW], all contiguous; n <= 16.  counts (u64 [4 + n*n + 1], device, ACCUMULATED into):
 *   [2*gt + pred]     localisation matrix, pred = pred_loc > 0.5 (strict);
 *   [4 + n*gt + pred] damage matrix of argmax (first maximum wins) over the pixels with label_loc > 0;
 *   [4 + n*n]         labels outside [0, 2) / [0, n), which the reference's Evaluator drops silently.                 */
int c3d_bda_confusion(const float* pred_cls, const float* pred_loc, const float* label_loc, const int64_t* label_cls, int64_t B,
                      int32_t n, int64_t HW, unsigned long long* counts, void* stream);

/* ---------------------------------------------------------------------------------------
 * SCD losses.  Logits are f32 NCHW views: element (b, c, p) at
 * x[b*bstride + c*cstride + p], p < HW, NC <= 8 classes; labels are int64 [B][HW].
 *   c3d_ce2d_*   : CrossEntropyLoss2d(ignore_index) = nll_loss(log_softmax(x, 1), target, 'mean' over the
 *                  non-ignored pixels) (reference model/utils.py:171-178; used with ignore_index=0 at
 *                  scripts/train_SCD.py:226).  sums2 = (sum nll, count), zeroed by the call.
 *   c3d_cossim_* : ChangeSimilarity = cosine_embedding_loss(softmax(x1), softmax(x2), +1 where
 *                  label_change == 0 / -1 elsewhere, margin 0, 'mean') (reference model/utils.py:180-203).
 * Backward writes dense [B][NC][HW] gradients scaled by dloss[0] (NULL = 1).
 * ------------------------------------------------------------------------------------ */
int c3d_ce2d_fwd(const float* logits, const int64_t* target, int64_t B, int32_t NC, int64_t HW, int64_t bstride,
                 int64_t cstride, int64_t ignore_index, double* sums2, float* loss, void* stream);
int c3d_ce2d_bwd(const float* logits, const int64_t* target, const double* sums2, const float* dloss, int64_t B,
                 int32_t NC, int64_t HW, int64_t bstride, int64_t cstride, int64_t ignore_index, float* dlogits,
                 void* stream);
int c3d_cossim_fwd(const float* x1, const float* x2, const int64_t* label_change, int64_t B, int32_t NC, int64_t HW,
                   int64_t bstride1, int64_t cstride1, int64_t bstride2, int64_t cstride2, double* sums1, float* loss,
                   void* stream);
int c3d_cossim_bwd(const float* x1, const float* x2, const int64_t* label_change, const float* dloss, int64_t B,
                   int32_t NC, int64_t HW, int64_t bstride1, int64_t cstride1, int64_t bstride2, int64_t cstride2,
                   float* dx1, float* dx2, void* stream);

/* ------------------------------------------------------------------------------------
 * On-device input pipeline of the BCD step (reference data/transforms.py:100-154: random_flip,
 * random_exchange, normalize, to_tensor as composed at scripts/train_BCD.py:262-270) over a raw uint8 batch
 * resident in HBM.  image6: u8 [B][H][W][6] (pre RGB | post RGB); label: u8 [B][H][W] or NULL;
 * flags: u8 [B][3] = (cv2.flip(.,0), cv2.flip(.,1), exchange pre/post) per sample, or NULL (no augmentation =
 * the validation transform); mean6 / std6: f32 [6] DEVICE vectors.  Outputs: pre, post f32 [B][3][H][W]
 * = ((u8/255) - mean)/std, bit-identical to the numpy arithmetic; label_out f32 [B][1][H][W] = ceil(u8/255).
 * ------------------------------------------------------------------------------------ */
/* The (B, 3, T = K+2, H, W) f32 clip the encoder feeds to the stem (reference model/trainer.py:155-162:
 * `torch.cat([x.unsqueeze(2), perception_frames.expand(B, ...), y.unsqueeze(2)], dim=2)`): frame 0 = pre [B][3][H][W],
 * frames 1..K = the learnable perception frames [3][K][H][W] shared by the batch, frame K+1 = post.  H*W % 4 == 0.  */
int c3d_build_clip(const float* pre, const float* post, const float* frames, float* clip, int32_t B, int32_t K,
                   int32_t H, int32_t W, void* stream);
int c3d_bcd_preprocess(const uint8_t* image6, const uint8_t* label, const uint8_t* flags, const float* mean6,
                       const float* std6, float* pre, float* post, float* label_out, int32_t B, int32_t H,
                       int32_t W, void* stream);
/* SCD labels (reference data/transforms.py:300-326, 341-357; scripts/train_SCD.py:207-213): label3 u8 [B][H][W][3] =
 * (pre classes, post classes, change), same flags as the image pass -> int64 [B][3][H][W]; an exchange swaps the two
 * class maps.  The SCD image goes through c3d_bcd_preprocess (same 6-channel arithmetic, label = NULL).             */
int c3d_scd_label_preprocess(const uint8_t* label3, const uint8_t* flags, int64_t* out, int32_t B, int32_t H, int32_t W,
                             void* stream);
/* BDA labels (reference data/transforms.py:502-526 BDATransforms.random_flip / random_exchange, :541-556 to_tensor;
 * scripts/train_BDA.py:194-195 `label[:, 0].float()`, `torch.prod(label, dim=1).long()`): label2 u8 [B][H][W][2] =
 * (localisation, damage class), flags u8 [B][3] as for the image pass (NULL = none) -> label_loc f32 [B][1][H][W],
 * label_cls int64 [B][H][W] = localisation x damage class (int64 product, as torch.prod of a uint8 tensor).  The two flips
 * apply; the exchange flag swaps the images only (BDATransforms.random_exchange leaves the label alone).  The BDA image
 * goes through c3d_bcd_preprocess (label = NULL).                                                                    */
int c3d_bda_label_preprocess(const uint8_t* label2, const uint8_t* flags, float* label_loc, int64_t* label_cls, int32_t B,
                             int32_t H, int32_t W, void* stream);
/* Change-captioning pairs (reference data/dataset.py:411-424, scripts/train_CC.py:466-469): img u8 [B][2][3][H][W] ->
 * pre, post f32 [B][3][H][W] = lut[channel][u8] (the host builds the 3 x 256 table with the reference's own arithmetic:
 * Normalize(FloatTensor(u8 / 255.))); swap u8 [B] or NULL exchanges the pair.  H*W % 4 == 0.                        */
int c3d_cc_preprocess(const uint8_t* img, const uint8_t* swap, const float* lut, float* pre, float* post, int32_t B,
                      int32_t H, int32_t W, void* stream);
/* File data sets: gather + the whole training transform chain of the BCD / SCD / BDA recipes (reference
 * data/transforms.py:166-207 and its two siblings: normalize -> scale -> random_crop_resize -> random_flip ->
 * random_exchange -> to_tensor) in one pass over a uint8 store that stays in HBM.
 *   store        u8 [N][Hs][Ws][6] (pre | post, HWC) at an even address; addressed with 64-bit offsets
 *   label_store  u8 [N][Hs][Ws][L], L = 1 (BCD) / 3 (SCD) / 2 (BDA); NULL with task = C3D_AUG_NONE
 *   table        i32 [B][8] DEVICE = (index, do_crop, x1, y1, flip0, flip1, exchange, reserved) per output sample; NULL =
 *                index b and no augmentation (the validation transform; needs B <= N).  The caller validates its host copy
 *                (0 <= index < N, 2 * x1 < W, 2 * y1 < H); the kernel clamps the index, the offsets and every source
 *                coordinate, so no table content can address memory outside the stores.
 *   mean6, std6  f32 [6] DEVICE vectors, as for c3d_bcd_preprocess
 * Outputs: pre, post f32 [B][3][H][W]; by task: BCD label_a = f32 [B][1][H][W] = ceil(u8 / 255); SCD label_a = int64
 * [B][3][H][W] (an exchange swaps the two class maps); BDA label_a = label_loc f32 [B][1][H][W], label_b = label_cls int64
 * [B][H][W] = loc x class (the exchange leaves both alone); label_b is NULL for the other tasks.
 * Source window: the whole Hs x Ws image (scale; the identity when Hs == H && Ws == W), or with do_crop
 * [y1 : H - y1, x1 : W - x1] of the image already scaled to H x W, resized back to H x W.  Images: cv2.INTER_LINEAR on the
 * normalised f32 image (coordinate (d + 0.5) * (src / dst) - 0.5, f32 floor and fraction, clamped with fraction 0 at the
 * borders, horizontal lerp on both rows, then vertical; fraction 0 copies the tap, so a zero table at the store's own size
 * reproduces the three plain passes bit for bit).  Labels: cv2.INTER_NEAREST with the exact quotient min(d * src / dst, src - 1).
 * With a table AND a store size other than H x W the reference resamples twice, and so does this entry: launch 1 scales
 * into `scratch` (f32 [2][B][3][H][W], required in that case only), launch 2 crops / flips / exchanges from it.  Every
 * other case is one launch.  W % 4 == 0 and Ws <= 1232 (C3D_E_UNSUPPORTED otherwise).                                  */
enum { C3D_AUG_NONE = 0, C3D_AUG_BCD = 1, C3D_AUG_SCD = 2, C3D_AUG_BDA = 3 };
int c3d_augment_gather(const uint8_t* store, const uint8_t* label_store, const int32_t* table, const float* mean6,
                       const float* std6, float* pre, float* post, void* label_a, void* label_b, float* scratch,
                       int32_t task, int32_t N, int32_t Hs, int32_t Ws, int32_t B, int32_t H, int32_t W, void* stream);

/* Whole-scene inference (change3d_amd/infer.py; the reference only validates on pre-cut crops): tile a uint8 scene pair that
 * stays in HBM, and put the per-tile predictions back together.  Per axis, for tile t and stride s (1 <= s <= t, t - s even;
 * C3D_E_BADARG otherwise): margin m = (t - s) / 2, n = ceil(extent / s) tiles, tile i starts at i*s - m, and k = ceil(t / s)
 * tile rows cover any scene row.  Coordinates outside the scene fold back as numpy's `reflect` does for ANY overhang
 * (period 2*(extent-1), extent 1 -> 0): a scene smaller than a tile or than the margin is legal.
 *   scene    u8 [Hs][Ws][6] (pre RGB | post RGB, the layout of c3d_bcd_preprocess) at an even address; any Ws; 64-bit offsets
 *   origins  i32 [n][2] DEVICE = (y, x) of each tile's first pixel, negative or overhanging as the geometry asks; every
 *            source coordinate is clamped after folding, so no table content can address memory outside the scene
 *   mean6, std6  f32 [6] DEVICE vectors, as for c3d_bcd_preprocess
 * Outputs: pre, post f32 [n][3][th][tw] = ((u8/255) - mean)/std, bit-identical to c3d_bcd_preprocess for a tile inside the
 * scene.  One launch.                                                                                                  */
int c3d_scene_gather(const uint8_t* scene, const int32_t* origins, const float* mean6, const float* std6, float* pre,
                     float* post, int32_t Hs, int32_t Ws, int32_t n, int32_t th, int32_t tw, void* stream);
/* The scene rows that became final with tile row `row`: [row*sy - my, (row+1)*sy - my) clipped to the scene, and for the last
 * tile row everything up to Hs (nothing follows it).  A margin of a stride or more can leave that range empty: 0 is returned
 * and nothing is launched.
 *   ring     f32 [ky][ncols][C][th][tw]: tile row r lives in slot r % ky; rows row-ky+1 .. row must be there.  ky * ncols * C *
 *            th * tw * 4 bytes must stay under 2 GiB (C3D_E_UNSUPPORTED); th, tw <= 4096
 *   wy, wx   f32 [th], [tw] DEVICE window vectors, every entry > 0; the weight of tile pixel (y, x) is wy[y] * wx[x]
 * Per pixel and channel: sum(w * p) / sum(w) over the covering tiles that exist (tile rows 0 .. row, every column), f32, in
 * a fixed order -- tile row ascending, then tile column ascending, one fused multiply-add per tap -- by one thread: no atomics,
 * two runs agree bit for bit.
 *   blend    f32 [C][Hs][Ws] or NULL
 *   cls      u8 [Hs][Ws] or NULL: C == 1: blend > 0.5 (the reference's binarisation); C > 1: argmax over channels, the lowest
 *            index on a tie (torch.argmax).  At least one of blend / cls is given.
 *   gate     u8 [Hs][Ws] or NULL: cls is multiplied by it where both are written -- the change mask over the two SCD class maps
 *            (reference scripts/train_SCD.py:148-154); its rows of this strip must have been stitched before on `stream`  */
int c3d_scene_stitch(const float* ring, const float* wy, const float* wx, float* blend, uint8_t* cls, const uint8_t* gate,
                     int32_t Hs, int32_t Ws, int32_t C, int32_t th, int32_t tw, int32_t sy, int32_t sx, int32_t row,
                     void* stream);

/* Test-time augmentation of whole-scene inference: every tile is predicted under a set of the eight flips and rotations of
 * the square, each view is undone on the output, and the results are averaged.  Views: a code v in 0..7 acts on a tile
 * A[th][tw] as  1. transpose if v & 4,  2. reverse the rows if v & 2,  3. reverse the columns if v & 1; in numpy
 *   V = A.swapaxes(-2, -1) if v & 4 else A;  V = V[..., ::-1, :] if v & 2 else V;  V = V[..., ::-1] if v & 1 else V
 * The inverse undoes the two reversals and then transposes; codes 5 and 6 (the quarter turns) are each other's inverse, every
 * other code is its own.  A view set is a bit mask over the codes (bit v = code v), its nv = popcount(view_mask) views are taken
 * in ascending code order: none = 0x01, hflip = 0x03, flips = 0x0f, d4 = 0xff.  C3D_E_BADARG for an empty mask, bits above 7,
 * or a transposing view (bits 4..7) with th != tw.
 *
 * c3d_scene_gather_views: the arguments of c3d_scene_gather; pre, post f32 [n * nv][3][th][tw], entry i * nv + j = view j of
 * exactly what c3d_scene_gather writes for tile i (same reflect fold, same 6 x 256 table, same values).  One launch: every
 * pixel of the scene is read once for all views; a transposing view goes through a 32 x 32 LDS block.                    */
enum { C3D_VIEWS_NONE = 0x01, C3D_VIEWS_HFLIP = 0x03, C3D_VIEWS_FLIPS = 0x0f, C3D_VIEWS_D4 = 0xff };
int c3d_scene_gather_views(const uint8_t* scene, const int32_t* origins, const float* mean6, const float* std6, float* pre,
                           float* post, int32_t Hs, int32_t Ws, int32_t n, int32_t th, int32_t tw, int32_t view_mask,
                           void* stream);
/* values f32 [cnt * nv][C][th][tw], the model's output for those entries in that order; dst f32 [cnt][C][th][tw], in
 * whole-scene inference the slot range ring[row % ky][col .. col + cnt) of c3d_scene_stitch's ring (the fold is the put):
 *   dst[i][c] = (V_v0^-1(values[i*nv + 0][c]) + V_v1^-1(values[i*nv + 1][c]) + ...) / (float)nv
 * plain f32 adds in ascending view order starting from the first view's value, one divide; every element is written once by
 * one thread, no atomics: two runs agree bit for bit, and view_mask == 1 copies `values` bit for bit.  One launch.          */
int c3d_scene_fold_views(const float* values, float* dst, int32_t cnt, int32_t C, int32_t th, int32_t tw, int32_t view_mask,
                         void* stream);

/* Objects of a scene map (csrc/scene_objects.hip): connected components of a u8 mask that stays in HBM, a minimum-area filter,
 * raster numbering and one table row per object.  Integer arithmetic and integer atomics only: every output is exact and two
 * runs agree bit for bit.  Nine launches and at most three memsets on `stream`, nothing is read back by the host; the
 * workspace is zeroed inside the call.  Inputs (device):
 *   mask      u8 [Hs][Ws], nonzero = foreground;  Hs * Ws < 2^31 (C3D_E_UNSUPPORTED beyond)
 *   cls_map   u8 [Hs][Ws] or NULL: the votes; a value >= n_cls is counted nowhere; 1 <= n_cls <= 16 as in c3d_bda_confusion
 *   score     f32 [Hs][Ws] or NULL
 *   connectivity 4 or 8;  min_area <= 1 keeps every component;  max_objects >= 1 rows of `table` (and of `hist`)
 * Outputs:
 *   labels    i32 [Hs][Ws]: 0 = background or a pixel of a removed component (fewer than min_area pixels); the kept ones are
 *             numbered 1 .. N in raster order of their first pixel (the smallest y*Ws + x), as scipy.ndimage.label numbers
 *   table     i32 [max_objects][8], row id-1 = (area, x0, y0, x1, y1, cls, first, score_q); rows past the last object are 0
 *               x0..y1  inclusive bounding box;  first = linear index of the first pixel
 *               cls     the class in [first_class, n_cls) with the most pixels of cls_map inside the object, the lowest index
 *                       on a tie; 0 when nobody votes or cls_map is NULL
 *               score_q (S + area/2) / area in integers, S = u64 sum over the object of
 *                       q = __float2uint_rn(fminf(fmaxf(p, 0), 1) * 65535.0f)  (NaN counts as 0); 0 when score is NULL
 *   hist      u32 [max_objects][n_cls] or NULL: the votes per object; untouched when cls_map is NULL
 *   object_cls u8 [Hs][Ws] or NULL: table[label-1].cls painted over the object, 0 elsewhere
 *   counts    i32 [2] = (N found, rows written = min(N, max_objects)).  Objects past max_objects keep their ids in `labels`,
 *             get object_cls 0 and are written nowhere else.  counts[0] = -1: a union-find walk reached its cap of Hs*Ws
 *             steps (parents only decrease, so this cannot happen; the cap keeps a corrupted workspace from spinning)
 *   ws        c3d_scene_label_ws_bytes(Hs, Ws, n_cls) bytes (n_cls = 1 without a class map), 256-byte aligned
 * Refused before anything is enqueued: connectivity other than 4 / 8, n_cls outside [1, 16] with a class map, max_objects <
 * 1, first_class < 0, a NULL mask / labels / table / counts / ws (C3D_E_BADARG); Hs * Ws >= 2^31 (C3D_E_UNSUPPORTED).  */
int64_t c3d_scene_label_ws_bytes(int32_t Hs, int32_t Ws, int32_t n_cls);      /* < 0: C3D_E_* */
/* extent of the LDS tile of the local labelling phase: scene sizes around its multiples are the ones to test */
int c3d_scene_label_tile(int32_t* th, int32_t* tw);
int c3d_scene_objects(const uint8_t* mask, const uint8_t* cls_map, const float* score, int32_t Hs, int32_t Ws,
                      int32_t connectivity, int32_t min_area, int32_t n_cls, int32_t first_class, int32_t max_objects,
                      int32_t* labels, int32_t* table, uint32_t* hist, uint8_t* object_cls, int32_t* counts, void* ws,
                      void* stream);

/* Objects of a prediction matched to the objects of a ground truth (csrc/objects_match.hip): the join of two c3d_scene_objects
 * results over the same Hs x Ws.  Every pixel with p = labels_p > 0 and g = labels_g > 0 adds 1 to the count of the exact
 * 64-bit key (p << 32) | g in an open-addressing table in `ws`; the pair (p, g, inter) matches iff
 * (double)inter > iou_thr * (double)union with union = area_p + area_g - inter, strictly, which for iou_thr >= 0.5 makes a
 * match unique on both sides.  One memset (the workspace) and four launches on `stream`; nothing is read back by the host, the
 * object counts are read from counts_p / counts_g on the device.  Integer arithmetic and integer atomics except sum_iou, which
 * one workgroup adds in a fixed order (ascending predicted id, 256 interleaved partial sums, then a fixed tree): two runs agree
 * bit for bit.  Inputs (device):
 *   labels_p, table_p, counts_p   labels i32 [Hs][Ws], table i32 [max_p][8] and counts i32 [2] of c3d_scene_objects on the
 *   labels_g, table_g, counts_g   prediction, and the same with max_g rows on the ground truth;  Hs * Ws < 2^31
 *   max_p, max_g   rows of table_p / table_g and of match_p / match_g (the max_objects of the two calls), >= 1.  The objects of
 *                  a side are its ids 1 .. rows, rows = counts[1] kept inside [0, max]; a label id above `rows` is treated as
 *                  background: its pixels are counted nowhere
 *   n_cls          1 <= n_cls <= 16: side of `conf`.  A table row's cls outside [0, n_cls) counts as class 0
 *   iou_thr        in [0.5, 1)
 *   table_capacity slots of the pair table: a power of two <= 2^32, as returned by c3d_objects_match_ws_bytes.  The capacity
 *                  that cannot overflow is the next power of two >= 2 * Hs * Ws (every pair owns at least one pixel, the table
 *                  is at most half full); a smaller one is legal and may set C3D_MATCH_ST_TABLE_FULL
 * Outputs:
 *   match_p   i32 [max_p][4], row id-1 = (partner id or 0, inter, union, covered); inter and union are 0 without a partner;
 *   match_g   i32 [max_g][4]  covered = pixels of the object inside ANY object of the other side.  Rows past the last object
 *             are 0, written by the call
 *   conf      i64 [n_cls][n_cls], row = ground-truth class, column = predicted class (table[..].cls): a matched pair counts at
 *             [cls_g][cls_p], a missed ground-truth object at [cls_g][0], a false alarm at [0][cls_p]; its sum is TP + FP + FN
 *   counts    i64 [6] = (pairs, TP, FP, FN, status, 0); FP = rows_p - TP, FN = rows_g - TP
 *   sum_iou   f64 [1] = sum over the matches of (double)inter / (double)union
 *   totals    i64 [5 + n_cls*n_cls] or NULL, total_iou f64 [1] or NULL: (TP, FP, FN, pairs) and conf are ADDED into
 *             totals[0..3] and totals[5..], status is OR-ed into totals[4], sum_iou is added to total_iou[0]; by one thread at
 *             the end of the last launch, so calls on one stream accumulate in stream order.  The caller zeroes them once
 *   ws        c3d_objects_match_ws_bytes(Hs, Ws, &table_capacity) = 256 + 12 * table_capacity bytes, 256-byte aligned
 * status bits (the call always ends, and writes nothing out of range):
 *   C3D_MATCH_ST_TABLE_FULL  an insert probed min(table_capacity, 4096) slots without finding its key or a free slot: its
 *                            pixels are missing.  That is also the worst case of an overflowing table: 4096 loads per dropped run
 *   C3D_MATCH_ST_TRUNCATED   counts_*[0] > counts_*[1] (objects past max_objects) or counts_*[1] > max_*: pixels of the ids
 *                            without a table row were counted nowhere
 *   C3D_MATCH_ST_BAD_COUNTS  counts_*[0] < 0 on either input (c3d_scene_objects reported an error)
 * Refused before anything is enqueued: a NULL pointer other than totals / total_iou / stream, Hs or Ws <= 0, n_cls outside
 * [1, 16], max_p < 1 or max_g < 1, iou_thr outside [0.5, 1) or NaN, a capacity that is no power of two in [1, 2^32]
 * (C3D_E_BADARG); Hs * Ws >= 2^31 (C3D_E_UNSUPPORTED).  c3d_objects_match_ws_bytes: *table_capacity in: 0 = the capacity that
 * cannot overflow for this scene, else a power of two, which is kept; out: the capacity used.  < 0: C3D_E_*.               */
#define C3D_MATCH_ST_TABLE_FULL 1
#define C3D_MATCH_ST_TRUNCATED 2
#define C3D_MATCH_ST_BAD_COUNTS 4
int64_t c3d_objects_match_ws_bytes(int32_t Hs, int32_t Ws, int64_t* table_capacity);
int c3d_objects_match(const int32_t* labels_p, const int32_t* table_p, const int32_t* counts_p, const int32_t* labels_g,
                      const int32_t* table_g, const int32_t* counts_g, int32_t Hs, int32_t Ws, int32_t max_p, int32_t max_g,
                      int32_t n_cls, double iou_thr, int64_t table_capacity, int32_t* match_p, int32_t* match_g, int64_t* conf,
                      int64_t* counts, double* sum_iou, int64_t* totals, double* total_iou, void* ws, void* stream);

/* Outlines of the objects of a scene map (csrc/scene_outlines.hip): the label map of c3d_scene_objects traced into closed
 * rectilinear polygon rings, one ring of positive area per object and one of negative area per hole, while it stays in HBM.
 * Integer arithmetic and integer atomics only: every output is exact and two runs agree bit for bit.  One memset and
 * 10 + ceil(log2(4 Hs Ws)) launches on `stream`, nothing is read back by the host, no workgroup waits for another; the call
 * zeroes what it needs of the workspace.  The definition:
 *   geometry    pixel (y, x) is the unit square [x, x+1] x [y, y+1]; vertices are lattice points (vx, vy), 0 <= vx <= Ws,
 *               0 <= vy <= Hs
 *   edges       a boundary edge of object `id` is a side of a pixel labelled id whose neighbour across that side has another
 *               label or lies outside the scene.  Pixels with a label <= 0 or above rows = clamp(counts_obj[1], 0,
 *               max_objects) own no edges
 *   direction   sides are numbered 0 top, 1 right, 2 bottom, 3 left and directed with the object on the right of travel in
 *               image coordinates (y down): top goes +x, right +y, bottom -x, left -y
 *   key         4 * (y * Ws + x) + side; Hs * Ws < 2^29 keeps it in i32 (C3D_E_UNSUPPORTED beyond)
 *   successor   the first existing boundary edge of the same id out of the edge's end vertex among: the right turn (the next
 *               side of the same pixel), straight on (the same side of the next pixel along the travel), the left turn (side
 *               (s+3)%4 of the diagonal pixel ahead on the outside).  connectivity 4 tries right, straight, left;
 *               connectivity 8 tries left, straight, right.  8-connected objects thus join across a diagonal and their holes
 *               split there, 4-connected objects split and their holes join: labelled with the same connectivity, every object
 *               has exactly one ring of positive area and one ring of negative area per hole.  A ring may touch itself at a
 *               vertex; it never crosses itself
 *   corners     a corner edge is one whose side differs from its predecessor's.  A ring's vertices are the start vertices of
 *               its corner edges in ring order, beginning at the corner edge with the smallest key (NOT the ring's smallest
 *               edge: the bottom side that a wide hole begins with is reached straight on and is no corner)
 *   order       rings ascend by that starting key over the whole scene; the rings of one object are not contiguous
 *   area        shoelace sum / 2 over the vertices: an integer, positive for outlines, negative for holes, fits i32
 *   perimeter   the number of unit edges of the ring
 * Inputs (device):
 *   labels, counts_obj   labels i32 [Hs][Ws] and counts i32 [2] of c3d_scene_objects;  max_objects as given to that call
 *   connectivity 4 or 8: the one the labels were made with
 * Outputs:
 *   rings     i32 [max_rings][8], 16-byte aligned, row r = (id, start, n_vertices, area, perimeter, x, y, 0): start = offset
 *             of the ring's first vertex in `vertices` = the vertices of all rings before it; (x, y) = that first vertex.
 *             Rows past the last written ring are 0, written by the call
 *   vertices  i32 [max_vertices][2] = (vx, vy), 8-byte aligned; rings contiguous, in ring order; neither the closing repeat of
 *             the first vertex nor a collinear vertex is stored.  Rows past counts[3] are left as they were
 *   counts    i32 [5] = (rings found, ring rows written, vertices found, vertices written, status)
 *   ws        c3d_scene_outlines_ws_bytes(Hs, Ws) bytes (about 133 per pixel: two buffers of 16 bytes for each of the 4 Hs Ws
 *             edges that some label map can own), 256-byte aligned
 * Truncation is prefix-shaped: ring rows are written for ring index < max_rings; a ring's vertices are written only if start +
 * n_vertices <= max_vertices, otherwise its row gets start = -1 and none of its vertices is written (so is every later ring's).
 * Nothing is ever written out of range.  status bits:
 *   C3D_OUTLINE_ST_TRUNCATED   found > written on either count, or counts_obj[0] > counts_obj[1]
 *   C3D_OUTLINE_ST_BAD_COUNTS  counts_obj[0] < 0 (c3d_scene_objects reported an error): nothing is traced, the counts are 0
 *   C3D_OUTLINE_ST_STEP_CAP    the fixed number of pointer-doubling rounds left a ring without an agreed start, or an index
 *                              derived from the workspace fell out of range (neither can happen: 2^rounds edges cover any ring;
 *                              the checks keep a corrupted workspace from being written through)
 * Refused before anything is enqueued: a NULL labels / counts_obj / rings / vertices / counts / ws, Hs or Ws <= 0, connectivity
 * other than 4 / 8, max_objects, max_rings or max_vertices < 1 (C3D_E_BADARG); Hs * Ws >= 2^29 (C3D_E_UNSUPPORTED).          */
#define C3D_OUTLINE_ST_TRUNCATED 1
#define C3D_OUTLINE_ST_BAD_COUNTS 2
#define C3D_OUTLINE_ST_STEP_CAP 4
int64_t c3d_scene_outlines_ws_bytes(int32_t Hs, int32_t Ws);            /* < 0: C3D_E_* */
int c3d_scene_outlines(const int32_t* labels, const int32_t* counts_obj, int32_t Hs, int32_t Ws, int32_t connectivity,
                       int32_t max_objects, int32_t max_rings, int32_t max_vertices, int32_t* rings, int32_t* vertices,
                       int32_t* counts, void* ws, void* stream);

/* Simplified polygons (csrc/scene_simplify.hip): Douglas-Peucker with a pixel tolerance on the ring table and vertex list of
 * c3d_scene_outlines while they stay in HBM, or on any table of that shape (rings may repeat a lattice point and may hold
 * collinear vertices).  Integer arithmetic only: floating point appears nowhere in a decision, every output is exact and two
 * runs agree bit for bit.  One memset and 6 launches on `stream`, nothing is read back by the host, no workgroup waits for
 * another: the rounds of the recursion run inside the kernels, one wave or one workgroup per ring.  The rule:
 *   tolerance   tol2_q = round(16 * tol * tol), sixteenths of a square pixel, 0 <= tol2_q <= C3D_SIMPLIFY_TOL2_Q_MAX
 *               (tol <= 1024).  Coordinates must lie in [0, 16384]; every quantity below then fits an unsigned 64-bit integer
 *   distance    a ring has the vertices v[0 .. n-1] in stored order, v[n] = v[0].  For a chord (a, b) and a vertex p let
 *               L2 = |b-a|^2, t = (p-a).(b-a), c = cross(b-a, p-a).  The squared distance of p to the SEGMENT is num / den:
 *                 L2 == 0     num = |p-a|^2        den = 1
 *                 t <= 0      num = |p-a|^2 * L2   den = L2
 *                 t >= L2     num = |p-b|^2 * L2   den = L2
 *                 otherwise   num = c * c          den = L2
 *               p is far iff 16 * num > tol2_q * den, strictly.  The vertices of one chord share den: the farthest has the
 *               largest num, the smallest index on ties
 *   per ring    n <= 3: copied.  Otherwise the anchors are A = 0 and B = the vertex with the largest |v[k]-v[0]|^2, smallest k
 *               on ties; the chains A..B and B..n are simplified by Douglas-Peucker: on a chord (i, j), j > i + 1, take the
 *               farthest interior vertex m; if m is far keep it and go on with (i, m) and (m, j), otherwise drop the whole
 *               interior.  If at most A and B survive, the vertex with the largest |cross(v[B]-v[A], v[k]-v[A])|, smallest k
 *               on ties, is kept too: a ring of non-zero area never falls under 3 vertices
 *   topology    none is promised: a simplified ring may touch or cross itself or its holes, as with any plain
 *               Douglas-Peucker.  Every dropped vertex lies within tol of the kept chord that spans it
 * Inputs (device): rings i32 [max_rings][8], vertices i32 [max_vertices][2], counts i32 [5] as c3d_scene_outlines writes them.
 * Rows r < clamp(counts[1], 0, max_rings) are read; vertex rows below clamp(counts[3], 0, max_vertices) may be named by them.
 * Like the outputs, `rings` must be 16-byte aligned and `vertices` 8-byte aligned: rows are loaded as vectors.
 * Outputs (must not alias the inputs):
 *   rings_out     i32 [max_rings][8], 16-byte aligned, same row order: (id, start', n', area2', perimeter, x, y, n): start'
 *                 and n' index vertices_out; area2' = the shoelace sum of the kept vertices = twice the signed area, an
 *                 integer that may be odd.  It is exact wherever it fits i32, which holds for every ring that does not wind
 *                 round the coordinate range several times (a traced ring never does); beyond that it is the sum modulo
 *                 2^32.  id, perimeter, x, y are copied; column 7 = the input's n_vertices.  Rows past the last are 0
 *   vertices_out  i32 [max_vertices][2], 8-byte aligned: the kept vertices, rings contiguous and in row order.  n' <= n, so
 *                 the input's written-vertex count always suffices.  Rows past counts_out[3] are left as they were
 *   counts_out    i32 [5] = (rings found, rows written, vertices kept, vertices written, status): kept == written; status =
 *                 the input's status with C3D_SIMPLIFY_ST_BAD_INPUT added where it applies
 *   ws            c3d_outlines_simplify_ws_bytes(max_rings, max_vertices) bytes (16 per ring row, 17 per vertex row),
 *                 256-byte aligned; the call zeroes what it needs of it
 * Rows that are not simplified get start' = -1, n' = 0, area2' = 0:
 *   start < 0                       a ring the outlines call had no room for: passed through, no new status bit
 *   out of range                    n < 0, start + n above the written vertices, a coordinate outside [0, 16384], or vertex
 *                                   ranges that overlap so far that the n of this and all earlier valid rows add up to more
 *                                   than max_vertices: C3D_SIMPLIFY_ST_BAD_INPUT.  Nothing is read or written out of range
 * Input status C3D_OUTLINE_ST_BAD_COUNTS: counts_out = (0, 0, 0, 0, C3D_OUTLINE_ST_BAD_COUNTS), all ring rows 0.
 * Refused before anything is enqueued (C3D_E_BADARG): a NULL pointer, max_rings or max_vertices < 1, tol2_q out of range.
 * c3d_outlines_simplify_limits: out[0] = the most vertices of a ring that one wave simplifies in registers, out[1] = the most
 * of a ring whose state one workgroup keeps in LDS; larger rings keep it in `ws`.  The results do not depend on the tier.      */
#define C3D_SIMPLIFY_ST_BAD_INPUT 8
#define C3D_SIMPLIFY_TOL2_Q_MAX (16ll * 1024 * 1024)
void c3d_outlines_simplify_limits(int32_t out[2]);
int64_t c3d_outlines_simplify_ws_bytes(int32_t max_rings, int32_t max_vertices);   /* < 0: C3D_E_* */
int c3d_outlines_simplify(const int32_t* rings, const int32_t* vertices, const int32_t* counts, int32_t max_rings,
                          int32_t max_vertices, int64_t tol2_q, int32_t* rings_out, int32_t* vertices_out, int32_t* counts_out,
                          void* ws, void* stream);

/* Polygon rings back to pixels (csrc/scene_fill.hip): the ring table and vertex list of c3d_scene_outlines or
 * c3d_outlines_simplify, or any table of that shape, filled into a label map and an object table while they stay in HBM.
 * Integer arithmetic only: floating point appears nowhere in a decision, every output is exact and two runs agree bit for bit.
 * Two memsets (the workspace header, the labels) and 8 launches on `stream`, nothing is read back by the host, no workgroup
 * waits for another, every loop is capped, and no workspace word is read before the call wrote it.  The rule:
 *   coordinates a vertex coordinate is an integer in units of 2^-f pixel, f = frac_bits in [0, 8], |coordinate| <= 32768 * 2^f.
 *               Pixel (y, x) is the square [x, x+1] x [y, y+1]; with s = 2^f and all coordinates doubled (X = 2 vx, Y = 2 vy)
 *               its centre is (Cx, Cy) = ((2x + 1) s, (2y + 1) s).  Every product below stays under 2^51
 *   crossing    a ring with the vertices v[0 .. n-1], closed by v[n] = v[0], has the edges (v[k-1], v[k]).  Rings with n < 3 and
 *               horizontal edges contribute nothing.  With an edge ordered so that Y0 < Y1 it is active on row y iff
 *               Y0 <= Cy < Y1, and it lies left of pixel (y, x) iff (Cx - X0) * (Y1 - Y0) > (X1 - X0) * (Cy - Y0), strictly
 *   inside      a pixel is inside object `id` iff the number of pairs (used ring of that id, active edge left of the pixel) is
 *               odd: even-odd over all rings of the id together.  Orientation does not matter, holes are further rings, a
 *               ring listed twice cancels itself, self-crossing rings follow even-odd.  The rings of one id need not be
 *               contiguous in the table
 *   label       labels[y][x] = the largest id the pixel is inside of, or 0: polygons that share an edge partition the pixels,
 *               overlapping ones are decided, not summed
 *   rows used   a row r < clamp(counts[1], 0, max_rings) with (id, start, n) = columns 0..2 (the others are ignored) is used iff
 *               start >= 0, n >= 0, start + n <= clamp(counts[3], 0, max_vertices), 1 <= id <= max_objects and every
 *               coordinate of the ring is in range.  A row with start < 0 (a ring the outlines call had no room for, or one
 *               the simplifier passed through) is skipped silently, whatever else it holds.  Any other skipped row sets
 *               C3D_FILL_ST_BAD_ID if its id is out of range, and C3D_FILL_ST_BAD_RING if its n is negative, its vertex range
 *               ends past the written vertices or -- where that range could be read -- a coordinate is out of range (a row
 *               may set both).  Nothing is read or written out of range
 * Inputs (device): rings i32 [max_rings][8], vertices i32 [max_vertices][2] (8-byte aligned), counts i32 [5];
 *   id_cls      u8 [max_objects] or NULL: the class of every id
 * Outputs:
 *   labels      i32 [Hs][Ws], 1 <= Hs, Ws <= 16384
 *   table       i32 [max_objects][8], 16-byte aligned, in the row format of c3d_scene_objects for the ids 1 .. K, K = the
 *               largest id of a used row: (area, x0, y0, x1, y1, cls, first, 0) with the inclusive box and first = the
 *               smallest linear index of the pixels labelled id, cls = id_cls[id-1], or 0 without id_cls.  An id that owns
 *               no pixel keeps a row of zeros except cls.  Rows past K are 0
 *   counts_obj  i32 [2] = (K, K): with labels and table, what c3d_objects_match takes
 *   mask        u8 [Hs][Ws] or NULL: labels > 0;   cls_map  u8 [Hs][Ws] or NULL: the table's cls painted over the object
 *   info        i32 [4] = (status, ring rows used, K, 0); status = counts[4] as it came, with the bits below added
 *   ws          c3d_rings_fill_ws_bytes(max_rings, max_vertices, max_objects, Hs, Ws) bytes, 256-byte aligned; a dirty one
 *               gives the same result
 * Input status C3D_OUTLINE_ST_BAD_COUNTS: labels, table, mask and cls_map all 0, counts_obj = (-1, 0), info = (counts[4], 0, 0, 0).
 * Refused before anything is enqueued: a NULL rings, vertices, counts, labels, table, counts_obj, info or ws, frac_bits outside
 * [0, 8], max_rings, max_vertices, max_objects, Hs or Ws < 1 (C3D_E_BADARG); Hs or Ws > 16384 (C3D_E_UNSUPPORTED).
 * c3d_rings_fill_limits: out[0] = the most rows and columns of an id's pixel box that one wave fills in registers, out[1] = the
 * rows of a band of a larger box, one workgroup each, bits in LDS.  The results do not depend on the tier.  Host only.       */
#define C3D_FILL_ST_BAD_ID 16
#define C3D_FILL_ST_BAD_RING 32
void c3d_rings_fill_limits(int32_t out[2]);
int64_t c3d_rings_fill_ws_bytes(int32_t max_rings, int32_t max_vertices, int32_t max_objects, int32_t Hs, int32_t Ws);   /* < 0: C3D_E_* */
int c3d_rings_fill(const int32_t* rings, const int32_t* vertices, const int32_t* counts, int32_t max_rings, int32_t max_vertices,
                   int32_t frac_bits, const uint8_t* id_cls, int32_t max_objects, int32_t Hs, int32_t Ws, int32_t* labels,
                   int32_t* table, int32_t* counts_obj, uint8_t* mask, uint8_t* cls_map, int32_t* info, void* ws, void* stream);

/* Convex hulls and minimum-area rectangles (csrc/scene_hull.hip): the ring table and vertex list of c3d_scene_outlines, or any
 * table of that shape with integer pixel corners (frac_bits 0), turned into the strictly convex hull and the oriented bounding
 * rectangle of every id while they stay in HBM.  Integer arithmetic only: floating point appears in no decision, every output
 * is exact and two runs agree bit for bit.  One memset and 9 launches on `stream`, nothing is read back by the host, no
 * workgroup waits for another, every loop is capped, and no workspace word is read before the call wrote it.  The rule:
 *   rows used   a row r < clamp(counts[1], 0, max_rings) with (id, start, n) = columns 0..2 (the others are ignored) is used iff
 *               start >= 0, n >= 0, start + n <= clamp(counts[3], 0, max_vertices), 1 <= id <= max_objects and every
 *               coordinate of the ring lies in [0, 16384].  A row with start < 0 is skipped silently; any other skipped row
 *               sets C3D_HULL_ST_BAD_ROW.  Nothing is read or written out of range.  K = the largest id of a used row
 *   points      the points of object `id` are all vertices of all used rows with that id: holes count and so do duplicates,
 *               this is a point set, not a polygon.  The rings of an id need not be contiguous in the table
 *   hull        the vertices of the strictly convex hull of the points: no vertex is collinear between its neighbours, a
 *               repeated point appears once.  With cross(a, b, c) = (b.x-a.x)(c.y-a.y) - (b.y-a.y)(c.x-a.x) it is stored as
 *               h[0 .. m-1]: h[0] = the point with the smallest (y, x); h[k+1] = the point q != h[k] for which
 *               cross(h[k], q, r) >= 0 holds for every point r, the farthest such q where several are collinear; the walk
 *               ends when it returns to h[0].  This is the direction the outlines are traced in (top goes +x, then +y):
 *               cross(h[k-1], h[k], h[k+1]) > 0 and the shoelace sum is positive.  m = 1 for a single point, 2 for collinear
 *               points
 *   rectangle   for m >= 3 and the hull edge k from P = h[k] to h[(k+1) % m]: d = the edge vector, L = |d|^2,
 *               t_j = (h[j]-P).d, c_j = cross(P, P+d, h[j]) >= 0.  The rectangle on that edge has the area
 *               (t_max - t_min) * c_max / L; the edge with the smallest area is chosen, the smallest k on ties.  Areas are
 *               compared exactly by cross-multiplication: t_max - t_min <= 2^30, c_max <= 2^29, L <= 2^29, so the products
 *               stay under 2^88 and the comparison is one of 128-bit integers.  The rectangle's corners are
 *               P + d t/L (+ n c_max/L) for t = t_min, t_max and n = (-d.y, d.x): rational, left to the caller
 * Inputs (device): rings i32 [max_rings][8], vertices i32 [max_vertices][2] (8-byte aligned), counts i32 [5].
 * Outputs:
 *   hulls          i32 [max_objects][8], 16-byte aligned.  Row id-1 for id <= K = (id, start, m, area2, 0, x, y, n_points):
 *                  start = the offset into hull_vertices = the m of all smaller ids; area2 = the shoelace sum of the hull,
 *                  twice its area, below 2^30; (x, y) = h[0]; n_points = the vertex rows of the id's used rings (INT32_MAX
 *                  where rows that share vertices add up to more).  An id without points gets (id, -1, 0, 0, 0, 0, 0, 0).
 *                  Rows past K are 0.  Columns 0..2 make this a ring table that c3d_rings_fill and c3d_outlines_simplify
 *                  accept as it is
 *   hull_vertices  i32 [max_hull_vertices][2], 8-byte aligned: the hulls, contiguous, in id order.  Rows past counts_out[3]
 *                  are left as they were
 *   rects          i64 [max_objects][8].  Row id-1 = (k, L, t_min, t_max, c_max, j_tmin, j_tmax, j_cmax) for the chosen edge,
 *                  the j being the smallest hull indices that attain the extremes; (-1, 0, ...) for m < 3.  Rows past K are 0
 *   counts_out     i32 [5] = (ids with points, K, hull vertices found, hull vertices written, status); status = counts[4] as
 *                  it came, with the bits below added
 *   ws             c3d_rings_hull_ws_bytes(max_rings, max_vertices, max_objects) bytes (5 per ring row, 4 per vertex row, 28
 *                  per id), 256-byte aligned; a dirty one gives the same result
 * Truncation is prefix-shaped as in c3d_scene_outlines: an id whose hull does not fit below max_hull_vertices gets start = -1
 * and none of its vertices is written, and so does every later id; the other columns and the rects rows stay correct;
 * C3D_HULL_ST_TRUNCATED is set.  max_hull_vertices >= the vertices written by the outlines call never truncates.
 * Input status C3D_OUTLINE_ST_BAD_COUNTS: all rows 0, counts_out = (0, 0, 0, 0, C3D_OUTLINE_ST_BAD_COUNTS).
 * Refused before anything is enqueued (C3D_E_BADARG): a NULL pointer, max_rings, max_vertices, max_objects or
 * max_hull_vertices < 1.
 * c3d_rings_hull_limits: out[0] = the most points of an id that one wave keeps in registers, out[1] = the most points of an
 * id whose candidate set one workgroup is sure to keep in LDS; a larger id whose candidates (the points not strictly inside the
 * octagon of its eight directional extremes) do not fit is walked in HBM.  The results do not depend on the tier.  Host only.  */
#define C3D_HULL_ST_BAD_ROW 64
#define C3D_HULL_ST_TRUNCATED 128
void c3d_rings_hull_limits(int32_t out[2]);
int64_t c3d_rings_hull_ws_bytes(int32_t max_rings, int32_t max_vertices, int32_t max_objects);   /* < 0: C3D_E_* */
int c3d_rings_hull(const int32_t* rings, const int32_t* vertices, const int32_t* counts, int32_t max_rings,
                   int32_t max_vertices, int32_t max_objects, int32_t max_hull_vertices, int32_t* hulls,
                   int32_t* hull_vertices, int64_t* rects, int32_t* counts_out, void* ws, void* stream);

/* Regularised footprints (csrc/scene_regular.hip): a ring table and vertex list with integer pixel corners, normally the
 * output of c3d_outlines_simplify, and the four outputs of c3d_rings_hull for the same ids, turned into rings whose edges are
 * parallel or perpendicular to the chosen rectangle edge of their id while everything stays in HBM.  Integer arithmetic only
 * in every decision, every output is exact and two runs agree bit for bit.  One memset and 5 launches on `stream`, nothing is
 * read back by the host, no workgroup waits for another, every loop is capped, and no workspace word is read before the call
 * wrote it.  The rule:
 *   rows used   as in c3d_rings_hull: a row r < clamp(counts[1], 0, max_rings) is used iff start >= 0, n >= 0,
 *               start + n <= clamp(counts[3], 0, max_vertices), 1 <= id <= max_objects and every coordinate of the ring lies
 *               in [0, 16384].  A row with start < 0 passes through (start' = -1, n' = 0) and sets no bit; any other skipped
 *               row gets the same and sets C3D_REGULAR_ST_BAD_ROW.  Nothing is read or written out of range
 *   direction   an id has one iff id <= clamp(counts_hull[1], 0, max_objects), rects[id-1][0] = k >= 0, hulls[id-1] has
 *               start >= 0, m >= 3, k < m and start + m <= clamp(counts_hull[3], 0, max_hull_vertices), and the hull vertices
 *               h[k], h[(k+1) % m] lie in [0, 16384] and differ.  Then d = h[(k+1) % m] - h[k], g = gcd(|d.x|, |d.y|),
 *               u = d / g, N = u.x^2 + u.y^2 <= 2^29.  Every ring of an id without a direction is copied
 *   frame       for a vertex (x, y): T = x u.x + y u.y, C = y u.x - x u.y, the frame coordinates times |u|; |T|, |C| <= 2^29
 *   classes     a ring v[0 .. n-1], closed by v[n] = v[0], has the edges e_k = (v[k], v[k+1]); e_k is H iff |dT| >= |dC|,
 *               otherwise V.  A ring with n < 4 or with a zero-length edge is copied
 *   runs        the junctions are the k in 0 .. n-1 with class(e_{k-1}) != class(e_k), indices cyclic, ascending
 *               k_0 < ... < k_{R-1}; R is even.  R < 4: the ring is copied.  The run that ends at k_j has the edges
 *               k_{j-1} .. k_j - 1, cyclic
 *   levels      with S = 2^frac_bits and fdiv the floor division, an H run gets Cq = fdiv(S * A + W, 2 W), W = sum |dT_e| > 0,
 *               A = sum |dT_e| * (C_e0 + C_e1) over its edges: the length-weighted mean of the edge midpoints' C, rounded half
 *               up at 1/S of a frame unit.  A V run gets Tq the same way from |dC_e| and T_e0 + T_e1.  A needs 128 bits; the
 *               quotient fits 38
 *   vertices    output vertex j belongs to junction k_j: Cq from whichever of the two runs that meet there is H, Tq from the
 *               other, and back in pixels at 1/S
 *                 Xq = fdiv(2 (Tq u.x - Cq u.y) + N, 2 N)      Yq = fdiv(2 (Tq u.y + Cq u.x) + N, 2 N)
 *               n' = R, in junction order.  Coincident or collinear output vertices stay; no topology is promised, as with
 *               c3d_outlines_simplify: compare the filled result with the pixels (c3d_rings_fill, c3d_objects_match)
 *   copied      n' = n, every coordinate times S
 * Inputs (device): rings i32 [max_rings][8] (16-byte aligned), vertices i32 [max_vertices][2] (8-byte aligned), counts i32 [5];
 * hulls i32 [max_objects][8], hull_vertices i32 [max_hull_vertices][2], rects i64 [max_objects][8], counts_hull i32 [5] as
 * c3d_rings_hull writes them.
 * Outputs (must not alias the inputs):
 *   rings_out     i32 [max_rings][8], 16-byte aligned, same row order: (id, start', n', flag, perimeter, x, y, n): flag = 1 for
 *                 a regularised ring, 0 for a copied one; id, perimeter, x, y are copied; column 7 = the input's n.  Rows past
 *                 the last are 0
 *   vertices_out  i32 [max_vertices][2], 8-byte aligned, in units of 2^-frac_bits pixel, rings contiguous and in row order:
 *                 what c3d_rings_fill takes with the same frac_bits.  Rows past counts_out[3] are left as they were
 *   counts_out    i32 [5] = (rings found, rows written, vertices out, vertices out, status); status = counts[4] |
 *                 counts_hull[4] with C3D_REGULAR_ST_BAD_ROW added where it applies
 *   ws            c3d_rings_regularize_ws_bytes(max_rings, max_vertices, max_objects) bytes (13 per ring row, 12 per vertex
 *                 row), 256-byte aligned; a dirty one gives the same result
 * n' <= n, so a table whose rows share no vertices always fits.  Where rows share so many that the n' of a row and all used
 * rows before it add up to more than max_vertices, that row is a skipped row (C3D_REGULAR_ST_BAD_ROW), and so is every later
 * row that would be used.
 * C3D_OUTLINE_ST_BAD_COUNTS in counts[4] or counts_hull[4]: all rows 0, counts_out = (0, 0, 0, 0, status).
 * Refused before anything is enqueued (C3D_E_BADARG): a NULL pointer, max_rings, max_vertices, max_objects or
 * max_hull_vertices < 1, frac_bits outside [0, 8].
 * c3d_rings_regularize_limits: out[0] = the most edges of a ring that one wave handles, a lane per edge, out[1] = the most of
 * a ring whose vertices, junctions and levels one workgroup keeps in LDS; a larger ring is read from HBM and keeps its lists
 * in `ws`.  The results do not depend on the tier.  Host only.                                                              */
#define C3D_REGULAR_ST_BAD_ROW 256
void c3d_rings_regularize_limits(int32_t out[2]);
int64_t c3d_rings_regularize_ws_bytes(int32_t max_rings, int32_t max_vertices, int32_t max_objects);   /* < 0: C3D_E_* */
int c3d_rings_regularize(const int32_t* rings, const int32_t* vertices, const int32_t* counts, int32_t max_rings,
                         int32_t max_vertices, const int32_t* hulls, const int32_t* hull_vertices, const int64_t* rects,
                         const int32_t* counts_hull, int32_t max_objects, int32_t max_hull_vertices, int32_t frac_bits,
                         int32_t* rings_out, int32_t* vertices_out, int32_t* counts_out, void* ws, void* stream);

/* Polygon scores (csrc/scene_polis.hip): PoLiS (Avbelj et al., 2015), a vertex Hausdorff distance and the vertex counts of
 * every pair (predicted object, its ground-truth partner) from two ring tables and the match_p of c3d_objects_match while all
 * of them stay in HBM.  One memset and 10 launches on `stream`, nothing is read back by the host, no workgroup waits for
 * another, every loop is capped, and no workspace word is read before the call wrote it.  Integers decide everything but the
 * distances, and every floating-point sum is taken in an order that depends on the inputs only: two runs agree bit for bit.
 * The rule:
 *   sides       P, the prediction, and G, the ground truth, each a ring table in the layout of c3d_scene_outlines: rings i32
 *               [max_rings][8] with (id, start, n) in columns 0..2 (the others are ignored), vertices i32 [max_vertices][2]
 *               (8-byte aligned), counts i32 [5]; each with its own f = frac_bits in [0, 8], coordinates in units of 2^-f pixel,
 *               |coordinate| <= 32768 * 2^f.  The ids of P are 1 .. max_p, those of G 1 .. max_g
 *   units       F = max(f_p, f_g); every coordinate is shifted left by F - f.  Distances are computed in those units and divided
 *               by 2^F at the end, which is exact
 *   rows used   as in c3d_rings_fill: a row r < clamp(counts[1], 0, max_rings) whose id lies in [1, max] is used iff start >= 0,
 *               n >= 0, start + n <= clamp(counts[3], 0, max_vertices) and every coordinate of the ring is in range.  A used
 *               ring with n < 3 contributes nothing.  An id that has a row with start < 0, or any other row that is not used,
 *               is INCOMPLETE; so is an id with more than RING_LIMIT rings of n >= 3 (c3d_rings_polis_limits: the step that
 *               restores the row order holds no more), and an id of a table whose rows share vertices once the vertices of
 *               the ids up to it add up to more than max_vertices.  Rows whose id lies outside [1, max] are ignored.  The rings
 *               of an id need not be contiguous in the table
 *   geometry    V(id) = the vertices of its used rings with n >= 3, in ascending row order and then by index; E(id) = the edges
 *               (v[k], v[(k+1) mod n]) of each of those rings, the closing edge included.  Edges never join two rings; holes
 *               are rings like any other
 *   distance    of a point p to an edge (a, b): e = b - a, w = p - a, L = e.e, t = w.e, c = w x e, all integers below 2^53 and
 *               so exact in a double.  L == 0 or t <= 0: v = (double)(w.w); t >= L: v = (double)|p - b|^2; otherwise
 *               v = ((double)c * (double)c) / (double)L.  d(p, E) = sqrt(min over the edges of v)
 *   objects     K_p = the largest id in [1, max_p] of a row r < clamp(counts_p[1], 0, max_rings_p) of P, used or not
 *   pair        for p <= K_p: g = match_p[p-1][0].  g outside [0, max_g] sets C3D_POLIS_ST_BAD_PARTNER and counts as 0.  The
 *               pair is scored iff g >= 1, neither id is incomplete, n_p = |V(p)| >= 1, n_g = |V(g)| >= 1 and
 *               2 * n_p * n_g <= max_pair_work.  Then mean_pg = the mean of d(v, E(g)) over V(p), mean_gp the other way round,
 *               PoLiS = (mean_pg + mean_gp) / 2, and hausdorff = the largest of all those n_p + n_g distances.  This is the
 *               VERTEX-TO-BOUNDARY form: it is NOT the Hausdorff distance of the two boundaries, whose maximum may fall
 *               inside an edge (a long edge of one polygon that passes far from the other is seen at its two ends only)
 * Inputs (device): the two sides; match_p i32 [max_p][4] as c3d_objects_match writes it (column 0 is read); max_pair_work >= 0,
 * the most point-edge evaluations one pair may cost.
 * Outputs:
 *   pair       f64 [max_p][4], 16-byte aligned, row p-1 = (polis, hausdorff, mean_pg, mean_gp) in pixels; zeros where the pair is
 *              not scored
 *   pair_n     i32 [max_p][4], 16-byte aligned, row p-1 = (g or 0, n_p, n_g, flag): n_p and n_g are 0 for an incomplete id and
 *              n_g is 0 without a partner; flag 0 scored, 1 no partner, 2 an incomplete or empty id on either side, 3 over
 *              max_pair_work.  Rows past K_p of both tables are 0, written by the call
 *   counts     i64 [8] = (scored, no partner, incomplete or empty, over work, sum n_p, sum n_g, status, 0), the sums over the
 *              scored pairs; status = counts_p[4] | counts_g[4] as they came, with C3D_POLIS_ST_BAD_PARTNER added
 *   sums       f64 [4] = (sum polis, sum hausdorff, max hausdorff, sum (double)n_p / (double)n_g) over the scored pairs, added
 *              by one workgroup in ascending p (256 interleaved partial sums, then a fixed tree)
 *   totals     i64 [8] or NULL, total_sums f64 [4] or NULL: counts[0..5] are ADDED into totals, status is OR-ed into totals[6];
 *              sums[0], [1], [3] are added into total_sums and slot 2 takes the maximum; by one thread at the end of the last
 *              launch, so calls on one stream accumulate in stream order (the convention of c3d_objects_match).  The caller
 *              zeroes them once
 *   ws         c3d_rings_polis_ws_bytes(...) bytes, 256-byte aligned; a dirty one gives the same result
 * Tiers.  A pair with n_p, n_g <= out[0] runs in one wave.  Every other pair is cut into jobs of (direction, out[1] vertices of
 * the id's vertex list) that read the other id's edges in tiles of out[2]; the sum of a job is a fixed tree, the jobs of a
 * pair are added in job order.  The tiers round a sum differently; both stay within (n + 8) 2^-53 relative of the exact mean.
 * The job table holds ceil(max_vertices_p / out[1]) + ceil(max_vertices_g / out[1]) + 2 max_p jobs, which suffices whenever no
 * ground-truth id is named twice (c3d_objects_match with iou_thr >= 0.5 never does); a pair of the job tier whose jobs no longer
 * fit, and every such pair after it, gets flag 3.  C3D_OUTLINE_ST_BAD_COUNTS in counts_p[4] or counts_g[4] empties that side.
 * Refused before anything is enqueued (C3D_E_BADARG): a NULL pointer other than totals / total_sums / stream, a frac_bits outside
 * [0, 8], a max below 1, max_pair_work < 0.
 * c3d_rings_polis_limits: out[0] = the most vertices of either id in the wave tier, out[1] = the vertices of a job, out[2] = the
 * edges of an LDS tile, out[3] = RING_LIMIT, out[4] = the most vertices of a ring that one wave checks and regroups; a longer ring
 * is spread over many workgroups.  The results do not depend on that.  Host only.                                             */
#define C3D_POLIS_ST_BAD_PARTNER 512
void c3d_rings_polis_limits(int32_t out[5]);
int64_t c3d_rings_polis_ws_bytes(int32_t max_rings_p, int32_t max_vertices_p, int32_t max_p, int32_t max_rings_g,
                                 int32_t max_vertices_g, int32_t max_g);   /* < 0: C3D_E_* */
int c3d_rings_polis(const int32_t* rings_p, const int32_t* vertices_p, const int32_t* counts_p, int32_t max_rings_p,
                    int32_t max_vertices_p, int32_t frac_bits_p, const int32_t* rings_g, const int32_t* vertices_g,
                    const int32_t* counts_g, int32_t max_rings_g, int32_t max_vertices_g, int32_t frac_bits_g,
                    const int32_t* match_p, int32_t max_p, int32_t max_g, int64_t max_pair_work, double* pair, int32_t* pair_n,
                    int64_t* counts, double* sums, int64_t* totals, double* total_sums, void* ws, void* stream);

/* Polygon validity (csrc/scene_valid.hip): for every object id of ONE ring table the proper crossings, collinear overlaps and
 * touches among its own edges, while the table stays in HBM.  One memset and 10 launches on `stream`, nothing is read back by
 * the host, no workgroup waits for another, every loop is capped, and no workspace word is read before the call wrote it.
 * Everything is an integer: |coordinate| <= 32768 * 2^8 = 2^23, differences below 2^25, every cross or dot product below 2^50;
 * nothing is rounded anywhere, and every sum is an integer atomic or a ballot count: the result is exact, equal from run to run
 * and on a dirty workspace, and independent of the tier.  The rule:
 *   table       a ring table in the layout of c3d_scene_outlines: rings i32 [max_rings][8] with (id, start, n) in columns 0..2
 *               (the others are ignored), vertices i32 [max_vertices][2] (8-byte aligned), counts i32 [5]; frac_bits in [0, 8]
 *               only sets the coordinate range, |coordinate| <= 32768 * 2^frac_bits.  The ids are 1 .. max_ids
 *   rows used   the rule of c3d_rings_polis for one side: a row r < clamp(counts[1], 0, max_rings) whose id lies in [1, max_ids]
 *               is used iff start >= 0, n >= 0, start + n <= clamp(counts[3], 0, max_vertices) and every coordinate of the ring
 *               is in range.  A used ring with n < 3 contributes nothing.  An id that has a row with start < 0, or any other row
 *               that is not used, is INCOMPLETE; so is an id with more than RING_LIMIT rings of n >= 3, and an id of a table
 *               whose rows share vertices once the vertices of the ids up to it add up to more than max_vertices.  Rows whose
 *               id lies outside [1, max_ids] are ignored.  C3D_OUTLINE_ST_BAD_COUNTS in counts[4] empties the table.  K = the
 *               largest id in [1, max_ids] of a row r < clamp(counts[1], 0, max_rings), used or not
 *   edges       E(id) = the edges (v[k], v[(k+1) mod n]) of its used rings with n >= 3, the closing edge included.  An edge with
 *               a == b is DEGENERATE: it is counted and takes part in no pair.  m = the number of the other, live, edges
 *   adjacent    two edges of the same ring whose indices differ by 1 modulo n.  In a triangle every pair is adjacent
 *   pair        for live edges (a, b) and (c, d): o1 = sign((b-a) x (c-a)), o2 = sign((b-a) x (d-a)), o3 = sign((d-c) x (a-c)),
 *               o4 = sign((d-c) x (b-c)).  The first class that applies:
 *                 cross     o1 o2 < 0 and o3 o4 < 0
 *                 overlap   all four are zero and the collinear segments share more than one point: with t(p) = (p-a).(b-a)
 *                           and L = (b-a).(b-a), max(min(t(c), t(d)), 0) < min(max(t(c), t(d)), L).  Adjacent pairs ARE
 *                           tested: a spike p -> q -> p' folded back on itself is an overlap
 *                 touch     the segments share exactly one point.  For an adjacent pair that point is their joint and is NOT
 *                           counted.  Otherwise touch_vv if the point is an end point of both edges, touch_ve if an end point
 *                           of one lies strictly inside the other
 *                 nothing   otherwise
 *   checked     an id <= K is checked iff it is complete, m >= 1 and m (m - 1) / 2 <= max_id_work; otherwise every pair count
 *               of its row is 0.  An id is VALID iff it is checked and cross == 0 and overlap == 0
 * Touches are reported and never disqualify: the 8-connected pinches of c3d_scene_outlines are vertex-vertex touches, and raw
 * traced rings are valid.  What this does NOT decide:
 *   - a ring that passes from one side of another ring to its other side exactly through a vertex is counted as touches only;
 *   - whether a hole still lies inside its shell is not examined;
 *   - edges of different ids are never compared (c3d_rings_conflicts does that).
 * Inputs (device): the table; max_id_work >= 0, the most edge pairs one id may cost (there is no spatial index: this cap stands
 * in for one, as max_pair_work does in c3d_rings_polis; a bounding-box reject in front of the four products is the only pruning
 * and changes no count).
 * Outputs:
 *   valid      i64 [max_ids][8], row id-1 = (flag, rings, m, degenerate, cross, overlap, touch_vv, touch_ve); flag 0 checked,
 *              1 empty (no used ring with n >= 3, or no live edge), 2 incomplete, 3 over max_id_work.  rings, m and degenerate
 *              are 0 for an incomplete id.  Rows past K are 0, written by the call
 *   counts     i64 [8] = (checked, invalid, empty, incomplete, over work, sum cross, sum overlap, status) over the ids 1 .. K,
 *              the sums over the checked ids; invalid = checked and not valid; status = counts[4] of the table as it came
 *   totals     i64 [8] or NULL: counts[0..6] are ADDED into it and status is OR-ed into totals[7] by one thread at the end of
 *              the last launch, so calls on one stream accumulate in stream order (the convention of c3d_objects_match).  The
 *              caller zeroes it once
 *   ws         c3d_rings_valid_ws_bytes(...) bytes, 256-byte aligned; a dirty one gives the same result
 * Tiers.  An id with at most out[0] edges (degenerate ones included) runs in one wave: a lane per edge, the other edge by
 * shuffle, counts by ballot.  A larger id is cut into chunks of out[1] edges; the job (id, chunk i) of an id of c chunks
 * compares chunk i with the chunks i, i+1, .., i + floor(c/2) (mod c), staged through LDS out[2] edges at a time, so every
 * unordered pair of chunks belongs to exactly one job; the job table holds ceil(max_vertices / out[1]) + max_ids jobs, which
 * suffices for every table.
 * Refused before anything is enqueued (C3D_E_BADARG): a NULL pointer other than totals / stream, frac_bits outside [0, 8],
 * a max below 1, max_id_work < 0.
 * c3d_rings_valid_limits: out[0] = the most edges of an id in the wave tier, out[1] = the edges of a chunk, out[2] = the edges
 * of an LDS tile, out[3] = RING_LIMIT, out[4] = the most vertices of a ring that one wave checks and regroups.  Host only.     */
void c3d_rings_valid_limits(int32_t out[5]);
int64_t c3d_rings_valid_ws_bytes(int32_t max_rings, int32_t max_vertices, int32_t max_ids);   /* < 0: C3D_E_* */
int c3d_rings_valid(const int32_t* rings, const int32_t* vertices, const int32_t* counts_in, int32_t max_rings,
                    int32_t max_vertices, int32_t frac_bits, int32_t max_ids, int64_t max_id_work, int64_t* valid,
                    int64_t* counts, int64_t* totals, void* ws, void* stream);

/* Polygon conflicts between objects (csrc/scene_conflicts.hip): for every object id of ONE ring table the proper crossings,
 * collinear overlaps and touches of its edges with the edges of every OTHER id, while the table stays in HBM.  One memset and 14
 * launches on `stream`, nothing is read back by the host, no workgroup waits for another, every loop is capped, and no workspace
 * word is read before the call wrote it.  Everything is an integer, as in c3d_rings_valid, and every sum is an integer atomic or
 * a ballot count; nothing depends on the order in which the device lists edges or fills cells: the result is exact, equal from
 * run to run and on a dirty workspace, and independent of the grid that finds the pairs.  The rule:
 *   table, rows used, INCOMPLETE ids, K, edges, DEGENERATE, live edges, m
 *               word for word those of c3d_rings_valid, which are those of c3d_rings_polis for one side, RING_LIMIT included.
 *               The edges of an incomplete id take part in nothing
 *   pairs       every unordered pair of live edges (a, b) of id i and (c, d) of id j with i != j, both ids complete.  Pairs of
 *               one id are never looked at (c3d_rings_valid does that)
 *   classes     with o1 .. o4 as in c3d_rings_valid, the first class that applies:
 *                 cross     o1 o2 < 0 and o3 o4 < 0
 *                 same      all four are zero, the collinear segments share more than one point (the t / L test of
 *                           c3d_rings_valid) and (b-a).(d-c) > 0
 *                 opposite  the same with (b-a).(d-c) < 0
 *                 touch     the segments share exactly one point: touch_vv if it is an end point of both edges, touch_ve if an
 *                           end point of one lies strictly inside the other.  There is no adjacency across ids: every such pair
 *                           counts
 *                 nothing   otherwise
 *   verdict     an id <= K is checked iff it is complete, m >= 1 and work <= max_work (below).  It is IN CONFLICT iff it is
 *               checked and cross + same > 0.  `opposite` is the shared wall of two pieces that meet and is reported only.
 *               Touches are reported only: 4-connected components meet corner to corner.  `same` means that both interiors lie
 *               on the same side of a common stretch; that reading assumes that every ring keeps its object on the side where
 *               c3d_scene_outlines puts it (a table whose rings were reversed turns shared walls into `same`)
 * What this does NOT decide:
 *   - a boundary that passes from one side of another id's boundary to its other side exactly through a vertex is touches only;
 *   - an object that lies wholly inside another without any edge contact is not seen;
 *   - nothing is said about an id against itself.
 * Raw traced rings never conflict: two directed pixel edges of different labels cannot cross, and a shared wall runs in opposite
 * directions.
 *   work        the implementation bins the live edges into a uniform grid of square cells of 2^s units whose origin is the
 *               lower corner of the bounding box of all live edges; an edge is entered in every cell its own bounding box
 *               covers.  s is the smallest shift in [0, 25] for which entries <= out[4] * n and cells <= out[5] * max(n, 1)
 *               (c3d_rings_conflicts_limits), n = the live edges of the complete ids; one cell always satisfies both, and n <=
 *               max_vertices, so both also hold against max_vertices.  work = the sum over the cells of n_c (n_c - 1) / 2 with
 *               n_c the entries of cell c: a function of the input only.  If work >
 *               max_work no pair is evaluated.  A pair of entries of a cell is evaluated iff the ids differ, the edges' bounding
 *               boxes meet and the cell holds the lower corner of the boxes' intersection, so every pair is evaluated once
 * Inputs (device): the table; max_work >= 0.
 * Outputs (all written by the call):
 *   conflict   i64 [max_ids][8], row id-1 = (flag, partner, m, cross, same, opposite, touch_vv, touch_ve); flag 0 checked, 1
 *              empty (no live edge), 2 incomplete, 3 over max_work, which then holds for every id that would otherwise be
 *              checked.  partner = the smallest other id with which this id has a cross or same pair, 0 if none.  The counts are
 *              this id's edges against all other ids, so an edge pair appears in two rows.  m is 0 for an incomplete id; for
 *              flags 2 and 3 the pair counts and partner are 0.  Rows past K are 0
 *   counts     i64 [8] = (checked, in conflict, empty, incomplete, over work, sum cross, sum same, status) over the ids 1 .. K;
 *              each edge pair is counted once in the sums; status = counts[4] of the table as it came
 *   info       i64 [8] = (live edges of complete ids, s, cells_x, cells_y, entries, work, sum opposite, sum touch_vv + touch_ve),
 *              pairs once.  Elements 1 .. 5 describe the grid and are the implementation's; the others are fixed by the rule
 *   totals     i64 [8] or NULL: counts[0..6] are ADDED into it and status is OR-ed into totals[7] by one thread at the end of
 *              the last launch, so calls on one stream accumulate in stream order.  The caller zeroes it once
 *   ws         c3d_rings_conflicts_ws_bytes(...) bytes, 256-byte aligned, a function of the three maxima alone; a dirty one
 *              gives the same result
 * Tiers.  A cell of at most out[0] entries runs in one wave: a lane per entry, the other entry by shuffle.  A larger cell is cut
 * into chunks of out[1] entries; the job (cell, chunk i) of a cell of c chunks compares chunk i with the chunks i, i+1, .., i +
 * floor(c/2) (mod c), staged through LDS out[2] entries at a time, so one crowded cell spreads over the compute units.
 * Registration is by bounding box: a long diagonal edge enters every cell of its box, which shows in `entries`; max_work stands
 * in for a finer index.
 * Refused before anything is enqueued (C3D_E_BADARG): a NULL pointer other than totals / stream, frac_bits outside [0, 8],
 * a max below 1, max_work < 0.
 * c3d_rings_conflicts_limits: out[0] = the most entries of a cell in the wave tier, out[1] = the entries of a chunk, out[2] = the
 * entries of an LDS tile, out[3] = RING_LIMIT, out[4] = the entry budget and out[5] = the cell budget per live edge (so per
 * vertex).  Host only.                                                                                                                       */
void c3d_rings_conflicts_limits(int32_t out[6]);
int64_t c3d_rings_conflicts_ws_bytes(int32_t max_rings, int32_t max_vertices, int32_t max_ids);   /* < 0: C3D_E_* */
int c3d_rings_conflicts(const int32_t* rings, const int32_t* vertices, const int32_t* counts_in, int32_t max_rings,
                        int32_t max_vertices, int32_t frac_bits, int32_t max_ids, int64_t max_work, int64_t* conflict,
                        int64_t* counts, int64_t* info, int64_t* totals, void* ws, void* stream);

/* Shared-wall simplification (csrc/scene_shared.hip): the traced rings of a label map that is still in HBM, cut at the lattice
 * points where three or more regions meet and simplified once per arc between two such nodes, so that the wall of A against B
 * is the wall of B against A, vertex for vertex, and an island's outline is the reverse of the hole it sits in.  A sibling of
 * c3d_outlines_simplify, which simplifies ring by ring and knows nothing of labels; that call is unchanged.  Integers only,
 * nothing is rounded, two runs agree bit for bit.  One memset and 10 launches on `stream`, nothing is read back, no workgroup
 * waits for another.  The rule:
 *   labels      l(y, x) = labels[y][x] if the pixel is in the scene and 1 <= value <= rows, else 0; rows = clamp(counts_obj[1],
 *               0, max_objects), as c3d_scene_outlines defines it
 *   nodes       for a lattice point (vx, vy) let a = l(vy-1, vx-1), b = l(vy-1, vx), c = l(vy, vx-1), d = l(vy, vx).  Its degree
 *               is [a != b] + [c != d] + [a != c] + [b != d]; it is a node iff degree >= 3.  Degree 4 includes the diagonal
 *               pinch a == d != b == c
 *   augmented   for every stored edge v[k] -> v[k+1] (v[n] = v[0]): v[k], then every lattice point strictly inside the edge that
 *               is a node, in travel order: a wall that runs straight through a T-junction gets the junction as a vertex, since
 *               the neighbours on the other side have their corner there.  Every augmented vertex carries `node` and `left` =
 *               the label left of the unit edge leaving it, the object on the right and y down: travelling +x it is l(y-1, x),
 *               +y l(y, x), -x l(y, x-1), -y l(y-1, x-1).  Between two nodes every lattice point has degree 2, so `left` is
 *               constant along an arc
 *   start       a ring with nodes starts at its first node in stored (augmented) order; one without at its vertex with the
 *               smallest (vy, vx), which is unique since such a ring visits no lattice point twice
 *   arcs        run between cyclically consecutive nodes; all nodes are kept.  A ring without nodes is one arc from its start to
 *               itself.  An arc whose two ends are the same lattice point is closed
 *   per arc     Douglas-Peucker with the segment distance num / den and the strict 16 num > tol2_q den of
 *               c3d_outlines_simplify.  The farthest vertex of a chord has the largest num; ties go to the smallest (vy, vx),
 *               NOT to the index: with the symmetric distance this makes the result independent of the direction of travel.  A
 *               chord whose two ends coincide always splits (in a traced ring only the chord of a whole closed arc is one; its
 *               num is |p - N|^2): a closed arc with interior vertices always keeps M, its interior vertex farthest from its
 *               node N, and goes on with the chains N..M and M..N.  If neither chain keeps anything the closed arc also keeps T,
 *               its interior vertex with the largest |cross(M - N, p - N)|, same tie, iff that cross product is not 0: a ring
 *               with at most one node never loses its area.  Open arcs have no such guard: it could not be decided identically
 *               from both sides
 * What follows from it:
 *   - every dropped vertex lies within tol of the kept chord that spans it
 *   - the twin property: for every output edge p -> q of id i with left = j > 0 the table holds the edge q -> p of id j with
 *     left = i, equally often (for a complete table of the same labels)
 *   - at tol2_q == 0 the output is the augmented ring, rotated to its start
 *   - a ring with two or more nodes may collapse (n' < 3 or area2' == 0); that is counted in info[5] and never repaired
 *   - chords of DIFFERENT arcs may still cross, and a neck narrower than the tolerance that collapses onto one line puts its two
 *     neighbours on that line from both sides: c3d_rings_conflicts finds both.  Neither is decided here
 * Inputs (device): labels i32 [Hs][Ws] and counts_obj i32 [2] of c3d_scene_objects / c3d_scene_split; rings, vertices, counts as
 * c3d_scene_outlines wrote them for those labels (alignment as for c3d_outlines_simplify); tol2_q as in c3d_outlines_simplify.
 * Outputs (must not alias the inputs):
 *   rings_out     i32 [max_rings][8], 16-byte aligned, input row order: (id, start', n', area2', perimeter, x', y', n); (x', y')
 *                 = the first output vertex = the ring's start; area2' as c3d_outlines_simplify defines it.  Rows past the last 0
 *   vertices_out  i32 [max_vertices_out][2], 8-byte aligned;  left_out i32 [max_vertices_out] = `left` of the edge leaving that
 *                 vertex.  Rows past counts_out[3] are left as they were
 *   counts_out    i32 [5] = (rings found, rows written, vertices kept, vertices written, status).  The table goes unchanged
 *                 into c3d_rings_fill, _hull, _valid, _conflicts, _polis and _regularize
 *   info          i32 [8] = (straight-through nodes inserted, node vertices, arcs, closed arcs, arcs with left > 0, collapsed
 *                 rings among the written ones, 0, 0); the first five over all simplified rows
 *   ws            c3d_outlines_simplify_shared_ws_bytes(Hs, Ws, max_rings, max_vertices) bytes (24 per ring row, 66 per vertex row:
 *                 room for 2 max_vertices augmented vertices; a quarter byte per lattice point for the two node bitmaps),
 *                 256-byte aligned; the call zeroes what it needs of it
 * Rows that are not simplified get start' = -1, n' = 0, area2' = 0 and keep the input's x, y:
 *   start < 0        passed through, no new status bit
 *   bad input        n < 4, start + n above the written vertices, a vertex outside [0, Ws] x [0, Hs], an edge that is zero or
 *                    not parallel to an axis, or augmented rings of this and all earlier valid rows that add up to more than
 *                    2 max_vertices: C3D_SIMPLIFY_ST_BAD_INPUT
 *   no room          truncation is prefix-shaped as in c3d_scene_outlines: a ring with start' + n' > max_vertices_out, and
 *                    every ring after it; counts_out[2] > counts_out[3] and C3D_OUTLINE_ST_TRUNCATED.  Every straight-through
 *                    node is a corner of some other ring, so 2 * (vertices written by the outlines call) always suffices
 * Nothing is read or written out of range.  Input status C3D_OUTLINE_ST_BAD_COUNTS: counts_out = (0, 0, 0, 0,
 * C3D_OUTLINE_ST_BAD_COUNTS), all ring rows and info 0.
 * Refused before anything is enqueued: a NULL pointer, Hs, Ws, max_objects, max_rings, max_vertices or max_vertices_out < 1,
 * max_objects or max_vertices above 2^30, tol2_q out of range (C3D_E_BADARG); Hs or Ws above 16384 (C3D_E_UNSUPPORTED).
 * c3d_outlines_simplify_shared_limits: out[0] = the most augmented vertices of a ring that one wave simplifies, out[1] = the most
 * of a ring whose state one workgroup keeps in LDS; larger rings keep it in `ws`.  The results do not depend on the tier.       */
void c3d_outlines_simplify_shared_limits(int32_t out[2]);
int64_t c3d_outlines_simplify_shared_ws_bytes(int32_t Hs, int32_t Ws, int32_t max_rings, int32_t max_vertices);   /* < 0: C3D_E_* */
int c3d_outlines_simplify_shared(const int32_t* labels, const int32_t* counts_obj, int32_t Hs, int32_t Ws, int32_t max_objects,
                                 const int32_t* rings, const int32_t* vertices, const int32_t* counts, int32_t max_rings,
                                 int32_t max_vertices, int64_t tol2_q, int32_t max_vertices_out, int32_t* rings_out,
                                 int32_t* vertices_out, int32_t* left_out, int32_t* counts_out, int32_t* info, void* ws,
                                 void* stream);

/* Crossing-free shared walls (csrc/scene_safe.hip): c3d_outlines_simplify_shared run in rounds with a tolerance per arc.  A
 * defect of the output -- two chords that cross, a neck that collapsed onto one line, a ring that lost or flipped its area --
 * is repaired locally: the arcs that take part in it get a quarter of their squared tolerance, every other arc keeps the
 * caller's.  Both neighbours of a wall see the same change, so the twin property survives, and at tolerance 0 an arc is its raw
 * augmented vertices, which never form a defect.  All of it is integers: exact, equal from run to run and on a dirty workspace.
 * c3d_outlines_simplify_shared, c3d_rings_conflicts and c3d_rings_valid are unchanged.  The rule:
 *   inputs      those of c3d_outlines_simplify_shared, and max_rounds in [1, 64].  Labels, nodes, augmentation, start, arcs and
 *               the per-arc Douglas-Peucker are word for word that call's, but that the arc's own tolerance stands where tol2_q
 *               stands there (the closed-arc guards M and T are decided without any tolerance, there and here)
 *   arc key     key(v, dir) = 4 * (vy * (Ws + 1) + vx) + dir with the four unit directions numbered as c3d_scene_outlines numbers
 *               sides: +x 0, +y 1, -x 2, -y 3.  An arc from lattice point s to lattice point e has the key min(key(s, first unit
 *               step), key(e, reverse of the last unit step)); a ring without nodes has s = e = its start.  A unit edge of the
 *               lattice lies on at most one wall, so two arcs share a key iff they are twins, or an island and the hole it sits in
 *   level       every arc has a level L >= 0, kept by key, 0 at first.  Its tolerance is tol2_q >> (2 L).  L_cap = the smallest L
 *               for which that is 0: there the arc is its raw augmented vertices.  tol2_q = 0 has L_cap = 0
 *   round       simplify every ring with the current levels; find the defects of the result; raise
 *   edges       every written output ring takes part, whatever its n'.  Its edges are v[k] -> v[(k + 1) mod n'].  An edge is live
 *               iff its ends differ, belongs to the arc of its start vertex, and two edges are adjacent iff they are in the same
 *               ring row and their indices differ by 1 modulo n'
 *   pair        an unordered pair of distinct live edges (a, b) of id i and (c, d) of id j, o1 .. o4 as in c3d_rings_valid, is
 *               DEFECTIVE iff it is a cross (o1 o2 < 0 and o3 o4 < 0); or collinear and shares more than one point (the t / L
 *               test of c3d_rings_valid; adjacent pairs are tested) unless i != j and (b-a).(d-c) < 0, which is a shared wall; or
 *               the segments share exactly one point, the pair is not adjacent, and that point is an end of one edge strictly
 *               inside the other (touch_ve).  Vertex-vertex touches are never a defect.  A defective pair marks the arcs of both
 *               edges
 *   ring        a written ring is DEFECTIVE iff n' < 3 or the sign of area2' is not the sign of column 3 of its input row.  It
 *               marks all its arcs
 *   raise       every marked arc with L < L_cap gets L + 1
 *   loop        at most max_rounds rounds.  The call stops after the first round that marks nothing
 *               (C3D_SAFE_ST_CONVERGED); after a round that marks something and raises nothing (C3D_SAFE_ST_DEFECTS_LEFT);
 *               after round max_rounds - 1 if it raised something (C3D_SAFE_ST_NOT_CONVERGED); after a round whose grid work
 *               (below) exceeds max_work, in which no pair is evaluated and nothing is raised (C3D_SAFE_ST_OVER_WORK).  The
 *               output is always that of the last simplify step that ran
 * Why it ends: levels only rise and are bounded by L_cap.  For a table that belongs to its labels two raw arcs never form a
 * defective pair: raw traced rings do not cross, shared walls run in opposite directions, and every straight-through junction is
 * an inserted node, so no vertex lies inside a raw edge.  A ring whose arcs are all raw keeps its area.  So every defect involves
 * an arc below L_cap, and that arc is raised: DEFECTS_LEFT needs a table that does not belong to its labels.
 * What is NOT promised: defects are what the pair rule sees.  A change of the cyclic order of the chords round a node is caught
 * only where it shows as one of those pairs or as a flipped ring; an object that moves wholly inside another without any contact
 * of edges is not seen (as in c3d_rings_conflicts).
 * What follows from it:
 *   - the twin property of c3d_outlines_simplify_shared holds in every round
 *   - at tol2_q == 0 the output is that of c3d_outlines_simplify_shared, in one round
 *   - if round 0 marks nothing, rings_out, vertices_out, left_out and counts_out are those of c3d_outlines_simplify_shared
 *   - on a converged output c3d_rings_valid reports 0 crossings, 0 overlaps and 0 touch_ve for every checked id,
 *     c3d_rings_conflicts 0 cross, 0 same and 0 touch_ve, and info[5] (collapsed) is 0
 * Outputs (must not alias the inputs; all taken from the last round that ran):
 *   rings_out, vertices_out, left_out, counts_out   as in c3d_outlines_simplify_shared; the prefix-shaped truncation at
 *                 max_vertices_out (at most 2^29 here) is decided in each round's scatter
 *   level_out     i32 [max_vertices_out]: the level of the arc of the edge leaving that vertex.  Rows of vertices_out, left_out
 *                 and level_out past counts_out[3] mean nothing: they are as they were, or an earlier round's where that round
 *                 wrote more (a truncated table only); nothing is written past max_vertices_out
 *   info          i32 [8] as there; info[6] = the shift s and info[7] = min(work, 2^31 - 1) of the last round's grid, which
 *                 are the implementation's
 *   safe          i64 [8] = (rounds run, rounds that raised, arcs with L > 0, arcs at L_cap, defective pairs in round 0,
 *                 defective pairs in the last round run, defective rings in round 0, status).  Pairs are counted once each, arcs
 *                 once per key, and the two arc counts are those of the levels that the last simplify step read.  In a round
 *                 over max_work the pairs count as 0
 *   work          the detector bins the live output edges into the grid of c3d_rings_conflicts (cells of 2^s units from the
 *                 lower corner of the box of all live edges, an edge in every cell its box covers, the smallest s in [0, 25] with
 *                 entries <= out[4] n and cells <= out[5] max(n, 1), n = the live edges); work = the sum over the cells of
 *                 n_c (n_c - 1) / 2.  A pair of entries of a cell is evaluated iff the boxes meet and the cell holds the lower
 *                 corner of their intersection, pairs of one id included: every pair once
 *   ws            c3d_outlines_simplify_safe_ws_bytes(...) bytes, 256-byte aligned: the shared call's (24 per ring row, 66 per
 *                 vertex row), 10 more per vertex row (direction and key of every augmented vertex), 4 per lattice point for the
 *                 level store (a byte per key: level, a `present` and a `mark` bit), and 76 per row of max_vertices_out for the
 *                 edge list and the grid.  The call zeroes what it needs of it
 * Two memsets and 7 + 16 max_rounds launches on `stream`: bitmaps, validation, offsets and the augmented rings with their arc
 * keys are built once; the rounds are launched ahead and every launch of a round after the stopping one returns at once on a
 * device word.  Nothing is read back, no workgroup waits for another, every loop is capped.  Every ring is simplified again in
 * every round.  Rows that are not simplified, bad input, BAD_COUNTS: as in c3d_outlines_simplify_shared; safe is then (1, 0, ..).
 * Refused before anything is enqueued: what c3d_outlines_simplify_shared refuses, a NULL level_out or safe, max_rounds outside
 * [1, 64], max_work < 0, max_vertices_out above 2^29 (C3D_E_BADARG); Hs or Ws above 16384 (C3D_E_UNSUPPORTED).
 * c3d_outlines_simplify_safe_limits: out[0], out[1] = the two tier limits of the Douglas-Peucker as in
 * c3d_outlines_simplify_shared_limits; out[2] = the most entries of a cell in the detector's wave tier, out[3] = the entries of a
 * chunk and of an LDS tile, out[4] = the entry budget and out[5] = the cell budget per live edge.  Host only.                  */
#define C3D_SAFE_ST_CONVERGED 0
#define C3D_SAFE_ST_NOT_CONVERGED 1
#define C3D_SAFE_ST_DEFECTS_LEFT 2
#define C3D_SAFE_ST_OVER_WORK 3
void c3d_outlines_simplify_safe_limits(int32_t out[6]);
int64_t c3d_outlines_simplify_safe_ws_bytes(int32_t Hs, int32_t Ws, int32_t max_rings, int32_t max_vertices,
                                            int32_t max_vertices_out);   /* < 0: C3D_E_* */
int c3d_outlines_simplify_safe(const int32_t* labels, const int32_t* counts_obj, int32_t Hs, int32_t Ws, int32_t max_objects,
                               const int32_t* rings, const int32_t* vertices, const int32_t* counts, int32_t max_rings,
                               int32_t max_vertices, int64_t tol2_q, int32_t max_rounds, int64_t max_work, int32_t max_vertices_out,
                               int32_t* rings_out, int32_t* vertices_out, int32_t* left_out, int32_t* level_out, int32_t* counts_out,
                               int32_t* info, int64_t* safe, void* ws, void* stream);

/* Distance transform (csrc/scene_edt.hip): the exact squared Euclidean distance transform of a u8 map [Hs][Ws] that is already
 * in HBM.  The rule:
 *   sites       the pixels with mask == 0; with C3D_EDT_INVERT (bit 0 of flags) the pixels with mask != 0
 *   border      with C3D_EDT_BORDER (bit 1) every position outside the scene is a site as well: the transform of the mask padded
 *               by one ring of sites (the outside is infinite, but one ring decides)
 *   distance    dist2[y][x] = the minimum over the sites (y', x') of (y - y')^2 + (x - x')^2, as i32; a site gets 0
 *   no site     where no site exists (none in the mask and no BORDER bit) every pixel gets C3D_EDT_FAR
 *   cap         cap2 = 0: none.  cap2 > 0: every pixel whose true value exceeds cap2 gets exactly C3D_EDT_FAR, every other pixel
 *               its true value; the search then stops after isqrt(cap2) steps and the output is still fully specified
 *   limits      1 <= Hs, Ws <= 16384, so that the largest true value, 2 * 16383^2, stays below FAR (C3D_E_UNSUPPORTED beyond)
 * Integer arithmetic only; three launches on `stream` (column sites as bits, column distances, row minimum), nothing is read
 * back by the host, no workgroup waits for another, and every word of `ws` is written before it is read: two runs agree bit for
 * bit, on a dirty workspace too.  The uncapped cost of a pixel grows with the distance to its nearest site along the row: a
 * scene with (nearly) no site costs O(Ws) per pixel.
 *   mask    u8 [Hs][Ws];  dist2  i32 [Hs][Ws], must not alias the mask
 *   ws      c3d_scene_edt_ws_bytes(Hs, Ws) bytes, 256-byte aligned: one u64 of site bits per column and chunk of rows, then
 *           the column distances as u16 [Hs][Ws]
 * Refused before anything is enqueued: a NULL mask, dist2 or ws, flags outside bits 0..1, cap2 < 0, Hs or Ws < 1
 * (C3D_E_BADARG); Hs or Ws > 16384 (C3D_E_UNSUPPORTED).
 * c3d_scene_edt_tile: out[0] = the rows of one chunk of the column pass, out[1] = the pixels of a row that one workgroup of the
 * row pass handles: the two extents at which the implementation changes path.  Host only.                                     */
#define C3D_EDT_INVERT 1
#define C3D_EDT_BORDER 2
#define C3D_EDT_FAR 0x3fffffff
int64_t c3d_scene_edt_ws_bytes(int32_t Hs, int32_t Ws);                 /* < 0: C3D_E_* */
int c3d_scene_edt_tile(int32_t out[2]);
int c3d_scene_edt(const uint8_t* mask, int32_t Hs, int32_t Ws, int32_t flags, int32_t cap2, int32_t* dist2, void* ws, void* stream);

/* Boundary counts of two u8 maps [Hs][Ws], a prediction and a ground truth (csrc/scene_edt.hip): what Boundary IoU (Cheng et
 * al., 2021) and the boundary F-measure with a pixel tolerance are made of.  P and G are the nonzero pixels of `pred` and `gt`.
 *   distances   dP, dG = the transform above of P and of G to their background (sites: mask == 0); `flags` may hold
 *               C3D_EDT_BORDER, which both take, and nothing else
 *   bands       Pd = P and dP <= d2, Gd likewise: the band of Boundary IoU of width d, with d2 = floor(d * d) (on the lattice
 *               dist <= d iff dist2 <= floor(d^2))
 *   contours    Pc = P and dP == 1: the pixels of P that are 4-adjacent to background; Gc likewise
 *   tolerance   eG = the transform with INVERT of Gc, the squared distance to the nearest ground-truth contour pixel; eP the
 *               same of Pc.  These two never take the BORDER bit.  An empty contour set is hit by nothing
 *   counts      i64 [8] = (|Pd and Gd|, |Pd or Gd|, |Pc|, |{p in Pc : eG <= tau2}|, |Gc|, |{p in Gc : eP <= tau2}|, 1, 0)
 *   totals      i64 [8] or NULL: the counts are ADDED into it by one thread at the end of the last launch, so calls on one
 *               stream accumulate in stream order (the convention of c3d_objects_match)
 *   ws          c3d_boundary_counts_ws_bytes(Hs, Ws) bytes, 256-byte aligned; the call zeroes what it needs of it
 * One memset and eight launches on `stream` (the transforms run capped at d2 and tau2, two maps per launch); integer atomics
 * only, so every count is exact and the same from run to run; nothing is read back by the host.
 * Refused before anything is enqueued: a NULL pred, gt, counts or ws, flags other than 0 or C3D_EDT_BORDER, d2 or tau2 outside
 * [1, C3D_BOUNDARY_R2_MAX] (radii up to 1024 px), Hs or Ws < 1 (C3D_E_BADARG); Hs or Ws > 16384 (C3D_E_UNSUPPORTED).          */
#define C3D_BOUNDARY_R2_MAX (1024 * 1024)
int64_t c3d_boundary_counts_ws_bytes(int32_t Hs, int32_t Ws);           /* < 0: C3D_E_* */
int c3d_boundary_counts(const uint8_t* pred, const uint8_t* gt, int32_t Hs, int32_t Ws, int32_t d2, int32_t tau2, int32_t flags,
                        int64_t* counts, int64_t* totals, void* ws, void* stream);

/* Touching objects split apart (csrc/scene_split.hip): c3d_scene_objects with every connected component cut into the pieces that
 * its necks join.  The arguments of c3d_scene_objects plus r2 >= 0, a squared radius in pixels, and max_rounds >= 1; the
 * connectivity c (4 or 8) is used everywhere below.
 *   core      mask != 0 and dist2 > r2, with dist2 = c3d_scene_edt(mask, flags = C3D_EDT_BORDER, cap2 = r2): the outside of the
 *             scene is background, and C3D_EDT_FAR is > r2.  With r2 == 0 the core is the mask and no transform is run
 *   seeds     the c-connected components of the core; a seed's id is the linear index y * Ws + x of its first pixel in raster
 *             order
 *   growth    inside one c-connected component of the mask, d(p, s) = the length of the shortest c-connected path from pixel p to
 *             any pixel of seed s with every step inside the mask.  A pixel of a component that holds at least one seed belongs
 *             to the seed with the lexicographically smallest (d(p, s), id(s)): the unique fixed point of
 *               key(p) = min(key(p), min over the c-neighbours q of p in the mask of key(q) + (1, 0)),  key = (0, id) on seeds.
 *             A component without a seed (thinner than the radius everywhere) stays one piece
 *   pieces    every piece is c-connected; with min_area <= 1 the pieces partition the mask.  Touching pieces share pixel edges,
 *             which c3d_scene_outlines cuts (it cuts wherever the neighbour has another label)
 *   outputs   labels, table, hist, object_cls, counts exactly as c3d_scene_objects defines them with "component" read as
 *             "piece": min_area filters pieces, pieces are numbered 1..N in raster order of their own first pixel (which may
 *             precede the seed's), the same eight columns, vote rule, score_q and truncation at max_objects
 *   info      i32 [4] = (status, number of seeds, relaxation rounds that changed something, 0)
 *               C3D_SPLIT_ST_NOT_CONVERGED  round max_rounds still changed something: the outputs are those of the partition
 *                                           reached so far with the unreached pixels as label 0 -- in bounds, otherwise
 *                                           unspecified
 *               C3D_SPLIT_ST_BAD_LABELS     the component labelling reported its error word (counts[0] = -1 as well)
 *   identity  r2 == 0 gives exactly the outputs of c3d_scene_objects
 *   ws        c3d_scene_split_ws_bytes(Hs, Ws, n_cls) bytes, 256-byte aligned
 * Integer arithmetic and integer atomics only: two runs agree bit for bit.  Nothing is read back by the host, no workgroup waits
 * for another, every in-kernel loop is capped, and no workspace word is read before the call wrote it (a dirty workspace gives the
 * same result).  Launches on `stream`: the memsets of c3d_scene_objects and four more, the labelling (3), with r2 > 0 the transform (3), the core (1)
 * and the labelling of the core (3), the keys (1), max_rounds growth rounds -- round k returns at once when round k-1 changed
 * nothing, and only the tiles next to a change run --, the piece roots (2), the tail of c3d_scene_objects (6) and info (1).
 * Refused before anything is enqueued: what c3d_scene_objects refuses, r2 outside [0, 2^20], max_rounds outside [1, 65536], a
 * NULL info (C3D_E_BADARG); r2 > 0 with Hs or Ws > 16384, the limit of c3d_scene_edt (C3D_E_UNSUPPORTED).
 * c3d_scene_split_tile: out[0], out[1] = rows and columns of the tile that one workgroup grows in LDS.  Host only.            */
#define C3D_SPLIT_ST_NOT_CONVERGED 1
#define C3D_SPLIT_ST_BAD_LABELS 2
int64_t c3d_scene_split_ws_bytes(int32_t Hs, int32_t Ws, int32_t n_cls);      /* < 0: C3D_E_* */
int c3d_scene_split_tile(int32_t out[2]);
int c3d_scene_split(const uint8_t* mask, const uint8_t* cls_map, const float* score, int32_t Hs, int32_t Ws, int32_t connectivity,
                    int32_t min_area, int32_t n_cls, int32_t first_class, int32_t max_objects, int32_t r2, int32_t max_rounds,
                    int32_t* labels, int32_t* table, uint32_t* hist, uint8_t* object_cls, int32_t* counts, int32_t* info, void* ws,
                    void* stream);

/* Class regions of a scene map (csrc/scene_regions.hip): the connected components of EQUAL nonzero key of a u8 key map that is
 * already in HBM.  Two pixels belong to one region iff a path of 4-adjacent (connectivity 4) or 8-adjacent (connectivity 8)
 * pixels of the same key joins them; key 0 is background.  This is scipy.ndimage.label(key == k, structure) for every k, taken
 * together.  At connectivity 8 two regions of different keys may both pass through one lattice point (A B / B A); that is
 * allowed and is what the rule above defines.
 *   key       u8 [Hs][Ws];  score f32 [Hs][Ws] or NULL;  Hs * Ws < 2^31
 *   labels, table, counts and the min_area / max_objects / truncation behaviour are exactly those of c3d_scene_objects with
 *             "component" read as "region": regions are numbered 1 .. N in raster order of their first pixel over ALL keys
 *             together; row = (area, x0, y0, x1, y1, cls, first, score_q) with cls = the region's key, exact, 1 .. 255 (it is
 *             not a vote)
 *   object_key u8 [Hs][Ws] or NULL: the key where labels > 0, else 0
 *   ws        c3d_scene_regions_ws_bytes(Hs, Ws) bytes, 256-byte aligned
 *   identity  on a key map of 0 / 1 every output equals c3d_scene_objects on it as a mask without a class map, except column 5
 * Integer arithmetic and integer atomics only: two runs agree bit for bit, and a dirty workspace gives the same result.  Nine
 * launches and at most two memsets on `stream`: the keyed local and seam phases, then the flatten and the tail of
 * c3d_scene_objects (count, scan, number, relabel_stats, finalise), then the keys.  Nothing is read back, no workgroup waits
 * for another, every walk is capped as there (counts[0] = -1 at the cap).  Refused before anything is enqueued: what
 * c3d_scene_objects refuses.
 * c3d_scene_regions_tile: the extent of the LDS tile of the keyed local phase.  Host only.                                  */
int64_t c3d_scene_regions_ws_bytes(int32_t Hs, int32_t Ws);                   /* < 0: C3D_E_* */
int c3d_scene_regions_tile(int32_t* th, int32_t* tw);
int c3d_scene_regions(const uint8_t* key, const float* score, int32_t Hs, int32_t Ws, int32_t connectivity, int32_t min_area,
                      int32_t max_objects, int32_t* labels, int32_t* table, uint8_t* object_key, int32_t* counts, void* ws,
                      void* stream);

/* The sieve of a key map (csrc/scene_sieve.hip): regions below min_area are absorbed by the neighbour they share the longest
 * border with, in rounds, on the device.  All integers; tests/sieve_reference.py restates it.  One ROUND on the current map K:
 *   1 Take the regions of K as c3d_scene_regions does.  Each is identified by its root, the linear index of its first pixel,
 *     and has an area.  A region is SMALL iff area < min_area.  If none is small, stop: converged.
 *   2 For every small region r and every pixel side between a pixel of r and a 4-adjacent pixel q of the scene outside r, add 1
 *     to border(r, n), n = the region of q, or BG if K[q] == 0.  Always 4-adjacency: a border is counted in pixel sides.
 *     Sides on the scene's edge count for nobody.  (A 4-adjacent pixel of equal key is always in r, so n never has r's key.)
 *   3 The target t(r) is the neighbour with the largest (border, area(n), -root(n)), compared lexicographically; BG has area =
 *     the number of zero pixels of K and root = -1, so BG wins a full tie.  A small region without a neighbour has no target.
 *   4 r MOVES iff it has a target and t(r) is BG, or t(r) is not small, or (area(t), root(t)) > (area(r), root(r)).  This
 *     breaks every cycle; the small region with the smallest (area, root) that has a target always moves, so a round that has
 *     something to do does something.
 *   5 Every pixel of a moving region takes the key of the END of its chain r -> t(r) -> t(t(r)) -> ..: the first region that
 *     does not move, or 0 for BG.  If nothing moves, stop: converged (a small region that fills its surroundings stays).
 *   6 The next round runs on the new map: regions of equal key that an absorbed speck used to separate are one from then on.
 * The call stops when it has converged; or when max_rounds rounds have moved something and the map after them still has a
 * region that would move (C3D_SIEVE_ST_NOT_CONVERGED); or when a round's border table did not fit (C3D_SIEVE_ST_TABLE_FULL):
 * that round moves nothing and the output is the map before it, so no result depends on arrival order.
 *   key, score, connectivity, max_objects   as in c3d_scene_regions;  min_area in [1, 2^20];  max_rounds in [1, 65536]
 *   table_capacity  slots of the border table, a power of two in [16, 2^31], as c3d_regions_sieve_ws_bytes returned it: 0 there
 *             asks for the one that cannot overflow (twice the ordered pairs that the pixel sides of the scene can hold; a
 *             region pair is one entry however long its border).  A smaller one overflows for certain when a round has more
 *             pairs than slots; probes are capped at 4096
 *   key_out   u8 [Hs][Ws], the final map; must not alias key
 *   labels, table, counts   exactly c3d_scene_regions(key_out, min_area = 1)
 *   info      i32 [8] = (status, rounds that moved something, regions moved over all rounds, pixels whose key changed, small
 *             regions left, regions of the input, most table entries of a round, 0).  C3D_SIEVE_ST_BAD_LABELS: a capped walk
 *             reached its cap (counts[0] = -1 as well)
 *   identity  min_area <= 1 gives key_out == key, info[1] == 0 and the outputs of c3d_scene_regions
 *   ws        c3d_regions_sieve_ws_bytes(Hs, Ws, &table_capacity) bytes, 256-byte aligned
 * Integer atomics only (maxima, counts, one compare-and-swap that never spins): two runs agree bit for bit, a dirty workspace
 * gives the same result.  Launches on `stream`: at most four memsets and a copy, max_rounds + 1 rounds of nine launches (the
 * last round only finds out whether something would still move) -- every kernel of a round after the stopping one returns at
 * once on a device word, and the grids are sized by the compute units and the pixels --, the tail of c3d_scene_objects (5),
 * the keys and info.  Nothing is read back, no workgroup waits for another, every loop is capped.  Refused before anything is
 * enqueued: what c3d_scene_regions refuses, a NULL or aliasing key_out, a NULL info, min_area / max_rounds / table_capacity
 * outside their ranges (C3D_E_BADARG).                                                                                      */
#define C3D_SIEVE_ST_NOT_CONVERGED 1
#define C3D_SIEVE_ST_TABLE_FULL 2
#define C3D_SIEVE_ST_BAD_LABELS 4
int64_t c3d_regions_sieve_ws_bytes(int32_t Hs, int32_t Ws, int64_t* table_capacity);   /* < 0: C3D_E_* */
int c3d_regions_sieve(const uint8_t* key, const float* score, int32_t Hs, int32_t Ws, int32_t connectivity, int32_t min_area,
                      int32_t max_rounds, int32_t max_objects, int64_t table_capacity, uint8_t* key_out, int32_t* labels,
                      int32_t* table, int32_t* counts, int32_t* info /* [8] */, void* ws, void* stream);

/* ------------------------------------------------------------------------------------
 * Residual-stage step driver: ONE call enqueues every kernel of `blocks[i](x)` for a whole X3D residual
 * stage (reference model/x3d.py:331-412 = ResStage of ResBlocks, driven by `self.x3d.blocks[i](x)` at
 * reference model/trainer.py:126-139), forward or backward, from C++ -- the ~25 launches per block are no
 * longer issued one by one through Python/ctypes (19-22 ms of host time per B=32 step in round 1).
 *
 * All pointers are device pointers; parameter / gradient / BN-buffer pointers are the tensors of the
 * reference's own module tree (state-dict keys in the comments).  Gradients are ACCUMULATED (+=).
 * The forward workspace `ws_fwd` (c3d_stage_ws_bytes) holds every activation the backward pass re-reads
 * (a, b, c, shortcut, block outputs), the BatchNorm scale/shift and mean/rstd vectors, SE gates and the
 * f64 statistics accumulators; the caller keeps it alive until c3d_stage_bwd has run.  `ws_bwd` holds the
 * backward temporaries.  Weight gradients run on an internal side stream that forks from / joins `stream`
 * with events (C3D_WGRAD_SIDE=0 disables it); c3d_side_join makes `stream` wait for everything issued
 * there so far (call it before reading parameter gradients and before freeing ws_fwd / ws_bwd).
 * Size limit: every activation tensor of a stage whose channel counts are <= 224 must stay under 2 GiB (32-bit byte offsets in
 * the narrow pointwise kernels); c3d_stage_ws_bytes / c3d_stage_fwd / c3d_stage_bwd return C3D_E_UNSUPPORTED for a larger
 * geometry BEFORE touching the device (bf16 at 256 x 256, T = 3: B <= 96 per GPU; f32: B <= 48).
 * ------------------------------------------------------------------------------------ */
typedef struct c3d_bn_ptrs {
  const float* gamma; const float* beta;       /* .weight / .bias                                       */
  float* running_mean; float* running_var;     /* .running_mean / .running_var (updated in training)    */
  int64_t* num_batches_tracked;                /* .num_batches_tracked (incremented in training)        */
  float* dgamma; float* dbeta;                 /* gradients (may be NULL in c3d_stage_fwd)              */
} c3d_bn_ptrs;

typedef struct c3d_block_desc {
  int32_t cin, cinner, cout, stride;           /* dim_in, dim_inner, dim_out, spatial stride (1|2)      */
  int32_t se_width;                            /* 0 = no SqueezeExcitation in this block                */
  int32_t has_sc_conv, has_sc_bn;              /* branch1_conv / branch1_norm present                   */
  int32_t reserved;
  const float* w_a; const float* w_b; const float* w_c; const float* w_sc;   /* branch2.conv_{a,b,c}.weight, branch1_conv.weight */
  float* dw_a; float* dw_b; float* dw_c; float* dw_sc;
  c3d_bn_ptrs bn_a, bn_b, bn_c, bn_sc;         /* branch2.norm_a, norm_b.0, norm_c, branch1_norm        */
  const float* se_w1; const float* se_b1; const float* se_w2; const float* se_b2;   /* norm_b.1.block.{0,2}.{weight,bias} */
  float* dse_w1; float* dse_b1; float* dse_w2; float* dse_b2;
} c3d_block_desc;

/* c3d_stage_desc.flags: the unfused launch sequences stay callable so that the fused ones are testable against them
 * bit for bit (tests/test_model_gpu.py::test_folded_batchnorm_launches_are_bit_identical_end_to_end).                */
enum {
  C3D_STAGE_SEPARATE_FINALIZE = 1,   /* c3d_bn_finalize / c3d_bn_bwd_coef launches instead of the consumers' prologues     */
  C3D_STAGE_NO_WEIGHT_IMAGES = 2,    /* every GEMM workgroup converts the f32 weights itself (no c3d_pw_pack_weights)      */
  C3D_STAGE_SEPARATE_RESIDUAL = 4,   /* c3d_block_out_fwd launches instead of the next block's conv_a prologue             */
  C3D_STAGE_SEPARATE_WGRAD = 8       /* every pointwise weight gradient through c3d_pw_wgrad on the side stream (round 3's   */
                                     /* sequence) instead of fused into the data-gradient launch where the shape allows it  */
};

typedef struct c3d_stage_desc {
  int32_t n_blocks;
  int32_t B, T, H, W;                          /* stage INPUT extent; block 0 applies the stride        */
  int32_t dtype;                               /* activation storage type                               */
  int32_t training;                            /* 1: batch statistics (+ running-stat update), 0: eval  */
  int32_t flags;                               /* C3D_STAGE_* (0 = the fused, measured-best launch sequence) */
  float momentum, eps;                         /* BatchNorm3d momentum / eps (0.1 / 1e-5)               */
  const c3d_block_desc* blocks;                /* HOST array of n_blocks descriptors                    */
} c3d_stage_desc;

/* bytes of the two workspaces and of the stage output y [B][T][Ho][Wo][cpad(cout)] / input gradient dx */
int c3d_stage_ws_bytes(const c3d_stage_desc* d, int64_t* ws_fwd_bytes, int64_t* ws_bwd_bytes, int64_t* y_bytes,
                       int64_t* dx_bytes);
/* x: [B][T][H][W][cpad(cin)] channels-last, storage dtype.  y: stage output (also re-read by backward).      */
int c3d_stage_fwd(const c3d_stage_desc* d, const void* x, void* ws_fwd, void* y, void* stream);
/* dy: gradient of y (same layout); dx: gradient of x (written).  x / y / ws_fwd as given to c3d_stage_fwd.
 * The weight gradients that are not fused into their data-gradient launch (c3d_pw_wgrad) are launched on the library's side stream, each forked ahead
 * of the data-gradient kernel that reads the same operands, with their grids capped (7/8 of the CUs for the pointwise
 * kernel: csrc/pw_common.h pw_wgrad_cap) so that the data-gradient chain finds free CUs; ws_bwd holds a ring of
 * three blocks' temporaries (one slot more for dx, which is also the next block's g: c3d_pw_args.add_sums), so the side
 * stream may lag the chain by two blocks.                                                                        */
int c3d_stage_bwd(const c3d_stage_desc* d, const void* x, const void* y, const void* dy, void* ws_fwd, void* ws_bwd,
                  void* dx, void* stream);
/* c3d_side_join(stream): `stream` waits (on the device) for everything the library has issued on its side stream so far.
 * CONTRACT: the fork / done events between the two streams are created with hipEventDisableSystemFence -- they order the two
 * queues of ONE device and carry no system-scope release.  After c3d_side_join the weight gradients are visible to later work
 * on `stream` on this device; a consumer OUTSIDE the device -- a peer GPU (RCCL), the host reading p.grad -- must be ordered
 * behind `stream` by the caller's own system-scope operation: a default-flag event / hipStreamSynchronize / a stream-ordered
 * D2H copy or collective enqueued on `stream` (each of these releases at system scope when it completes).  torch's
 * stream.synchronize(), tensor.cpu() and torch.distributed collectives issued on `stream` all qualify
 * (tests/test_dp_gpu.py::test_side_join_then_host_readback_and_allreduce).                                                    */
int c3d_side_join(void* stream);
/* Run-time options of the library (process-wide; not thread-safe; all default to 1).  These are the ONLY run-time
 * switches: the product library never reads the environment (tuning knobs exist in the -DC3D_TUNING build only).
 *   C3D_OPT_SIDE_STREAM : 0 = weight gradients inline on the caller's stream (needed when the step is captured in a HIP
 *                         graph, and for one-kernel-at-a-time traces)
 *   C3D_OPT_STEM_MFMA   : 0 = scalar-FMA stem kernels (csrc/stem.hip) instead of the matrix-core ones (bit-identical
 *                         u / dv / dx: tests/test_model_gpu.py::test_stem_mfma_kernels_equal_the_scalar_kernels);
 *                         1 = f32 matrix-core kernels everywhere; 2 (default) = c3d_stem_bwd_wx of bf16 storage multiplies on
 *                         the bf16 matrix cores (x and w_t rounded to bf16 for the products, f32 sums)
 *   C3D_OPT_CONVT_MFMA  : 0 = scalar ConvTranspose2d kernels on the bf16 path too
 *   C3D_OPT_FUSE_WGRAD  : which pointwise weight gradients the stage driver fuses into their data-gradient launch where the
 *                         shape allows it (c3d_pw_args.wg_mode): bit 0 = conv_a, bit 1 = conv_c; default = measured best
 *   C3D_OPT_FOLD_SE     : 0 = c3d_bn_se_finalize launches for the blocks with SqueezeExcitation (default 1: conv_c's workgroups
 *                         compute the gate of their samples, c3d_pw_args.se_w1)
 *   C3D_OPT_MASK_IN_DGRAD : a BITFIELD, default 3 (the value is masked with 3).  bit 0: conv_a's data-gradient launch of the block
 *                         ABOVE stores dx * (y > 0) -- c3d_block_out_bwd of this block only sums; bit 1 (needs bit 0): the same
 *                         epilogue also takes this block's BatchNorm_c-backward sums (c3d_pw_args.add_sums / C3D_WG_MASKSUM) and
 *                         the c3d_block_out_bwd launch is gone (35 of 41 per BCD step).  0 = c3d_block_out_bwd does everything;
 *                         1 = the round-4 mask-only path (a caller that passes 1 meaning "on" gets THAT, not the default)
 *   C3D_OPT_DW_RING     : c3d_dw333_bwd_fused (bf16, stride 1) fed by an LDS-DMA ring (global_load_lds_dwordx4, two tiles ahead
 *                         for T <= 3, one for T = 5) instead of register prefetch: bit 0 = on, bit 2 = the requests are issued
 *                         one per tap step instead of in a burst, bit 3 = also on maps under 64 x 64; results are bit-identical
 *                         to the register-prefetch kernel; default 13 (round 6, same-call A/B: 20.13 -> 20.05 ms with bit 3)
 *   C3D_OPT_PW_WGRAD_V2 : 0 = c3d_pw_wgrad of bf16 dense rows on the first kernel (operand-split staging, 32-row tiles;
 *                         csrc/pw_wgrad.hip) instead of the flat-staged, transposing-read one (csrc/pw_wgrad_v2.hip, default 1);
 *                         same operand arithmetic, products summed in another order (f32 rounding apart); bit 1 SET = the stage
 *                         driver's separate weight gradients each launch their own reducer (default: chained,
 *                         c3d_pw_wgrad_args.chain -- bit-identical gradients either way)
 *   C3D_OPT_DW_FWD_HV   : c3d_dw333_fwd, stride 1, three frames, on half-vector lanes (a lane = 4 channels x 4 output rows, tap
 *                         walk column -> frame -> input row: half the LDS reads per FMA; csrc/dw_conv.hip): bit 0 = bf16
 *                         storage, bit 1 = f32 storage; the taps are summed in another order than the 8-channel lanes (f32
 *                         rounding apart); bit 2 = the STRIDE-2 forward (bf16) on eight waves per tile instead of four -- two
 *                         waves per channel vector, one half vector each; its 131 KB tile allows one workgroup per CU -- same
 *                         tap order per channel: bit-identical outputs.  Default 5
 *   C3D_OPT_PW_CFWD     : bit field, which forward GEMMs of the training path run on the workgroup-cooperative kernel
 *                         (csrc/pw_cfwd.hip) instead of the wave-private-tile one.  bit 0: conv_c (C3D_PRO_BN_SE_SWISH +
 *                         C3D_EPI_STATS, BatchNorm_b / SE gate rebuilt from the per-sample sums); bit 1: conv_a with the
 *                         previous block's residual add in its prologue (C3D_PRO_AFFINE2 + pro_out + C3D_EPI_STATS).
 *                         Outputs (and pro_out) bit-identical, BatchNorm statistics to f32 rounding.  Default 3
 *   C3D_OPT_PW_CDG      : bit field.  bit 0: the conv_a data gradient with its weight gradient fused (C3D_PRO_AFFINE2 +
 *                         C3D_EPI_ADD + C3D_WG_ROWS, dense shortcut gradient), bit 1: the conv_c one (C3D_PRO_AFFINE2 +
 *                         C3D_EPI_SWISH_SE_BWD + C3D_WG_SWISH, rows_per_sample a multiple of the tile's rows) run on the
 *                         workgroup-cooperative kernels (csrc/pw_cdgrad.hip) where they apply -- all three stage widths of
 *                         X3D-L, the 216-wide layers included, which the wave-private kernel's fused variant (accumulator
 *                         image in LDS) left to separate c3d_pw_wgrad launches; c3d_stage_bwd then asks for the fused form
 *                         there too.  Data gradients bit-identical, sums / dW to f32 rounding.  Default 3
 *   C3D_OPT_DW_T4       : four-frame clips (T = 4: building damage assessment, num_perception_frame = 2) run on four-frame
 *                         instantiations of c3d_dw333_fwd / c3d_dw333_bwd_fused (csrc/dw_conv.hip, csrc/dw_bwd_fused.hip): LDS
 *                         tile, staging slots, tap loops and accumulators sized for four frames, the bf16 stride-1 backward on
 *                         an LDS-DMA ring of two slots with the `a` rows in LDS.  0 = T = 4 runs on the five-frame (SCD)
 *                         instantiation with a zero fifth frame.  Same tap order per output: outputs and data gradients
 *                         bit-identical, statistics / dW to f32 rounding.  T <= 3 and T = 5 are not affected.  Default 1   */
enum { C3D_OPT_SIDE_STREAM = 0, C3D_OPT_STEM_MFMA = 1, C3D_OPT_CONVT_MFMA = 2, C3D_OPT_FUSE_WGRAD = 3, C3D_OPT_FOLD_SE = 4,
       C3D_OPT_MASK_IN_DGRAD = 5, C3D_OPT_DW_RING = 6, C3D_OPT_PW_WGRAD_V2 = 7, C3D_OPT_DW_FWD_HV = 8, C3D_OPT_PW_CFWD = 9,
       C3D_OPT_PW_CDG = 10, C3D_OPT_DW_T4 = 11 };
int c3d_set_option(int32_t option, int32_t value);
/* Per-launch profile of the stage driver: between c3d_prof_begin and c3d_prof_end every kernel c3d_stage_fwd /
 * c3d_stage_bwd enqueue is bracketed by a HIP event pair on its launch stream and billed its algorithmic bytes
 * (the tensors it must read / write once).  flags bit 0: weight gradients inline on the main stream (an event pair
 * then brackets exactly one kernel), bit 1: pointwise rows are keyed by shape and mode.  c3d_prof_end synchronises
 * the device and returns one row per kernel entry (aggregated).  Not thread-safe; meant for bench.py / tools.      */
typedef struct c3d_prof_row {
  char name[64];
  int32_t launches, reserved;
  float ms_total, reserved2;
  double bytes_total;
} c3d_prof_row;
int c3d_prof_begin(int32_t flags);
int c3d_prof_end(c3d_prof_row* rows, int32_t cap, int32_t* n_rows);
/* Eval / inference (reference scripts/train_BCD.py:92-154 `val()` under model.eval() + torch.no_grad()): BatchNorm
 * folded into the convolution weights.  c3d_stage_fold_bn writes, once per set of weights, W' = W * gamma/sqrt(var+eps)
 * (rows of conv_a / conv_b / conv_c / branch1_conv) and the remaining per-channel biases into `fold`
 * (c3d_stage_fold_bytes); c3d_stage_fwd_folded then runs the stage with 4-5 launches per block (no statistics, no
 * finalize kernels, no saved activations: `ws` is a small ring of c3d_stage_fold_bytes' ws_eval_bytes).          */
int c3d_stage_fold_bytes(const c3d_stage_desc* d, int64_t* fold_bytes, int64_t* ws_eval_bytes);
int c3d_stage_fold_bn(const c3d_stage_desc* d, void* fold, void* stream);
int c3d_stage_fwd_folded(const c3d_stage_desc* d, const void* fold, const void* x, void* ws, void* y, void* stream);
/* byte offsets (into ws_fwd) and sizes of what block `blk` stored: name is one of "a","b","c","sc","mr_a","mr_b",
 * "mr_c","mr_sc","ss_a","ss_b","ss_c","ss_sc","gate" -- test / debug access (returns C3D_E_BADARG if absent). */
int c3d_stage_saved(const c3d_stage_desc* d, int32_t blk, const char* name, int64_t* offset, int64_t* bytes);
/* name of the kernel the calling thread launched last through the library's large-LDS launcher (every pointwise GEMM,
 * weight-gradient, depthwise, stem, decoder and attention kernel goes through it), with its template arguments as the
 * demangler spells them (bf16 storage is `unsigned short`), e.g. "dw_fwd_v2_kernel<unsigned short, 3, true, true>"; ""
 * before the first launch.  Host-only, test / debug: the dispatchers fall through to another kernel where one does not
 * apply, and this is how a test knows which one it measured.  The string belongs to the calling thread and is valid until
 * its next call.                                                                                                     */
const char* c3d_last_kernel(void);
/* how many kernels the calling thread has launched through that launcher so far.  c3d_pw_gemm may answer one call with two
 * of them (a workgroup's rows span more samples than its in-kernel SE gate holds: c3d_bn_se_finalize, then the GEMM), and
 * the name above is the GEMM's either way; the difference of this count around a call tells the two apart.  Host-only. */
int64_t c3d_launch_count(void);

/* ------------------------------------------------------------------------------------
 * Caption decoder of the change-captioning path (reference model/caption_decoder.py:526-613 CaptionDecoder, :316-423
 * Mesh_TransformerDecoderLayer, :272-314 PositionalEncoding; loss: scripts/train_CC.py:124-132).  Activations are
 * sequence-first rows (row = l*B + b, nn.MultiheadAttention's default layout) of Dp = round_up(D, 8) elements in the
 * storage dtype; the linear layers run on c3d_pw_gemm / c3d_pw_wgrad (bias through c3d_pw_args.bias, bias gradient
 * through c3d_col_sum).  Dropout masks are counter-based: (seed, element index) -> keep/drop, regenerated in backward.
 * ------------------------------------------------------------------------------------ */
/* out[l*B+b] = dropout_p(emb[tokens[b][l]] + pe[l]); tokens int64 [B][L]; emb f32 [V][D]; pe f32 [>=L][D].  A token
 * outside [0, V) is clamped to the nearest valid row (0 or V-1), in the forward and in the gradient alike: no read or
 * atomic ever leaves the table.  Padding columns of out are written as 0.                                          */
int c3d_cap_embed_fwd(const int64_t* tokens, const float* emb, const float* pe, void* out, int32_t B, int32_t L,
                      int32_t D, int32_t V, float p, uint64_t seed, int32_t dtype, void* stream);
/* demb[tokens[b][l]] += dropout-mask * dout[l*B+b]   (f32 atomics)                                                */
int c3d_cap_embed_bwd(const int64_t* tokens, const void* dout, float* demb, int32_t B, int32_t L, int32_t D, int32_t V,
                      float p, uint64_t seed, int32_t dtype, void* stream);
/* y = x * mask(seed) / (1-p): the same call is the forward and (on the gradient) the backward                     */
int c3d_cap_dropout(const void* x, void* y, int64_t rows, int32_t D, float p, uint64_t seed, int32_t dtype, void* stream);
/* y = LayerNorm(x + a) (a may be NULL), mr f32 [rows][2] = saved (mean, rstd); backward: dx (= gradient of x and of a),
 * dgamma / dbeta accumulated (+=)                                                                                 */
int c3d_cap_layernorm_fwd(const void* x, const void* a, const float* gamma, const float* beta, void* y, float* mr,
                          int64_t rows, int32_t D, float eps, int32_t dtype, void* stream);
int c3d_cap_layernorm_bwd(const void* x, const void* a, const void* dy, const float* gamma, const float* mr, void* dx,
                          float* dgamma, float* dbeta, int64_t rows, int32_t D, int32_t dtype, void* stream);
/* multi-head attention, one workgroup per (sample, head): q/k/v/o rows (l*B+b) with leading dimensions ld* (elements),
 * head h at column h*hd; P f32 [H*B][Lq][Lk] = softmax(scale*q.k^T (+causal mask)) BEFORE dropout (saved for backward);
 * o = dropout_p(P) v.  hd <= 64 (C3D_E_BADARG beyond).  Each (sample, head) lives in LDS, with hs = hd | 1:
 *   forward  4 * (2*Lk*hs + Lq*hs + 4*Lk)      bytes,
 *   backward 4 * (2*Lk*hs + 2*Lq*hs + Lq*Lk)   bytes (the whole [Lq][Lk] matrix),
 * and either entry returns C3D_E_UNSUPPORTED, writing nothing, above 160 KB.  The backward limit is the tighter one (Lq 52,
 * hd 24: Lk <= 376 against Lk <= 734): a caller that trains must check the backward size before it runs the forward
 * (model/caption_decoder.py check_attention_geometry).                                                             */
int c3d_cap_attn_fwd(const void* q, const void* k, const void* v, int32_t ldq, int32_t ldk, int32_t ldv, void* o, int32_t ldo,
                     float* P, int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd, float scale, int32_t causal,
                     float p, uint64_t seed, int32_t dtype, void* stream);
int c3d_cap_attn_bwd(const void* q, const void* k, const void* v, int32_t ldq, int32_t ldk, int32_t ldv, const void* dout,
                     int32_t ldo, const float* P, void* dq, void* dk, void* dv, int32_t lddq, int32_t lddk, int32_t lddv,
                     int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd, float scale, float p, uint64_t seed,
                     int32_t dtype, void* stream);
/* CrossEntropyLoss(ignore_index) over the decoded steps (pack_padded_sequence of scripts/train_CC.py:124-132 without the
 * gather): logits rows (l*B+b) of round_up(V,8) columns; target = caps[b][l+1] (caps int64 [B][L], sorted by length);
 * a step counts iff l < declen[b] (int64 [B]) and target != ignore_index; loss = mean; lse f32 [L*B];
 * acc2 f64 [3] = (sum of the negative log-likelihoods, counted steps, top-1 hits = caption_accuracy(scores, targets, 1)
 * of reference model/utils.py:493-507 before its percentage scaling).  A counted step whose target lies outside [0, V)
 * makes the loss NaN (torch.nn.CrossEntropyLoss trips a device assert there): never silently ignored.  The last step
 * (l = L-1) has no target and never counts.  When NO step counts (every declen 0, or every target ignore_index) the loss
 * is 0, acc2 = (0, 0, 0) and c3d_cap_ce_bwd writes a zero gradient -- torch's mean over nothing would be NaN; here such a
 * batch is a step without a decoder update, not a poisoned one.                                                    */
int c3d_cap_ce_fwd(const void* logits, const int64_t* caps, const int64_t* declen, double* acc2, float* lse, float* loss,
                   int32_t B, int32_t L, int32_t V, int64_t ignore_index, int32_t dtype, void* stream);
int c3d_cap_ce_bwd(const void* logits, const int64_t* caps, const int64_t* declen, const double* acc2, const float* lse,
                   const float* dloss, void* dlogits, int32_t B, int32_t L, int32_t V, int64_t ignore_index, int32_t dtype,
                   void* stream);
/* clip_gradient (reference model/utils.py:481-491): g = clamp(g, -limit, limit) over a flat f32 gradient buffer with
 * torch.clamp_'s semantics: +-inf go to the limit, NaN stays NaN (clipping never hides a diverged gradient);
 * limit <= 0 or NaN is C3D_E_BADARG.                                                                               */
int c3d_clamp_(float* g, int64_t n, float limit, void* stream);

/* ------------------------------------------------------------------------------------
 * Batched beam search of the captioning evaluation (reference scripts/train_CC.py:214-330, the loop inside `evaluate()`,
 * with the decoder arithmetic of model/caption_decoder.py:316-423 / :526-613 in evaluation mode): one workgroup per image
 * pair runs the whole search -- incremental decoding over a key/value cache, log-softmax, top-k and all beam bookkeeping on
 * the device, no host synchronisation, no wait on another workgroup.  Semantics of the reference loop, kept: at step 1 only
 * hypothesis 0 is expanded; a hypothesis leaves the beam when it emits end_id and the beam shrinks; the loop ends when the
 * beam is empty or after step max_len - 1; completed hypotheses are recorded in rank order within a step; the winner is the
 * FIRST maximum of the completed scores (-1: no hypothesis completed, no caption); scores accumulate in f32.  Equal
 * candidate scores are ordered by the lower flat index hypothesis * V + word (torch.topk documents no order).
 * ------------------------------------------------------------------------------------ */
#define C3D_CAP_BEAM_MAX 8      /* hypotheses per pair */
#define C3D_CAP_BEAM_LAYERS 8   /* decoder layers */
typedef struct c3d_cap_beam_layer {
  const float *sa_in_w, *sa_in_b;   /* self_attn.in_proj_weight [3D][D], in_proj_bias [3D] */
  const float *sa_out_w, *sa_out_b; /* self_attn.out_proj [D][D], [D] */
  const float *n1_g, *n1_b;         /* norm1 */
  const float *ca_q_w, *ca_q_b;     /* multihead_attn2.in_proj_weight[:D] [D][D], in_proj_bias[:D] */
  const float *ca_out_w, *ca_out_b; /* multihead_attn2.out_proj */
  const float *n2_g, *n2_b;         /* norm2 */
  const void* kv;                   /* projected memory of ALL pairs, rows (s*B + b) of [K | V] = 2D elements of `dtype`:
                                     * indexed by pair, shared by the pair's hypotheses */
} c3d_cap_beam_layer;
typedef struct c3d_cap_beam_args {
  int32_t B, S, D, H, n_layer, V, beam, max_len, start_id, end_id, dtype;
  float ln_eps;
  const float *emb, *pe;            /* vocab_embedding.weight [V][D]; position table [>= max_len][D] */
  const float *wdc_w, *wdc_b;       /* vocabulary projection [V][D], [V] */
  c3d_cap_beam_layer layers[C3D_CAP_BEAM_LAYERS];
  void* ws;                         /* c3d_cap_beam_plan's ws_bytes: the self-attention key/value cache */
  /* results, per pair: completed hypotheses in the order they completed */
  int32_t* comp_seq;                /* [B][beam][max_len + 1], start token first; the caller zeroes it */
  int32_t* comp_len;                /* [B][beam] */
  float* comp_score;                /* [B][beam] */
  int32_t* meta;                    /* [B][4]: completed count, winner index or -1, steps decoded, live count at the end */
  /* optional (NULL: off).  trace [B][max_len-1][1 + 3*beam] int32, zeroed by the caller: per step the live count before the
   * step, then per selected candidate in rank order (parent, word, score as f32 bits).
   * Test surface: forced [B][max_len-1][beam][2] int32 = (parent, word) taken INSTEAD of the top-k (teacher forcing; scores
   * are still the candidates'); logits_out f32 [B][max_len-1][beam][V]: the vocabulary logits of every expanded hypothesis. */
  int32_t* trace;
  const int32_t* forced;
  float* logits_out;
} c3d_cap_beam_args;
/* The limits, host only (no runtime call): 0 and the workspace / dynamic-LDS bytes of a search over B pairs, or
 * C3D_E_UNSUPPORTED (nothing may be launched): beam <= 8, n_layer <= 8, D a multiple of 8 and <= 256, head width D/H <= 32,
 * max_len <= 64, and an LDS plan (hidden rows, k x V f32 logits, one probability row of max(S, max_len) per wave) within
 * 160 KB -- at D = 192, V = 501: S <= 3000 for every beam.                                                         */
int c3d_cap_beam_plan(int32_t S, int32_t D, int32_t H, int32_t n_layer, int32_t V, int32_t beam, int32_t max_len,
                      int32_t dtype, int64_t B, int64_t* ws_bytes, int64_t* lds_bytes);
/* Replaces the per-pair host loop of reference scripts/train_CC.py:248-330 (one decoder pass over the whole 52-token window
 * per step, torch topk, host bookkeeping).  One launch on `stream`; C3D_E_UNSUPPORTED exactly where the plan says so. */
int c3d_cap_beam_search(const c3d_cap_beam_args* a, void* stream);

/* ------------------------------------------------------------------------------------
 * Caption metrics of the captioning validation (csrc/caption_metrics.hip): the BLEU-1..4 statistics, ROUGE-L and CIDEr of
 * reference eval_func/bleu/bleu_scorer.py:60-83, rouge/rouge.py:23-128, cider/cider_scorer.py:93-182 and the change /
 * no-change bookkeeping of scripts/train_CC.py:347-376, on token ids.  Integers are exact; ROUGE-L and CIDEr are float64 with
 * the reference's operations (sums in ascending first-occurrence position).  METEOR is not computed.
 * Sentences are compact rows of L <= 64 int32 tokens in [0, 65534] with their lengths; at most 7 references per image and 8
 * no-change sentences (C3D_E_UNSUPPORTED beyond).
 * ------------------------------------------------------------------------------------ */
#define C3D_CAP_METRICS_MAX_REFS 7
#define C3D_CAP_METRICS_MAX_NOCHANGE 8
#define C3D_CAP_TOTALS 17
/* out [rows][64] / out_len [rows] = the tokens of raw [rows][L_in] that are none of start_id / end_id / pad_id, in order (the
 * list comprehension of reference scripts/train_CC.py:336-343), the rest of the row -1.  A row that keeps more than 64 tokens
 * keeps its first 64 and reports its true length, which c3d_cap_metrics refuses as a bad sentence.  One launch.          */
int c3d_cap_strip(const int32_t* raw, int64_t rows, int32_t L_in, int32_t start_id, int32_t end_id, int32_t pad_id,
                  int32_t* out, int32_t* out_len, void* stream);
typedef struct c3d_cap_metrics_args {
  int32_t N, R, L, M;               /* images of the corpus, references per image, row stride (<= 64), selected images */
  int32_t n_nochange, reserved;     /* rows of `nochange` (0: no bookkeeping) */
  int64_t table_capacity;           /* slots of the document-frequency table, a power of two (c3d_cap_metrics_plan) */
  const int32_t *hyp, *hyp_len;     /* [N][L], [N]; a hypothesis may be empty */
  const int32_t *refs, *ref_len;    /* [N][R][L], [N][R]; a reference may not be empty */
  const int32_t* sel;               /* [M] image indices or NULL (M = N, every image in order).  The document frequency is
                                     * counted over the selected images only: one upload serves every subset */
  const int32_t *nochange, *nochange_len;   /* [n_nochange][L], [n_nochange] or NULL */
  void* ws;                         /* ws_bytes of the plan, 256-byte aligned; zeroed inside the call.  After the call:
                                     * u32 status at 0, u64 keys [capacity] at 256, u32 counts [capacity] behind them -- an
                                     * n-gram's key is four 16-bit fields of token + 1, first token lowest, 0 = no token;
                                     * slot order varies from run to run, counts do not (test / debug access) */
  /* per selected image, in selection order */
  int32_t* stats;                   /* [M][10] testlen, closest reference length (a tie goes to the shorter), guess[4], correct[4] */
  int32_t* lcs;                     /* [M][R] LCS length of the hypothesis and each reference */
  int32_t* flags;                   /* [M] bit 0: reference 1 (reference 0 when R == 1) is a no-change sentence; bit 1: the
                                     * hypothesis is one */
  double *rouge, *cider;            /* [M] */
  int64_t* totals;                  /* [C3D_CAP_TOTALS]: 0..9 the column sums of stats; 10 images with flag bit 0; 11 those of
                                     * them with bit 1; 12 images without bit 0; 13 those of them without bit 1; 14 / 15 the sums
                                     * of rouge / cider (float64 bits, fixed-order tree); 16 status, 0 = fine, else bits: 1 the
                                     * table is full (a probe reached its cap of `table_capacity` steps; cider is 0 then), 2 a
                                     * selection index outside [0, N) (the image scores 0), 4 a sentence with a length outside
                                     * [0, L], a token outside [0, 65534] or an empty reference (scored as empty) */
} c3d_cap_metrics_args;
/* Host only.  table_capacity is in/out: <= 0 asks for the default, the next power of two >= 2 * 4 * ref_tokens (ref_tokens =
 * the sum of the reference lengths; <= 0: N * R * L) -- at most half full with every n-gram distinct; a positive value must be
 * a power of two and is kept (C3D_E_BADARG otherwise).  ws_bytes = 256 + 12 * table_capacity.                          */
int c3d_cap_metrics_plan(int32_t N, int32_t R, int32_t L, int64_t ref_tokens, int64_t* ws_bytes, int64_t* table_capacity);
/* One memset and three launches on `stream` (statistics and table, CIDEr, reduction); nothing is read back by the host. */
int c3d_cap_metrics(const c3d_cap_metrics_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CHANGE3D_HIP_H */
