// Launch hints passed between translation units of the library (not part of the C ABI).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>
#include "../../include/change3d_hip.h"

// Set by the stage driver around launches it places on its side stream; read by pw_wgrad_cap (pw_common.h), defined in pw_wgrad.hip
extern thread_local int c3d_side_launch;

// c3d_set_option (stage_driver.hip): kernel-family selectors with a parity test between the two implementations
extern int c3d_option_stem_mfma;    // 2: + c3d_stem_bwd_wx of bf16 storage on the bf16 matrix cores, 1: stem on the f32 matrix cores
                                    // (stem_mfma.hip), 0: scalar-FMA kernels (stem.hip)
extern int c3d_option_convt_mfma;   // 1: bf16 ConvTranspose2d on the matrix cores (convt_mfma.hip), 0: decoder.hip's
extern int c3d_option_dw_ring;      // C3D_OPT_DW_RING (include/change3d_hip.h): LDS-DMA ring variant of the bf16 stride-1 depthwise backward
extern int c3d_option_dw_fwd_hv;     // C3D_OPT_DW_FWD_HV: stride-1 three-frame depthwise forward on half-vector lanes (bit 0 bf16, bit 1 f32 storage)
extern int c3d_option_dw_t4;         // C3D_OPT_DW_T4: four-frame clips (BDA) on the TT = 4 instantiations of the depthwise kernels (0: the five-frame ones)
extern int c3d_option_pw_cfwd;       // C3D_OPT_PW_CFWD: conv_c forward of the training path on csrc/pw_cfwd.hip
extern int c3d_option_pw_cdg;        // C3D_OPT_PW_CDG: conv_a (bit 0) / conv_c (bit 1) data + weight gradient on csrc/pw_cdgrad.hip
// The cooperative conv_a / conv_c data + weight gradient (pw_cdgrad.hip).  _shape: does the kernel hold the layer (workspace
// plans, made before any pointer exists); _accepts: does the launch function take exactly these arguments -- the stage driver
// skips the separate weight-gradient launch on it.  parts_out != NULL: the partials stay in wg_ws, their count is reported
// and the caller launches c3d_detail_pw_wgrad_reduce; NULL: the reducer follows on `stream`.
bool c3d_detail_pw_cdg_a_shape(int Kp, int Np, int64_t M);
bool c3d_detail_pw_cdg_c_shape(int Kp, int Np, int64_t M, int64_t rows_per_sample);
bool c3d_detail_pw_cdg_a_accepts(const c3d_pw_args* args);
bool c3d_detail_pw_cdg_c_accepts(const c3d_pw_args* args);
int c3d_detail_pw_cdg_a(const c3d_pw_args* args, int* parts_out, void* stream);
int c3d_detail_pw_cdg_c(const c3d_pw_args* args, int* parts_out, void* stream);
int c3d_detail_pw_wgrad_reduce(const float* ws, float* dw, int N, int K, int parts, int sn, int sk, hipStream_t stream);   // pw_wgrad.hip
extern int c3d_option_pw_wgrad_v2;  // C3D_OPT_PW_WGRAD_V2: 1 = c3d_pw_wgrad of bf16 dense rows on csrc/pw_wgrad_v2.hip, 0 = pw_wgrad.hip's kernel
void c3d_detail_pw_wgrad_v2_forget(const float* ws);   // pending partials of a chained c3d_pw_wgrad launch that sit in `ws`: forgotten, NOT reduced
