// Launch hints passed between translation units of the library (not part of the C ABI).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>
#include "../../include/change3d_hip.h"

// Set by the stage driver around launches it places on its side stream; read by pw_wgrad_cap (pw_common.h), defined in pw_wgrad.hip
extern thread_local int c3d_side_launch;

// The runtime switches of c3d_set_option: defined in options.hip, documented at their ids in include/change3d_hip.h
extern int c3d_option_stem_mfma;       // C3D_OPT_STEM_MFMA
extern int c3d_option_convt_mfma;      // C3D_OPT_CONVT_MFMA
extern int c3d_option_dw_ring;         // C3D_OPT_DW_RING
extern int c3d_option_pw_wgrad_v2;     // C3D_OPT_PW_WGRAD_V2, bit 0
extern int c3d_option_dw_fwd_hv;       // C3D_OPT_DW_FWD_HV
extern int c3d_option_pw_cfwd;         // C3D_OPT_PW_CFWD
extern int c3d_option_pw_cdg;          // C3D_OPT_PW_CDG
extern int c3d_option_dw_t4;           // C3D_OPT_DW_T4
// ...and the ones the stage driver alone reads: kept out of the library's dynamic symbol table
#pragma GCC visibility push(hidden)
extern int c3d_option_side_stream;     // C3D_OPT_SIDE_STREAM
extern int c3d_option_fuse_wgrad;      // C3D_OPT_FUSE_WGRAD
extern int c3d_option_fold_se;         // C3D_OPT_FOLD_SE
extern int c3d_option_mask_in_dgrad;   // C3D_OPT_MASK_IN_DGRAD
extern int c3d_option_wgrad_chain;     // C3D_OPT_PW_WGRAD_V2, bit 1 clear
#pragma GCC visibility pop
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
void c3d_detail_pw_wgrad_v2_forget(const float* ws);   // pending partials of a chained c3d_pw_wgrad launch that sit in `ws`: forgotten, NOT reduced
