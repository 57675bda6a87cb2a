// Device-side pieces shared by the workgroup-cooperative pointwise kernels (pw_cfwd.hip, pw_cdgrad.hip, pw_wgrad_v2.hip): rows
// come in through bounds-checked buffer resources as flat 16-byte items, the packed weight image through LDS-DMA.
// The rotated weight-image DMA loop itself stays in each kernel: as a function it compiles to a different branch layout.
// (pw_gemm_impl.h keeps its own BufIO / Raw: templated on the storage type.)
#pragma once
#include "common.h"

namespace {

// Offset of a lane without an item: out of range of every resource (a call's tensors stay under 2 GiB, pw_common.h
// pw_fits_u32), so the load returns zeros, touches no memory and still counts in vmcnt -- counted waits stay exact.
constexpr uint32_t CO_OOB = 0x80000000u;

typedef uint32_t co_u32x4_t __attribute__((ext_vector_type(4)));
typedef short co_s16x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* co_lds_ptr_t;
typedef const __attribute__((address_space(1))) void* co_glb_ptr_t;
typedef __attribute__((address_space(3))) co_s16x4_t* co_lds_s16x4_ptr_t;   // operand of the transposing LDS read

__device__ __forceinline__ __amdgpu_buffer_rsrc_t co_rsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, p ? (int)bytes : 0, 0x00020000);
}
__device__ __forceinline__ uint4 co_load(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  const co_u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
  return make_uint4(v[0], v[1], v[2], v[3]);
}
// bf16 x 8 -> f32 x 8
__device__ __forceinline__ void co_cvt(const uint4& v, float (&f)[8]) {
  f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
  f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
  f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}
// eight consecutive floats of LDS
__device__ __forceinline__ void co_ld8(const float* p, float (&f)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

}  // namespace
