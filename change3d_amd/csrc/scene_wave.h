// Integer wave and workgroup helpers of the scene files: reductions and scans over the 64 lanes of a wave by shuffles, and
// over the waves of a workgroup through one word of LDS per wave.  Integers only, so the grouping changes no result.
// (common.h has the float wave_sum.)  A file that needs one includes this header and keeps no copy.
#pragma once
#include "common.h"

namespace c3d_wave {

typedef unsigned long long u64;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_max64(u64 v) {
  for (int d = 32; d; d >>= 1) {
    const u64 o = shfl64(v, (int)((threadIdx.x & 63) ^ d));
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ u64 wave_min64(u64 v) {
  for (int d = 32; d; d >>= 1) {
    const u64 o = shfl64(v, (int)((threadIdx.x & 63) ^ d));
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ u64 wave_sum64(u64 v) {
  for (int d = 32; d; d >>= 1) v += shfl64(v, (int)((threadIdx.x & 63) ^ d));
  return v;
}
__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
  for (int d = 32; d; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
  return v;
}
__device__ __forceinline__ uint32_t wave_min32u(uint32_t v) {
  for (int d = 32; d; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, d);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ int wave_min32(int v) {
  for (int d = 32; d; d >>= 1) {
    const int o = __shfl_xor(v, d);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ int wave_max32(int v) {
  for (int d = 32; d; d >>= 1) {
    const int o = __shfl_xor(v, d);
    v = o > v ? o : v;
  }
  return v;
}
// exclusive prefix sum over the lanes of a wave; *all = the wave's sum
__device__ __forceinline__ uint32_t wave_excl_scan32(uint32_t v, uint32_t* all) {
  const int lane = threadIdx.x & 63;
  uint32_t inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = (uint32_t)__shfl((int)inc, lane >= d ? lane - d : lane);
    if (lane >= d) inc += t;
  }
  *all = (uint32_t)__shfl((int)inc, 63);
  return inc - v;
}

// exclusive prefix of v over the workgroup's threads; `all` = the sum.  part: one word of LDS per wave; the caller syncs
// before reusing it
__device__ __forceinline__ u64 block_excl_scan64(u64 v, u64* part, u64* all) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  u64 inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const u64 t = shfl64(inc, lane >= d ? lane - d : lane);
    if (lane >= d) inc += t;
  }
  if (lane == 63) part[wave] = inc;
  __syncthreads();
  u64 before = 0, sum = 0;
  for (int w = 0; w < waves; ++w) {
    before += w < wave ? part[w] : 0ull;
    sum += part[w];
  }
  *all = sum;
  return before + inc - v;
}

// the same for 32-bit sums.  WAVES: the waves of the workgroup where the caller knows them, so that the loop over them unrolls
template <int WAVES = 0>
__device__ __forceinline__ uint32_t block_excl_scan32(uint32_t v, uint32_t* part, uint32_t* all) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = WAVES ? WAVES : (int)(blockDim.x >> 6);
  uint32_t total;
  const uint32_t excl = wave_excl_scan32(v, &total);
  if (lane == 63) part[wave] = total;
  __syncthreads();
  uint32_t before = 0, sum = 0;
  for (int w = 0; w < waves; ++w) {
    before += w < wave ? part[w] : 0u;
    sum += part[w];
  }
  *all = sum;
  return before + excl;
}

// exclusive prefix maximum of v (>= -1) over the workgroup's threads; `all` = the maximum.  part as above
__device__ __forceinline__ int block_excl_max32(int v, int* part, int* all) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  int inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl(inc, lane >= d ? lane - d : lane);
    if (lane >= d) inc = t > inc ? t : inc;
  }
  const int up = __shfl(inc, lane ? lane - 1 : 0);
  if (lane == 63) part[wave] = inc;
  __syncthreads();
  int before = -1, top = -1;
  for (int w = 0; w < waves; ++w) {
    if (w < wave) before = part[w] > before ? part[w] : before;
    top = part[w] > top ? part[w] : top;
  }
  *all = top;
  const int mine = lane ? up : -1;
  return mine > before ? mine : before;
}

}  // namespace c3d_wave
