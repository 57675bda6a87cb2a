// The three stages of c3d_scene_objects (csrc/scene_objects.hip) as host functions, for the entries that build on them
// (csrc/scene_split.hip).  c3d_scene_objects itself is clear + label_roots + objects_tail; the kernels live in
// scene_objects.hip only.  The front of every such workspace is the one of c3d_scene_label_ws_bytes: a header of 256 bytes
// (word 0: the error word of the union-find walks, word 1: the objects found; the words from C3D_DETAIL_HEADER_FREE on are
// the caller's), then the u32 [N] of areas at c3d_detail_area_offset().
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

enum { C3D_DETAIL_WS_ERR = 0, C3D_DETAIL_WS_FOUND = 1, C3D_DETAIL_HEADER_FREE = 8, C3D_DETAIL_HEADER_WORDS = 64 };

// area[r] += 1 for every lane with r >= 0, called by whole waves.  One atomic per wave and root for the two most frequent
// leaders' roots (a wave is 64 consecutive pixels: inside a large object all of them share the root), one per lane for what
// is left.
__device__ __forceinline__ void c3d_detail_wave_area_add(uint32_t* area, int r) {
  const int lane = threadIdx.x & 63;
  bool open = r >= 0;
  for (int round = 0; round < 2; ++round) {
    const unsigned long long m = __ballot(open);
    if (!m) break;
    const int leader = __ffsll((long long)m) - 1;
    const int r0 = __shfl(r, leader);
    const unsigned long long same = __ballot(open && r == r0);
    if (lane == leader) atomicAdd(area + r0, (uint32_t)__popcll(same));
    if (r == r0) open = false;
  }
  if (open) atomicAdd(area + r, 1u);
}

// ------------------------------------------------------------------------------------------------ the union-find walks
// of the labelling kernels (csrc/scene_objects.hip, csrc/scene_regions.hip): parent pointers towards the smaller index, a
// root points at itself.  Every walk is capped and sets the error word where the cap is reached.
constexpr int C3D_DETAIL_TILE = 64 * 64;                   // cells of the LDS tile of a local phase: the cap of a walk inside it

__device__ __forceinline__ int ld_agent(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ld_wg(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// root of `a` in the LDS tile; parents are read while other waves lower them, which only shortens the walk
__device__ __forceinline__ int lds_find(const int32_t* lab, int a, uint32_t* err) {
  for (int step = 0; step <= C3D_DETAIL_TILE; ++step) {
    const int p = ld_wg(lab + a);
    if (p == a) return a;
    a = p;
  }
  atomicOr(err, 1u);
  return a;
}

__device__ __forceinline__ void lds_unite(int32_t* lab, int a, int b, uint32_t* err) {
  for (int step = 0; step <= C3D_DETAIL_TILE; ++step) {
    a = lds_find(lab, a, err);
    b = lds_find(lab, b, err);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(lab + a, b);
    if (old == a) return;
    a = old;
  }
  atomicOr(err, 1u);
}

// Parents are read with agent-scope atomic loads: a plain load could see an older parent from another XCD's L2.  Even that
// would be correct -- a stale "root" fails its atomicMin (old != a) and the loop goes on from `old` -- but the walk is shorter
// with current values.
__device__ __forceinline__ int g_find(const int32_t* L, int a, int cap, uint32_t* err) {
  for (int step = 0; step <= cap; ++step) {
    const int p = ld_agent(L + a);
    if (p == a) return a;
    a = p;
  }
  atomicOr(err, 1u);
  return a;
}

__device__ __forceinline__ void g_unite(int32_t* L, int a, int b, int cap, uint32_t* err) {
  for (int step = 0; step <= cap; ++step) {
    a = g_find(L, a, cap, err);
    b = g_find(L, b, cap, err);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(L + a, b);                   // device scope: performed at the memory side, seen by every XCD
    if (old == a) return;
    a = old;
  }
  atomicOr(err, 1u);
}

int64_t c3d_detail_label_ws_bytes(int64_t N, int n_cls);   // what c3d_scene_label_ws_bytes returns for N pixels
int64_t c3d_detail_area_offset();                          // byte offset of the u32 [N] of areas
int64_t c3d_detail_ssum_offset(int64_t N);                 // byte offset of the u64 score sums, one per table row

// The memsets: header and areas, and the score sums and votes of the rows that can be used.  hist / n_cls as the entry got them.
int c3d_detail_objects_clear(void* ws, int64_t N, const uint8_t* cls_map, const float* score, int n_cls, uint32_t* hist,
                             int max_objects, hipStream_t st);

// Launches 1..3 (local, seam, flatten): L[p] = the smallest linear index of p's component, -1 on the background.  `area`
// u32 [N], zeroed, gets the pixel count at every root; NULL: not counted.  `phases` < 3 stops after that many launches
// (the instrumented build of c3d_scene_objects; 3 everywhere else).
int c3d_detail_label_roots(const uint8_t* mask, int32_t* L, uint32_t* err, uint32_t* area, int Hs, int Ws, int conn8, int phases,
                           hipStream_t st);

// Launch 3 alone, for a caller with union-find phases of its own (csrc/scene_regions.hip): every L[p] >= 0 becomes its root,
// `area` u32 [N], zeroed, gets the pixel count at every root.
int c3d_detail_label_flatten(int32_t* L, uint32_t* err, uint32_t* area, int N, hipStream_t st);

// The keyed labelling of csrc/scene_regions.hip (three launches): L[p] = the smallest linear index of p's region of equal
// nonzero key, -1 where key is 0; areas as above.  `stop` NULL: launch 3 is c3d_detail_label_flatten.  `stop` a device word:
// every launch returns at once when it is nonzero (the rounds of csrc/scene_sieve.hip), and the flatten is a gated twin.
int c3d_detail_region_roots(const uint8_t* key, int32_t* L, uint32_t* err, uint32_t* area, int Hs, int Ws, int conn8,
                            const uint32_t* stop, hipStream_t st);

// A scene of N pixels holds at most ceil(N / 2) components of a mask, which is what the label workspace is laid out for, but
// N regions of a key map (a 4-connected checkerboard of two keys).  The region workspace is the label workspace of one
// class with the score sums grown to N rows; c3d_detail_region_clear is c3d_detail_objects_clear on it.
int64_t c3d_detail_region_ws_bytes(int64_t N);
int c3d_detail_region_clear(void* ws, int64_t N, const float* score, int max_objects, hipStream_t st);

// table[k][5] = key[table[k][6]] for the rows k < counts[1], and object_key (may be NULL) = key where labels > 0, else 0.
int c3d_detail_region_keys(const uint8_t* key, const int32_t* labels, int32_t* table, const int32_t* counts, uint8_t* object_key,
                           int Hs, int Ws, int max_objects, hipStream_t st);

// Launches 4..9 (count, scan, number, relabel_stats, finalise, paint) on a root map: L[p] = the index of the first pixel of
// p's object (L[r] == r there), -1 elsewhere, with the area of every object at its root in the workspace.
int c3d_detail_objects_tail(const uint8_t* cls_map, const float* score, int Hs, int Ws, int min_area, int n_cls, int first_class,
                            int max_objects, int32_t* labels, int32_t* table, uint32_t* hist, uint8_t* object_cls, int32_t* counts,
                            void* ws, int phases, hipStream_t st);
