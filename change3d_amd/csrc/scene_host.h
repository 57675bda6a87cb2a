// Host-side helpers of the scene files: the layout of a workspace and the size of a grid.  A file that needs one includes this
// header and keeps no copy.
#pragma once
#include <cstdint>

namespace c3d_host {

inline int64_t up256(int64_t b) { return (b + 255) & ~(int64_t)255; }

// The arrays of a workspace, one after the other in steps of 256 bytes.  A plan names every array once, by take(): with a base
// the pointer is set, without one (the ..._ws_bytes entries) only `at` moves, so the size and the pointers cannot disagree.
struct Layout {
  char* base;
  int64_t at;                                              // the first byte not taken yet
  template <class T> void take(T*& p, int64_t bytes) {
    p = base ? reinterpret_cast<T*>(base + at) : nullptr;
    at += up256(bytes);
  }
};

// workgroups for `items` at `per_block` each: at least one, at most max_grid (the kernels stride over the rest)
inline unsigned grid_for(int64_t items, int per_block, int max_grid) {
  const int64_t g = (items + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > max_grid ? max_grid : g));
}

}  // namespace c3d_host
