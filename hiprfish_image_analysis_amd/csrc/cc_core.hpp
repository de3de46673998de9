// cc_core.hpp -- the union-find of the connected components, shared by the 2-D tiles (label.hip)
// and the 3-D bricks (volume.hip): the larger root is linked under the smaller by atomicMin, so a
// root is its component's least index.  Reads may be stale; correctness comes from atomicMin's
// returned value (retry on the true parent, indices strictly decrease).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hrf_cc {

// what connects: non-zero pixels of EQUAL value (a mask, optionally inverted, or labels)
struct MaskV {
  const uint8_t *p;
  int inv;
  __device__ __forceinline__ int32_t operator()(int64_t i) const { return (int32_t)((p[i] != 0) ^ inv); }
};
struct LabelV {
  const int32_t *p;
  __device__ __forceinline__ int32_t operator()(int64_t i) const { return p[i]; }
};

__device__ __forceinline__ int find_lds(volatile int32_t *lp, int x) {
  int y = lp[x];
  while (y != x) {
    x = y;
    y = lp[x];
  }
  return x;
}

__device__ __forceinline__ void union_lds(int32_t *lp, int a, int b) {
  volatile int32_t *v = lp;
  for (;;) {
    a = find_lds(v, a);
    b = find_lds(v, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&lp[a], b);
    if (old == a) return;
    a = old;
  }
}

__device__ __forceinline__ int32_t find_g(const int32_t *par, int32_t x) {
  int32_t y = par[x];
  while (y != x) {
    x = y;
    y = par[x];
  }
  return x;
}

__device__ __forceinline__ void union_g(int32_t *par, int32_t a, int32_t b) {
  for (;;) {
    a = find_g(par, a);
    b = find_g(par, b);
    if (a == b) return;
    if (a < b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    const int32_t old = atomicMin(&par[a], b);
    if (old == a) return;
    a = old;
  }
}

}  // namespace hrf_cc
