// rag_core.hpp -- the barcode x barcode count of one label edge (biofilm_analysis.py:1277-1295),
// shared by the dense 2-D edge matrix (rag.hip) and the sparse 3-D edge keys (report3.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hrf {

// An undirected edge (a, b), 1 <= a < b, gives +1 at adj[bc[a]][bc[b]] and adj[bc[b]][bc[a]] (the
// reference visits each edge from both endpoints); barcodes outside [0, R) are not counted.  With
// keep and adjf, the filtered matrix counts it too when both labels are kept (biofilm :1290-1291:
// both endpoint rows typed 'cell').
__device__ __forceinline__ void count_edge(int64_t a, int64_t b, const int32_t *__restrict__ bc,
                                           const uint8_t *__restrict__ keep, int32_t R,
                                           unsigned long long *__restrict__ adj,
                                           unsigned long long *__restrict__ adjf) {
  if (a < 1 || b <= a) return;
  const int32_t ba = bc[a], bb = bc[b];
  if (ba < 0 || ba >= R || bb < 0 || bb >= R) return;
  atomicAdd(&adj[(int64_t)ba * R + bb], 1ull);
  atomicAdd(&adj[(int64_t)bb * R + ba], 1ull);
  if (adjf && keep && keep[a] && keep[b]) {
    atomicAdd(&adjf[(int64_t)ba * R + bb], 1ull);
    atomicAdd(&adjf[(int64_t)bb * R + ba], 1ull);
  }
}

}  // namespace hrf
