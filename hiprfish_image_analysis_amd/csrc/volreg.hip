// volreg.hip -- assembly of registered biofilm z-stacks (hiprfish_imaging_biofilm_analysis.py).
//
// hrf_volume_taverage_dev: get_registered_average_image_from_tstack (:134-165).  The T time
//   points of one laser, each (X, Y, Z, C) f32, are shifted to t = 0 with zero fill, added in f64
//   in t order, divided by T and stored as f32 (round to nearest; the f32 stack is this project's
//   storage convention).
// hrf_volume_assemble_dev: get_t_average_image (:536-558, fill keep) and generate_3d_segmentation
//   (:428-450, fill zero).  L lasers (X, Y, Z, C_l) shifted by their own (sx, sy, sz) and
//   concatenated on C.  Keep: the reference assigns a volume onto itself and numpy copies the
//   overlapping source first, so the result is the source everywhere with the destination box
//   overwritten by the shifted source.
// Shift s on an axis of length n: dst[max(0, s) : n + min(0, s)] = src[-min(0, s) : n - max(0, s)],
// i.e. dst[i] = src[i - s] wherever 0 <= i - s < n.  The shifts are read from device memory (no
// host round trip after the estimate).
//
// Both kernels walk chunks of consecutive voxels (64..512, about 2048 elements) on a resident grid.  Per chunk the source
// voxel of every (time point | laser, voxel) pair is resolved once into LDS, then the chunk's
// elements are produced with consecutive lanes on consecutive elements: every voxel-channel
// is read once per source and written once, both in runs of whole voxel rows.  A thread issues the
// loads of eight elements before it uses one (one load per wave in flight left the kernels at a
// fifth of the HBM rate).
// With a sum output the chunk's f32 results also stay in LDS and eight lanes per voxel reduce them
// in numpy's pairwise order (hrf_channel_sum's: lane j holds r[j], three xor levels are
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), lane 0 adds the tail), raw or as log(sum + 1e-8) (:537).
// Voxel indices fit int32 (X Y Z < 2^31 - 2 as in volume.hip); element indices are 64-bit.
#include <algorithm>

#include "common.hpp"
#include "detmath.h"

namespace {

constexpr int VT = 256;        // threads per workgroup
constexpr int VP_MIN = 64, VP_MAX = 512;   // voxels per chunk: about UE * VT elements, a multiple of 32
constexpr int MAX_SRC = 16;    // time points (t-average) or lasers (assembly)
constexpr int MAX_C = 128;     // channels of the output row (one numpy pairwise block)

struct Srcs {
  const float *p[MAX_SRC];
  int32_t c0[MAX_SRC + 1];     // assembly: first output channel of each laser, c0[n] = total
};

// the source voxel of destination voxel v under shift (sx, sy, sz); -1 outside the box
__device__ __forceinline__ int64_t shifted_voxel(int64_t v, int64_t X, int64_t Y, int64_t Z, int sx, int sy, int sz) {
  const int64_t z = v % Z, xy = v / Z;
  const int64_t y = xy % Y, x = xy / Y;
  const int64_t qx = x - sx, qy = y - sy, qz = z - sz;
  if (qx < 0 || qx >= X || qy < 0 || qy >= Y || qz < 0 || qz >= Z) return -1;
  return (qx * Y + qy) * Z + qz;
}

// np.sum(row) of the np rows of C f32 values in sb, numpy's pairwise order, into dsum; then one
// lane per voxel takes log(s + 1e-8) (mode 1) and stores: the correctly rounded log is a long f64
// sequence, run on full waves here and not on every eighth lane
__device__ __forceinline__ void chunk_sums(const float *sb, double *dsum, int np, int vp, int C, int64_t v0, int mode,
                                           double *__restrict__ sum_out) {
  const int tid = threadIdx.x, j = tid & 7;
  const int main_n = C < 8 ? 0 : C - (C % 8);
  for (int part = 0; part < vp / (VT / 8); ++part) {
    const int pi = part * (VT / 8) + (tid >> 3);
    const float *a = sb + (pi < np ? pi : 0) * C;
    double res = 0.0;
    if (C >= 8) {
      double r = (double)a[j];
      for (int i = 8; i < main_n; i += 8) r += (double)a[i + j];
      r = r + __shfl_xor(r, 1, 64);
      r = r + __shfl_xor(r, 2, 64);
      r = r + __shfl_xor(r, 4, 64);
      res = r;
      if (j == 0)
        for (int i = main_n; i < C; ++i) res += (double)a[i];
    } else if (j == 0) {
      for (int i = 0; i < C; ++i) res += (double)a[i];
    }
    if (j == 0 && pi < np) dsum[pi] = 0.0 + res;
  }
  __syncthreads();
  for (int i = tid; i < np; i += VT) {
    double sv = dsum[i];
    if (mode == 1) sv = hrf_cr_log(sv + 1e-8);
    sum_out[v0 + i] = sv;
  }
}

constexpr int UE = 8;           // elements a thread has in flight: its loads are issued before any is used

// element e of a chunk (e < 8192) -> its voxel e / C; the float quotient is exact here: (e + 0.5) / C
// is at least 0.5 / 128 from an integer and the rounding error stays below 8192 * 2^-22
__device__ __forceinline__ int voxel_of(int e, float invC) { return (int)(((float)e + 0.5f) * invC); }

// LDS: (sum_out: double dsum[VP], float sb[VP * C]) int32 voff[T * VP] (source voxel, -1 outside
// the box)
__global__ __launch_bounds__(VT) void taverage_kernel(Srcs S, int T, const int32_t *__restrict__ shifts, int64_t X,
                                                      int64_t Y, int64_t Z, int C, int VP, float *__restrict__ dst,
                                                      double *__restrict__ sum_out, int sum_mode) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *dsum = reinterpret_cast<double *>(smem);
  float *sb = reinterpret_cast<float *>(dsum + (sum_out ? VP : 0));
  int32_t *voff = reinterpret_cast<int32_t *>(sb + (sum_out ? VP * C : 0));
  const int64_t V = X * Y * Z, nchunks = (V + VP - 1) / VP;
  const double dT = (double)T;
  const float invC = 1.0f / (float)C;
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int64_t v0 = ch * VP;
    const int np = (int)min((int64_t)VP, V - v0);
    for (int i = VP + threadIdx.x; i < T * VP; i += VT) {          // t = 0 is read in place
      const int t = i / VP, pi = i - t * VP;
      voff[i] = pi < np ? (int32_t)shifted_voxel(v0 + pi, X, Y, Z, shifts[3 * t], shifts[3 * t + 1], shifts[3 * t + 2])
                        : -1;
    }
    __syncthreads();
    const int nel = np * C;
    const int64_t e0 = v0 * C;
    for (int eb = threadIdx.x; eb < nel; eb += UE * VT) {
      int el[UE], pi[UE], c[UE];
      float x[UE];
      double acc[UE];
#pragma unroll
      for (int u = 0; u < UE; ++u) {
        el[u] = eb + u * VT < nel ? eb + u * VT : 0;               // past the chunk: element 0 again, not stored
        pi[u] = voxel_of(el[u], invC);
        c[u] = el[u] - pi[u] * C;
      }
      const float *__restrict__ s0 = S.p[0] + e0;
#pragma unroll
      for (int u = 0; u < UE; ++u) x[u] = s0[el[u]];
#pragma unroll
      for (int u = 0; u < UE; ++u) acc[u] = (double)x[u];          // image_registered = image_0.copy()
      for (int t = 1; t < T; ++t) {                                // += image_registered_hold, t order
        const float *__restrict__ st = S.p[t];
        const int32_t *vo = voff + t * VP;
#pragma unroll
        for (int u = 0; u < UE; ++u) {
          const int32_t q = vo[pi[u]];
          x[u] = q >= 0 ? st[(int64_t)q * C + c[u]] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < UE; ++u) acc[u] += (double)x[u];
      }
#pragma unroll
      for (int u = 0; u < UE; ++u)
        if (eb + u * VT < nel) {
          const float o = (float)(acc[u] / dT);                    // :165, stored f32
          dst[e0 + el[u]] = o;
          if (sum_out) sb[el[u]] = o;
        }
    }
    if (sum_out) {
      __syncthreads();
      chunk_sums(sb, dsum, np, VP, C, v0, sum_mode, sum_out);
    }
    __syncthreads();
  }
}

// LDS: double dsum[VP], float sb[VP * Ctot], int32 voff[L * VP].  The lasers are gathered one after the other
// into the chunk's rows in LDS (reads in runs of whole source rows), then the chunk is written out
// in one contiguous run.
__global__ __launch_bounds__(VT) void assemble3_kernel(Srcs S, int L, const int32_t *__restrict__ shifts, int64_t X,
                                                       int64_t Y, int64_t Z, int keep, int VP,
                                                       float *__restrict__ dst, double *__restrict__ sum_out,
                                                       int sum_mode) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int C = S.c0[L];
  double *dsum = reinterpret_cast<double *>(smem);
  float *sb = reinterpret_cast<float *>(dsum + VP);
  int32_t *voff = reinterpret_cast<int32_t *>(sb + VP * C);
  const int64_t V = X * Y * Z, nchunks = (V + VP - 1) / VP;
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int64_t v0 = ch * VP;
    const int np = (int)min((int64_t)VP, V - v0);
    for (int i = threadIdx.x; i < L * VP; i += VT) {
      const int l = i / VP, pi = i - l * VP;
      int64_t q = -1;
      if (pi < np) {
        q = shifts ? shifted_voxel(v0 + pi, X, Y, Z, shifts[3 * l], shifts[3 * l + 1], shifts[3 * l + 2]) : v0 + pi;
        if (q < 0 && keep) q = v0 + pi;                             // outside the box the source stays
      }
      voff[i] = (int32_t)q;
    }
    __syncthreads();
    for (int l = 0; l < L; ++l) {
      const int cb = S.c0[l], cl = S.c0[l + 1] - cb, nl = np * cl;
      const float invC = 1.0f / (float)cl;
      const float *__restrict__ sl = S.p[l];
      const int32_t *vo = voff + l * VP;
      for (int eb = threadIdx.x; eb < nl; eb += UE * VT) {
        int at[UE];
        float x[UE];
#pragma unroll
        for (int u = 0; u < UE; ++u) {
          const int e = eb + u * VT < nl ? eb + u * VT : 0;
          const int pi = voxel_of(e, invC), c = e - pi * cl;
          const int32_t q = vo[pi];
          at[u] = pi * C + cb + c;
          x[u] = q >= 0 ? sl[(int64_t)q * cl + c] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < UE; ++u)
          if (eb + u * VT < nl) sb[at[u]] = x[u];
      }
    }
    __syncthreads();
    if (dst) {
      const int nel = np * C;                                       // v0 is a multiple of 32: 16-byte aligned
      float4 *d4 = reinterpret_cast<float4 *>(dst + v0 * C);
      const float4 *s4 = reinterpret_cast<const float4 *>(sb);
      for (int e = threadIdx.x; e < (nel >> 2); e += VT) d4[e] = s4[e];
      for (int e = (nel & ~3) + threadIdx.x; e < nel; e += VT) dst[v0 * C + e] = sb[e];
    }
    if (sum_out) chunk_sums(sb, dsum, np, VP, C, v0, sum_mode, sum_out);
    __syncthreads();
  }
}

// a chunk of about UE * VT elements, so that a thread's UE slots are filled at any C
int chunk_voxels(int C) { return std::max(VP_MIN, std::min(VP_MAX, (UE * VT / C) & ~31)); }

bool volume_ok(int64_t X, int64_t Y, int64_t Z) {
  return X >= 1 && Y >= 1 && Z >= 1 && X <= INT32_MAX && Y <= INT32_MAX && Z <= INT32_MAX &&
         X * Y < ((int64_t)1 << 31) && X * Y * Z < ((int64_t)1 << 31) - 2;
}

}  // namespace

extern "C" {

hrf_status hrf_volume_taverage_dev(const float *const *src_host, int32_t T, const int32_t *shifts_dev, int64_t X,
                                   int64_t Y, int64_t Z, int32_t C, float *dst, double *sum_out, int32_t sum_mode,
                                   hrf_stream_t stream) {
  HRF_REQUIRE(T >= 1 && T <= MAX_SRC, "volume_taverage: 1..16 time points");
  HRF_REQUIRE(C >= 1 && C <= MAX_C, "volume_taverage: C must be 1..128");
  HRF_REQUIRE(volume_ok(X, Y, Z), "volume_taverage: X Y Z must stay below 2^31 - 2");
  HRF_REQUIRE(sum_mode == 0 || sum_mode == 1, "volume_taverage: sum_mode 0 (sum) or 1 (log(sum + 1e-8))");
  HRF_REQUIRE(src_host && dst && (T == 1 || shifts_dev), "volume_taverage: null buffer");
  Srcs S{};
  for (int t = 0; t < T; ++t) {
    HRF_REQUIRE(src_host[t], "volume_taverage: null time point");
    HRF_REQUIRE(src_host[t] != dst, "volume_taverage: dst must not alias a time point");
    S.p[t] = src_host[t];
  }
  const int VP = chunk_voxels(C);
  const size_t shm = sizeof(int32_t) * T * VP + (sum_out ? sizeof(double) * VP + sizeof(float) * VP * C : 0);
  const int64_t nch = hrf::cdiv(X * Y * Z, VP);
  taverage_kernel<<<hrf::resident_grid(taverage_kernel, VT, shm, nch), VT, shm, (hipStream_t)stream>>>(
      S, T, shifts_dev, X, Y, Z, C, VP, dst, sum_out, sum_mode);
  HRF_LAUNCHED();
  return HRF_OK;
}

hrf_status hrf_volume_assemble_dev(const float *const *src_host, const int32_t *channels_host,
                                   const int32_t *shifts_dev, int32_t nlaser, int64_t X, int64_t Y, int64_t Z,
                                   int32_t fill, float *dst, double *sum_out, int32_t sum_mode, hrf_stream_t stream) {
  HRF_REQUIRE(nlaser >= 1 && nlaser <= MAX_SRC, "volume_assemble: 1..16 lasers");
  HRF_REQUIRE(volume_ok(X, Y, Z), "volume_assemble: X Y Z must stay below 2^31 - 2");
  HRF_REQUIRE(fill == 0 || fill == 1, "volume_assemble: fill 0 (zero) or 1 (keep)");
  HRF_REQUIRE(sum_mode == 0 || sum_mode == 1, "volume_assemble: sum_mode 0 (sum) or 1 (log(sum + 1e-8))");
  HRF_REQUIRE(src_host && channels_host && (dst || sum_out), "volume_assemble: null buffer");
  HRF_REQUIRE(((uintptr_t)dst & 15) == 0, "volume_assemble: dst must be 16-byte aligned");
  Srcs S{};
  int64_t ctot = 0;
  for (int l = 0; l < nlaser; ++l) {
    HRF_REQUIRE(src_host[l] && src_host[l] != dst, "volume_assemble: null laser, or dst aliases one");
    HRF_REQUIRE(channels_host[l] >= 1 && channels_host[l] <= MAX_C, "volume_assemble: channels per laser 1..128");
    S.p[l] = src_host[l];
    S.c0[l] = (int32_t)ctot;
    ctot += channels_host[l];
  }
  HRF_REQUIRE(ctot <= MAX_C, "volume_assemble: at most 128 channels in all");
  S.c0[nlaser] = (int32_t)ctot;
  const int VP = chunk_voxels((int)ctot);
  const size_t shm = sizeof(double) * VP + sizeof(float) * VP * ctot + sizeof(int32_t) * nlaser * VP;
  const int64_t nch = hrf::cdiv(X * Y * Z, VP);
  assemble3_kernel<<<hrf::resident_grid(assemble3_kernel, VT, shm, nch), VT, shm, (hipStream_t)stream>>>(
      S, nlaser, shifts_dev, X, Y, Z, fill, VP, dst, sum_out, sum_mode);
  HRF_LAUNCHED();
  return HRF_OK;
}

}  // extern "C"
