// mosaic.hip -- tiled 3-D biofilm mosaics (hiprfish_imaging_biofilm_analysis.py:1064-1102,
// generate_3d_segmentation_tile_memory_efficient).
//
// hrf_volume_tsum_masked_dev: get_registered_image_from_tstack_tile (:203-236) and :1073-1076.
//   The T time points of one tile, each (X, Y, Z, C) f32, are shifted to t = 0 with zero fill and
//   added in f64 in t order -- no division by T, no rounding to f32 -- then summed over C in
//   numpy's pairwise order (np.sum(axis=3) of the f64 stack).  mask = the AND over t >= 1 of each
//   time point's coverage box; sum_filtered = sum * mask.  One pass: every source element is read
//   once (T C 4 bytes per voxel), 9 bytes per voxel are written, the (X, Y, Z, C) f64 stack exists
//   only as one chunk's rows in LDS.  The chunk walk is volreg.hip's taverage_kernel's: the source
//   voxel of every (t, voxel) pair is resolved once into LDS, consecutive lanes take consecutive
//   elements, a thread issues the loads of eight elements before it uses one.
// hrf_mosaic_accumulate3: :1098-1101.  A gather: every canvas voxel walks the tiles in index
//   order k = i n + j and adds sum_filtered * mask of each tile whose box holds it, which is the
//   f64 order of the reference's `+=` per tile; no atomics.  count = the covering tiles whose mask
//   is set there, 0 -> 1; full = the sum / count.
// Shift convention as volreg.hip: dst[i] = src[i - s] wherever 0 <= i - s < n.
#include <algorithm>

#include "vol.hpp"

namespace {

constexpr int VT = 256;                  // threads per workgroup
constexpr int VP_MIN = 32, VP_MAX = 512; // voxels per chunk: about UE * VT elements, a multiple of 32
constexpr int MAX_T = 16;                // time points
constexpr int MAX_C = 128;               // channels (one numpy pairwise block)
constexpr int UE = 8;                    // elements a thread has in flight
constexpr int MAX_TILES = 64;

struct Srcs {
  const float *p[MAX_T];
};

// the source voxel of destination voxel v under shift (sx, sy, sz); -1 outside the box
__device__ __forceinline__ int64_t shifted_voxel(int64_t v, int64_t X, int64_t Y, int64_t Z, int sx, int sy, int sz) {
  const int64_t z = v % Z, xy = v / Z;
  const int64_t y = xy % Y, x = xy / Y;
  const int64_t qx = x - sx, qy = y - sy, qz = z - sz;
  if (qx < 0 || qx >= X || qy < 0 || qy >= Y || qz < 0 || qz >= Z) return -1;
  return (qx * Y + qy) * Z + qz;
}

// element e of a chunk (e < 8192) -> its voxel e / C; the float quotient is exact here: (e + 0.5) / C
// is at least 0.5 / 128 from an integer and the rounding error stays below 8192 * 2^-22
__device__ __forceinline__ int voxel_of(int e, float invC) { return (int)(((float)e + 0.5f) * invC); }

// LDS: double dsum[VP], double sb[VP * C] (the chunk's rows of the f64 time sum), int32 voff[T * VP]
// (source voxel, -1 outside the box; row 0 unused: t = 0 is read in place)
__global__ __launch_bounds__(VT) void tsum_masked_kernel(Srcs S, int T, const int32_t *__restrict__ shifts, int64_t X,
                                                         int64_t Y, int64_t Z, int C, int VP,
                                                         double *__restrict__ sum_out, uint8_t *__restrict__ mask_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *dsum = reinterpret_cast<double *>(smem);
  double *sb = dsum + VP;
  int32_t *voff = reinterpret_cast<int32_t *>(sb + VP * C);
  const int64_t V = X * Y * Z, nchunks = (V + VP - 1) / VP;
  const float invC = 1.0f / (float)C;
  const int tid = threadIdx.x, j = tid & 7;
  const int main_n = C < 8 ? 0 : C - (C % 8);
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int64_t v0 = ch * VP;
    const int np = (int)min((int64_t)VP, V - v0);
    for (int i = VP + tid; i < T * VP; i += VT) {
      const int t = i / VP, pi = i - t * VP;
      voff[i] = pi < np ? (int32_t)shifted_voxel(v0 + pi, X, Y, Z, shifts[3 * t], shifts[3 * t + 1], shifts[3 * t + 2])
                        : -1;
    }
    __syncthreads();
    const int nel = np * C;
    const int64_t e0 = v0 * C;
    for (int eb = tid; eb < nel; eb += UE * VT) {
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
        if (eb + u * VT < nel) sb[el[u]] = acc[u];
    }
    __syncthreads();
    // np.sum(row) per voxel, numpy's pairwise order: lane j of eight holds r[j], three xor levels
    // are ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), lane 0 adds the tail; fewer than 8: 0.0 + a[0] + ...
    for (int part = 0; part < VP / (VT / 8); ++part) {
      const int pi = part * (VT / 8) + (tid >> 3);
      const double *a = sb + (pi < np ? pi : 0) * C;
      double res = 0.0;
      if (C >= 8) {
        double r = a[j];
        for (int i = 8; i < main_n; i += 8) r += a[i + j];
        r = r + __shfl_xor(r, 1, 64);
        r = r + __shfl_xor(r, 2, 64);
        r = r + __shfl_xor(r, 4, 64);
        res = r;
        if (j == 0)
          for (int i = main_n; i < C; ++i) res += a[i];
      } else if (j == 0) {
        for (int i = 0; i < C; ++i) res += a[i];
      }
      if (j == 0 && pi < np) dsum[pi] = res;
    }
    __syncthreads();
    for (int i = tid; i < np; i += VT) {
      int m = 1;                                                   // shift_filter_mask, all ones for T = 1
      for (int t = 1; t < T; ++t) m &= voff[t * VP + i] >= 0;
      sum_out[v0 + i] = dsum[i] * (double)m;                       // :1076
      mask_out[v0 + i] = (uint8_t)m;
    }
    __syncthreads();
  }
}

struct Tiles {
  const double *sum[MAX_TILES];
  const uint8_t *mask[MAX_TILES];
  int32_t o[MAX_TILES][3];
};

// one thread per canvas voxel, z fastest; the canvas has fewer than 2^31 - 2 voxels
__global__ __launch_bounds__(256) void mosaic_accumulate3_kernel(Tiles Tl, int ntiles, int TX, int TY, int TZ, int CY,
                                                                 int CZ, int64_t n, double *__restrict__ full,
                                                                 int32_t *__restrict__ count) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
    const int z = (int)(v % CZ);
    const int xy = (int)(v / CZ);
    const int y = xy % CY, x = xy / CY;
    double acc = 0.0;                                              // np.zeros, then += per tile in k order
    int cnt = 0;
    for (int k = 0; k < ntiles; ++k) {
      const int qx = x - Tl.o[k][0], qy = y - Tl.o[k][1], qz = z - Tl.o[k][2];
      if ((unsigned)qx >= (unsigned)TX || (unsigned)qy >= (unsigned)TY || (unsigned)qz >= (unsigned)TZ) continue;
      const int64_t q = ((int64_t)qx * TY + qy) * TZ + qz;
      const int m = Tl.mask[k][q] != 0;
      acc += Tl.sum[k][q] * (double)m;                             // :1098
      cnt += m;                                                    // :1099
    }
    if (cnt == 0) cnt = 1;                                         // :1100
    full[v] = acc / (double)cnt;                                   // :1101
    if (count) count[v] = cnt;
  }
}

// a chunk of about UE * VT elements, so that a thread's UE slots are filled at any C
int chunk_voxels(int C) { return std::max(VP_MIN, std::min(VP_MAX, (UE * VT / C) & ~31)); }

}  // namespace

extern "C" {

hrf_status hrf_volume_tsum_masked_dev(const float *const *src_host, int32_t T, const int32_t *shifts_dev, int64_t X,
                                      int64_t Y, int64_t Z, int32_t C, double *sum_filtered, uint8_t *mask,
                                      hrf_stream_t stream) {
  HRF_REQUIRE(T >= 1 && T <= MAX_T, "volume_tsum_masked: 1..16 time points");
  HRF_REQUIRE(C >= 1 && C <= MAX_C, "volume_tsum_masked: C must be 1..128");
  HRF_REQUIRE(X >= 1 && Y >= 1 && Z >= 1, "volume_tsum_masked: empty volume");
  HRF_TRY(hrf_vol::check_vol(X, Y, Z, "volume_tsum_masked"));
  HRF_REQUIRE(src_host && sum_filtered && mask && (T == 1 || shifts_dev), "volume_tsum_masked: null buffer");
  Srcs S{};
  for (int t = 0; t < T; ++t) {
    HRF_REQUIRE(src_host[t], "volume_tsum_masked: null time point");
    S.p[t] = src_host[t];
  }
  const int VP = chunk_voxels(C);
  const size_t shm = sizeof(double) * VP + sizeof(double) * VP * C + sizeof(int32_t) * T * VP;
  const int64_t nch = hrf::cdiv(X * Y * Z, VP);
  tsum_masked_kernel<<<hrf::resident_grid(tsum_masked_kernel, VT, shm, nch), VT, shm, (hipStream_t)stream>>>(
      S, T, shifts_dev, X, Y, Z, C, VP, sum_filtered, mask);
  HRF_LAUNCHED();
  return HRF_OK;
}

hrf_status hrf_mosaic_accumulate3(const double *const *tile_sums_host, const uint8_t *const *tile_masks_host,
                                  const int32_t *origins_host, int32_t ntiles, int64_t TX, int64_t TY, int64_t TZ,
                                  int64_t CX, int64_t CY, int64_t CZ, double *full, int32_t *count,
                                  hrf_stream_t stream) {
  HRF_REQUIRE(ntiles >= 1 && ntiles <= MAX_TILES, "mosaic_accumulate3: 1..64 tiles (got %d)", (int)ntiles);
  HRF_REQUIRE(TX >= 1 && TY >= 1 && TZ >= 1 && CX >= 1 && CY >= 1 && CZ >= 1, "mosaic_accumulate3: empty extent");
  HRF_TRY(hrf_vol::check_vol(TX, TY, TZ, "mosaic_accumulate3 (tile)"));
  HRF_TRY(hrf_vol::check_vol(CX, CY, CZ, "mosaic_accumulate3 (canvas)"));
  HRF_REQUIRE(tile_sums_host && tile_masks_host && origins_host && full, "mosaic_accumulate3: null buffer");
  Tiles Tl{};
  const int64_t T3[3] = {TX, TY, TZ}, C3[3] = {CX, CY, CZ};
  for (int k = 0; k < ntiles; ++k) {
    HRF_REQUIRE(tile_sums_host[k] && tile_masks_host[k], "mosaic_accumulate3: null tile %d", k);
    HRF_REQUIRE((const void *)tile_sums_host[k] != (const void *)full, "mosaic_accumulate3: full aliases tile %d", k);
    for (int a = 0; a < 3; ++a) {
      const int64_t o = origins_host[3 * k + a];
      // the reference would wrap a negative index or fail to broadcast past the far face
      HRF_REQUIRE(o >= 0 && o + T3[a] <= C3[a],
                  "mosaic_accumulate3: tile %d leaves the canvas on axis %d (origin %lld, tile %lld, canvas %lld)", k, a,
                  (long long)o, (long long)T3[a], (long long)C3[a]);
      Tl.o[k][a] = (int32_t)o;
    }
    Tl.sum[k] = tile_sums_host[k];
    Tl.mask[k] = tile_masks_host[k];
  }
  const int64_t n = CX * CY * CZ;
  mosaic_accumulate3_kernel<<<(unsigned)std::min<int64_t>(hrf::cdiv(n, 256), 8192), 256, 0, (hipStream_t)stream>>>(
      Tl, ntiles, (int)TX, (int)TY, (int)TZ, (int)CY, (int)CZ, n, full, count);
  HRF_LAUNCHED();
  return HRF_OK;
}

}  // extern "C"
