// biofilm2d.hip -- what the 2-D biofilm segmentation (biofilm_analysis.py:322-419) needs beyond the
// synthetic-community chain: binary dilation / erosion by a disk of radius up to 1023 (:407-413),
// log / log10 of an f64 image (:327, :383), the per-cluster means of the positive registered sums
// (:385-388) and the largest label of a label image (:411-412, :417-418).
//
// Disk morphology.  disk(r) = {(dy, dx): dy^2 + dx^2 <= r^2}, so p = (y, x) is hit by a set pixel iff
// some column x + d, |d| <= r, holds a set pixel within h[|d|] = floor(sqrt(r^2 - d^2)) rows of y.
// Two passes of exact integer arithmetic replace the 31,417-tap stencil of disk(100):
//   A  g[y][x] = min(r + 1, distance along column x from row y to the nearest set pixel), u16.
//      One thread per column and band of DISK_BAND rows: a downward sweep that starts r rows above
//      the band, then an upward sweep that starts r rows below it.  Loads are coalesced along x.
//   B  out[y][x] = any |d| <= r, 0 <= x + d < W: g[y][x + d] <= h[|d|].  One workgroup per row
//      segment of 256 pixels; the segment of g with its r-pixel halo and the table h are staged in
//      LDS; a thread walks d outwards from 0 and stops at its first hit, the wave leaves the loop
//      when a ballot finds no lane still searching.
// The only intermediate is g, 2 bytes per pixel.  Erosion is the dilation of the complement,
// complemented inside the image (skimage's border value 1); border value 0 also clears every pixel
// whose disk leaves the image, which it does exactly when its bounding square does.
#include <cmath>

#include "common.hpp"
#include "detmath.h"
#include "devmem.hpp"
#include "wave.hpp"

namespace {

constexpr int DISK_RMAX = 1023;
constexpr int DISK_BAND = 32;    // rows per workgroup of pass A
constexpr int DISK_SEG = 256;    // pixels per workgroup of pass B (and columns per workgroup of pass A)
constexpr int DISK_STEP = 4;     // offsets tried between two ballots
constexpr int64_t DISK_MAX_GROUPS = (int64_t)1 << 24;

struct DiskTab {
  uint16_t h[DISK_RMAX + 1];     // h[d] = floor(sqrt(r^2 - d^2)), d = 0..r
};

__global__ void __launch_bounds__(DISK_SEG)
disk_column_kernel(const uint8_t *__restrict__ mask, int64_t H, int64_t W, int r, int invert,
                   uint16_t *__restrict__ g) {
  const int64_t gx = (W + DISK_SEG - 1) / DISK_SEG;
  const int64_t x = (int64_t)(blockIdx.x % gx) * DISK_SEG + threadIdx.x;
  if (x >= W) return;
  const int64_t y0 = (int64_t)(blockIdx.x / gx) * DISK_BAND;
  const int64_t y1 = y0 + DISK_BAND < H ? y0 + DISK_BAND : H;
  const int cap = r + 1;
  int d = cap;
  for (int64_t y = y0 - r > 0 ? y0 - r : 0; y < y1; ++y) {
    const int set = (mask[y * W + x] != 0) ^ invert;
    d = set ? 0 : (d < cap ? d + 1 : cap);
    if (y >= y0) g[y * W + x] = (uint16_t)d;
  }
  d = cap;
  for (int64_t y = y1 - 1 + r < H - 1 ? y1 - 1 + r : H - 1; y >= y0; --y) {
    const int set = (mask[y * W + x] != 0) ^ invert;
    d = set ? 0 : (d < cap ? d + 1 : cap);
    if (y < y1 && d < (int)g[y * W + x]) g[y * W + x] = (uint16_t)d;
  }
}

// border0: the erosion with border value 0 (invert is set then)
__global__ void __launch_bounds__(DISK_SEG)
disk_row_kernel(const uint16_t *__restrict__ g, int64_t H, int64_t W, int r, int invert, int border0,
                const DiskTab tab, uint8_t *__restrict__ out) {
  __shared__ uint16_t sg[DISK_SEG + 2 * DISK_RMAX + 2];
  __shared__ uint16_t sh[DISK_RMAX + 1 + DISK_STEP];
  const int tid = threadIdx.x;
  const int64_t gx = (W + DISK_SEG - 1) / DISK_SEG;
  const int64_t y = blockIdx.x / gx;
  const int64_t x0 = (int64_t)(blockIdx.x % gx) * DISK_SEG;
  const uint16_t *row = g + y * W;
  for (int i = tid; i < DISK_SEG + 2 * r; i += DISK_SEG) {
    const int64_t xx = x0 - r + i;
    sg[i] = xx >= 0 && xx < W ? row[xx] : (uint16_t)0xffff;
  }
  for (int i = tid; i <= r; i += DISK_SEG) sh[i] = tab.h[i];
  __syncthreads();
  const int64_t x = x0 + tid;
  const int c = tid + r;
  bool hit = sg[c] <= r;                       // d = 0: h[0] = r
  bool done = hit || x >= W;
  for (int d = 1; d <= r; d += DISK_STEP) {
    if (__ballot(!done) == 0) break;
    if (!done) {
      const int de = d + DISK_STEP <= r + 1 ? d + DISK_STEP : r + 1;
      for (int e = d; e < de; ++e) {
        const int he = sh[e];
        hit |= sg[c - e] <= he || sg[c + e] <= he;
      }
      done = hit;
    }
  }
  if (x < W) {
    int v = (int)hit ^ invert;
    if (border0 && (y < r || y + r >= H || x < r || x + r >= W)) v = 0;
    out[y * W + x] = (uint8_t)v;
  }
}

hrf_status disk_check(const char *who, const void *mask, int64_t H, int64_t W, int32_t radius, const void *out,
                      const void *work, int64_t work_bytes) {
  HRF_REQUIRE(H >= 0 && W >= 0, "%s: negative extent", who);
  HRF_REQUIRE(radius >= 1 && radius <= DISK_RMAX, "%s: radius %d outside 1..%d", who, (int)radius, DISK_RMAX);
  HRF_REQUIRE(H == 0 || W < ((int64_t)1 << 31) / H, "%s: image too large (%lld x %lld, limit 2^31 - 1 pixels)", who,
              (long long)H, (long long)W);
  if (H == 0 || W == 0) return HRF_OK;
  HRF_REQUIRE(mask && out && work, "%s: null buffer", who);
  HRF_REQUIRE(work_bytes >= hrf_disk_workspace_bytes(H, W, radius), "%s: workspace of %lld bytes, %lld needed", who,
              (long long)work_bytes, (long long)hrf_disk_workspace_bytes(H, W, radius));
  // one workgroup per row and segment: a launch holds fewer than 2^32 threads
  HRF_REQUIRE(H * hrf::cdiv(W, DISK_SEG) < DISK_MAX_GROUPS, "%s: %lld rows of %lld segments, limit %lld workgroups", who,
              (long long)H, (long long)hrf::cdiv(W, DISK_SEG), (long long)DISK_MAX_GROUPS);
  return HRF_OK;
}

hrf_status disk_run(const uint8_t *mask, int64_t H, int64_t W, int r, int invert, int border0, uint8_t *out,
                    void *work, hipStream_t s) {
  if (H == 0 || W == 0) return HRF_OK;
  DiskTab tab;
  for (int d = 0; d <= DISK_RMAX; ++d) {
    int h = 0;
    if (d <= r) {
      const int v = r * r - d * d;
      h = (int)std::sqrt((double)v);
      while (h * h > v) --h;
      while ((h + 1) * (h + 1) <= v) ++h;
    }
    tab.h[d] = (uint16_t)h;
  }
  uint16_t *g = (uint16_t *)work;
  const int64_t gx = hrf::cdiv(W, DISK_SEG);
  disk_column_kernel<<<(unsigned)(gx * hrf::cdiv(H, DISK_BAND)), DISK_SEG, 0, s>>>(mask, H, W, r, invert, g);
  HRF_LAUNCHED();
  disk_row_kernel<<<(unsigned)(gx * H), DISK_SEG, 0, s>>>(g, H, W, r, invert, border0, tab, out);
  HRF_LAUNCHED();
  return HRF_OK;
}

// ---- log / log10 -------------------------------------------------------------------------------
template <bool BASE10>
__global__ void log_kernel(const double *__restrict__ x, int64_t n, double *__restrict__ o) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x)
    o[p] = BASE10 ? hrf_cr_log10(x[p]) : hrf_cr_log(x[p]);
}

template <bool BASE10>
hrf_status log_run(const char *who, const double *x, int64_t n, double *out, hipStream_t s) {
  HRF_REQUIRE(n >= 0, "%s: negative size", who);
  if (n == 0) return HRF_OK;
  HRF_REQUIRE(x && out, "%s: null buffer", who);
  log_kernel<BASE10><<<hrf::stream_grid(n), 256, 0, s>>>(x, n, out);
  HRF_LAUNCHED();
  return HRF_OK;
}

// ---- per-cluster sums of the positive values ---------------------------------------------------
// Workgroup b of G takes the elements b * 256 + t + i * G * 256 in order of i; a thread's running
// sum, the LDS tree over the 256 threads and the tree over the G partials all have a fixed order,
// so the result depends on (n, k) and the data only.
constexpr int CPM_BLOCK = 256;
constexpr int CPM_KMAX = 64;

__device__ __forceinline__ void cpm_tree(double *ss, long long *sc, int tid) {
  for (int o = CPM_BLOCK / 2; o > 0; o >>= 1) {
    __syncthreads();
    if (tid < o) {
      ss[tid] += ss[tid + o];
      sc[tid] += sc[tid + o];
    }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(CPM_BLOCK)
cpm_partial_kernel(const int32_t *__restrict__ labels, const double *__restrict__ values, int64_t n, int k,
                   double *__restrict__ psum, long long *__restrict__ pcnt) {
  __shared__ double ss[CPM_BLOCK];
  __shared__ long long sc[CPM_BLOCK];
  const int tid = threadIdx.x;
  for (int c = 0; c < k; ++c) {
    double s = 0.0;
    long long cnt = 0;
    for (int64_t p = (int64_t)blockIdx.x * CPM_BLOCK + tid; p < n; p += (int64_t)gridDim.x * CPM_BLOCK) {
      const double v = values[p];
      if (labels[p] == c && v > 0.0) {
        s += v;
        ++cnt;
      }
    }
    ss[tid] = s;
    sc[tid] = cnt;
    cpm_tree(ss, sc, tid);
    if (tid == 0) {
      psum[(int64_t)c * gridDim.x + blockIdx.x] = ss[0];
      pcnt[(int64_t)c * gridDim.x + blockIdx.x] = sc[0];
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(CPM_BLOCK)
cpm_final_kernel(const double *__restrict__ psum, const long long *__restrict__ pcnt, int G, double *__restrict__ sums,
                 int64_t *__restrict__ counts) {
  __shared__ double ss[CPM_BLOCK];
  __shared__ long long sc[CPM_BLOCK];
  const int tid = threadIdx.x, c = blockIdx.x;
  double s = 0.0;
  long long cnt = 0;
  for (int b = tid; b < G; b += CPM_BLOCK) {
    s += psum[(int64_t)c * G + b];
    cnt += pcnt[(int64_t)c * G + b];
  }
  ss[tid] = s;
  sc[tid] = cnt;
  cpm_tree(ss, sc, tid);
  if (tid == 0) {
    sums[c] = ss[0];
    counts[c] = (int64_t)sc[0];
  }
}

// ---- largest label -----------------------------------------------------------------------------
__global__ void zero_i32_kernel(int32_t *p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0;
}

__global__ void __launch_bounds__(256)
label_hist_kernel(const int32_t *__restrict__ labels, int64_t n, int32_t maxlab, int32_t *__restrict__ cnt) {
  // every lane of a wave runs the same number of iterations (agg_atomic_add needs the whole wave)
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += stride) {
    const int64_t p = base + threadIdx.x;
    const int32_t l = p < n ? labels[p] : 0;
    const bool ok = l >= 1 && l <= maxlab;
    hrf::agg_atomic_add<int32_t>(cnt, ok ? l : 0, 1, ok);
  }
}

// the most frequent label, the lowest among equals: np.argmax over the areas in label order
__global__ void __launch_bounds__(256)
label_argmax_kernel(const int32_t *__restrict__ cnt, int32_t maxlab, int32_t *__restrict__ out) {
  __shared__ int32_t sc[256], sl[256];
  const int tid = threadIdx.x;
  int32_t best = 0, lab = 0;
  for (int64_t l = 1 + tid; l <= maxlab; l += 256) {
    const int32_t c = cnt[l];
    if (c > best) {
      best = c;
      lab = (int32_t)l;
    }
  }
  sc[tid] = best;
  sl[tid] = lab;
  for (int o = 128; o > 0; o >>= 1) {
    __syncthreads();
    if (tid < o) {
      const int32_t c = sc[tid + o], l = sl[tid + o];
      if (c > sc[tid] || (c == sc[tid] && c > 0 && l < sl[tid])) {
        sc[tid] = c;
        sl[tid] = l;
      }
    }
  }
  if (tid == 0) {
    out[0] = sc[0] > 0 ? sl[0] : 0;
    out[1] = sc[0];
  }
}

}  // namespace

extern "C" {

int64_t hrf_disk_workspace_bytes(int64_t H, int64_t W, int32_t radius) {
  if (H < 0 || W < 0 || radius < 1 || radius > DISK_RMAX) return -1;
  if (H != 0 && W >= ((int64_t)1 << 31) / H) return -1;
  return ((2 * H * W + 255) & ~(int64_t)255) + 256;
}

hrf_status hrf_binary_dilation_disk(const uint8_t *mask, int64_t H, int64_t W, int32_t radius, uint8_t *out,
                                    void *work, int64_t work_bytes, hrf_stream_t stream) {
  HRF_TRY(disk_check("binary_dilation_disk", mask, H, W, radius, out, work, work_bytes));
  return disk_run(mask, H, W, radius, 0, 0, out, work, (hipStream_t)stream);
}

hrf_status hrf_binary_erosion_disk(const uint8_t *mask, int64_t H, int64_t W, int32_t radius, int32_t border_value,
                                   uint8_t *out, void *work, int64_t work_bytes, hrf_stream_t stream) {
  HRF_TRY(disk_check("binary_erosion_disk", mask, H, W, radius, out, work, work_bytes));
  HRF_REQUIRE(border_value == 0 || border_value == 1, "binary_erosion_disk: border_value must be 0 or 1");
  return disk_run(mask, H, W, radius, 1, border_value == 0, out, work, (hipStream_t)stream);
}

hrf_status hrf_log10_f64(const double *x, int64_t n, double *out, hrf_stream_t stream) {
  return log_run<true>("log10", x, n, out, (hipStream_t)stream);
}

hrf_status hrf_log_f64(const double *x, int64_t n, double *out, hrf_stream_t stream) {
  return log_run<false>("log", x, n, out, (hipStream_t)stream);
}

hrf_status hrf_cluster_positive_means(const int32_t *labels, const double *values, int64_t n, int32_t k, double *sums,
                                      int64_t *counts, hrf_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  HRF_REQUIRE(n >= 0, "cluster_positive_means: negative size");
  HRF_REQUIRE(k >= 1 && k <= CPM_KMAX, "cluster_positive_means: k = %d outside 1..%d", (int)k, CPM_KMAX);
  HRF_REQUIRE(sums && counts && (n == 0 || (labels && values)), "cluster_positive_means: null buffer");
  const int G = (int)hrf::stream_grid(n, CPM_BLOCK);
  hrf::StreamBuf<char> part;
  HRF_HIP(part.alloc((size_t)G * k * 16, s));
  double *psum = (double *)(char *)part;
  long long *pcnt = (long long *)(psum + (size_t)G * k);
  cpm_partial_kernel<<<G, CPM_BLOCK, 0, s>>>(labels, values, n, k, psum, pcnt);
  HRF_LAUNCHED();
  cpm_final_kernel<<<k, CPM_BLOCK, 0, s>>>(psum, pcnt, G, sums, counts);
  HRF_LAUNCHED();
  HRF_HIP(part.free());
  return HRF_OK;
}

hrf_status hrf_largest_label(const int32_t *labels, int64_t n, int32_t maxlab, int32_t *out, int32_t *work,
                             hrf_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  HRF_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "largest_label: size outside 0..2^31 - 1");
  HRF_REQUIRE(maxlab >= 0 && maxlab < 0x7fffffff, "largest_label: maxlab out of range");
  HRF_REQUIRE(out && work && (n == 0 || labels), "largest_label: null buffer");
  zero_i32_kernel<<<hrf::stream_grid((int64_t)maxlab + 1), 256, 0, s>>>(work, (int64_t)maxlab + 1);
  HRF_LAUNCHED();
  if (n > 0 && maxlab > 0) {
    label_hist_kernel<<<hrf::stream_grid(n), 256, 0, s>>>(labels, n, maxlab, work);
    HRF_LAUNCHED();
  }
  label_argmax_kernel<<<1, 256, 0, s>>>(work, maxlab, out);
  HRF_LAUNCHED();
  return HRF_OK;
}

}  // extern "C"
