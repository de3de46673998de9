// xcorr_fft.hpp -- what the 2-D (xcorr.hip) and 3-D (xcorr3.hip) registration correlations share:
// the LDS Stockham FFT, the column-tile moves, the four-step column passes A and B (B fused with
// the conjugate product and its inverse) and the twiddle tables.  Internal linkage: each unit
// instantiates what it launches (and keeps its own small twiddle cache).
#pragma once
#include <cmath>
#include <vector>

#include <cstdlib>

#include "devmem.hpp"

namespace {


constexpr int XT = 256;      // threads per workgroup
constexpr int TCA = 32;      // columns per tile, column pass A (512-byte row segments)
constexpr int TCB = 16;      // columns per tile, fused pass B (two tiles in LDS)

__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 conj2(double2 a) { return make_double2(a.x, -a.y); }

// In-place Stockham FFT (radix 4, a final radix 2 when LG is odd) of NB = 2^LGNB transforms of
// M = 2^LG points in LDS.  Rows (NB = 1): element i at buf[i].  Columns (COLS): element i of
// transform b at buf[i * NB + b] (a tile of NB adjacent columns), consecutive lanes on
// consecutive columns so every LDS access is conflict-free.  tw[j * ts] = exp(-2 pi i j / M);
// INV: the conjugate (unnormalised inverse).  Each stage reads its inputs into registers, then
// (after a barrier) writes its outputs; sizes are compile-time, so a thread holds at most
// ceil(NB M / 4 / XT) butterflies.
template <int LG, int LGNB, bool INV>
__device__ __forceinline__ void lds_fft(double2 *buf, const double2 *__restrict__ tw, int ts) {
  constexpr int M = 1 << LG, NB = 1 << LGNB;
  const int tid = threadIdx.x;
#pragma unroll
  for (int lgLs = 0; lgLs + 2 <= LG; lgLs += 2) {
    constexpr int Q = M >= 4 ? M >> 2 : 1;  // (the loop does not run for M < 4)
    constexpr int NBF = NB * Q;
    constexpr int MB = (NBF + XT - 1) / XT;
    const int Ls = 1 << lgLs;
    double2 o[MB][4];
    int ob[MB];
#pragma unroll
    for (int r = 0; r < MB; ++r) {
      const int u = tid + r * XT;
      ob[r] = -1;
      if (NBF % XT == 0 || u < NBF) {
        const int b = u & (NB - 1), j = u >> LGNB;
        const int k = j & (Ls - 1), g = j >> lgLs;
        double2 x0 = buf[j * NB + b], x1 = buf[(j + Q) * NB + b], x2 = buf[(j + 2 * Q) * NB + b],
                x3 = buf[(j + 3 * Q) * NB + b];
        if (lgLs > 0) {  // the first stage's twiddles are all 1
          const int step = (k << (LG - lgLs - 2)) * ts;  // k * M / (4 Ls)
          double2 w1 = tw[step], w2 = tw[2 * step], w3 = tw[3 * step];
          if (INV) {
            w1 = conj2(w1);
            w2 = conj2(w2);
            w3 = conj2(w3);
          }
          x1 = cmul(x1, w1);
          x2 = cmul(x2, w2);
          x3 = cmul(x3, w3);
        }
        const double2 a0 = cadd(x0, x2), a1 = csub(x0, x2), a2 = cadd(x1, x3), a3 = csub(x1, x3);
        // -i a3 = (a3.y, -a3.x); +i a3 = (-a3.y, a3.x)
        const double2 mi = INV ? make_double2(-a3.y, a3.x) : make_double2(a3.y, -a3.x);
        o[r][0] = cadd(a0, a2);
        o[r][1] = cadd(a1, mi);
        o[r][2] = csub(a0, a2);
        o[r][3] = csub(a1, mi);
        ob[r] = ((g << (lgLs + 2)) + k) * NB + b;
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < MB; ++r)
      if (ob[r] >= 0) {
        const int st = Ls * NB;
        buf[ob[r]] = o[r][0];
        buf[ob[r] + st] = o[r][1];
        buf[ob[r] + 2 * st] = o[r][2];
        buf[ob[r] + 3 * st] = o[r][3];
      }
    __syncthreads();
  }
  if (LG & 1) {  // radix-2 stage, Ls = M / 2
    constexpr int Q = M >> 1;
    constexpr int NBF = NB * Q;
    constexpr int MB = (NBF + XT - 1) / XT;
    double2 o[MB][2];
    int ob[MB];
#pragma unroll
    for (int r = 0; r < MB; ++r) {
      const int u = tid + r * XT;
      ob[r] = -1;
      if (NBF % XT == 0 || u < NBF) {
        const int b = u & (NB - 1), j = u >> LGNB;
        const double2 x0 = buf[j * NB + b];
        double2 w = tw[j * ts];
        if (INV) w = conj2(w);
        const double2 x1 = cmul(buf[(j + Q) * NB + b], w);
        o[r][0] = cadd(x0, x1);
        o[r][1] = csub(x0, x1);
        ob[r] = j * NB + b;
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < MB; ++r)
      if (ob[r] >= 0) {
        buf[ob[r]] = o[r][0];
        buf[ob[r] + Q * NB] = o[r][1];
      }
    __syncthreads();
  }
}

// load / store one column tile: rows r(i) = r0 + i * rstep (i < n) of columns [c0, c0 + TC)
template <int TC>
__device__ __forceinline__ void tile_load(const double2 *__restrict__ img, int P, int64_t r0, int64_t rstep, int n,
                                          int c0, double2 *buf) {
  for (int e = threadIdx.x; e < n * TC; e += XT) {
    const int i = e / TC, c = e - i * TC;
    buf[e] = c0 + c < P ? img[(r0 + i * rstep) * P + c0 + c] : make_double2(0.0, 0.0);
  }
}
template <int TC>
__device__ __forceinline__ void tile_store(double2 *__restrict__ img, int P, int64_t r0, int64_t rstep, int n, int c0,
                                           const double2 *buf) {
  for (int e = threadIdx.x; e < n * TC; e += XT) {
    const int i = e / TC, c = e - i * TC;
    if (c0 + c < P) img[(r0 + i * rstep) * P + c0 + c] = buf[e];
  }
}

constexpr int lg2c(int n) { return n <= 1 ? 0 : 1 + lg2c(n / 2); }

// 2 / 4. column pass A (forward) or its inverse: image img0 + blockIdx.z, n2 = blockIdx.y,
// tile blockIdx.x; rows n2 + H2 * i, i < H1
template <int LGH1, int LGH2, bool INV>
__global__ __launch_bounds__(XT) void xc_col_a_kernel(double2 *__restrict__ spec, int img0, int P,
                                                      const double2 *__restrict__ twH, int ta, int nimgs) {
  constexpr int H1 = 1 << LGH1, H2 = 1 << LGH2;
  constexpr int64_t H = (int64_t)H1 * H2;
  __shared__ double2 buf[H1 * TCA];
  for (int64_t job = blockIdx.x; job < (int64_t)ta * H2 * nimgs; job += gridDim.x) {  // (img, n2, tile)
  const int tx = (int)(job % ta), n2 = (int)((job / ta) % H2), iz = (int)(job / ((int64_t)ta * H2));
  const int c0 = tx * TCA;
  double2 *img = spec + (int64_t)(img0 + iz) * H * P;
  tile_load<TCA>(img, P, n2, H2, H1, c0, buf);
  __syncthreads();
  if (INV) {  // conj twiddle on element k1, then the inverse DFT over k1
    for (int e = threadIdx.x; e < H1 * TCA; e += XT) buf[e] = cmul(buf[e], conj2(twH[n2 * (e / TCA)]));
    __syncthreads();
    lds_fft<LGH1, lg2c(TCA), true>(buf, twH, H2);
  } else {
    lds_fft<LGH1, lg2c(TCA), false>(buf, twH, H2);
    for (int e = threadIdx.x; e < H1 * TCA; e += XT) buf[e] = cmul(buf[e], twH[n2 * (e / TCA)]);
    __syncthreads();
  }
  tile_store<TCA>(img, P, n2, H2, H1, c0, buf);
  __syncthreads();
  }
}

// 3. column pass B + product + inverse pass B: k1 = blockIdx.y, tile blockIdx.x; rows H2 k1 + n2
template <int LGH1, int LGH2>
__global__ __launch_bounds__(XT) void xc_col_b_kernel(double2 *__restrict__ spec, int nimg, int P,
                                                      const double2 *__restrict__ twH) {
  constexpr int H1 = 1 << LGH1, H2 = 1 << LGH2;
  constexpr int64_t H = (int64_t)H1 * H2;
  __shared__ double2 A[H2 * TCB], B[H2 * TCB];
  const int64_t r0 = (int64_t)blockIdx.y * H2;
  const int c0 = blockIdx.x * TCB;
  tile_load<TCB>(spec, P, r0, 1, H2, c0, A);
  __syncthreads();
  lds_fft<LGH2, lg2c(TCB), false>(A, twH, H1);
  for (int t = 1; t < nimg; ++t) {
    double2 *img = spec + (int64_t)t * H * P;
    tile_load<TCB>(img, P, r0, 1, H2, c0, B);
    __syncthreads();
    lds_fft<LGH2, lg2c(TCB), false>(B, twH, H1);
    // numpy: src_freq * target_freq.conj()
    for (int e = threadIdx.x; e < H2 * TCB; e += XT) {
      const double2 a = A[e], b = B[e];
      B[e] = make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
    }
    __syncthreads();
    lds_fft<LGH2, lg2c(TCB), true>(B, twH, H1);
    tile_store<TCB>(img, P, r0, 1, H2, c0, B);
    __syncthreads();
  }
}

// a resident grid for the walking passes (one workgroup per job lost in round 3's A/B)
template <class Kern>
unsigned xgrid(Kern k, int64_t njobs) {
  return hrf::resident_grid(k, XT, 0, njobs);
}

int ilog2(int64_t n) {
  int l = 0;
  while ((int64_t)1 << l < n) ++l;
  return ((int64_t)1 << l) == n ? l : -1;
}

// exp(-2 pi i j / N), j < N, per (device, N): uploaded once (synchronously, on first use)
hrf::DeviceTables<int64_t, double2> g_tw;

hrf_status twiddles(int64_t N, const double2 **out) {
  auto build = [N](std::vector<double2> &h) {
    h.resize((size_t)N);
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (int64_t j = 0; j < N; ++j) {
      const long double a = two_pi * (long double)j / (long double)N;
      h[(size_t)j] = make_double2((double)cosl(a), (double)-sinl(a));
    }
  };
  return g_tw.get(N, build, out);
}

}  // namespace
