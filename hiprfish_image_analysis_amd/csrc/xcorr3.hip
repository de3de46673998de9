// xcorr3.hip -- the registration cross-correlations of (n, X, Y, Z) volumes, xcorr.hip's
// pipeline with one more axis (biofilm :143, :537: skimage.feature.register_translation on
// channel sums and on log channel sums of z-stacks; upsample_factor 1).
//
// Spectrum layout spec[((img X + x) Y + y) Pz + k],
// Pz = Z / 2 + 1, one spectrum per volume:
//   z forward: Z-lines are short (64 in the project's volumes), so a workgroup takes NB adjacent
//     lines as one batch of lds_fft (NB M = 1024 points, at most 256 lines);
//   y forward: per (img, x) a (Y, Pz) matrix, four-step passes A and B in place.  The result stays
//     in the passes' own order (row H2 k1 + k2 holds frequency k1 + H1 k2): the product is
//     elementwise and the inverse passes B, A undo it.  A tile is 32 adjacent (x, k) pairs of the
//     flattened (X Pz) column index, so tiles stay full although Pz is odd;
//   x: the (X, Y Pz) matrix through xc_col_a_kernel / xc_col_b_kernel / xc_col_a_kernel as they
//     are (P = Y Pz): forward A, B fused with the product and its inverse, inverse A;
//   y inverse B, A; z inverse with |cc| and the first maximum of each job's lines (C order);
//   per target the first maximum over its jobs -> the wrapped, clamped (sx, sy, sz).
// Scale: X Y Z / 2 times numpy.fft.ifftn.
#include "xcorr_fft.hpp"

namespace {

template <int LGM, int LGNB>
__global__ __launch_bounds__(XT) void xc3_z_fwd_kernel(const double *__restrict__ vols, double2 *__restrict__ spec,
                                                       const double2 *__restrict__ twZ, int64_t njobs) {
  constexpr int M = 1 << LGM, NB = 1 << LGNB, P = M + 1;
  __shared__ double2 buf[M * NB];
  for (int64_t job = blockIdx.x; job < njobs; job += gridDim.x) {  // lines job NB .. job NB + NB - 1
    const double2 *src = reinterpret_cast<const double2 *>(vols) + job * (M * NB);
    for (int g = threadIdx.x; g < M * NB; g += XT) buf[(g & (M - 1)) * NB + (g >> LGM)] = src[g];
    __syncthreads();
    lds_fft<LGM, LGNB, false>(buf, twZ, 2);
    double2 *dst = spec + job * (NB * P);
    for (int g = threadIdx.x; g < NB * P; g += XT) {
      const int b = g / P, k = g - b * P;
      const double2 zk = buf[(k & (M - 1)) * NB + b], zc = conj2(buf[((M - k) & (M - 1)) * NB + b]);
      const double2 e = make_double2(0.5 * (zk.x + zc.x), 0.5 * (zk.y + zc.y));
      const double2 d = make_double2(0.5 * (zk.x - zc.x), 0.5 * (zk.y - zc.y));
      const double2 od = make_double2(d.y, -d.x);  // -i d
      dst[g] = cadd(e, cmul(twZ[k], od));
    }
    __syncthreads();
  }
}

// y passes: ISA pass A (rows o + nout i, twiddle exp(-+2 pi i o i / Y)), else pass B (rows
// (o << LG) + i); i < 2^LG, o < nout = Y >> LG, which is also the twiddle stride of both
template <int LG, bool INV, bool ISA>
__global__ __launch_bounds__(XT) void xc3_y_kernel(double2 *__restrict__ spec, int img0, int nimgs, int X, int Y,
                                                   int Pz, const double2 *__restrict__ twY, int ntile) {
  constexpr int R = 1 << LG;
  __shared__ double2 buf[R * TCA];
  const int nout = Y >> LG;
  const int c = threadIdx.x & (TCA - 1), i0 = threadIdx.x / TCA;
  const int64_t ncol = (int64_t)X * Pz;
  for (int64_t job = blockIdx.x; job < (int64_t)ntile * nout * nimgs; job += gridDim.x) {  // (img, o, tile)
    const int tx = (int)(job % ntile), o = (int)((job / ntile) % nout), iz = (int)(job / ((int64_t)ntile * nout));
    const int64_t q = (int64_t)tx * TCA + c;
    const bool ok = q < ncol;
    const int64_t x = ok ? q / Pz : 0, k = ok ? q - x * Pz : 0;
    double2 *col = spec + (((int64_t)(img0 + iz) * X + x) * Y) * Pz + k;
    const int64_t r0 = ISA ? o : (int64_t)o << LG, rstep = ISA ? nout : 1;
    for (int i = i0; i < R; i += XT / TCA) {
      double2 v = ok ? col[(r0 + i * rstep) * Pz] : make_double2(0.0, 0.0);
      if (INV && ISA) v = cmul(v, conj2(twY[o * i]));
      buf[i * TCA + c] = v;
    }
    __syncthreads();
    lds_fft<LG, lg2c(TCA), INV>(buf, twY, nout);
    if (ok)
      for (int i = i0; i < R; i += XT / TCA) {
        double2 v = buf[i * TCA + c];
        if (!INV && ISA) v = cmul(v, twY[o * i]);
        col[(r0 + i * rstep) * Pz] = v;
      }
    __syncthreads();
  }
}

struct JobBest {
  double v;
  int64_t idx;  // (x Y + y) Z + z within the target's surface
};

// z inverse of the targets' lines (spec1: target 1's first line); job = NB adjacent lines
template <int LGM, int LGNB>
__global__ __launch_bounds__(XT) void xc3_z_inv_kernel(const double2 *__restrict__ spec1, const double2 *__restrict__ twZ,
                                                       JobBest *__restrict__ jobbest, double *__restrict__ cc_out,
                                                       int64_t njobs, int64_t jobs_per_target) {
  constexpr int M = 1 << LGM, NB = 1 << LGNB, P = M + 1, G = XT / NB;
  static_assert(NB <= XT && G <= M, "a line has at least one point per scanning thread");
  __shared__ double2 buf[M * NB];
  __shared__ double lv[XT];
  __shared__ int lc[XT];
  __shared__ long long li[XT / 64];
  for (int64_t job = blockIdx.x; job < njobs; job += gridDim.x) {
    const double2 *Xs = spec1 + job * (NB * P);
    for (int g = threadIdx.x; g < NB * M; g += XT) {
      const int b = g >> LGM, k = g & (M - 1);
      const double2 xk = Xs[b * P + k], xc = conj2(Xs[b * P + M - k]);
      const double2 e = make_double2(0.5 * (xk.x + xc.x), 0.5 * (xk.y + xc.y));
      const double2 d = make_double2(0.5 * (xk.x - xc.x), 0.5 * (xk.y - xc.y));
      const double2 o = cmul(d, conj2(twZ[k]));
      buf[k * NB + b] = make_double2(e.x - o.y, e.y + o.x);  // e + i o
    }
    __syncthreads();
    lds_fft<LGM, LGNB, true>(buf, twZ, 2);
    if (cc_out) {  // the correlation surfaces themselves (tests): X Y Z / 2 times numpy.fft.ifftn
      double2 *o = reinterpret_cast<double2 *>(cc_out) + job * (M * NB);
      for (int g = threadIdx.x; g < M * NB; g += XT) o[g] = buf[(g & (M - 1)) * NB + (g >> LGM)];
    }
    // the first max |cc| of line b: G threads take its points i = g, g + G, ... in increasing order
    const int b = threadIdx.x & (NB - 1), g = threadIdx.x >> LGNB;
    double bv = -1.0;
    int bc = 0x7fffffff;
    for (int i = g; i < M; i += G) {
      const double2 z = buf[i * NB + b];
      const double a0 = fabs(z.x), a1 = fabs(z.y);
      if (a0 > bv) {
        bv = a0;
        bc = 2 * i;
      }
      if (a1 > bv) {
        bv = a1;
        bc = 2 * i + 1;
      }
    }
    lv[threadIdx.x] = bv;
    lc[threadIdx.x] = bc;
    __syncthreads();
    long long bi = LLONG_MAX;
    if (threadIdx.x < NB) {  // g == 0: this line's first maximum, then its index in the surface
      for (int q = 1; q < G; ++q) {
        const double ov = lv[q * NB + b];
        const int oc = lc[q * NB + b];
        if (ov > bv || (ov == bv && oc < bc)) {
          bv = ov;
          bc = oc;
        }
      }
      bi = ((job % jobs_per_target) * NB + b) * (2 * M) + bc;
    } else {
      bv = -1.0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(bv, o, 64);
      const long long oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    __syncthreads();  // lv is read above and reused below
    if ((threadIdx.x & 63) == 0) {
      lv[threadIdx.x >> 6] = bv;
      li[threadIdx.x >> 6] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int q = 1; q < XT / 64; ++q)
        if (lv[q] > bv || (lv[q] == bv && li[q] < bi)) {
          bv = lv[q];
          bi = li[q];
        }
      jobbest[job] = JobBest{bv, bi};
    }
    __syncthreads();
  }
}

// per target (blockIdx.x): the first maximum over its jobs -> shift[1 + t]; shift[0] = (0, 0, 0)
__global__ __launch_bounds__(XT) void xc3_shifts_kernel(const JobBest *__restrict__ jobbest, int64_t jobs_per_target,
                                                        int64_t X, int64_t Y, int64_t Z, int32_t clamp,
                                                        int32_t *__restrict__ shift) {
  __shared__ double rv[XT / 64];
  __shared__ long long ri[XT / 64];
  const JobBest *jb = jobbest + (int64_t)blockIdx.x * jobs_per_target;
  double bv = -1.0;
  long long bi = LLONG_MAX;
  for (int64_t j = threadIdx.x; j < jobs_per_target; j += XT) {
    const JobBest q = jb[j];
    if (q.v > bv) {  // increasing jobs per thread: the first kept on ties
      bv = q.v;
      bi = q.idx;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const long long oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    rv[threadIdx.x >> 6] = bv;
    ri[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < XT / 64; ++q)
      if (rv[q] > bv || (rv[q] == bv && ri[q] < bi)) {
        bv = rv[q];
        bi = ri[q];
      }
    int64_t s[3] = {bi / (Y * Z), (bi / Z) % Y, bi % Z};
    const int64_t n[3] = {X, Y, Z};
    int32_t *out = shift + 3 * (1 + blockIdx.x);
    for (int a = 0; a < 3; ++a) {
      if (s[a] > n[a] / 2) s[a] -= n[a];  // midpoints = fix(n / 2)
      if (clamp >= 0 && (s[a] > clamp || s[a] < -clamp)) s[a] = 0;
      out[a] = (int32_t)s[a];
    }
    if (blockIdx.x == 0) shift[0] = shift[1] = shift[2] = 0;
  }
}

constexpr int z_lgnb(int lgm) { return 10 - lgm > 8 ? 8 : 10 - lgm; }  // NB M = 1024, NB <= 256

bool supported3(int32_t nimg, int64_t X, int64_t Y, int64_t Z) {
  const int lx = ilog2(X), ly = ilog2(Y), lz = ilog2(Z);
  return nimg >= 2 && nimg <= 16 && lx >= 4 && lx <= 12 && ly >= 4 && ly <= 12 && lz >= 2 && lz <= 11 &&
         X * Y * Z < ((int64_t)1 << 31) - 2;
}

template <int LG, bool INV, bool ISA>
void launch_y(double2 *spec, int img0, int nimgs, int X, int Y, int Pz, const double2 *twY, hipStream_t s) {
  const int ntile = (int)hrf::cdiv((int64_t)X * Pz, TCA);
  const int64_t njobs = (int64_t)ntile * (Y >> LG) * nimgs;
  xc3_y_kernel<LG, INV, ISA><<<xgrid(xc3_y_kernel<LG, INV, ISA>, njobs), XT, 0, s>>>(spec, img0, nimgs, X, Y, Pz, twY,
                                                                                   ntile);
}

// pass A (size 2^(lgY / 2)) or pass B (size 2^(lgY - lgY / 2)) of the y axis
template <bool INV, bool ISA>
void launch_y_lg(int lgY, double2 *spec, int img0, int nimgs, int X, int Y, int Pz, const double2 *twY, hipStream_t s) {
  switch (ISA ? lgY / 2 : lgY - lgY / 2) {
    case 2: launch_y<2, INV, ISA>(spec, img0, nimgs, X, Y, Pz, twY, s); break;
    case 3: launch_y<3, INV, ISA>(spec, img0, nimgs, X, Y, Pz, twY, s); break;
    case 4: launch_y<4, INV, ISA>(spec, img0, nimgs, X, Y, Pz, twY, s); break;
    case 5: launch_y<5, INV, ISA>(spec, img0, nimgs, X, Y, Pz, twY, s); break;
    case 6: launch_y<6, INV, ISA>(spec, img0, nimgs, X, Y, Pz, twY, s); break;
  }
}

}  // namespace

extern "C" {

int64_t hrf_xcorr3_workspace_bytes(int32_t nimg, int64_t X, int64_t Y, int64_t Z) {
  if (!supported3(nimg, X, Y, Z)) return -1;
  const int64_t Pz = Z / 2 + 1;
  const int64_t jobs = ((int64_t)nimg - 1) * X * Y >> z_lgnb(ilog2(Z) - 1);
  return (int64_t)nimg * X * Y * Pz * (int64_t)sizeof(double2) + jobs * (int64_t)sizeof(JobBest) + 256;
}

static hrf_status xcorr3_run(const double *vols, int32_t nimg, int64_t X, int64_t Y, int64_t Z, void *work,
                             int32_t clamp, int32_t *shifts_dev, double *cc_out, hrf_stream_t stream) {
  HRF_REQUIRE(supported3(nimg, X, Y, Z), "xcorr3_shifts: power-of-two sizes 16..4096 (X, Y) / 4..2048 (Z), "
                                         "X Y Z < 2^31 - 2, 2..16 volumes");
  HRF_REQUIRE(vols && work, "xcorr3_shifts: null buffer");
  hipStream_t s = (hipStream_t)stream;
  const double2 *twX = nullptr, *twY = nullptr, *twZ = nullptr;
  if (hrf_status st = twiddles(X, &twX)) return st;
  if (hrf_status st = twiddles(Y, &twY)) return st;
  if (hrf_status st = twiddles(Z, &twZ)) return st;
  const int lgX = ilog2(X), lgY = ilog2(Y), lgM = ilog2(Z) - 1;
  const int Pz = (int)(Z / 2 + 1), P = (int)(Y * Pz);
  double2 *spec = reinterpret_cast<double2 *>(work);
  JobBest *jobbest = reinterpret_cast<JobBest *>(spec + (int64_t)nimg * X * Y * Pz);
  const int64_t lines = X * Y;  // per volume
  int64_t jobs_per_target = 0;
  switch (lgM) {
#define HRF_ZF(L)                                                                                               \
  case L: {                                                                                                     \
    const int64_t nj = nimg * lines >> z_lgnb(L);                                                               \
    xc3_z_fwd_kernel<L, z_lgnb(L)><<<xgrid(xc3_z_fwd_kernel<L, z_lgnb(L)>, nj), XT, 0, s>>>(vols, spec, twZ, nj); \
    jobs_per_target = lines >> z_lgnb(L);                                                                       \
    break;                                                                                                      \
  }
    HRF_ZF(1) HRF_ZF(2) HRF_ZF(3) HRF_ZF(4) HRF_ZF(5) HRF_ZF(6) HRF_ZF(7) HRF_ZF(8) HRF_ZF(9) HRF_ZF(10)
#undef HRF_ZF
  }
  launch_y_lg<false, true>(lgY, spec, 0, nimg, (int)X, (int)Y, Pz, twY, s);
  launch_y_lg<false, false>(lgY, spec, 0, nimg, (int)X, (int)Y, Pz, twY, s);
  const unsigned ta = (unsigned)hrf::cdiv(P, TCA), tb = (unsigned)hrf::cdiv(P, TCB);
  switch (lgX) {
#define HRF_XC(LH)                                                                                        \
  case LH: {                                                                                              \
    constexpr int L1 = LH / 2, L2 = LH - LH / 2;                                                          \
    xc_col_a_kernel<L1, L2, false><<<xgrid(xc_col_a_kernel<L1, L2, false>, (int64_t)ta * (1 << L2) * nimg), XT, 0, \
                                     s>>>(spec, 0, P, twX, (int)ta, nimg);                                  \
    xc_col_b_kernel<L1, L2><<<dim3(tb, 1u << L1), XT, 0, s>>>(spec, nimg, P, twX);                        \
    xc_col_a_kernel<L1, L2, true><<<xgrid(xc_col_a_kernel<L1, L2, true>, (int64_t)ta * (1 << L2) * (nimg - 1)),   \
                                    XT, 0, s>>>(spec, 1, P, twX, (int)ta, nimg - 1);                       \
    break;                                                                                                \
  }
    HRF_XC(4) HRF_XC(5) HRF_XC(6) HRF_XC(7) HRF_XC(8) HRF_XC(9) HRF_XC(10) HRF_XC(11) HRF_XC(12)
#undef HRF_XC
  }
  launch_y_lg<true, false>(lgY, spec, 1, nimg - 1, (int)X, (int)Y, Pz, twY, s);
  launch_y_lg<true, true>(lgY, spec, 1, nimg - 1, (int)X, (int)Y, Pz, twY, s);
  const double2 *spec1 = spec + lines * Pz;
  switch (lgM) {
#define HRF_ZI(L)                                                                                               \
  case L: {                                                                                                     \
    const int64_t nj = (nimg - 1) * jobs_per_target;                                                            \
    xc3_z_inv_kernel<L, z_lgnb(L)><<<xgrid(xc3_z_inv_kernel<L, z_lgnb(L)>, nj), XT, 0, s>>>(                    \
        spec1, twZ, jobbest, cc_out, nj, jobs_per_target);                                                      \
    break;                                                                                                      \
  }
    HRF_ZI(1) HRF_ZI(2) HRF_ZI(3) HRF_ZI(4) HRF_ZI(5) HRF_ZI(6) HRF_ZI(7) HRF_ZI(8) HRF_ZI(9) HRF_ZI(10)
#undef HRF_ZI
  }
  if (shifts_dev)
    xc3_shifts_kernel<<<(unsigned)(nimg - 1), XT, 0, s>>>(jobbest, jobs_per_target, X, Y, Z, clamp, shifts_dev);
  HRF_LAUNCHED();
  return HRF_OK;
}

hrf_status hrf_xcorr3_shifts_dev(const double *vols, int32_t nimg, int64_t X, int64_t Y, int64_t Z, void *work,
                                 int32_t clamp, int32_t *shifts_dev, hrf_stream_t stream) {
  HRF_REQUIRE(shifts_dev, "xcorr3_shifts: null buffer");
  return xcorr3_run(vols, nimg, X, Y, Z, work, clamp, shifts_dev, nullptr, stream);
}

hrf_status hrf_xcorr3_surfaces_dev(const double *vols, int32_t nimg, int64_t X, int64_t Y, int64_t Z, void *work,
                                   double *cc_out, hrf_stream_t stream) {
  HRF_REQUIRE(cc_out, "xcorr3_surfaces: null buffer");
  return xcorr3_run(vols, nimg, X, Y, Z, work, -1, nullptr, cc_out, stream);
}

}  // extern "C"
