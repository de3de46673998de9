// classify_exact.hip -- from a screen's output to the restated answer: the exact section of the
// prepared library, the list pass, the screens' error bounds and the host driver of certificate +
// list pass.
//
// The MFMA sweeps (classify_screen.hip) are a SCREEN: split-fp16 (or f32-MFMA) scores within a bound
// of the exact segmented-cosine score.  Every sweep also reports, per pixel, an upper bound s2 on the
// device score of every library row other than its best row b1 (the runner-up, `second`).  The refine:
//  * rescores b1 in f64 exactly as the restatement does (oracle seg_dist / oracle_segcos variant
//    0: the three sums in channel order, 1 - d / sqrt(nx * ny), the segment mean) from the pixel's
//    f32 values -- the stack, or the five shifted acquisitions of a registered tile -- and the f32
//    library promoted to f64 (the restatement's ref64);
//  * certifies b1 when D(b1) < 1 - (s2 + eps) / nseg - 1e-12, eps the screen's proven error bound
//    (screen_eps below): then every other row r has S_exact(r) <= s2 + eps, i.e. its restated
//    distance exceeds D(b1), so b1 is the restatement's argmin and D(b1) its distance, bit for bit;
//  * answers an all-zero pixel from the library alone (every segment one-zero or both-zero:
//    D(r) = (nonzero segments of r) / nseg, its first argmin precomputed at prepare time);
//  * lists every other pixel (ties, near-ties, NaN / inf values) for the list pass, which finds the
//    rows that can be the restated argmin and rescores those in f64 -- lowest row on ties.  Where
//    the screen's table is the 16x16x32 library image (E. coli layout: mode 2, the pixel table)
//    refine_cand_kernel finds them with one more MFMA sweep of that image against a threshold
//    proven from the screen's bound; elsewhere (modes 0 and 1, the community layout's 32x32x16
//    table) refine_list_kernel scores all rows in f32 with its own proven bound (fmaf chains on
//    the raw values) and keeps the rows within twice that bound of the best.
// The exact section's layout is ExactLayout's (classify_types.hpp).  The certificate's device code is
// classify_refine.hpp's refine_pixels64; its two kernels (refine_best_kernel and the fused table
// sweep) are compiled together in classify_screen.hip, see there.
#include "classify_refine.hpp"

using namespace hrf_cls;

namespace {

__global__ __launch_bounds__(256) void exact_prep_kernel(const float *__restrict__ ref, int32_t R, int32_t C,
                                                         Bounds bd, int32_t CP, int32_t RT, float *__restrict__ lib32,
                                                         float *__restrict__ libT, double *__restrict__ ny,
                                                         float *__restrict__ iy) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t e = t0; e < (int64_t)R * CP; e += stride) {
    const int64_t r = e / CP;
    const int c = (int)(e - r * CP);
    lib32[e] = c < C ? ref[r * C + c] : 0.0f;
  }
  for (int64_t e = t0; e < (int64_t)C * RT; e += stride) {
    const int64_t c = e / RT, r = e - c * RT;
    libT[e] = r < R ? ref[r * C + c] : 0.0f;
  }
  for (int64_t e = t0; e < (int64_t)R * bd.nseg; e += stride) {
    const int64_t r = e / bd.nseg;
    const int sg = (int)(e - r * bd.nseg);
    double v = 0.0;
    for (int i = bd.b[sg]; i < bd.b[sg + 1]; ++i) {
      const double y = (double)ref[r * C + i];
      v += y * y;
    }
    ny[e] = v;
    iy[e] = v > 0.0 ? (float)(1.0 / sqrt(v)) : 0.0f;
  }
}

// one thread: the all-zero pixel's answer (oracle_classify's loop on x = 0) and the tiny-row flag
__global__ void exact_hdr_kernel(const double *__restrict__ ny, int32_t R, int32_t C, int32_t nseg,
                                 ExactHdr *__restrict__ hdr) {
  double best = __builtin_inf();
  int32_t bi = 0, tiny = 0;
  for (int r = 0; r < R; ++r) {
    double sum = 0.0;
    for (int sg = 0; sg < nseg; ++sg) {
      const double v = ny[(int64_t)r * nseg + sg];
      sum += v == 0.0 ? 0.0 : 1.0;
      // the pixel side's gate (refine_list_kernel: v < 1e-30 || v > 1e30) on the library; the
      // negated compare also takes NaN and inf
      tiny |= ((v > 0.0 && v < 1e-30) || !(v < 1e30)) ? 1 : 0;
    }
    const double d = sum / nseg;
    if (d < best) {
      best = d;
      bi = r;
    }
  }
  hdr->R = R;
  hdr->C = C;
  hdr->nseg = nseg;
  hdr->idx0 = bi;
  hdr->D0 = best;
  hdr->tiny = tiny;
  for (int i = 0; i < 4; ++i) hdr->zero[i] = 0.0f;
}

// The list pass of the screens without a 16x16x32 image (modes 0 and 1, the community layout).
// Listed pixels, in batches of LIST_NP per workgroup (grid-strided over the device count), so
// each library value read from L2 serves LIST_NP pixels:
//  1. the batch's values (32 threads per pixel, lane = channel) and finiteness; per pixel and
//     segment the f64 sum of squares nx (channel order) and the f32 reciprocal norm ix;
//  2. every row's f32 score for every pixel of the batch (thread = 4 rows): per segment an fmaf
//     chain of the raw products d, cos = d * ix * iy (both-zero 1, one-zero 0), summed in f32; its
//     error is at most eps32 (screen_eps) -- so only rows within 2 eps32 of a pixel's best f32
//     score can be its restated argmin;
//  3. those rows (every row for a pixel with non-finite values or norms out of the f32 pass's
//     range) rescored exactly (exact_dist), minimum with the lowest row on ties, as
//     oracle_classify's first-minimum loop.
#ifndef HRF_LIST_LV
#define HRF_LIST_LV 4  // list pass: channels whose library loads are in flight together
#endif
constexpr int LIST_NP = 8;     // pixels per batch (stage 1 maps 32 threads per pixel)
constexpr int LIST_NT = 256;   // threads per workgroup
static_assert(LIST_NP * 32 == LIST_NT, "stage 1 loads one pixel per 32 threads");
__global__ __launch_bounds__(LIST_NT) void refine_list_kernel(PixSrc S, int32_t C, Bounds bd, ExactPtr E,
                                                              const ExactHdr *__restrict__ hdr, int32_t R,
                                                              double eps32, const int32_t *__restrict__ list,
                                                              const int32_t *__restrict__ cnt,
                                                              int32_t *__restrict__ stats,
                                                              int32_t *__restrict__ best_idx,
                                                              float *__restrict__ best_dist) {
  __shared__ float xb[LIST_NP][128];
  __shared__ float ixb[LIST_NP][SMAX];
  __shared__ int fullb[LIST_NP];
  __shared__ float thrb[LIST_NP];
  __shared__ double redd[LIST_NT / 64][LIST_NP];
  __shared__ int redr[LIST_NT / 64][LIST_NP];
  constexpr int CAND = 1024;  // sparse candidates per batch; a pixel that overflows is scored in full
  __shared__ int32_t cand[CAND];
  __shared__ int ncand;
  extern __shared__ float scb[];  // LIST_NP x RT f32 scores
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int n = *cnt;
  const int nseg = bd.nseg;
  for (int64_t b0 = (int64_t)blockIdx.x * LIST_NP; b0 < n; b0 += (int64_t)gridDim.x * LIST_NP) {
    const int nb = (int)min((int64_t)LIST_NP, n - b0);
    // 1. values: pixel j = t / 32, channels (t & 31) + 32 m
    {
      const int j = t >> 5, k0 = t & 31;
      bool bad = false;
      if (j < nb) {
        const int64_t p = list[b0 + j];
        int32_t off[XLMAX];
        src_offsets(S, p, true, off);
        for (int k = k0; k < C; k += 32) {
          int q = 0;
          for (int qq = 1; qq < S.n; ++qq) q = k >= S.c0[qq] ? qq : q;
          const float v = off[q] >= 0 ? S.src[q][off[q] + k - S.c0[q]] : 0.0f;
          xb[j][k] = v;
          bad = bad || !__builtin_isfinite(v);
        }
      }
      if (t < LIST_NP) fullb[t] = hdr->tiny;
      __syncthreads();
      if (bad) atomicOr(&fullb[j], 1);
    }
    if (t < nb * nseg) {
      const int j = t / nseg, sg = t - j * nseg;
      double v = 0.0;
      for (int i = bd.b[sg]; i < bd.b[sg + 1]; ++i) {
        const double xd = (double)xb[j][i];
        v += xd * xd;
      }
      ixb[j][sg] = v > 0.0 ? (float)(1.0 / sqrt(v)) : 0.0f;
      if (v > 0.0 && (v < 1e-30 || v > 1e30)) atomicOr(&fullb[j], 1);
    }
    __syncthreads();
    // 2. f32 scores, thread = rows r0 + t + 256 u
    for (int r0 = 0; r0 < E.RT; r0 += 4 * LIST_NT) {
      float sc[LIST_NP][4];
#pragma unroll
      for (int j = 0; j < LIST_NP; ++j)
#pragma unroll
        for (int u = 0; u < 4; ++u) sc[j][u] = 0.0f;
      for (int sg = 0; sg < nseg; ++sg) {
        float d[LIST_NP][4];
#pragma unroll
        for (int j = 0; j < LIST_NP; ++j)
#pragma unroll
          for (int u = 0; u < 4; ++u) d[j][u] = 0.0f;
        // LV channels' loads in flight together (clamped addresses, no branch around a load; rows
        // past RT are never stored), then their fmaf chains in channel order
        constexpr int LV = HRF_LIST_LV;
        const int ce = bd.b[sg + 1];
        for (int i0 = bd.b[sg]; i0 < ce; i0 += LV) {
          float y[LV][4];
#pragma unroll
          for (int v = 0; v < LV; ++v) {
            const int i = min(i0 + v, ce - 1);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int r = min(r0 + t + LIST_NT * u, E.RT - 1);
              y[v][u] = E.libT[(int64_t)i * E.RT + r];
            }
          }
#pragma unroll
          for (int v = 0; v < LV; ++v) {
            const bool ok = i0 + v < ce;  // (a select, not a branch: a branch would take the loads with it)
            const int i = ok ? i0 + v : i0;
#pragma unroll
            for (int j = 0; j < LIST_NP; ++j) {
              const float x = xb[j][i];
#pragma unroll
              for (int u = 0; u < 4; ++u) d[j][u] = ok ? __builtin_fmaf(x, y[v][u], d[j][u]) : d[j][u];
            }
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int r = r0 + t + LIST_NT * u;
          const float iyv = r < R ? E.iy[(int64_t)r * nseg + sg] : 0.0f;
#pragma unroll
          for (int j = 0; j < LIST_NP; ++j) {
            const float ix = ixb[j][sg];
            const float c = ix == 0.0f ? (iyv == 0.0f ? 1.0f : 0.0f) : (iyv == 0.0f ? 0.0f : (d[j][u] * ix) * iyv);
            sc[j][u] += c;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = r0 + t + LIST_NT * u;
        if (r < E.RT)
#pragma unroll
          for (int j = 0; j < LIST_NP; ++j) scb[j * E.RT + r] = r < R ? sc[j][u] : -__builtin_inff();
      }
    }
    __syncthreads();
    // per pixel: the best f32 score -> the candidate threshold (wave w takes pixels w, w + 4)
    for (int j = w; j < nb; j += LIST_NT / 64) {
      float mx = -__builtin_inff();
      for (int r = lane; r < R; r += 64) mx = fmaxf(mx, scb[j * E.RT + r]);
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      if (lane == 0) {
        float th = mx - (float)(2.0 * eps32) * 1.0001f;
        thrb[j] = th - fabsf(th) * 1e-6f;  // the subtraction's own rounding, generously
        // an overflowed f32 pass (mx +inf: the threshold is NaN and no row meets it) would answer
        // row 0 at distance inf: every row of such a pixel is scored exactly instead.  With the
        // pixel's and the library's range gates (sums of squares <= 1e30 both: no partial sum of a
        // segment's products passes sqrt(nx ny) <= 1e30) the pass cannot overflow; this is the
        // guard behind them.
        if (!(fabsf(thrb[j]) < __builtin_inff())) atomicOr(&fullb[j], 1);
      }
    }
    __syncthreads();
    // 3. exact distances: the candidates of the other pixels compacted into one list shared by
    //    all threads (a handful per pixel), every row of the full-path pixels; per pixel the
    //    minimum, lowest row on ties, whatever order the rows were visited in
    if (t == 0) ncand = 0;
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
      if (fullb[j]) continue;
      const float th = thrb[j];
      for (int r = t; r < R; r += LIST_NT)
        if (scb[j * E.RT + r] >= th) {
          const int k = atomicAdd(&ncand, 1);
          if (k < CAND) cand[k] = (j << 16) | r;
          else atomicOr(&fullb[j], 2);
        }
    }
    __syncthreads();
    double bdv[LIST_NP];
    int brv[LIST_NP];
#pragma unroll
    for (int j = 0; j < LIST_NP; ++j) {
      bdv[j] = __builtin_inf();
      brv[j] = 0x7fffffff;
    }
    auto take = [&](int j, int r, double D) {
#pragma unroll
      for (int jj = 0; jj < LIST_NP; ++jj)
        if (jj == j && (D < bdv[jj] || (D == bdv[jj] && r < brv[jj]))) {
          bdv[jj] = D;
          brv[jj] = r;
        }
    };
    // sparse candidates, one thread each (all of a batch's candidates at once): the restatement's
    // arithmetic (exact_dist) bit for bit
    const int nc = min(ncand, CAND);
    if (t < nb && fullb[t]) atomicAdd(stats + 1, 1);  // statistics: pixels scored in full
    if (t == 0) atomicAdd(stats, nc);                  // and sparse candidates
    for (int k = t; k < nc; k += LIST_NT) {
      const int j = cand[k] >> 16, r = cand[k] & 0xffff;
      if (fullb[j]) continue;
      int nz = 0;
      take(j, r, exact_dist(xb[j], E, r, C, bd, &nz));
    }
    for (int j = 0; j < nb; ++j)
      if (fullb[j])
        for (int r = t; r < R; r += LIST_NT) {
          int nz = 0;
          take(j, r, exact_dist(xb[j], E, r, C, bd, &nz));
        }
#pragma unroll
    for (int j = 0; j < LIST_NP; ++j) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const double ob = __shfl_xor(bdv[j], o, 64);
        const int orr = __shfl_xor(brv[j], o, 64);
        if (ob < bdv[j] || (ob == bdv[j] && orr < brv[j])) {
          bdv[j] = ob;
          brv[j] = orr;
        }
      }
      if (lane == 0) {
        redd[w][j] = bdv[j];
        redr[w][j] = brv[j];
      }
    }
    __syncthreads();
    if (t < nb) {
      double bv = redd[0][t];
      int br = redr[0][t];
      for (int ww = 1; ww < LIST_NT / 64; ++ww) {
        const double ob = redd[ww][t];
        const int orr = redr[ww][t];
        if (ob < bv || (ob == bv && orr < br)) {
          bv = ob;
          br = orr;
        }
      }
      const int64_t p = list[b0 + t];
      best_idx[p] = br == 0x7fffffff ? 0 : br;
      best_dist[p] = (float)bv;
    }
    __syncthreads();
  }
}

// ---- the list pass on a 16x16x32 library image: an MFMA candidate sweep ---------------------------
// Where the screen's table is the 16x16x32 image (E. coli layout: mode 2 and the pixel table) the
// candidates come from one more sweep of that image instead of the f32 scoring of every row.  The
// rule: with S the restated score (nseg (1 - D)) and S_dev the sweep's, |S_dev(r) - S(r)| <= eps for
// every row r of a pixel inside the screen bound's premises (screen_eps; eps = eps_base + eps_zero
// per all-zero segment).  For the restated argmin r* and the pixel's screen row b1,
//   S_dev(r*) >= S(r*) - eps >= S(b1) - eps,
// and S(b1) is taken from b1's exact distance, which the kernel computes anyway (b1 is always a
// candidate).  The bound holds for this sweep because it runs the screen's arithmetic on the screen's
// operands: the B operands built as hrf_pix::prep_tile builds them (f32 sums of squares in channel
// order, v_rsq, the f64 redo below 1e-30, one f32 multiply, the hi/lo split, the bias column), the
// MFMA order of sweep_w16 (cross products first, hi * hi' last, the indicator step always on: it
// adds exact zeros where no segment is all zero).  Equality of its bits with the screen's is not
// part of the argument, and b1 need not be the screen's argmax: any real row gives a valid threshold.
//
// A workgroup takes 64 listed pixels, one 16-pixel MFMA group per wave, grid-strided over the device
// count (a count of zero costs the launch).  Per batch:
//  1. the raw f32 values through PixSrc (4 threads per pixel) and their finiteness;
//  2. wave 0: the segment norms and the normalised values; wave 1: b1's exact distance, the range
//     gate and the all-zero segments (exact_dist), hence the threshold
//     thr = nseg (1 - D(b1) - 1e-12) - eps, rounded down;
//  3. every wave: its group's split-fp16 B operands, then the sweep of the image through three LDS
//     chunk buffers (LDS-DMA, two chunks in flight); the epilogue holds no keys: acc >= thr appends
//     (pixel, row) to an LDS list.  Padding rows (r >= R) are masked in the compare;
//  4. the candidates rescored as the restatement does (exact_dist, one thread each), the minimum with
//     the lowest row on ties through two LDS atomic-min rounds (an order-preserving key of the f64
//     distance, then the row among the candidates that reach it).
// Scored on every row in f64 instead, as before: pixels with non-finite values, with a segment sum
// of squares outside NX_MIN / NX_MAX, without a real b1, every pixel of a library flagged tiny, and
// a pixel whose candidates did not fit the list.
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) void glb_void_t;

constexpr int CAND_NW = 4;             // waves per workgroup, one 16-pixel group each
constexpr int CAND_NP = 16 * CAND_NW;  // listed pixels per batch
constexpr int CAND_NT = 64 * CAND_NW;
constexpr int CAND_CR = 32;            // image rows per LDS chunk
constexpr int CAND_NBUF = 3;           // chunk buffers: two chunks in flight behind the one in use
constexpr int CAND_MAX = 1024;         // candidates per batch; a pixel that overflows is scored in full
static_assert(CAND_NP == 64 && CAND_NT == 4 * CAND_NP, "a lane per pixel (stages 2, 4), four threads per pixel (1)");

// f64 distance <-> a u64 that orders as the distance does (no NaN; -0 is canonicalised)
__device__ __forceinline__ unsigned long long dist_key(double D) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(D + 0.0);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_dist(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

template <class L>
constexpr size_t cand_lds_bytes() {
  constexpr int XS = (L::C + 3) & ~3;
  return (size_t)CAND_NBUF * CAND_CR * (128 * hrf_pix::lay_kt<L>() + L::PADB) + sizeof(float) * CAND_NP * XS +
         (sizeof(double) + sizeof(int32_t)) * CAND_MAX;
}

template <class L>
__global__ __launch_bounds__(CAND_NT, 2) void refine_cand_kernel(RefineArgs A, int32_t R,
                                                                 int32_t *__restrict__ stats,
                                                                 int32_t *__restrict__ best_idx,
                                                                 float *__restrict__ best_dist) {
  constexpr int C = L::C, NSEG = L::NSEG, KT = hrf_pix::lay_kt<L>(), KP = 32 * KT;
  constexpr int ROWB = 4 * KP + L::PADB, CHB = CAND_CR * ROWB, NPC = CHB / 1024;
  constexpr int XS = (C + 3) & ~3;  // floats per pixel of the value buffers
  static_assert(CHB % 1024 == 0, "a chunk must be whole 1 KiB LDS-DMA pieces");
  static_assert(CAND_NP * XS * 4 <= CAND_NBUF * CHB, "the normalised values alias the chunk buffers");
  static_assert(32 * KT <= XS + 1 && C < 32 * KT, "a B-operand read stays inside its pixel's row");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  char *ldsb = reinterpret_cast<char *>(lds);
  float *xn = lds;                                                   // normalised values (before the first DMA)
  float *xb = reinterpret_cast<float *>(ldsb + CAND_NBUF * CHB);     // raw values
  double *candD = reinterpret_cast<double *>(xb + CAND_NP * XS);     // candidates' exact distances
  int32_t *cand = reinterpret_cast<int32_t *>(candD + CAND_MAX);     // (pixel << 16) | row
  __shared__ float thrb[CAND_NP];
  __shared__ int fullb[CAND_NP];
  __shared__ uint32_t zxs[CAND_NP];
  __shared__ unsigned long long minkey[CAND_NP];
  __shared__ int minrow[CAND_NP];
  __shared__ double redd[CAND_NW];
  __shared__ int redr[CAND_NW];
  __shared__ int ncand;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int rl = lane & 15, Q = lane >> 4;
  const int n = *A.cnt;
  const char *img = reinterpret_cast<const char *>(A.img);
  const int nch = A.img_rows / CAND_CR;
  const int tiny = A.hdr->tiny;
  for (int64_t b0 = (int64_t)blockIdx.x * CAND_NP; b0 < n; b0 += (int64_t)gridDim.x * CAND_NP) {
    const int nb = (int)min((int64_t)CAND_NP, n - b0);
    if (t < CAND_NP) fullb[t] = tiny ? 1 : 0;
    if (t == 0) ncand = nb;  // entries 0 .. nb - 1: every pixel's b1
    __syncthreads();
    // 1. values: pixel j = t / 4, channels (t & 3) + 4 m (one pass: every load of the batch in
    //    flight together); rows past the batch and the row pad read as zero
    {
      const int j = t >> 2, k0 = t & 3;
      float *px = xb + j * XS;
      bool bad = false;
      if (j < nb) {
        const int64_t p = A.list[b0 + j];
        int32_t off[XLMAX];
        src_offsets(A.S, p, true, off);
        float v[XS / 4];
#pragma unroll
        for (int m = 0; m < XS / 4; ++m) {
          const int k = k0 + 4 * m;
          const int kc = k < C ? k : C - 1;  // (a readable channel for the pad)
          int q = 0;
          for (int qq = 1; qq < A.S.n; ++qq) q = kc >= A.S.c0[qq] ? qq : q;
          const int32_t o = off[q];
          v[m] = *(o >= 0 ? A.S.src[q] + (o + kc - A.S.c0[q]) : A.hdr->zero);
        }
#pragma unroll
        for (int m = 0; m < XS / 4; ++m) {
          const float x = k0 + 4 * m < C ? v[m] : 0.0f;
          px[k0 + 4 * m] = x;
          bad = bad || !__builtin_isfinite(x);
        }
      } else {
        for (int k = k0; k < XS; k += 4) px[k] = 0.0f;
      }
      if (bad) atomicOr(&fullb[j], 1);
    }
    __syncthreads();
    // 2. wave 0: the norms (prep_tile's arithmetic), lane = pixel; wave 1: b1 and the threshold
    if (w == 0) {
      const float *px = xb + lane * XS;
      float *pn = xn + lane * XS;
      float nn[NSEG];
#pragma unroll
      for (int s = 0; s < NSEG; ++s) nn[s] = 0.0f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float x = px[c];
        nn[hrf_pix::lay_seg<L>(c)] = __builtin_fmaf(x, x, nn[hrf_pix::lay_seg<L>(c)]);
      }
      float inv[NSEG];
      uint32_t zx = 0;
#pragma unroll
      for (int s = 0; s < NSEG; ++s) {
        inv[s] = rsqrtf(nn[s]);
        if (!(nn[s] >= 1e-30f)) {  // zero, or an f32 underflow: decide from the bits, redo in f64
          uint32_t nz = 0;
          double td = 0.0;
          for (int c = L::b(s); c < L::b(s + 1); ++c) {
            const float x = px[c];
            nz |= __float_as_uint(x) << 1;
            td += (double)x * (double)x;
          }
          inv[s] = nz ? (float)(1.0 / sqrt(td)) : 0.0f;
          zx |= (nz ? 0u : 1u) << s;
        }
      }
#pragma unroll
      for (int c = 0; c < C; ++c) pn[c] = px[c] * inv[hrf_pix::lay_seg<L>(c)];
      zxs[lane] = zx;
    } else if (w == 1) {
      float th = __builtin_inff();
      if (lane < nb) {
        const int64_t p = A.list[b0 + lane];
        const int b1 = best_idx[p];
        const bool brow = b1 >= 0 && b1 < R;
        const int b1c = brow ? b1 : 0;
        int nz = 0;
        bool rok = true;
        const double D1 = exact_dist(xb + lane * XS, A.E, b1c, C, A.bd, &nz, &rok);
        const double eps = A.eps_base + A.eps_zero * nz;
        th = (float)((double)NSEG * (1.0 - D1 - 1e-12) - eps * 1.0001);
        th = th - fabsf(th) * 1e-6f;  // the conversion's own rounding, generously
        // (a NaN or infinite threshold -- a NaN distance of b1 -- meets no row: such a pixel is scored in full)
        if (!brow || !rok || !(fabsf(th) < __builtin_inff())) atomicOr(&fullb[lane], 1);
        cand[lane] = (lane << 16) | b1c;
        candD[lane] = D1;
      }
      thrb[lane] = th;
    }
    __syncthreads();
    // 3. this wave's B operands: pixel 16 w + (lane & 15), columns 32 t + 8 Q + q; column C is the
    //    validity-bias column (1), columns past it 0
    const int jj = 16 * w + rl;
    h8 bh[KT], bl[KT];
    {
      const float *pc = xn + jj * XS + 8 * Q;
#pragma unroll
      for (int tt = 0; tt < KT; ++tt) {
        h8 vh, vl;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int k = 32 * tt + 8 * Q + q;
          float x = 0.0f;
          if (32 * tt + 24 + q < C) {  // every lane quarter's column is a channel
            x = pc[32 * tt + q];
          } else {
            const float xv = pc[min(32 * tt + q, XS - 1 - 8 * Q)];  // (clamped inside the pixel's row)
            x = k < C ? xv : (k == C ? 1.0f : 0.0f);
          }
          const _Float16 hv = (_Float16)x;
          vh[q] = hv;
          vl[q] = (_Float16)(x - (float)hv);
        }
        bh[tt] = vh;
        bl[tt] = vl;
      }
    }
    h8 bz;  // the pixel's zero-segment indicators: fp16 1.0 in slot q < NSEG of quarter 0
    {
      const uint32_t m = Q == 0 ? (zxs[jj] & ((1u << NSEG) - 1u)) : 0u;
#pragma unroll
      for (int q = 0; q < 8; ++q) bz[q] = (_Float16)(((m >> q) & 1u) ? 1.0f : 0.0f);
    }
    const bool live = jj < nb && !fullb[jj];
    const float th = live ? thrb[jj] : __builtin_inff();
    const int b1r = live ? (cand[jj] & 0xffff) : -1;
    __syncthreads();  // the normalised values are consumed: the chunk buffers take their place
    auto issue = [&](int c) {
      const char *g = img + (int64_t)c * CHB + lane * 16;
      char *l = ldsb + (c % CAND_NBUF) * CHB;
      for (int q = w; q < NPC; q += CAND_NW)
        __builtin_amdgcn_global_load_lds((glb_void_t *)(g + q * 1024), (lds_void_t *)(l + q * 1024), 16, 0, 0);
    };
    // pieces this wave issues per chunk: the wait for chunk c leaves chunk c + 1's outstanding
    constexpr int MINE_LO = NPC / CAND_NW;
    const bool more = w < NPC % CAND_NW;
    issue(0);
    if (nch > 1) issue(1);
    for (int c = 0; c < nch; ++c) {
      // chunk c landed: this wave's LDS-DMA of it retired (in issue order; the barrier's wait does
      // not count it), then the barrier covers every wave's pieces; everyone is past chunk c - 1,
      // whose buffer chunk c + 2 takes
      if (c + 1 >= nch) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (more) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(MINE_LO + 1) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(MINE_LO) : "memory");
      __syncthreads();
      if (c + 2 < nch) issue(c + 2);
      const char *buf = ldsb + (c % CAND_NBUF) * CHB;
#pragma unroll
      for (int rb = 0; rb < CAND_CR; rb += 16) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        const char *row = buf + (rb + rl) * ROWB + 16 * Q;
        const h8 az = *reinterpret_cast<const h8 *>(buf + (rb + rl) * ROWB + 4 * KP);
#pragma unroll
        for (int tt = 0; tt < KT; ++tt) {
          const h8 ah = *reinterpret_cast<const h8 *>(row + 64 * tt);
          const h8 al = *reinterpret_cast<const h8 *>(row + 2 * KP + 64 * tt);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[tt], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[tt], acc, 0, 0, 0);
        }
#pragma unroll
        for (int tt = 0; tt < KT; ++tt) {
          const h8 ah = *reinterpret_cast<const h8 *>(row + 64 * tt);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[tt], acc, 0, 0, 0);
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(az, bz, acc, 0, 0, 0);
        // this lane's rows 4 Q .. 4 Q + 3 of the block, pixel jj
        const int r0 = c * CAND_CR + rb + 4 * Q;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = r0 + i;
          if (live && acc[i] >= th && r < R && r != b1r) {
            const int k = atomicAdd(&ncand, 1);
            if (k < CAND_MAX) cand[k] = (jj << 16) | r;
            else atomicOr(&fullb[jj], 2);
          }
        }
      }
    }
    __syncthreads();
    // 4. exact distances (the restatement's arithmetic, bit for bit): the sparse candidates, one
    //    thread each, then every row of the full-path pixels; the minimum, lowest row on ties
    const int nc = min(ncand, CAND_MAX);
    if (t < CAND_NP) {
      minkey[t] = dist_key(__builtin_inf());
      minrow[t] = 0x7fffffff;
    }
    if (t < nb && fullb[t]) atomicAdd(stats + 1, 1);  // statistics: pixels scored in full
    if (t == 0) atomicAdd(stats, nc);                  // and sparse candidates
    __syncthreads();
    for (int k = t; k < nc; k += CAND_NT) {
      const int j = cand[k] >> 16, r = cand[k] & 0xffff;
      if (fullb[j]) continue;
      double D;
      if (k < nb) {
        D = candD[k];
      } else {
        int nz = 0;
        D = exact_dist(xb + j * XS, A.E, r, C, A.bd, &nz);
        candD[k] = D;
      }
      if (D == D) atomicMin(&minkey[j], dist_key(D));
    }
    __syncthreads();
    for (int k = t; k < nc; k += CAND_NT) {
      const int j = cand[k] >> 16, r = cand[k] & 0xffff;
      if (fullb[j]) continue;
      const double D = candD[k];
      if (D == D && dist_key(D) == minkey[j]) atomicMin(&minrow[j], r);
    }
    for (int j = 0; j < nb; ++j) {
      if (!fullb[j]) continue;  // (workgroup-uniform)
      double bv = __builtin_inf();
      int br = 0x7fffffff;
      for (int r = t; r < R; r += CAND_NT) {
        int nz = 0;
        const double D = exact_dist(xb + j * XS, A.E, r, C, A.bd, &nz);
        if (D < bv || (D == bv && r < br)) {
          bv = D;
          br = r;
        }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const double ob = __shfl_xor(bv, o, 64);
        const int orr = __shfl_xor(br, o, 64);
        if (ob < bv || (ob == bv && orr < br)) {
          bv = ob;
          br = orr;
        }
      }
      if (lane == 0) {
        redd[w] = bv;
        redr[w] = br;
      }
      __syncthreads();
      if (t == 0) {
        for (int ww = 1; ww < CAND_NW; ++ww)
          if (redd[ww] < bv || (redd[ww] == bv && redr[ww] < br)) {
            bv = redd[ww];
            br = redr[ww];
          }
        minkey[j] = dist_key(bv);
        minrow[j] = br;
      }
      __syncthreads();
    }
    __syncthreads();
    if (t < nb) {
      const int64_t p = A.list[b0 + t];
      const int br = minrow[t];
      best_idx[p] = br == 0x7fffffff ? 0 : br;
      best_dist[p] = (float)key_dist(minkey[t]);
    }
    __syncthreads();
  }
}

// The screen's proven error bound, in score units (score = sum over segments of the cosine of the
// segment-normalised vectors, plus the zero-segment indicators), for a pixel with no all-zero
// segment (eps_zero per all-zero segment on top).  u = 2^-24.  Terms, per segment s of n_s channels:
//  (a) the pixel's f32 normalisation: f32 sum of squares (<= n_s u), v_rsq (<= 2 u), the product
//      (u): the segment cosine moves by <= (n_s / 2 + 4) u;
//  (b) the library's normalisation (f64, rounded to f32): <= 1.01 u;
//  (c) split fp16 (v = hi + lo + e, |e| <= 2^-22 |v| + 2^-25; lo * lo' dropped):
//      <= 3 * 2^-22 + 2^-24 * 1.01 sqrt(n_s)  (sum |x| <= sqrt(n_s) for a unit segment);
//  (d) the MFMA accumulation: each f16 MFMA output within KMFMA u (|C_in| + sum |a b|) of the exact
//      (hrf_probe_mfma_f16: tests/test_classify_exact_gpu.py measures <= 7.6 on gfx950 and asserts
//      <= 12; the bound uses 16), and every partial sum of an output is <= A = sum |products| <=
//      1.002 nseg (+1 per all-zero segment: the indicator terms), so NM MFMAs per output add
//      <= KMFMA u NM A.  The f32 MFMA (mode 0) is a k-ordered fmaf chain (cdna_hip_programming.md
//      "FP32-input MFMA"): <= KP u A.
// The keyed sweeps' 4 truncated bits are covered by reporting s2 with them set (key_score_hi).
constexpr double KMFMA = 16.0;
constexpr double U24 = 1.0 / 16777216.0;
ScreenEps screen_eps(const Bounds &bd, double nmfma, bool f32chain, int kp) {
  double a = 0.0, c = 0.0, e32 = 0.0;
  for (int sg = 0; sg < bd.nseg; ++sg) {
    const int ns = bd.b[sg + 1] - bd.b[sg];
    a += ns / 2.0 + 4.0 + 1.01;
    c += 12.0 + 1.01 * sqrt((double)ns);
    e32 += ns + 4.01;
  }
  e32 += (double)bd.nseg * bd.nseg;
  const double A = 1.002 * bd.nseg + 0.01;
  const double per = f32chain ? (double)kp : KMFMA * nmfma;
  ScreenEps e;
  e.base = U24 * (a + c + per * A) * 1.01;
  e.zero = U24 * per * 1.01;
  e.eps32 = U24 * e32 * 1.01;
  return e;
}

}  // namespace

namespace hrf_cls {

// the exact section (refine): f32 library row- and channel-major, ny, iy, header
void exact_prepare(const float *ref, int32_t R, int32_t C, const Geometry &g, void *refx, hipStream_t s) {
  const ExactLayout &el = g.el;
  char *sec = (char *)refx + el.off;
  exact_prep_kernel<<<hrf::stream_grid((int64_t)C * el.RT), 256, 0, s>>>(
      ref, R, C, g.bd, el.CP, el.RT, (float *)(sec + el.lib32), (float *)(sec + el.libT), (double *)(sec + el.ny),
      (float *)(sec + el.iy));
  exact_hdr_kernel<<<1, 1, 0, s>>>((const double *)(sec + el.ny), R, C, g.bd.nseg, (ExactHdr *)sec);
}

// MFMAs accumulated into one score by each screen (the bound's NM): screen 0 = mode 0 (f32 chain,
// KP fmas), 1 = mode 1 (32x32x16, indicator columns), 2 = mode 2 in-kernel (E. coli: the 16x16x32
// w16 sweep, community: the 32x32x16 lay sweep; + the indicator k-step), 3 = the pixel-table w16t
ScreenEps eps_of_screen(int screen, const Bounds &bd, int C, int kp) {
  const int lay = layout_id(bd, C);
  if (screen == 0) return screen_eps(bd, 0, true, kp);
  if (screen == 1) return screen_eps(bd, 3 * (kp / 16), false, kp);
  if (screen == 2 && lay == 2) {  // classify_pixels_lay_kernel: cross products first, as w16
    const int ks = (C + 1 + 15) / 16;
    return screen_eps(bd, ks + 1 + 2.0 * ks * 0x1p-9, false, kp);
  }
  // w16 / w16t: the 2 KT cross-product MFMAs meet accumulators below 2^-9 A (their products are
  // <= 2^-10 A in all), then KT hi * hi' MFMAs and the indicator step at full magnitude
  const int kt = (C + 1 + 31) / 32;
  return screen_eps(bd, kt + 1 + 2.0 * kt * 0x1p-9, false, kp);
}

// the refine's arguments for `screen`'s output on refx; fuse: the table sweep (screen 3) runs the
// certificate itself (classify_pixels_w16t_kernel<..., true>), else refine_best_kernel does
hrf_status refine_args(const PixSrc &S, int64_t P, int32_t C, const void *refx, int32_t R, const Bounds &bd,
                       int32_t screen, void *work, int64_t work_bytes, RefineArgs *A, hipStream_t s) {
  HRF_REQUIRE(screen >= 0 && screen <= 3, "classify_refine: screen must be 0..3");
  Geometry g;
  if (hrf_status st = resolve(C, bd.b, bd.nseg, R, screen == 3 ? 2 : screen, &g)) return st;
  HRF_REQUIRE(C <= 128 && R <= LIST_RMAX, "classify_refine: C <= 128 and R <= %d required", LIST_RMAX);
  HRF_REQUIRE(work_bytes >= hrf_classify_refine_work_bytes(P), "classify_refine: work buffer too small");
  HRF_REQUIRE(refx && work, "classify_refine: null buffer");
  const ExactLayout &el = g.el;
  const char *sec = (const char *)refx + el.off;
  A->S = S;
  A->E.lib32 = (const float *)(sec + el.lib32);
  A->E.libT = (const float *)(sec + el.libT);
  A->E.ny = (const double *)(sec + el.ny);
  A->E.iy = (const float *)(sec + el.iy);
  A->E.CP = el.CP;
  A->E.RT = el.RT;
  A->hdr = (const ExactHdr *)sec;
  const ScreenEps ep = eps_of_screen(screen, bd, C, g.kp);
  A->eps_base = ep.base;
  A->eps_zero = ep.zero;
  A->cnt = (int32_t *)work;
  A->list = (int32_t *)((char *)work + 16);
  A->bd = bd;
  // the candidate sweep reads the 16x16x32 image of the E. coli layout (mode 2 and the pixel table)
  const bool image = (screen == 2 || screen == 3) && g.lay == 1;
  A->img = image ? refx : nullptr;
  A->img_rowb = (int32_t)g.rowb;
  A->img_rows = g.rpad;
  HRF_HIP(hipMemsetAsync(A->cnt, 0, 4 * sizeof(int32_t), s));  // count + the list pass's statistics
  return HRF_OK;
}

// the list pass over what the certificate left (device-held count)
hrf_status refine_list(const RefineArgs &A, int64_t P, int32_t C, int32_t R, const Bounds &bd, int32_t screen,
                       int32_t *best_idx, float *best_dist, hipStream_t s) {
  Geometry g;
  if (hrf_status st = resolve(C, bd.b, bd.nseg, R, screen == 3 ? 2 : screen, &g)) return st;
  if (A.img) {  // candidates from an MFMA sweep of the library image
    using L = LayEcoli;
    HRF_REQUIRE(A.img_rowb == 128 * hrf_pix::lay_kt<L>() + L::PADB && A.img_rows % CAND_CR == 0,
                "classify_refine: the library image does not have the 16x16x32 sweep's geometry");
    const size_t shm = cand_lds_bytes<L>();
    (void)hipFuncSetAttribute((const void *)refine_cand_kernel<L>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    const unsigned grid = hrf::resident_grid(refine_cand_kernel<L>, CAND_NT, shm, hrf::cdiv(P, CAND_NP));
    refine_cand_kernel<L><<<grid, CAND_NT, shm, s>>>(A, R, A.cnt + 1, best_idx, best_dist);
    HRF_LAUNCHED();
    return HRF_OK;
  }
  const ScreenEps ep = eps_of_screen(screen, bd, C, g.kp);
  const size_t shm = sizeof(float) * LIST_NP * (size_t)A.E.RT;  // 128 KB at R = LIST_RMAX
  (void)hipFuncSetAttribute((const void *)refine_list_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  const unsigned grid = hrf::resident_grid(refine_list_kernel, LIST_NT, shm, hrf::cdiv(P, LIST_NP));
  refine_list_kernel<<<grid, LIST_NT, shm, s>>>(A.S, C, bd, A.E, A.hdr, R, ep.eps32, A.list, A.cnt, A.cnt + 1, best_idx,
                                             best_dist);
  HRF_LAUNCHED();
  return HRF_OK;
}

hrf_status refine(const PixSrc &S, int64_t P, int32_t C, const void *refx, int32_t R, const Bounds &bd, int32_t screen,
                  const float *second, int32_t *best_idx, float *best_dist, void *work, int64_t work_bytes,
                  hipStream_t s) {
  if (P == 0) return HRF_OK;
  HRF_REQUIRE(second && best_idx && best_dist, "classify_refine: null buffer");
  RefineArgs A;
  if (hrf_status st = refine_args(S, P, C, refx, R, bd, screen, work, work_bytes, &A, s)) return st;
  refine_best(A, P, C, bd, second, best_idx, best_dist, s);  // the certificate (classify_screen.hip)
  HRF_LAUNCHED();
  return refine_list(A, P, C, R, bd, screen, best_idx, best_dist, s);
}

hrf_status pixsrc_of(const float *const *src_host, const int32_t *channels_host, const int32_t *shifts_dev,
                     int32_t nlaser, int64_t H, int64_t W, int32_t apply_mask, int32_t C, PixSrc *S) {
  HRF_REQUIRE(nlaser >= 1 && nlaser <= XLMAX && src_host && channels_host && H >= 0 && W >= 1,
              "classify_refine: bad pixel source");
  *S = PixSrc{};
  S->n = nlaser;
  S->c0[0] = 0;
  for (int q = 0; q < nlaser; ++q) {
    HRF_REQUIRE(src_host[q] && channels_host[q] >= 1, "classify_refine: laser %d missing", q);
    S->src[q] = src_host[q];
    S->c0[q + 1] = S->c0[q] + channels_host[q];
    S->mdiv[q] = ((uint64_t)1 << 32) / (uint64_t)channels_host[q] + (((uint64_t)1 << 32) % (uint64_t)channels_host[q] ? 1 : 0);
  }
  for (int q = nlaser; q < XLMAX; ++q) S->c0[q + 1] = S->c0[nlaser];
  HRF_REQUIRE(S->c0[nlaser] == C, "classify_refine: the lasers hold %d channels, the library %d", S->c0[nlaser], C);
  HRF_REQUIRE(H * W * (int64_t)C < ((int64_t)1 << 31), "classify_refine: H * W * C must be < 2^31");
  S->dsh = shifts_dev;
  S->H = H;
  S->W = W;
  S->apply_mask = apply_mask;
  return HRF_OK;
}

}  // namespace hrf_cls
