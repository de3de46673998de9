// classify_screen.hip -- the per-pixel screens: everything that produces (best row, score,
// runner-up bound) per pixel.  The library-table builders, the three generations of MFMA sweeps on a
// (P, C) stack (modes 0, 1, 2), the sweep on a prepared pixel table (alone, or with the certificate
// fused in) and beside it the certificate as a kernel of its own, their host launchers, and the MFMA
// accumulation probe.  classify.hip's header describes the method and maps the units.
#include "classify_refine.hpp"

using namespace hrf_cls;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// workgroups per CU the fused table sweep (w16t with FUSE) is built for.  Round 6: 2 (256 VGPRs).
// The runner-up tracking (t2, the refine's certificate) does not fit the 168 VGPRs of three: at three
// the E. coli table sweep reloaded B operands from scratch every chunk, 2.87 ms per 2048^2 tile
// against 1.77 ms at two (round 5's three-per-CU kernel without t2: 1.69-1.81).
#ifndef HRF_W16T_OCC
#define HRF_W16T_OCC 2
#endif
// The screens (hrf_classify_pixels_screen mode 2, hrf_classify_pixels_table): three 16-pixel groups
// per wave (72 B-operand VGPRs instead of 96) fit three workgroups per CU with the runner-up keys
// (165 VGPRs, no spills): 1.76-1.78 ms alone against 1.75 at four groups and two per CU, but
// 866 vs 842 Mpix/s in the bench (three interleaved pairs, profiles/r6_screen_ng3_ab.txt).  The
// fused certificate keeps four groups (64 pixels per wave) at two per CU.
#ifndef HRF_W16T_NG
#define HRF_W16T_NG 3
#endif
#ifndef HRF_W16T_SCREEN_OCC
#define HRF_W16T_SCREEN_OCC 3
#endif

// A library segment the screens can normalise: a finite, non-zero sum of squares nn.  A segment
// holding a NaN or an inf (nn is then NaN or inf; finite f32 values cannot overflow the f64 sum)
// is written to the MFMA tables as an all-zero segment with its zero-segment indicator set, so no
// NaN reaches a screen's argmax.  Its screen term is then 1 against a pixel's all-zero segment
// (restated: 0, the one-zero case) and 0 against any other (restated: a NaN distance, which never
// wins): the screen over-scores such a row and never under-scores it, so the certificate's
// premise -- no other row's restated score above the runner-up bound -- holds, and the exact
// section keeps the raw values for the f64 passes.
__device__ __forceinline__ bool seg_live(double nn) { return nn > 0.0 && nn < __builtin_inf(); }

// refx[r][0..C) = ref / |ref_seg| (0 if the norm is 0), refx[r][C+s] = (norm_s == 0),
// zero padding to KP columns and to Rpad rows.
__global__ void ref_prep_kernel(const float *__restrict__ ref, int32_t R, int32_t C, Bounds bd, int32_t KP,
                                int32_t Rpad, float *__restrict__ refx) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= Rpad) return;
  float *o = refx + r * KP;
  for (int k = 0; k < KP; ++k) o[k] = 0.0f;
  if (r >= R) return;
  const float *x = ref + r * C;
  for (int s = 0; s < bd.nseg; ++s) {
    double nn = 0.0;
    for (int c = bd.b[s]; c < bd.b[s + 1]; ++c) nn += (double)x[c] * (double)x[c];
    const bool live = seg_live(nn);
    const double inv = live ? 1.0 / sqrt(nn) : 0.0;
    for (int c = bd.b[s]; c < bd.b[s + 1]; ++c) o[c] = live ? (float)((double)x[c] * inv) : 0.0f;
    o[C + s] = live ? 0.0f : 1.0f;
  }
}

template <int KS>
__global__ __launch_bounds__(256) void classify_pixels_kernel(const float *__restrict__ stack, int64_t P, int32_t C,
                                                                  Bounds bd, const float *__restrict__ refx,
                                                                  int32_t R, int32_t Rpad,
                                                                  int32_t *__restrict__ best_idx,
                                                                  float *__restrict__ best_dist,
                                                                  float *__restrict__ second) {
  constexpr int KP = 2 * KS;
  constexpr int STRIDE = KP + 2;  // == 2 (mod 4): conflict-free ds_read_b64 over 32 rows
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int64_t pbase = (int64_t)blockIdx.x * 256 + w * 64;

  // ---- stage this wave's two 32-pixel groups, build the B operand in registers ----
  float bx[2][KS];
  float *stg = lds + w * (32 * C);
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int64_t p0 = pbase + g * 32;
    const int64_t np = std::max<int64_t>(0, std::min<int64_t>(32, P - p0));
    const int64_t nel = np * C;
    const float *src = stack + p0 * C;
    for (int64_t e = lane; e < 32 * C; e += 64) stg[e] = e < nel ? src[e] : 0.0f;
    __syncthreads();
    // segment norms of pixel j (f64 accumulation, as the restatement)
    float inv[SMAX];
    float zf[SMAX];
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
      inv[s] = 0.0f;
      zf[s] = 0.0f;
      if (s < bd.nseg) {
        double nn = 0.0;
        for (int c = bd.b[s]; c < bd.b[s + 1]; ++c) {
          const double v = (double)stg[j * C + c];
          nn += v * v;
        }
        inv[s] = nn > 0 ? (float)(1.0 / sqrt(nn)) : 0.0f;
        zf[s] = nn > 0 ? 0.0f : 1.0f;
      }
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = h * KS + s;
      float v = 0.0f;
      if (k < C) {
        float iv = inv[0];
#pragma unroll
        for (int q = 1; q < SMAX; ++q)
          if (q < bd.nseg && k >= bd.b[q]) iv = inv[q];
        v = (float)((double)stg[j * C + k] * (double)iv);
      } else if (k < C + bd.nseg) {
        float z = zf[0];
#pragma unroll
        for (int q = 1; q < SMAX; ++q)
          if (q == k - C) z = zf[q];
        v = z;
      }
      bx[g][s] = v;
    }
    __syncthreads();
  }

  float best[2] = {-__builtin_inff(), -__builtin_inff()};
  float sec[2] = {-__builtin_inff(), -__builtin_inff()};  // runner-up score (any row but the best)
  int bidx[2] = {0, 0};

  // ---- sweep the reference library in LDS chunks ----
  // The next chunk is prefetched into registers while the current one feeds the MFMAs, so
  // the L2 latency of the table hides behind ~25K MFMA cycles per chunk.
  constexpr int PF = (RCH * (KP / 2) + 255) / 256;  // float2 per thread per chunk
  float2 pf[PF];
  auto prefetch = [&](int r0) {
    const float2 *gsrc = reinterpret_cast<const float2 *>(refx + (int64_t)r0 * KP);
#pragma unroll
    for (int q = 0; q < PF; ++q) {
      const int e = tid + q * 256;
      if (e < RCH * (KP / 2)) pf[q] = gsrc[e];
    }
  };
  prefetch(0);
  for (int r0 = 0; r0 < Rpad; r0 += RCH) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PF; ++q) {
      const int e = tid + q * 256;
      if (e < RCH * (KP / 2)) {
        const int rr = e / (KP / 2), cc = e - rr * (KP / 2);
        reinterpret_cast<float2 *>(lds + rr * STRIDE)[cc] = pf[q];
      }
    }
    __syncthreads();
    if (r0 + RCH < Rpad) prefetch(r0 + RCH);
#pragma unroll 1
    for (int rb = 0; rb < RCH; rb += 32) {
      f32x16 acc0 = {0}, acc1 = {0};
      const float *arow = lds + (rb + j) * STRIDE + h * KS;
#pragma unroll
      for (int s = 0; s < KS; s += 2) {
        const float2 a = *reinterpret_cast<const float2 *>(arow + s);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bx[0][s], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bx[1][s], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bx[0][s + 1], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bx[1][s + 1], acc1, 0, 0, 0);
      }
      // rows (references) of this lane: (reg&3) + 8*(reg>>2) + 4*h, increasing in reg
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int r = r0 + rb + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        const bool ok = r < R;
        if (ok) {
          sec[0] = fmaxf(sec[0], fminf(best[0], acc0[reg]));
          sec[1] = fmaxf(sec[1], fminf(best[1], acc1[reg]));
        }
        if (ok && acc0[reg] > best[0]) {
          best[0] = acc0[reg];
          bidx[0] = r;
        }
        if (ok && acc1[reg] > best[1]) {
          best[1] = acc1[reg];
          bidx[1] = r;
        }
      }
    }
  }
  // merge the two lane halves holding the same pixel column
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const float ob = __shfl_xor(best[g], 32, 64);
    const int oi = __shfl_xor(bidx[g], 32, 64);
    sec[g] = fmaxf(fmaxf(sec[g], __shfl_xor(sec[g], 32, 64)), fminf(best[g], ob));
    if (ob > best[g] || (ob == best[g] && oi < bidx[g])) {
      best[g] = ob;
      bidx[g] = oi;
    }
    const int64_t p = pbase + g * 32 + j;
    if (h == 0 && p < P) {
      best_idx[p] = bidx[g];
      best_dist[p] = ((float)bd.nseg - best[g]) / (float)bd.nseg;
      if (second) second[p] = sec[g];
    }
  }
}

// ---- mode 1: split-fp16 MFMA ----------------------------------------------------------------
// Each normalised operand value v (|v| <= 1) is carried as hi = fp16(v) and lo = fp16(v - hi);
// score = sum(hi*hi' + hi*lo' + lo*hi') in one f32 accumulator.  Per product the error is the
// dropped lo*lo' (<= 2^-22) plus lo's fp16 rounding (<= 2^-25 absolute, subnormal spacing),
// so a 100-term score is within ~1e-6 of the exact f32 dot product; the three products are
// v_mfma_f32_32x32x16_f16 at 16x the f32-MFMA rate.
//
// Reference table rows (global AND LDS image): {hi[0..KP), lo[0..KP), 16 B pad} fp16, so the
// row pitch 4*KP+16 is 16 x odd (conflict-free ds_read_b128 over 32 rows) and a 64-row chunk
// is a whole number of 1 KiB LDS-DMA pieces.  Column C+nseg is a validity bias: 0 for real
// rows, -1024 for the padding rows past R, against 1.0 on the pixel side, so padding rows
// never win the argmax and the epilogue needs no bounds test.
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) void glb_void_t;

__global__ void ref_prep_f16_kernel(const float *__restrict__ ref, int32_t R, int32_t C, Bounds bd, int32_t KP,
                                    int32_t Rpad, _Float16 *__restrict__ refh) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= Rpad) return;
  _Float16 *hi = refh + r * (2 * KP + 8);
  _Float16 *lo = hi + KP;
  for (int k = 0; k < 2 * KP + 8; ++k) hi[k] = (_Float16)0.0f;
  hi[C + bd.nseg] = (_Float16)(r < R ? 0.0f : -1024.0f);
  if (r >= R) return;
  const float *x = ref + r * C;
  for (int s = 0; s < bd.nseg; ++s) {
    double nn = 0.0;
    for (int c = bd.b[s]; c < bd.b[s + 1]; ++c) nn += (double)x[c] * (double)x[c];
    const bool live = seg_live(nn);
    const double inv = live ? 1.0 / sqrt(nn) : 0.0;
    for (int c = bd.b[s]; c < bd.b[s + 1]; ++c) {
      const float v = live ? (float)((double)x[c] * inv) : 0.0f;
      const _Float16 h = (_Float16)v;
      hi[c] = h;
      lo[c] = (_Float16)(v - (float)h);
    }
    hi[C + s] = (_Float16)(live ? 0.0f : 1.0f);
  }
}

// Raw spectra of one 32-pixel group: 32*C floats = 8*C float4, at most 16 per lane (C <= 128).
// All loads of both groups are issued before any is consumed, so a wave pays the HBM latency
// once per tile instead of once per element.
constexpr int LDV = 16;
__device__ __forceinline__ void load_group(const float *__restrict__ stack, int64_t P, int32_t C, int64_t p0, int lane,
                                           float4 (&v)[LDV], int npmax = 32) {
  const int64_t np = std::max<int64_t>(0, std::min<int64_t>(npmax, P - p0));
  const int64_t nel = np * C;  // valid floats of this group
  const float *src = stack + p0 * C;
  const int nv = 8 * C;
#pragma unroll
  for (int i = 0; i < LDV; ++i) {
    const int e4 = lane + 64 * i;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e4 < nv) {
      const int64_t e = 4 * (int64_t)e4;
      if (e + 4 <= nel) {
        x = *reinterpret_cast<const float4 *>(src + e);
      } else {
        x.x = e + 0 < nel ? src[e + 0] : 0.f;
        x.y = e + 1 < nel ? src[e + 1] : 0.f;
        x.z = e + 2 < nel ? src[e + 2] : 0.f;
        x.w = e + 3 < nel ? src[e + 3] : 0.f;
      }
    }
    v[i] = x;
  }
}

// Per-workgroup column map for the B operand: segk[k] = the slot of column k in a pixel's
// 24-float multiplier row {1/norm_s (0..7), zero-indicator_s (8..15), bias 1.0 (16), 0 (17)}.
constexpr int MROW = 24;
__device__ __forceinline__ void build_segk(const Bounds &bd, int32_t C, int KP, uint8_t *segk) {
  for (int k = threadIdx.x; k < KP; k += blockDim.x) {
    int v = 0x80 | 17;  // bit 7: not a channel (the value is the multiplier slot itself)
    if (k < C) {
      v = 0;
      for (int t = 1; t < bd.nseg; ++t) v += k >= bd.b[t];
    } else if (k < C + bd.nseg) {
      v = 0x80 | (8 + (k - C));
    } else if (k == C + bd.nseg) {
      v = 0x80 | 16;
    }
    segk[k] = (uint8_t)v;
  }
}

// Stage one loaded group in LDS and build its split-fp16 B operand (lane = pixel j, half h
// holds columns 16s + 8h + q): column k = raw[k] * mult[segk[k]] (raw = 1 past C), i.e. the
// channel scaled by its segment's 1/norm, then the zero-segment indicators, the bias column
// 1.0 and zeros.  The two half-waves of a pixel split each segment's channels for the norm.
template <int KS16>
__device__ __forceinline__ void build_b_f16(const float4 (&v)[LDV], int32_t C, const Bounds &bd, float *stg,
                                            float *mult, const uint8_t *segk, int lane, int j, int h,
                                            h8 (&bh)[KS16], h8 (&bl)[KS16]) {
  const int nv = 8 * C;
#pragma unroll
  for (int i = 0; i < LDV; ++i) {
    const int e4 = lane + 64 * i;
    if (e4 < nv) reinterpret_cast<float4 *>(stg)[e4] = v[i];
  }
  __syncthreads();
  const float *px = stg + j * C;
  float *mj = mult + j * MROW;
#pragma unroll
  for (int s = 0; s < SMAX; ++s) {
    if (s < bd.nseg) {
      double n0 = 0.0, n1 = 0.0;
      const int c1 = bd.b[s + 1];
      int c = bd.b[s] + h;
      for (; c + 2 < c1; c += 4) {
        const double x0 = (double)px[c], x1 = (double)px[c + 2];
        n0 += x0 * x0;
        n1 += x1 * x1;
      }
      if (c < c1) {
        const double x0 = (double)px[c];
        n0 += x0 * x0;
      }
      double nn = n0 + n1;
      nn += __shfl_xor(nn, 32, 64);
      if (h == 0) {
        mj[s] = nn > 0 ? (float)(1.0 / sqrt(nn)) : 0.0f;
        mj[8 + s] = nn > 0 ? 0.0f : 1.0f;
      }
    }
  }
  if (h == 0) {
    mj[16] = 1.0f;
    mj[17] = 0.0f;
  }
  __syncthreads();
  // per-lane bases + immediate offsets; the raw read past C lands in LDS and is discarded
  const float *pc = px + 8 * h;
  const uint8_t *sk = segk + 8 * h;
#pragma unroll
  for (int s = 0; s < KS16; ++s) {
    h8 vh, vl;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      // the channel test comes from the column map (a load), not from k < C, which the
      // compiler would hoist out of the tile loop as 56 live masks
      const int code = sk[16 * s + q];
      const float m = mj[code & 31];
      float x = (code & 0x80) ? m : pc[16 * s + q] * m;
      asm volatile("" : "+v"(x));  // round to f32 first: no fused multiply-to-f16
      const _Float16 hv = (_Float16)x;
      vh[q] = hv;
      vl[q] = (_Float16)(x - (float)hv);
    }
    bh[s] = vh;
    bl[s] = vl;
  }
  __syncthreads();
}

// One workgroup = 4 waves x 64 pixels, held as split-fp16 B operands in VGPRs for the whole
// sweep.  The library streams through two LDS chunk buffers by LDS-DMA
// (global_load_lds_dwordx4, no VGPR staging): chunk c+1 is in flight while chunk c feeds the
// MFMAs, one barrier per chunk.  The argmax is fused (lane = pixel column, 16 rows per tile).
template <int KS16>
__global__ __launch_bounds__(256, 2) void classify_pixels_f16_kernel(const float *__restrict__ stack, int64_t P,
                                                                     int32_t C, Bounds bd,
                                                                     const _Float16 *__restrict__ refh, int32_t R,
                                                                     int32_t Rpad, int32_t *__restrict__ best_idx,
                                                                     float *__restrict__ best_dist,
                                                                     float *__restrict__ second) {
  constexpr int KP = 16 * KS16;
  constexpr int ROWB = 4 * KP + 16;
  constexpr int CHB = RCH * ROWB;
  constexpr int NPC = CHB / 1024;  // LDS-DMA pieces per chunk
  static_assert(CHB % 1024 == 0, "chunk must be whole 1 KiB pieces");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  char *ldsb = reinterpret_cast<char *>(lds);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int64_t pbase = (int64_t)blockIdx.x * 256 + w * 64;

  h8 bh0[KS16], bl0[KS16], bh1[KS16], bl1[KS16];
  // staging aliases the chunk buffers (done before the first DMA): raw rows, multiplier rows,
  // column map
  float *stg = lds + w * (32 * C);
  float *mult = lds + 4 * 32 * C + w * (32 * MROW);
  uint8_t *segk = reinterpret_cast<uint8_t *>(lds + 4 * 32 * (C + MROW));
  build_segk(bd, C, KP, segk);
  {
    float4 v0[LDV], v1[LDV];
    load_group(stack, P, C, pbase, lane, v0);
    load_group(stack, P, C, pbase + 32, lane, v1);
    build_b_f16<KS16>(v0, C, bd, stg, mult, segk, lane, j, h, bh0, bl0);
    build_b_f16<KS16>(v1, C, bd, stg, mult, segk, lane, j, h, bh1, bl1);
  }

  const char *gref = reinterpret_cast<const char *>(refh);
  auto issue = [&](int c) {
    const char *g = gref + (int64_t)c * CHB + lane * 16;
    char *l = ldsb + (c & 1) * CHB;
    for (int q = w; q < NPC; q += 4)
      __builtin_amdgcn_global_load_lds((glb_void_t *)(g + q * 1024), (lds_void_t *)(l + q * 1024), 16, 0, 0);
  };
  issue(0);

  float best0 = -__builtin_inff(), best1 = -__builtin_inff();
  float sec0 = -__builtin_inff(), sec1 = -__builtin_inff();  // runner-up scores
  int bi0 = 0, bi1 = 0;  // wave-uniform part of the row index (4h added at the end)
  // Software-pipelined argmax: the scores of block b are compared while block b+1's MFMAs
  // run (a slice of the 16 registers after each k-step), so the epilogue's VALU fills the MFMA
  // issue gaps instead of following them.  Blocks are still consumed in increasing row order.
  f32x16 pv0, pv1;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) pv0[reg] = pv1[reg] = -__builtin_inff();
  int pr = 0;  // first row of the pending block
  auto epi = [&](int lo, int hi) {
#pragma unroll
    for (int reg = lo; reg < hi; ++reg) {
      const int r = pr + (reg & 3) + 8 * (reg >> 2);
      const float s0 = pv0[reg], s1 = pv1[reg];
      sec0 = fmaxf(sec0, fminf(best0, s0));
      sec1 = fmaxf(sec1, fminf(best1, s1));
      if (s0 > best0) {
        best0 = s0;
        bi0 = r;
      }
      if (s1 > best1) {
        best1 = s1;
        bi1 = r;
      }
    }
  };
  const int nch = Rpad / RCH;
  for (int c = 0; c < nch; ++c) {
    // chunk c landed: this wave's LDS-DMA retired (hipcc does not count global_load_lds for the
    // barrier's wait, so the vmcnt(0) is explicit), then the barrier covers every wave's pieces;
    // everyone is past chunk c-1
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (c + 1 < nch) issue(c + 1);
    const char *buf = ldsb + (c & 1) * CHB;
#pragma unroll
    for (int rb = 0; rb < RCH; rb += 32) {
      f32x16 acc0 = {0}, acc1 = {0};
      const char *row = buf + (rb + j) * ROWB + 16 * h;
#pragma unroll
      for (int s = 0; s < KS16; ++s) {
        const h8 ah = *reinterpret_cast<const h8 *>(row + 32 * s);
        const h8 al = *reinterpret_cast<const h8 *>(row + 2 * KP + 32 * s);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh0[s], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh1[s], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl0[s], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl1[s], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh0[s], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh1[s], acc1, 0, 0, 0);
        epi((16 * s) / KS16, (16 * (s + 1)) / KS16);  // previous block, slice s
      }
      pv0 = acc0;
      pv1 = acc1;
      pr = c * RCH + rb;
    }
  }
  epi(0, 16);  // the last block
  float best[2] = {best0, best1};
  float sec[2] = {sec0, sec1};
  int bidx[2] = {bi0 + 4 * h, bi1 + 4 * h};
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const float ob = __shfl_xor(best[g], 32, 64);
    const int oi = __shfl_xor(bidx[g], 32, 64);
    sec[g] = fmaxf(fmaxf(sec[g], __shfl_xor(sec[g], 32, 64)), fminf(best[g], ob));
    if (ob > best[g] || (ob == best[g] && oi < bidx[g])) {
      best[g] = ob;
      bidx[g] = oi;
    }
    const int64_t p = pbase + g * 32 + j;
    if (h == 0 && p < P) {
      best_idx[p] = bidx[g];
      best_dist[p] = ((float)bd.nseg - best[g]) / (float)bd.nseg;
      if (second) second[p] = sec[g];
    }
  }
}

// ---- mode 2: split-fp16 MFMA on the reference channel layouts ---------------------------------
// The E. coli (95 channels, lasers 405/488/514/561/633: train_reference.py:1401) and
// synthetic-community (63 channels, 488/514/561/633: :1488) layouts as compile-time segment
// maps.  Every B-operand column's segment is then known at compile time, so the operand build
// is straight-line code (a select only where the two lane halves straddle a segment bound)
// with no LDS table lookups, and K = C + 1 (channels + the validity-bias column) instead of
// C + nseg + 1.  The zero-segment indicator terms (+1 for a segment that is zero in both the
// pixel and the reference row) are one extra hi-only k-step, run only by workgroups holding a
// pixel with an all-zero segment (workgroup-uniform branch to a second copy of the sweep): its
// A operand is the row's pad, which holds the row's indicators as fp16 1/0 (exact products, so
// the sum equals adding the integer count after the products); its B operand is the pixel's
// indicators.  95 -> 96 columns: 6 k-steps per 32-row block instead of 7, 19 MFMAs instead of
// 18 in the zero-segment copy.
using hrf_pix::LayEcoli;  // pixtable.hpp
using hrf_pix::LayMulti;

// segment of B-operand column k: 0..NSEG-1 for a channel, -1 for the bias column (k == C),
// -2 for zero padding
template <class L>
__host__ __device__ constexpr int col_seg(int k) {
  if (k > L::C) return -2;
  if (k == L::C) return -1;
  int s = 0;
  for (int t = 1; t < L::NSEG; ++t) s += k >= L::b(t) ? 1 : 0;
  return s;
}
template <class L>
constexpr int lay_ks16() {
  return (L::C + 1 + 15) / 16;
}

// Stage one loaded group in LDS and build its split-fp16 B operand (lane = pixel j, half h
// holds columns 16s + 8h + q).  Segment norms: f32 sums of the lane's own columns plus the
// other half's (one shuffle), 1/sqrt by v_rsq (both within ~1e-7 of the restatement's f64,
// far inside the classifier's 1e-5); a segment is zero when all its values are +-0 (exact,
// from the bit patterns), and a sum that underflows f32 is redone in f64.  zx = the pixel's
// all-zero segments; neg = some value is negative.
template <class L, int KS>
__device__ __forceinline__ void build_b_lay(const float4 (&v)[LDV], float *stg, int lane, int j, int h,
                                            h8 (&bh)[KS], h8 (&bl)[KS], uint32_t &zx, uint32_t &neg) {
  const int nv = 8 * L::C;
#pragma unroll
  for (int i = 0; i < LDV; ++i) {
    const int e4 = lane + 64 * i;
    if (e4 < nv) reinterpret_cast<float4 *>(stg)[e4] = v[i];
  }
  __syncthreads();
  const float *pc = stg + j * L::C + 8 * h;
  float raw[KS][8];
  float nn[L::NSEG];
  uint32_t nzs[L::NSEG];
  uint32_t sgn = 0;
#pragma unroll
  for (int s = 0; s < L::NSEG; ++s) {
    nn[s] = 0.0f;
    nzs[s] = 0u;
  }
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int sa = col_seg<L>(16 * s + q), sb = col_seg<L>(16 * s + 8 + q);
      const float r = pc[16 * s + q];  // past the row end: another pixel's value, masked here
      const float x = h ? (sb >= 0 ? r : 0.0f) : (sa >= 0 ? r : 0.0f);
      raw[s][q] = x;
      const uint32_t xb = __float_as_uint(x);
      sgn |= xb;
      const uint32_t mag = xb << 1;  // non-zero iff |x| != 0
      if (sa == sb) {
        if (sa >= 0) {
          nn[sa >= 0 ? sa : 0] = __builtin_fmaf(x, x, nn[sa >= 0 ? sa : 0]);
          nzs[sa >= 0 ? sa : 0] |= mag;
        }
      } else {
        const float x2 = x * x;
        if (sa >= 0) {
          nn[sa >= 0 ? sa : 0] += h ? 0.0f : x2;
          nzs[sa >= 0 ? sa : 0] |= h ? 0u : mag;
        }
        if (sb >= 0) {
          nn[sb >= 0 ? sb : 0] += h ? x2 : 0.0f;
          nzs[sb >= 0 ? sb : 0] |= h ? mag : 0u;
        }
      }
    }
  neg = sgn >> 31;
  float inv[L::NSEG];
  zx = 0;
#pragma unroll
  for (int s = 0; s < L::NSEG; ++s) {
    const float t = nn[s] + __shfl_xor(nn[s], 32, 64);
    const uint32_t nz = nzs[s] | __shfl_xor(nzs[s], 32, 64);
    inv[s] = nz ? rsqrtf(t) : 0.0f;
    zx |= (nz ? 0u : 1u) << s;
    if (nz && !(t >= 1e-30f)) {  // f32 underflow (|x| < ~1e-19 throughout): redo in f64
      double td = 0.0;
#pragma unroll
      for (int ss = 0; ss < KS; ++ss)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int sa = col_seg<L>(16 * ss + q), sb = col_seg<L>(16 * ss + 8 + q);
          const double x = (double)raw[ss][q];
          if ((h ? sb : sa) == s) td += x * x;
        }
      td += __shfl_xor(td, 32, 64);
      inv[s] = (float)(1.0 / sqrt(td));
    }
  }
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    h8 vh, vl;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int sa = col_seg<L>(16 * s + q), sb = col_seg<L>(16 * s + 8 + q);
      const float ma = sa >= 0 ? inv[sa >= 0 ? sa : 0] : (sa == -1 ? 1.0f : 0.0f);
      const float mb = sb >= 0 ? inv[sb >= 0 ? sb : 0] : (sb == -1 ? 1.0f : 0.0f);
      float x;
      if (sa >= 0 && sb >= 0)
        x = raw[s][q] * (h ? mb : ma);
      else
        x = h ? (sb >= 0 ? raw[s][q] * mb : mb) : (sa >= 0 ? raw[s][q] * ma : ma);
      asm volatile("" : "+v"(x));  // round to f32 first: no fused multiply-to-f16
      const _Float16 hv = (_Float16)x;
      vh[q] = hv;
      vl[q] = (_Float16)(x - (float)hv);
    }
    bh[s] = vh;
    bl[s] = vl;
  }
  __syncthreads();
}

// The library sweep of one workgroup (see classify_pixels_f16_kernel).  ZS adds the
// zero-segment indicator terms popcount(zx & zr) to every score, as a seventh MFMA per pixel
// group and block: A = the row's indicator fp16s in its pad (every lane reads its row's pad;
// the h = 1 half meets B = 0), B = the pixel's indicators (h = 0 lanes, k < NSEG).  KEYED (all scores >= 0:
// no negative value in the workgroup's pixels or the library) runs the argmax on integer
// keys: score bits with the low 4 mantissa bits replaced by 15 - register (so the max also
// names the register, lower rows winning ties), a max tree per block and one compare per
// block -- about half the VALU of a compare-and-select per score.  The 4 dropped bits are
// <= 2^-19 relative (< 1e-5 of a distance): the keyed score IS the truncated one (it is the
// distance reported), and its argmax keeps the reference's tie rule on it -- within a block the
// code makes the lowest row win equal scores, across blocks (and chunks) only a strictly greater
// score replaces the running best, so equal scores anywhere in the library go to the lowest r.
// Runner-up tracking (the refine's certificate, hrf_classify_pixels_refine): the second-largest key
// of {a >= b} and k is med3(a, b, k) (v_med3_i32); a key's score bits with the 4 position bits set
// bound every untruncated score that truncates to them (negative keys -- padding rows only -- keep
// their truncated value, the larger one)
__device__ __forceinline__ int med3i(int a, int b, int c) { return max(min(a, b), min(max(a, b), c)); }
__device__ __forceinline__ float key_score_hi(int k) {
  return __int_as_float(k >= 0 ? ((k & -16) | 15) : (k & -16));
}
// the same bound from a truncated score (keyed sweeps) or the exact one (compare-select sweeps)
__device__ __forceinline__ float score_hi(float s, bool keyed) { return keyed ? key_score_hi(__float_as_int(s)) : s; }

template <int KS16, int ROWB, int NW, int NSEG, bool ZS, bool KEYED>
__device__ __forceinline__ void lay_sweep(const char *__restrict__ gref, char *ldsb, int nch, int lane, int w, int h,
                                          const h8 (&bh0)[KS16], const h8 (&bl0)[KS16], const h8 (&bh1)[KS16],
                                          const h8 (&bl1)[KS16], uint32_t zx0, uint32_t zx1, float &best0,
                                          float &best1, int &bi0, int &bi1, float &sec0, float &sec1) {
  constexpr int KP = 16 * KS16;
  constexpr int CHB = RCH * ROWB;
  constexpr int NPC = CHB / 1024;
  const int j = lane & 31;
  auto issue = [&](int c) {
    const char *g = gref + (int64_t)c * CHB + lane * 16;
    char *l = ldsb + (c & 1) * CHB;
    for (int q = w; q < NPC; q += NW)
      __builtin_amdgcn_global_load_lds((glb_void_t *)(g + q * 1024), (lds_void_t *)(l + q * 1024), 16, 0, 0);
  };
  issue(0);
  f32x16 pv0, pv1;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) pv0[reg] = pv1[reg] = -__builtin_inff();
  int pr = 0;  // first row of the pending block
  h8 bz0, bz1;  // ZS: the pixels' zero-segment indicators (B operand of the extra k-step)
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    bz0[q] = (_Float16)((h == 0 && q < NSEG && ((zx0 >> q) & 1u)) ? 1.0f : 0.0f);
    bz1[q] = (_Float16)((h == 0 && q < NSEG && ((zx1 >> q) & 1u)) ? 1.0f : 0.0f);
  }
  // KEYED: key = the best so far (a later block's best replaces it on a strictly greater score only);
  // t1 / t2 = the largest / second-largest keys seen (t1 doubles as the block's best, see sweep_w16)
  int key0 = INT32_MIN, key1 = INT32_MIN;
  int t10 = INT32_MIN, t11 = INT32_MIN, t20 = INT32_MIN, t21 = INT32_MIN;
  auto epi = [&](int lo, int hi) {
#pragma unroll
    for (int reg = lo; reg < hi; ++reg) {
      const int r = pr + (reg & 3) + 8 * (reg >> 2);
      const float s0 = pv0[reg], s1 = pv1[reg];
      if (KEYED) {
        const int q0 = (__float_as_int(s0) & -16) | (15 - reg), q1 = (__float_as_int(s1) & -16) | (15 - reg);
        t20 = med3i(t10, t20, q0);
        t21 = med3i(t11, t21, q1);
        t10 = max(t10, q0);
        t11 = max(t11, q1);
      } else {
        sec0 = fmaxf(sec0, fminf(best0, s0));
        sec1 = fmaxf(sec1, fminf(best1, s1));
        if (s0 > best0) {
          best0 = s0;
          bi0 = r;
        }
        if (s1 > best1) {
          best1 = s1;
          bi1 = r;
        }
      }
    }
    if (KEYED && hi == 16) {  // the pending block is complete: a later block wins on a greater score only
      if ((t10 >> 4) > (key0 >> 4)) {
        key0 = t10;
        bi0 = pr;
      }
      if ((t11 >> 4) > (key1 >> 4)) {
        key1 = t11;
        bi1 = pr;
      }
    }
  };
  for (int c = 0; c < nch; ++c) {
    // chunk c landed: this wave's LDS-DMA retired (hipcc does not count global_load_lds for the
    // barrier's wait, so the vmcnt(0) is explicit), then the barrier covers every wave's pieces;
    // everyone is past chunk c-1
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (c + 1 < nch) issue(c + 1);
    const char *buf = ldsb + (c & 1) * CHB;
#pragma unroll
    for (int rb = 0; rb < RCH; rb += 32) {
      f32x16 acc0 = {0}, acc1 = {0};
      const char *row = buf + (rb + j) * ROWB + 16 * h;
      h8 az;
      if (ZS) az = *reinterpret_cast<const h8 *>(buf + (rb + j) * ROWB + 4 * KP);
      // the cross products (hi * lo', lo * hi') first, then hi * hi': the small products meet an
      // accumulator of ~2^-10 of a score (screen_eps counts KS16 + 1 full-magnitude MFMAs)
#pragma unroll
      for (int s = 0; s < KS16; ++s) {
        const h8 ah = *reinterpret_cast<const h8 *>(row + 32 * s);
        const h8 al = *reinterpret_cast<const h8 *>(row + 2 * KP + 32 * s);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl0[s], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl1[s], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh0[s], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh1[s], acc1, 0, 0, 0);
        epi((16 * s) / KS16, (16 * (s + 1)) / KS16);  // previous block, slice s
      }
#pragma unroll
      for (int s = 0; s < KS16; ++s) {
        const h8 ah = *reinterpret_cast<const h8 *>(row + 32 * s);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh0[s], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh1[s], acc1, 0, 0, 0);
      }
      if (ZS) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(az, bz0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(az, bz1, acc1, 0, 0, 0);
      }
      pv0 = acc0;
      pv1 = acc1;
      pr = c * RCH + rb;
    }
  }
  epi(0, 16);  // the last block
  if (KEYED) {
    const int g0 = 15 - (key0 & 15), g1 = 15 - (key1 & 15);
    bi0 += (g0 & 3) + 8 * (g0 >> 2);
    bi1 += (g1 & 3) + 8 * (g1 >> 2);
    best0 = __int_as_float(key0 & -16);
    best1 = __int_as_float(key1 & -16);
    sec0 = key_score_hi(t20);
    sec1 = key_score_hi(t21);
  }
}

template <class L, int NW>
__global__ __launch_bounds__(64 * NW, 8 / NW) void classify_pixels_lay_kernel(const float *__restrict__ stack, int64_t P,
                                                                     const _Float16 *__restrict__ refh, int32_t R,
                                                                     int32_t Rpad, int32_t *__restrict__ best_idx,
                                                                     float *__restrict__ best_dist,
                                                                     float *__restrict__ second) {
  constexpr int KS16 = lay_ks16<L>();
  constexpr int KP = 16 * KS16;
  constexpr int ROWB = 4 * KP + L::PADB;
  static_assert((RCH * ROWB) % 1024 == 0, "chunk must be whole 1 KiB pieces");
  static_assert(L::NSEG <= 6, "the pad holds 6 indicators (fp16 6-7 of row 0: the negative flag)");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int64_t pbase = (int64_t)blockIdx.x * (64 * NW) + w * 64;

  h8 bh0[KS16], bl0[KS16], bh1[KS16], bl1[KS16];
  uint32_t zx0 = 0, zx1 = 0, ng0 = 0, ng1 = 0;
  float *stg = lds + w * (32 * L::C);  // staging aliases the chunk buffers (before the first DMA)
  {
    float4 v0[LDV], v1[LDV];
    load_group(stack, P, L::C, pbase, lane, v0);
    load_group(stack, P, L::C, pbase + 32, lane, v1);
    build_b_lay<L, KS16>(v0, stg, lane, j, h, bh0, bl0, zx0, ng0);
    build_b_lay<L, KS16>(v1, stg, lane, j, h, bh1, bl1, zx1, ng1);
  }
  // the library's "has a negative value" flag sits in row 0's pad (ref_negflag_kernel)
  const uint32_t libneg = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(refh) + 4 * KP + 12);
  float best0 = -__builtin_inff(), best1 = -__builtin_inff();
  float sec0 = -__builtin_inff(), sec1 = -__builtin_inff();
  int bi0 = 0, bi1 = 0;  // wave-uniform part of the row index (4h added at the end)
  const char *gref = reinterpret_cast<const char *>(refh);
  char *ldsb = reinterpret_cast<char *>(lds);
  const int nch = Rpad / RCH;
  // every wave of the workgroup takes the same branch (the chunk barriers are shared)
  const bool zs = __syncthreads_or((zx0 | zx1) != 0);
  const bool keyed = !libneg && !__syncthreads_or((ng0 | ng1) != 0);
#define HRF_SWEEP(Z, K) \
  lay_sweep<KS16, ROWB, NW, L::NSEG, Z, K>(gref, ldsb, nch, lane, w, h, bh0, bl0, bh1, bl1, zx0, zx1, best0, best1, bi0, \
                                           bi1, sec0, sec1)
  if (keyed) {
    if (zs) HRF_SWEEP(true, true);
    else HRF_SWEEP(false, true);
  } else {
    if (zs) HRF_SWEEP(true, false);
    else HRF_SWEEP(false, false);
  }
#undef HRF_SWEEP
  float best[2] = {best0, best1};
  float sec[2] = {sec0, sec1};
  int bidx[2] = {bi0 + 4 * h, bi1 + 4 * h};
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const float ob = __shfl_xor(best[g], 32, 64);
    const int oi = __shfl_xor(bidx[g], 32, 64);
    sec[g] = fmaxf(fmaxf(sec[g], __shfl_xor(sec[g], 32, 64)), fminf(score_hi(best[g], keyed), score_hi(ob, keyed)));
    if (ob > best[g] || (ob == best[g] && oi < bidx[g])) {
      best[g] = ob;
      bidx[g] = oi;
    }
    const int64_t p = pbase + g * 32 + j;
    if (h == 0 && p < P) {
      best_idx[p] = bidx[g];
      best_dist[p] = ((float)L::NSEG - best[g]) / (float)L::NSEG;
      if (second) second[p] = sec[g];
    }
  }
}

// ---- the same sweep on v_mfma_f32_16x16x32_f16 (E. coli layout) -------------------------------
// Same table, same split-fp16 products, same argmax rules; the MFMA shape differs: A = 16
// library rows x 32 columns (lane: row lane & 15, columns 32t + 8Q..+7, Q = lane >> 4), B = 32
// columns x 16 pixels (lane: pixel lane & 15, the same columns), C = 16 x 16 (lane: pixel lane &
// 15, rows 4Q..4Q+3).  A wave holds four 16-pixel groups.  At equal cycles per flop, this
// shape holds a higher clock than 32x32x16 under load (MI355X_MICROARCH.md, matrix-core DVFS).
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- round 3: the 16x16x32 sweep with a lane-per-pixel prologue and per-chunk argmax keys ----
// Same table, products, scores and tie rules as the 32x32x16 form; what changes against round 2's
// first 16x16x32 kernel (lay16, removed in round 5 after losing every A/B) is the instruction
// count around the MFMAs (lay16 issued ~2.3 VALU per MFMA over its life, which with two waves per
// SIMD left the matrix pipe idle ~40 % of the time):
//  * prologue: in the B-operand layout a lane's columns 32t + 8Q + q belong to a segment that
//    depends on the lane quarter Q, a runtime value, so lay16's operand build selected among all
//    NSEG segments for every value (~830 v_cndmask per wave).  Here the segment norms are taken by
//    one lane per staged pixel walking its C channels -- every channel's segment a compile-time
//    constant -- and the pixel is normalised in place in LDS; the B-operand lanes then only read
//    and split into hi/lo fp16;
//  * sweep: the argmax folds each block's 16 keys into a per-chunk key with v_max3 and compares
//    with the running best once per chunk (the key's low 4 bits name the row within the chunk:
//    4 * block + register, blocks of 16 rows, CR <= 64), instead of a compare-and-select per
//    block;
//  * NW waves per workgroup share CR-row chunks through NBUF LDS buffers (template parameters;
//    the defaults are the measured best, DESIGN.md "Per-pixel classifier").
using hrf_pix::lay_seg;

// One staged 32-pixel group (row-major, stride C floats, at stg): lanes 0..31 (pixel = lane)
// take the segment norms, flag all-zero segments (zx) and negative values (neg), and rewrite
// the pixel normalised.  Same arithmetic as build_b_lay (f32 sums, v_rsq, f64 redo when a sum
// underflows f32), summed in channel order.
template <class L>
__device__ __forceinline__ void norm_pixels_w16(float *stg, int lane, uint32_t &zx, uint32_t &neg) {
  zx = 0;
  neg = 0;
  if (lane < 32) {
    float *px = stg + lane * L::C;
    float nn[L::NSEG];
#pragma unroll
    for (int s = 0; s < L::NSEG; ++s) nn[s] = 0.0f;
    uint32_t sg = 0;
#pragma unroll
    for (int c = 0; c < L::C; ++c) {
      const float x = px[c];
      nn[lay_seg<L>(c)] = __builtin_fmaf(x, x, nn[lay_seg<L>(c)]);
      sg |= __float_as_uint(x);
    }
    neg = sg >> 31;
    float inv[L::NSEG];
#pragma unroll
    for (int s = 0; s < L::NSEG; ++s) {
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
    for (int c = 0; c < L::C; ++c) px[c] = px[c] * inv[lay_seg<L>(c)];
  }
}

// B operand of 16-pixel sub-group g of the normalised staged group: lane pixel (lane & 15) + 16g,
// columns 32t + 8Q + q; column C is the validity-bias column (1), columns past it 0.
template <class L, int KT>
__device__ __forceinline__ void split_b_w16(const float *stg, int lane, int g, h8 (&bh)[KT], h8 (&bl)[KT]) {
  const int jj = (lane & 15) + 16 * g, Q = lane >> 4;
  const float *pc = stg + jj * L::C + 8 * Q;
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    h8 vh, vl;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      float x = pc[32 * t + q];  // past the row end: another pixel's value, replaced below
      if (32 * t + 24 + q >= L::C) {  // only the last columns depend on Q
        const int k = 32 * t + 8 * Q + q;
        x = k < L::C ? x : (k == L::C ? 1.0f : 0.0f);
      }
      const _Float16 hv = (_Float16)x;
      vh[q] = hv;
      vl[q] = (_Float16)(x - (float)hv);
    }
    bh[t] = vh;
    bl[t] = vl;
  }
}

template <int KT, int ROWB, int NW, int NSEG, bool ZS, bool KEYED, int NBUF, int CR, bool PIPE, int NG = 4>
__device__ __forceinline__ void sweep_w16(const char *__restrict__ gref, char *ldsb, int nch, int lane, int w,
                                          const h8 (&bh)[NG][KT], const h8 (&bl)[NG][KT], const uint32_t zxp,
                                          float (&best)[NG], int (&bi)[NG], float (&sec)[NG]) {
  static_assert(NG >= 1 && NG <= 4, "16-pixel groups per wave: 8 bits of zxp / bic each");
  constexpr int KP = 32 * KT;
  constexpr int CHB = CR * ROWB;
  constexpr int NPC = (CHB + 1023) / 1024;  // 1 KiB LDS-DMA pieces per chunk (the last may be partial)
  constexpr int NB = CR / 16;               // 16-row blocks per chunk
  static_assert(CR % 16 == 0 && NB <= 4, "chunk keys hold 4 * block + register in 4 bits");
  const int rl = lane & 15, Q = lane >> 4;
  auto issue = [&](int c) {
    const char *g = gref + (int64_t)c * CHB + lane * 16;
    char *l = ldsb + (c % NBUF) * CHB;
    for (int q = w; q < NPC; q += NW)
      if (CHB % 1024 == 0 || q * 1024 + lane * 16 < CHB)
        __builtin_amdgcn_global_load_lds((glb_void_t *)(g + q * 1024), (lds_void_t *)(l + q * 1024), 16, 0, 0);
  };
  // pieces this wave issues per chunk (the waitcnt below leaves chunk c + 1's outstanding)
  const int mine = (NPC - w + NW - 1) / NW;
  constexpr int MINE_LO = NPC / NW;
  issue(0);
  if (NBUF >= 3 && nch > 1) issue(1);
  f32x4 pv[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int i = 0; i < 4; ++i) pv[g][i] = -__builtin_inff();
  int pr = 0;  // first row of the pending block
  // ZS: the pixels' indicator B operand (fp16 1.0 = 0x3c00 in slot q < NSEG of quarter 0 where
  // segment q is all zero), rebuilt per use from zxp (group g's all-zero segments in bits 8g..8g+7)
  // instead of held in 16 VGPRs
  auto bz_of = [&](int g) -> h8 {
    const uint32_t m = Q == 0 ? ((zxp >> (8 * g)) & ((1u << NSEG) - 1u)) : 0u;
    uint32_t d[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = (((m >> (2 * i)) & 1u) * 0x3c00u) | (((m >> (2 * i + 1)) & 1u) * 0x3c000000u);
    return __builtin_bit_cast(h8, d);
  };
  // keyed: key = the running best (replaced by a chunk's best only on a strictly greater score),
  // t1 / t2 = the largest and second-largest keys seen (t1 also serves as the chunk's best: a key
  // from an earlier chunk that was not adopted has key's score)
  int key[NG], t1[NG], t2[NG];
  uint32_t bic = 0;  // keyed: the chunk of each group's key, 8 bits per group
#pragma unroll
  for (int g = 0; g < NG; ++g) key[g] = t1[g] = t2[g] = INT32_MIN;
  // fold the pending block into the chunk keys, groups [g0, g1); after the chunk's last block,
  // the chunk key against the running best (strictly greater score, the position code left out:
  // earlier chunks win ties, so equal scores keep the lowest row across the whole library)
  auto epi = [&](int g0, int g1) {
    const int pb = (pr / 16) % NB;
#pragma unroll
    for (int g = g0; g < g1; ++g) {
      if (KEYED) {
        const int base = 15 - 4 * pb;
        const int k0 = (__float_as_int(pv[g][0]) & -16) | (base - 0);
        const int k1 = (__float_as_int(pv[g][1]) & -16) | (base - 1);
        const int k2 = (__float_as_int(pv[g][2]) & -16) | (base - 2);
        const int k3 = (__float_as_int(pv[g][3]) & -16) | (base - 3);
        t2[g] = med3i(t1[g], t2[g], k0);
        t1[g] = max(t1[g], k0);
        t2[g] = med3i(t1[g], t2[g], k1);
        t1[g] = max(t1[g], k1);
        t2[g] = med3i(t1[g], t2[g], k2);
        t1[g] = max(t1[g], k2);
        t2[g] = med3i(t1[g], t2[g], k3);
        t1[g] = max(t1[g], k3);
      } else {
        // row by row, the runner-up before the best: min(best, s) is the loser of each compare, so
        // the runner-up also sees two rows of this lane's own four (rows 4Q + i of the block).
        // Taking the four runner-up updates first lost exactly those: a near-duplicate pair in
        // adjacent rows was then certified on the first of the two.
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          sec[g] = fmaxf(sec[g], fminf(best[g], pv[g][i]));
          if (pv[g][i] > best[g]) {
            best[g] = pv[g][i];
            bi[g] = pr + i;
          }
        }
      }
    }
    if (KEYED && g1 == NG && pb == NB - 1) {
      const uint32_t cc = (uint32_t)(pr / CR);
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        if ((t1[g] >> 4) > (key[g] >> 4)) {  // t1 is then this chunk's
          key[g] = t1[g];
          bic = (bic & ~(0xffu << (8 * g))) | (cc << (8 * g));
        }
      }
    }
  };
  for (int c = 0; c < nch; ++c) {
    if (NBUF == 2 || c + 1 >= nch) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (mine > MINE_LO) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(MINE_LO + 1) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(MINE_LO) : "memory");
    if (NW > 1) __syncthreads();  // every wave's pieces of c landed; everyone is past chunk c - 1
    if (c + NBUF - 1 < nch) issue(c + NBUF - 1);
    const char *buf = ldsb + (c % NBUF) * CHB;
#pragma unroll
    for (int rb = 0; rb < CR; rb += 16) {
      f32x4 acc[NG];
#pragma unroll
      for (int g = 0; g < NG; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
      const char *row = buf + (rb + rl) * ROWB + 16 * Q;
      h8 az;
      if (ZS) az = *reinterpret_cast<const h8 *>(buf + (rb + rl) * ROWB + 4 * KP);
      // the cross products (hi * lo', lo * hi', each ~2^-11 of a score) first, then the hi * hi'
      // products: the accumulator the small products meet stays ~2^-10 of a score, so only KT
      // (+ the indicator step) MFMAs per score round at the score's magnitude (screen_eps)
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        const h8 ah = *reinterpret_cast<const h8 *>(row + 64 * t);
        const h8 al = *reinterpret_cast<const h8 *>(row + 2 * KP + 64 * t);
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[g][t], acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[g][t], acc[g], 0, 0, 0);
        if (PIPE) epi((NG * t) / KT, (NG * (t + 1)) / KT);  // previous block, slice t
      }
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        const h8 ah = *reinterpret_cast<const h8 *>(row + 64 * t);
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[g][t], acc[g], 0, 0, 0);
      }
      if (ZS) {
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(az, bz_of(g), acc[g], 0, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) pv[g] = acc[g];
      pr = c * CR + rb;
      if (!PIPE) epi(0, NG);  // this block at once (the other waves on the SIMD cover the MFMA latency)
    }
  }
  if (PIPE) epi(0, NG);  // the last block (the end of the last chunk: finalises its key)
  if (KEYED) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int code = 15 - (key[g] & 15);
      bi[g] = CR * (int)((bic >> (8 * g)) & 0xffu) + 16 * (code >> 2) + (code & 3);
      best[g] = __int_as_float(key[g] & -16);
      sec[g] = key_score_hi(t2[g]);
    }
  }
}

// The workgroup's variant of sweep_w16, in a kernel that holds zs (some pixel has an all-zero segment)
// and keyed (no pixel value and no library value is negative), both workgroup-uniform since the
// chunk barriers are shared.  A macro and not a function: the optimiser simplifies a callee on its
// own before inlining it, and the sweeps came out as different device code behind a forceinline
// dispatcher (profiles/classify_split_kernel_resources.txt).
#define HRF_SWEEP_W16_ANY()                                                                                        \
  do {                                                                                                             \
    if (keyed) {                                                                                                   \
      if (zs) HRF_SWEEP_W16(true, true);                                                                           \
      else HRF_SWEEP_W16(false, true);                                                                             \
    } else {                                                                                                       \
      if (zs) HRF_SWEEP_W16(true, false);                                                                          \
      else HRF_SWEEP_W16(false, false);                                                                            \
    }                                                                                                              \
  } while (0)
#define HRF_SWEEP_W16(Z, K) \
  sweep_w16<KT, ROWB, NW, L::NSEG, Z, K, NBUF, CR, (OCC < 3), NG>(gref, ldsb, nch, lane, w, bh, bl, zxp, best, bi, sec)

// The epilogue of a 16-pixel group: the four lane quarters hold rows 4Q..4Q+3 of every block for the
// same pixel column; merge their best scores b (ties to the lower row idx) and runner-up bounds sc.
// Every quarter ends with the merged result.
__device__ __forceinline__ void merge_quarters_w16(float &b, int &idx, float &sc, bool keyed) {
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const float ob = __shfl_xor(b, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    sc = fmaxf(fmaxf(sc, __shfl_xor(sc, o, 64)), fminf(score_hi(b, keyed), score_hi(ob, keyed)));
    if (ob > b || (ob == b && oi < idx)) {
      b = ob;
      idx = oi;
    }
  }
}

template <class L, int NW, int NBUF, int CR, int OCC, int NG = 4>
__global__ __launch_bounds__(64 * NW, OCC) void classify_pixels_w16_kernel(const float *__restrict__ stack,
                                                                     int64_t P, const _Float16 *__restrict__ refh,
                                                                     int32_t R, int32_t Rpad,
                                                                     int32_t *__restrict__ best_idx,
                                                                     float *__restrict__ best_dist,
                                                                     float *__restrict__ second) {
  constexpr int KT = (L::C + 1 + 31) / 32;
  constexpr int KP = 32 * KT;
  constexpr int ROWB = 4 * KP + L::PADB;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  static_assert(NG == 3 || NG == 4, "a wave holds 3 or 4 16-pixel groups");
  const int64_t pbase = (int64_t)blockIdx.x * (16 * NG * NW) + w * (16 * NG);
  h8 bh[NG][KT], bl[NG][KT];
  uint32_t zxp = 0, ng = 0;  // all-zero segments of the NG 16-pixel groups, 8 bits each
  float *stg = lds + w * (32 * L::C);  // staging aliases the chunk buffers (before the first DMA)
  {
    // both halves' loads in flight at once where the registers allow (two waves per SIMD);
    // at three, the second half is loaded after the first is staged
    constexpr int NV = OCC < 3 ? 2 : 1;
    float4 v[NV][LDV];
    // (NG = 3: the second half is one 16-pixel group; the rest of its staging reads as zero)
    load_group(stack, P, L::C, pbase, lane, v[0]);
    if (NV == 2) load_group(stack, P, L::C, pbase + 32, lane, v[NV - 1], 16 * (NG - 2));
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if (NV == 1 && half == 1) load_group(stack, P, L::C, pbase + 32, lane, v[0], 16 * (NG - 2));
#pragma unroll
      for (int i = 0; i < LDV; ++i) {
        const int e4 = lane + 64 * i;
        if (e4 < 8 * L::C) reinterpret_cast<float4 *>(stg)[e4] = v[NV == 2 ? half : 0][i];
      }
      __syncthreads();
      uint32_t zxh, ngp;
      norm_pixels_w16<L>(stg, lane, zxh, ngp);
      ng |= ngp;
      __syncthreads();
      split_b_w16<L, KT>(stg, lane, 0, bh[2 * half], bl[2 * half]);
      if (2 * half + 1 < NG) split_b_w16<L, KT>(stg, lane, 1, bh[(2 * half + 1) % NG], bl[(2 * half + 1) % NG]);
      zxp |= (uint32_t)__shfl(zxh, lane & 15, 64) << (16 * half);
      if (2 * half + 1 < NG) zxp |= (uint32_t)__shfl(zxh, 16 + (lane & 15), 64) << (16 * half + 8);
      __syncthreads();
    }
  }
  const uint32_t libneg = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(refh) + 4 * KP + 12);
  float best[NG], sec[NG];
  int bi[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    best[g] = sec[g] = -__builtin_inff();
    bi[g] = 0;
  }
  const char *gref = reinterpret_cast<const char *>(refh);
  char *ldsb = reinterpret_cast<char *>(lds);
  const int nch = Rpad / CR;
  const bool zs = __syncthreads_or(zxp != 0);
  const bool keyed = !libneg && !__syncthreads_or(ng != 0);
  HRF_SWEEP_W16_ANY();
  const int Q = lane >> 4;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    float b = best[g], sc = sec[g];
    int idx = bi[g] + 4 * Q;
    merge_quarters_w16(b, idx, sc, keyed);
    const int64_t p = pbase + 16 * g + (lane & 15);
    if (Q == 0 && p < P) {
      best_idx[p] = idx;
      best_dist[p] = ((float)L::NSEG - b) / (float)L::NSEG;
      if (second) second[p] = sc;
    }
  }
}

// ---- the B operands from a pixel table (pixtable.hpp) ------------------------------------------
// Standalone producer: 64 pixels per workgroup staged through LDS (coalesced float4 loads).
template <class L>
__global__ __launch_bounds__(256) void pixtable_prep_kernel(const float *__restrict__ stack, int64_t P,
                                                            uint4 *__restrict__ table, uint8_t *__restrict__ flags) {
  __shared__ __attribute__((aligned(16))) float tile[64 * L::C];
  const int64_t p0 = (int64_t)blockIdx.x * 64;
  const int np = (int)min((int64_t)64, P - p0);
  const int nel = np * L::C;
  const float *src = stack + p0 * L::C;
  for (int e = threadIdx.x; e < (nel >> 2); e += 256)
    reinterpret_cast<float4 *>(tile)[e] = reinterpret_cast<const float4 *>(src)[e];
  for (int e = ((nel >> 2) << 2) + threadIdx.x; e < nel; e += 256) tile[e] = src[e];
  __syncthreads();
  hrf_pix::prep_tile<L>(tile, nullptr, np, p0, table, flags);
}

// classify_pixels_w16_kernel with the prologue replaced by direct loads of the prepared operands.
// FUSE (round 6): the f64 refine follows the sweep in the same workgroup (refine_pixels on the
// freed chunk buffers, each wave its four 16-pixel groups), so its loads and f64 work overlap the
// other resident workgroup's MFMA sweep, and the screen's rows and bounds never leave registers.
template <class L, int NW, int NBUF, int CR, int OCC, bool FUSE, int NG = 4>
__global__ __launch_bounds__(64 * NW, OCC) void classify_pixels_w16t_kernel(const uint4 *__restrict__ table,
                                                                      const uint8_t *__restrict__ flags, int64_t P,
                                                                      const _Float16 *__restrict__ refh, int32_t R,
                                                                      int32_t Rpad, int32_t *__restrict__ best_idx,
                                                                      float *__restrict__ best_dist,
                                                                      float *__restrict__ second, RefineArgs A) {
  constexpr int KT = (L::C + 1 + 31) / 32;
  constexpr int KP = 32 * KT;
  constexpr int ROWB = 4 * KP + L::PADB;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  static_assert(!FUSE || NG == 4, "the fused refine takes 64 pixels per wave");
  const int64_t pbase = (int64_t)blockIdx.x * (16 * NG * NW) + w * (16 * NG);
  h8 bh[NG][KT], bl[NG][KT];
  uint32_t zxp = 0, ng = 0;  // all-zero segments of the NG 16-pixel groups, 8 bits each
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int64_t g16 = pbase / 16 + g;
    const uint4 *e = table + g16 * (int64_t)(KT * 128) + lane;
    // (NG < 4: the table holds whole 256-pixel blocks, a 16 NG NW-pixel workgroup can pass them)
    const bool gv = NG == 4 || 16 * g16 < P;
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      const uint4 hv = gv ? e[t * 128] : uint4{0, 0, 0, 0}, lv = gv ? e[t * 128 + 64] : uint4{0, 0, 0, 0};
      bh[g][t] = *reinterpret_cast<const h8 *>(&hv);
      bl[g][t] = *reinterpret_cast<const h8 *>(&lv);
    }
    const int64_t p = pbase + 16 * g + (lane & 15);
    const uint32_t f = p < P ? flags[p] : 0x1fu;
    zxp |= (f & 0x1fu) << (8 * g);
    ng |= f >> 7;
  }
  const uint32_t libneg = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(refh) + 4 * KP + 12);
  float best[NG], sec[NG];
  int bi[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    best[g] = sec[g] = -__builtin_inff();
    bi[g] = 0;
  }
  const char *gref = reinterpret_cast<const char *>(refh);
  char *ldsb = reinterpret_cast<char *>(lds);
  const int nch = Rpad / CR;
  const bool zs = __syncthreads_or(zxp != 0);
  const bool keyed = !libneg && !__syncthreads_or(ng != 0);
  HRF_SWEEP_W16_ANY();
  const int Q = lane >> 4;
  int b1g[NG];
  float s2g[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    float b = best[g], sc = sec[g];
    int idx = bi[g] + 4 * Q;
    merge_quarters_w16(b, idx, sc, keyed);
    b1g[g] = idx;  // every quarter lane holds pixel (lane & 15) + 16 g's merged result
    s2g[g] = sc;
    const int64_t p = pbase + 16 * g + (lane & 15);
    if (!FUSE && Q == 0 && p < P) {
      best_idx[p] = idx;
      best_dist[p] = ((float)L::NSEG - b) / (float)L::NSEG;
      if (second) second[p] = sc;
    }
  }
  if constexpr (FUSE) {
    __syncthreads();  // every wave is done with the chunk buffers: they become the refine's slices
    constexpr int64_t SL = (refine_slice_bytes() + 15) / 16 * 16;
    char *slice = ldsb + w * SL;
    // lane l holds pixel pbase + l's merged result in quarter Q = l >> 4's slot
    const int b1 = Q == 0 ? b1g[0] : Q == 1 ? b1g[1 % NG] : Q == 2 ? b1g[2 % NG] : b1g[3 % NG];
    const float s2 = Q == 0 ? s2g[0] : Q == 1 ? s2g[1 % NG] : Q == 2 ? s2g[2 % NG] : s2g[3 % NG];
    refine_pixels64<HRF_REFINE_G>(A, L::C, A.bd, pbase, P, b1, s2, slice, best_idx, best_dist, true);
  }
}

#undef HRF_SWEEP_W16
#undef HRF_SWEEP_W16_ANY

// The unfused certificate: one wave = 64 consecutive pixels of a screen's output (refine_pixels64).
// It is compiled beside the fused sweep, the other user of refine_pixels64: the optimiser
// specialises a device function for the callers its unit holds, and alone in classify_exact.hip
// this kernel came out as different code (136 instead of 150 VGPRs).
__global__ __launch_bounds__(64, HRF_REFINE_WPE) void refine_best_kernel(RefineArgs A, int64_t P, int32_t C, Bounds bd,
                                                         const float *__restrict__ second,
                                                         int32_t *__restrict__ best_idx,
                                                         float *__restrict__ best_dist) {
  extern __shared__ __attribute__((aligned(16))) char rslice[];
  const int lane = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * 64, p = p0 + lane;
  const bool valid = p < P;
  const int b1 = valid ? best_idx[p] : 0;
  const float sec2 = valid ? second[p] : 0.0f;
  refine_pixels64<HRF_REFINE_G>(A, C, bd, p0, P, b1, sec2, rslice, best_idx, best_dist, false);
}

// mode-2 table: {hi[KP], lo[KP], pad 16 B} fp16 per row, KP = 16 * ceil((C + 1) / 16); column C
// is the validity bias (0 real rows, -1024 padding rows); pad fp16 s (s < nseg) = 1 when the row's
// segment s is all zero (the indicator k-step's A operand), fp16 6-7 of row 0 = the library's
// negative-value flag.
__global__ void ref_prep_lay_kernel(const float *__restrict__ ref, int32_t R, int32_t C, Bounds bd, int32_t KP,
                                    int32_t Rpad, int32_t rowh, _Float16 *__restrict__ refh) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= Rpad) return;
  _Float16 *hi = refh + r * rowh;
  _Float16 *lo = hi + KP;
  for (int k = 0; k < rowh; ++k) hi[k] = (_Float16)0.0f;
  hi[C] = (_Float16)(r < R ? 0.0f : -1024.0f);
  if (r >= R) return;
  const float *x = ref + r * C;
  for (int s = 0; s < bd.nseg; ++s) {
    double nn = 0.0;
    for (int c = bd.b[s]; c < bd.b[s + 1]; ++c) nn += (double)x[c] * (double)x[c];
    const bool live = seg_live(nn);
    const double inv = live ? 1.0 / sqrt(nn) : 0.0;
    for (int c = bd.b[s]; c < bd.b[s + 1]; ++c) {
      const float v = live ? (float)((double)x[c] * inv) : 0.0f;
      const _Float16 h = (_Float16)v;
      hi[c] = h;
      lo[c] = (_Float16)(v - (float)h);
    }
    if (!live) hi[2 * KP + s] = (_Float16)1.0f;
  }
}

// row 0's last pad word (byte 4*KP + 12) = 1 when any library value is negative (the keyed argmax
// needs every score >= 0); one workgroup, after ref_prep_lay_kernel
__global__ __launch_bounds__(256) void ref_negflag_kernel(const float *__restrict__ ref, int64_t n, int32_t KP,
                                                          _Float16 *__restrict__ refh) {
  int neg = 0;
  for (int64_t i = threadIdx.x; i < n; i += 256) neg |= ref[i] < 0.0f;
  neg = __syncthreads_or(neg);
  if (threadIdx.x == 0) *reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(refh) + 4 * KP + 12) = (uint32_t)neg;
}

template <class L, int NW, int NB, int CR, int OCC, int NG>
hrf_status launch_w16_lay(const float *stack, int64_t P, const void *refx, int32_t R, int32_t rpad, int32_t *best_idx,
                          float *best_dist, float *second, hipStream_t s) {
  constexpr int KT = (L::C + 1 + 31) / 32;
  const size_t shm = std::max<size_t>((size_t)NB * CR * (128 * KT + L::PADB), sizeof(float) * NW * 32 * L::C);
  HRF_REQUIRE(shm * OCC <= 160 * 1024 + 1024, "classify: w16 configuration exceeds the LDS");
  (void)hipFuncSetAttribute((const void *)classify_pixels_w16_kernel<L, NW, NB, CR, OCC, NG>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  classify_pixels_w16_kernel<L, NW, NB, CR, OCC, NG><<<(unsigned)hrf::cdiv(P, 16 * NG * NW), 64 * NW, shm, s>>>(
      stack, P, (const _Float16 *)refx, R, rpad, best_idx, best_dist, second);
  return HRF_OK;
}

// The table sweep: 4 waves, 2 buffers of 64 rows, OCC workgroups per CU, NG 16-pixel groups per wave.
// FUSE: the certificate follows in the same workgroup (A: its arguments), on the freed chunk buffers.
template <class L, int OCC, bool FUSE, int NG>
void launch_w16t(const void *table, const uint8_t *flags, int64_t P, const void *refx, int32_t R, int32_t rpad,
                 int32_t *best_idx, float *best_dist, float *second, const RefineArgs &A, hipStream_t s) {
  constexpr int KT = (L::C + 1 + 31) / 32;
  constexpr int64_t SL = (refine_slice_bytes() + 15) / 16 * 16;
  const size_t shm = std::max<size_t>((size_t)2 * 64 * (128 * KT + L::PADB), FUSE ? (size_t)(4 * SL) : 0);
  (void)hipFuncSetAttribute((const void *)classify_pixels_w16t_kernel<L, 4, 2, 64, OCC, FUSE, NG>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  classify_pixels_w16t_kernel<L, 4, 2, 64, OCC, FUSE, NG><<<(unsigned)hrf::cdiv(P, 64 * NG), 256, shm, s>>>(
      (const uint4 *)table, flags, P, (const _Float16 *)refx, R, rpad, best_idx, best_dist, second, A);
}

}  // namespace

namespace hrf_cls {

void screen_prepare(const float *ref, int32_t R, int32_t C, const Geometry &g, int32_t mode, void *refx, hipStream_t s) {
  const unsigned grid = (unsigned)hrf::cdiv(g.rpad, 128);
  if (mode == 2) {
    ref_prep_lay_kernel<<<grid, 128, 0, s>>>(ref, R, C, g.bd, g.kp, g.rpad, (int32_t)(g.rowb / 2), (_Float16 *)refx);
    ref_negflag_kernel<<<1, 256, 0, s>>>(ref, (int64_t)R * C, g.kp, (_Float16 *)refx);
  } else if (mode == 0)
    ref_prep_kernel<<<grid, 128, 0, s>>>(ref, R, C, g.bd, g.kp, g.rpad, (float *)refx);
  else
    ref_prep_f16_kernel<<<grid, 128, 0, s>>>(ref, R, C, g.bd, g.kp, g.rpad, (_Float16 *)refx);
}

hrf_status screen_stack(const float *stack, int64_t P, int32_t C, const void *refx, int32_t R, const Geometry &g,
                        int32_t mode, int32_t *best_idx, float *best_dist, float *second, hipStream_t s) {
  const Bounds &bd = g.bd;
  const int32_t kp = g.kp, rpad = g.rpad;
  if (P == 0) return HRF_OK;
  HRF_REQUIRE(stack && refx && best_idx && best_dist, "classify_pixels: null buffer");
  const unsigned grid = (unsigned)hrf::cdiv(P, 256);
  if (mode == 2) {
    HRF_REQUIRE(g.lay != 0, "classify: mode 2 needs the E. coli or multispecies channel layout");
    if (g.lay == 1) {
      // E. coli layout: the 16x16x32 sweep with the lane-per-pixel prologue
      // (classify_pixels_w16_kernel) -- 4 waves, 2 buffers of 64 rows, HRF_W16T_SCREEN_OCC workgroups
      // per CU (rounds 3-5: three, 1.76 vs 1.83 ms for round 2's lay16 form, 2.13-2.20 for the
      // 32x32x16 form, on a 2048^2 tile at R = 1023; DESIGN.md "Per-pixel classifier")
      if (hrf_status st = launch_w16_lay<LayEcoli, 4, 2, 64, HRF_W16T_SCREEN_OCC, HRF_W16T_NG>(
              stack, P, refx, R, rpad, best_idx, best_dist, second, s))
        return st;
      HRF_LAUNCHED();
      return HRF_OK;
    }
    // community layout (R = 127: a two-chunk sweep, where the 32x32x16 form's shorter prologue
    // wins, 0.34 vs 0.44 ms): 4 waves per workgroup share the library chunks streamed through LDS
    const size_t shm = std::max<size_t>((size_t)2 * RCH * (size_t)g.rowb, sizeof(float) * 4 * 32 * C);
    (void)hipFuncSetAttribute((const void *)classify_pixels_lay_kernel<LayMulti, 4>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    classify_pixels_lay_kernel<LayMulti, 4><<<(unsigned)hrf::cdiv(P, 256), 256, shm, s>>>(
        stack, P, (const _Float16 *)refx, R, rpad, best_idx, best_dist, second);
    HRF_LAUNCHED();
    return HRF_OK;
  }
  if (mode == 1) {
    const int ks16 = kp / 16;
    const size_t shm = std::max<size_t>((size_t)2 * RCH * (4 * kp + 16), sizeof(float) * 4 * 32 * (C + MROW) + 128);
    HRF_REQUIRE(shm <= 160 * 1024, "classify_pixels: C too large for LDS staging");
#define HRF_CP16(K)                                                                                          \
  case K:                                                                                                    \
    hipFuncSetAttribute((const void *)classify_pixels_f16_kernel<K>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                        (int)shm);                                                                           \
    classify_pixels_f16_kernel<K><<<grid, 256, shm, s>>>(stack, P, C, bd, (const _Float16 *)refx, R, rpad,     \
                                                         best_idx, best_dist, second);                       \
    break;
    switch (ks16) {
      HRF_CP16(1)
      HRF_CP16(2)
      HRF_CP16(3)
      HRF_CP16(4)
      HRF_CP16(5)
      HRF_CP16(6)
      HRF_CP16(7)
      HRF_CP16(8)
      default:
        HRF_REQUIRE(false, "classify_pixels: unsupported K");
    }
#undef HRF_CP16
    HRF_LAUNCHED();
    return HRF_OK;
  }
  const int ks = kp / 2;
  const size_t shm = sizeof(float) * std::max<size_t>((size_t)RCH * (kp + 2), (size_t)4 * 32 * C);
  HRF_REQUIRE(shm <= 160 * 1024, "classify_pixels: C too large for LDS staging");
#define HRF_CP(K)                                                                                          \
  case K:                                                                                                  \
    hipFuncSetAttribute((const void *)classify_pixels_kernel<K>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                        (int)shm);                                                                         \
    classify_pixels_kernel<K><<<grid, 256, shm, s>>>(stack, P, C, bd, (const float *)refx, R, rpad, best_idx,   \
                                                     best_dist, second);                                   \
    break;
  switch (ks) {
    HRF_CP(8)
    HRF_CP(16)
    HRF_CP(18)
    HRF_CP(24)
    HRF_CP(32)
    HRF_CP(34)
    HRF_CP(40)
    HRF_CP(50)
    HRF_CP(56)
    HRF_CP(64)
    default:
      HRF_REQUIRE(false, "classify_pixels: unsupported K");
  }
#undef HRF_CP
  HRF_LAUNCHED();
  return HRF_OK;
}

// Standalone producer of the pixel table (lay = layout_id, 1 or 2)
hrf_status pixtable_prepare(const float *stack, int64_t P, int lay, void *table, uint8_t *flags, hipStream_t s) {
  const unsigned g = (unsigned)hrf::cdiv(P, 64);
  if (lay == 1)
    pixtable_prep_kernel<LayEcoli><<<g, 256, 0, s>>>(stack, P, (uint4 *)table, flags);
  else
    pixtable_prep_kernel<LayMulti><<<g, 256, 0, s>>>(stack, P, (uint4 *)table, flags);
  HRF_LAUNCHED();
  return HRF_OK;
}

void refine_best(const RefineArgs &A, int64_t P, int32_t C, const Bounds &bd, const float *second, int32_t *best_idx,
                 float *best_dist, hipStream_t s) {
  refine_best_kernel<<<(unsigned)hrf::cdiv(P, 64), 64, (size_t)refine_slice_bytes(), s>>>(A, P, C, bd, second, best_idx,
                                                                                          best_dist);
}

hrf_status screen_table(const void *table, const uint8_t *flags, int64_t P, const void *refx, int32_t R,
                        const Geometry &g, int32_t *best_idx, float *best_dist, float *second, const RefineArgs *fuse,
                        hipStream_t s) {
  auto go = [&](auto lay_tag) {
    using L = decltype(lay_tag);
    if (fuse)
      launch_w16t<L, HRF_W16T_OCC, true, 4>(table, flags, P, refx, R, g.rpad, best_idx, best_dist, nullptr, *fuse, s);
    else
      launch_w16t<L, HRF_W16T_SCREEN_OCC, false, HRF_W16T_NG>(table, flags, P, refx, R, g.rpad, best_idx, best_dist,
                                                              second, RefineArgs{}, s);
  };
  if (g.lay == 1) go(LayEcoli{});
  else go(LayMulti{});
  HRF_LAUNCHED();
  return HRF_OK;
}

}  // namespace hrf_cls

// ---- MFMA accumulation probe ------------------------------------------------------------------
// The per-pixel screen's error bound (hrf_classify_pixels_refine) assumes how an f16 MFMA adds
// its products to the f32 accumulator.  This runs ONE v_mfma_f32_16x16x32_f16 (shape 0) or
// v_mfma_f32_32x32x16_f16 (shape 1) per tile on caller data so tests/test_classify_exact_gpu.py
// can pin that model on the device: A (M x K) and B (K x N) f16 row-major, C and D (M x N) f32.
namespace {
__global__ __launch_bounds__(64) void mfma_probe_kernel(int shape, const _Float16 *__restrict__ a,
                                                        const _Float16 *__restrict__ b, const float *__restrict__ c,
                                                        float *__restrict__ d) {
  const int t = blockIdx.x, lane = threadIdx.x;
  h8 av, bv;
  if (shape == 0) {  // 16 x 16 x 32: lane row/col lane & 15, k 8Q..8Q+7, D rows 4Q..4Q+3
    const _Float16 *A = a + (int64_t)t * 16 * 32, *B = b + (int64_t)t * 32 * 16;
    const float *Cm = c + (int64_t)t * 256;
    float *Dm = d + (int64_t)t * 256;
    const int j = lane & 15, Q = lane >> 4;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      av[q] = A[j * 32 + 8 * Q + q];
      bv[q] = B[(8 * Q + q) * 16 + j];
    }
    f32x4 acc;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = Cm[(4 * Q + i) * 16 + j];
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, acc, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) Dm[(4 * Q + i) * 16 + j] = acc[i];
  } else {  // 32 x 32 x 16: lane row/col lane & 31, k 8h..8h+7, D rows (reg & 3) + 8 (reg >> 2) + 4h
    const _Float16 *A = a + (int64_t)t * 32 * 16, *B = b + (int64_t)t * 16 * 32;
    const float *Cm = c + (int64_t)t * 1024;
    float *Dm = d + (int64_t)t * 1024;
    const int j = lane & 31, h = lane >> 5;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      av[q] = A[j * 16 + 8 * h + q];
      bv[q] = B[(8 * h + q) * 32 + j];
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = Cm[((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + j];
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, bv, acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) Dm[((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + j] = acc[r];
  }
}
}  // namespace

extern "C" hrf_status hrf_probe_mfma_f16(int32_t shape, const void *a, const void *b, const float *c, float *d,
                                         int32_t ntiles, hrf_stream_t stream) {
  HRF_REQUIRE((shape == 0 || shape == 1) && ntiles >= 0 && (ntiles == 0 || (a && b && c && d)),
              "probe_mfma_f16: bad arguments");
  if (ntiles == 0) return HRF_OK;
  mfma_probe_kernel<<<(unsigned)ntiles, 64, 0, (hipStream_t)stream>>>(shape, (const _Float16 *)a,
                                                                      (const _Float16 *)b, c, d);
  HRF_LAUNCHED();
  return HRF_OK;
}
