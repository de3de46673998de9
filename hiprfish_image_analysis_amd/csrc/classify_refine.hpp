// classify_refine.hpp -- the certificate's device code: one wave rescores its 64 pixels' screen rows
// in f64 (refine_pixels64).  Instantiated by the fused table sweep and by refine_best_kernel (both
// in classify_screen.hip); the list pass (classify_exact.hip) uses exact_dist and src_offsets.
#pragma once
#include "classify_types.hpp"

namespace hrf_cls {

__device__ __forceinline__ bool src_covered(int64_t r, int64_t c, int64_t H, int64_t W, int dr, int dc) {
  return r >= (dr > 0 ? dr : 0) && r < H + (dr < 0 ? dr : 0) && c >= (dc > 0 ? dc : 0) && c < W + (dc < 0 ? dc : 0);
}

// element offsets (from src[q]) of pixel p's run in every laser, -1 where it reads as zero
__device__ __forceinline__ void src_offsets(const PixSrc &S, int64_t p, bool valid, int32_t (&off)[XLMAX]) {
  const int64_t r = p / S.W, c = p - r * S.W;
  bool ok = valid;
  if (S.apply_mask && S.dsh)
    for (int q = 0; q < S.n; ++q) ok = ok && src_covered(r, c, S.H, S.W, S.dsh[2 * q], S.dsh[2 * q + 1]);
#pragma unroll
  for (int q = 0; q < XLMAX; ++q) {
    off[q] = -1;
    if (q < S.n && ok) {
      const int dr = S.dsh ? S.dsh[2 * q] : 0, dc = S.dsh ? S.dsh[2 * q + 1] : 0;
      if (src_covered(r, c, S.H, S.W, dr, dc))
        off[q] = (int32_t)(((r - dr) * S.W + (c - dc)) * (int64_t)(S.c0[q + 1] - S.c0[q]));
    }
  }
}

// f64 restated distance of the pixel (f32 values x[0..C), stride 1) to a library row (yv: its f32
// values, float4-aligned, CP = C rounded to 4; nyr: its segment sums of squares): the
// restatement's seg_dist per segment in channel order, their sum, / nseg.  nz: the pixel's
// all-zero segments; in_range: every non-zero segment's sum of squares lies where the screen's f32
// normalisation is exact to its bound (no f32 overflow, no overflowing f64-redo reciprocal).
// NC > 0: the channel loop unrolled to NC (yv then indexes registers with constants); 0: a loop.
constexpr double NX_MIN = 1e-70, NX_MAX = 1e37;
template <int NC, class YV, class NY>
__device__ __forceinline__ double exact_dist_y(const float *x, YV yv, NY nyr, int C, const Bounds &bd, int *nz,
                                               bool *in_range) {
  double sum = 0.0;
  int zc = 0;
  bool rok = true;
  for (int sg = 0; sg < bd.nseg; ++sg) {
    const double ny = nyr(sg);  // issued before the segment's channels: its latency overlaps them
    double nx = 0.0, dd = 0.0;
    // 16 channels' loads issued together (clamped channel, the sum selected: a branch around the
    // sums would take the loads with it and wait for each), then their sums in channel order
    const int cb = bd.b[sg], ce = bd.b[sg + 1];
    for (int c0 = cb; c0 < ce; c0 += 16) {
      float xv[16], yy[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int c = min(c0 + u, ce - 1);
        xv[u] = x[c];
        yy[u] = yv(c);
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const bool ok = c0 + u < ce;
        const double xd = (double)xv[u], yd = (double)yy[u];
        dd = ok ? dd + xd * yd : dd;
        nx = ok ? nx + xd * xd : nx;
      }
    }
    const double sd = (nx == 0.0 && ny == 0.0) ? 0.0 : ((nx == 0.0 || ny == 0.0) ? 1.0 : 1.0 - dd / sqrt(nx * ny));
    sum += sd;
    zc += nx == 0.0 ? 1 : 0;
    rok = rok && (nx == 0.0 || (nx >= NX_MIN && nx <= NX_MAX));
  }
  *nz = zc;
  if (in_range) *in_range = rok;
  return sum / bd.nseg;
}
__device__ __forceinline__ double exact_dist(const float *x, const ExactPtr &E, int r, int C, const Bounds &bd,
                                             int *nz, bool *in_range = nullptr) {
  const float *yr = E.lib32 + (int64_t)r * E.CP;
  const double *nyr = E.ny + (int64_t)r * bd.nseg;
  return exact_dist_y<0>(x, [&](int c) { return yr[c]; }, [&](int sg) { return nyr[sg]; }, C, bd, nz, in_range);
}

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// One wave refines the 64 consecutive pixels p0 .. p0 + 63 (lane = pixel: b1 = its screen row,
// sec2 = the runner-up bound).  The values and rows stream through the wave's LDS slice in chunks
// of RCK channels (lane = (pixel, channel) pairs, every load of a chunk in flight, stored as
// (x, y) pairs), and every lane carries its pixel's f64 sums across the chunks in channel order,
// so the slice stays small (more waves resident) and all 64 lanes do the f64 work.  Then the
// certificate: best_dist (and best_idx with write_idx) for a certified row, the header's answer
// for an all-zero pixel, the list otherwise.
// G chunks' loads are issued together (branch-free: clamped addresses, the value selected after
// the load), so a wave waits for memory once per G chunks rather than once per chunk.
#ifndef HRF_REFINE_WPE
#define HRF_REFINE_WPE 3  // refine_best_kernel: waves per SIMD the register budget allows
#endif
#ifndef HRF_REFINE_RCK
#define HRF_REFINE_RCK 16
#endif
constexpr int RCK = HRF_REFINE_RCK;  // channels per chunk
#ifndef HRF_REFINE_G
#define HRF_REFINE_G 2  // chunks whose loads are in flight together
#endif
__host__ __device__ constexpr int64_t refine_slice_bytes() {
  return (int64_t)64 * (4 * XLMAX + 4) + (int64_t)64 * (RCK + 1) * 8;
}
template <int G>
__device__ __forceinline__ void refine_pixels64(const RefineArgs &A, int C, const Bounds &bd, int64_t p0, int64_t P,
                                                int b1, float sec2, char *slice, int32_t *__restrict__ best_idx,
                                                float *__restrict__ best_dist, bool write_idx) {
  int32_t *offs = reinterpret_cast<int32_t *>(slice);                 // XLMAX x 64
  int32_t *b1s = offs + XLMAX * 64;                                   // 64
  float2 *xy = reinterpret_cast<float2 *>(b1s + 64);                  // 64 x (RCK + 1) (x, y)
  const PixSrc &S = A.S;
  const ExactPtr &E = A.E;
  const int lane = threadIdx.x & 63;
  const int64_t p = p0 + lane;
  const bool valid = p < P;
  const int Rr = A.hdr->R;
  const bool brow = b1 >= 0 && b1 < Rr;
  const int64_t brw = brow ? b1 : 0;
  // the row's segment sums of squares, every load in flight (clamped index, constant register index)
  double nyv[SMAX];
#pragma unroll
  for (int q = 0; q < SMAX; ++q) nyv[q] = E.ny[brw * bd.nseg + (q < bd.nseg ? q : 0)];
  {
    int32_t off[XLMAX];
    src_offsets(S, p, valid, off);
#pragma unroll
    for (int q = 0; q < XLMAX; ++q) offs[q * 64 + lane] = off[q];
    b1s[lane] = (int32_t)brw;
  }
  wave_lds_sync();
  // staging: element lane + 64 u of a chunk = pixel il + 4 u, channel k0 + kl
  const int kl = lane & (RCK - 1), il = lane / RCK;
  double nx = 0.0, dd = 0.0, sum = 0.0;
  int sg = 0, send = bd.b[1], zc = 0;
  bool rok = true;
  for (int k00 = 0; k00 < C; k00 += G * RCK) {
    float xv[G][RCK], yv[G][RCK];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int c = k00 + g * RCK + kl;
      const int ca = c < C ? c : C - 1;  // a readable channel for the padding lanes
      // this lane's laser for channel ca (uniform candidates, per-lane selects: no indexed registers)
      int qc = 0, cq = 0;
      const float *sp = S.src[0];
      for (int q = 1; q < S.n; ++q)
        if (ca >= S.c0[q]) {
          qc = q;
          sp = S.src[q];
          cq = S.c0[q];
        }
      int o[RCK], rb[RCK];
#pragma unroll
      for (int u = 0; u < RCK; ++u) {
        const int i = il + (64 / RCK) * u;
        o[u] = offs[qc * 64 + i];
        rb[u] = b1s[i];
      }
#pragma unroll
      for (int u = 0; u < RCK; ++u) {
        // unconditional loads (a selected address, not a selected value: the compiler would sink a
        // load whose value is selected into a branch and wait for it there); the padding lanes'
        // values are never read
        xv[g][u] = *(o[u] >= 0 ? sp + (o[u] + ca - cq) : A.hdr->zero);
        yv[g][u] = E.lib32[(int64_t)rb[u] * E.CP + ca];
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int k0 = k00 + g * RCK;
      if (k0 >= C) break;
#pragma unroll
      for (int u = 0; u < RCK; ++u) xy[(il + (64 / RCK) * u) * (RCK + 1) + kl] = make_float2(xv[g][u], yv[g][u]);
      wave_lds_sync();
      const float2 *row = xy + lane * (RCK + 1);
#pragma unroll
      for (int k = 0; k < RCK; ++k) {
        if (k0 + k >= C) break;
        const float2 v = row[k];
        const double xd = (double)v.x, yd = (double)v.y;
        dd += xd * yd;
        nx += xd * xd;
        if (k0 + k + 1 == send) {  // the segment's restated distance, in segment order
          double ny = nyv[0];
#pragma unroll
          for (int q = 1; q < SMAX; ++q) ny = sg == q ? nyv[q] : ny;
          const double sd = (nx == 0.0 && ny == 0.0) ? 0.0 : ((nx == 0.0 || ny == 0.0) ? 1.0 : 1.0 - dd / sqrt(nx * ny));
          sum += sd;
          zc += nx == 0.0 ? 1 : 0;
          rok = rok && (nx == 0.0 || (nx >= NX_MIN && nx <= NX_MAX));
          nx = dd = 0.0;
          ++sg;
          send = bd.b[sg + 1];
        }
      }
      wave_lds_sync();  // the chunk is consumed before the next one is staged
    }
  }
  const double D = sum / bd.nseg;
  bool listed = false;
  if (valid) {
    if (!brow) {  // no real row won the screen (cannot happen with R >= 1): list it
      listed = true;
    } else if (zc == bd.nseg) {  // all-zero pixel: the library's own answer
      best_idx[p] = A.hdr->idx0;
      best_dist[p] = (float)A.hdr->D0;
    } else if (!rok) {  // outside the screen bound's premises
      listed = true;
    } else {
      const double eps = A.eps_base + A.eps_zero * zc;
      const double lim = 1.0 - ((double)sec2 + eps) / bd.nseg - 1e-12;
      if (D < lim) {  // certified (NaN anywhere fails the compare)
        if (write_idx) best_idx[p] = b1;
        best_dist[p] = (float)D;
      } else {
        listed = true;
      }
    }
  }
  const unsigned long long m = __ballot(listed);
  if (m) {
    int base = 0;
    if (lane == __ffsll((long long)m) - 1) base = atomicAdd(A.cnt, __popcll(m));
    base = __shfl(base, __ffsll((long long)m) - 1, 64);
    if (listed) {
      A.list[base + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)p;
      if (write_idx) best_idx[p] = b1;  // the list pass's reference row (the unfused screen stored it)
    }
  }
}

}  // namespace hrf_cls
