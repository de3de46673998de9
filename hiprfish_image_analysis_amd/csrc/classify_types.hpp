// classify_types.hpp -- what more than one classifier unit needs on the host side: the segment
// bounds, the prepared library's geometry and exact section, the refine's kernel arguments, and the
// functions the units call across (classify.hip's header maps the units).
#pragma once
#include <algorithm>

#include "common.hpp"
#include "pixtable.hpp"

namespace hrf_cls {

using hrf_pix::LayEcoli;
using hrf_pix::LayMulti;

constexpr int SMAX = 8;
struct Bounds {
  int32_t b[SMAX + 1];
  int32_t nseg;
};
inline hrf_status make_bounds(const int32_t *bounds_host, int32_t nseg, int32_t C, Bounds *bd) {
  HRF_REQUIRE(nseg >= 1 && nseg <= SMAX && bounds_host, "classify: 1..8 segments required");
  HRF_REQUIRE(bounds_host[0] == 0 && bounds_host[nseg] == C, "classify: segment bounds must span [0, C)");
  for (int s = 0; s < nseg; ++s) HRF_REQUIRE(bounds_host[s] < bounds_host[s + 1], "classify: empty segment");
  for (int s = 0; s <= SMAX; ++s) bd->b[s] = s <= nseg ? bounds_host[s] : C;
  bd->nseg = nseg;
  return HRF_OK;
}

constexpr int RCH = 64;  // references per LDS chunk (prefetched into registers)
constexpr int XLMAX = 8;
constexpr int LIST_RMAX = 4096;
inline int64_t al256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// 1 = E. coli layout, 2 = synthetic-community layout, 0 = other
template <class L>
bool is_layout(const Bounds &bd, int C) {
  if (C != L::C || bd.nseg != L::NSEG) return false;
  for (int s = 0; s <= L::NSEG; ++s)
    if (bd.b[s] != L::b(s)) return false;
  return true;
}
inline int layout_id(const Bounds &bd, int C) {
  if (is_layout<LayEcoli>(bd, C)) return 1;
  if (is_layout<LayMulti>(bd, C)) return 2;
  return 0;
}
// bytes per row of a mode-1/2 table: hi | lo | pad (the reference layouts' pads differ)
inline int64_t table_rowb(int mode, int lay, int kp) {
  if (mode == 2 && lay == 1) return 4 * kp + LayEcoli::PADB;
  if (mode == 2 && lay == 2) return 4 * kp + LayMulti::PADB;
  return 4 * kp + 16;
}

// ---- the exact section (its use: classify_exact.hip) ---------------------------------------------
// The prepared library (refx) carries the exact section after its MFMA table: a header, the f32
// library row-major (pitch CP = C rounded to 4, float4 rows), channel-major (pitch RT = R rounded
// to 64, coalesced for the list kernel), the f64 segment sums of squares ny (the restatement's
// |y|^2) and f32 reciprocal segment norms iy.
struct ExactHdr {
  int32_t R, C, nseg, idx0;  // idx0 / D0: the all-zero pixel's argmin and distance
  double D0;
  int32_t tiny;              // some row has 0 < ny < 1e-30, ny >= 1e30 or a non-finite ny: the list
                             // kernel's f32 pass is not safe (underflow / overflow of its raw products)
  float zero[4];             // 0: what an uncovered pixel's channel reads (a load that needs no branch)
};
struct ExactLayout {
  int64_t off;  // section offset from the start of refx
  int32_t CP, RT;
  int64_t lib32, libT, ny, iy, total;  // offsets inside the section
};
inline ExactLayout exact_layout(int64_t rowb, int rpad, int R, int C, int nseg) {
  ExactLayout e;
  e.off = al256((int64_t)rpad * rowb);
  e.CP = (C + 3) & ~3;
  e.RT = (R + 63) & ~63;
  e.lib32 = 256;
  e.libT = al256(e.lib32 + (int64_t)R * e.CP * 4);
  e.ny = al256(e.libT + (int64_t)C * e.RT * 4);
  e.iy = al256(e.ny + (int64_t)R * nseg * 8);
  e.total = al256(e.iy + (int64_t)R * nseg * 4);
  return e;
}
struct ExactPtr {
  const float *lib32, *libT, *iy;
  const double *ny;
  int32_t CP, RT;
};

// Pixel source: the registered value of pixel p (row r = p / W, column c = p % W) at channel k of
// laser q is src[q][((r - dr_q) W + (c - dc_q)) cl_q + (k - c0_q)], 0 outside the laser's frame and,
// with apply_mask, outside any laser's frame (register_assemble's stack; stack.hip).  A plain (P, C)
// stack is one laser with no shift.
struct PixSrc {
  const float *src[XLMAX];
  int32_t c0[XLMAX + 1];
  uint64_t mdiv[XLMAX];  // ceil(2^32 / cl): e / cl = (e * mdiv) >> 32 for e < 2^32 / cl
  int32_t n;
  const int32_t *dsh;    // device (dr, dc) pairs, or null (no shift)
  int64_t H, W;
  int32_t apply_mask;
};

// Everything the refine of a screen's output needs (kernel argument of the fused sweep)
struct RefineArgs {
  PixSrc S;
  ExactPtr E;
  const ExactHdr *hdr;
  double eps_base, eps_zero;
  int32_t *list, *cnt;
  Bounds bd;  // (kernel-argument memory: indexed by a runtime segment without a scratch copy)
  // the list pass's candidate sweep: the library's 16x16x32 MFMA image (the start of refx), its row
  // pitch in bytes and its rows; null where the screen's table is no such image (the list pass then
  // scores every row in f32)
  const void *img;
  int32_t img_rowb, img_rows;
};

struct ScreenEps {
  double base, zero, eps32;
};

// The geometry an entry point's (C, bounds, nseg, R, mode) resolve to: the checked bounds, the
// reference layout (layout_id), the table's padded columns, rows and row bytes, the exact section.
struct Geometry {
  Bounds bd;
  int32_t lay, kp, rpad;
  int64_t rowb;
  ExactLayout el;
};
inline hrf_status resolve(int32_t C, const int32_t *bounds_host, int32_t nseg, int32_t R, int32_t mode, Geometry *g) {
  if (hrf_status s = make_bounds(bounds_host, nseg, C, &g->bd)) return s;
  if (hrf_status s = hrf_classify_geometry(C, nseg, R, mode, &g->kp, &g->rpad)) return s;
  g->lay = layout_id(g->bd, C);
  g->rowb = mode == 0 ? 4 * (int64_t)g->kp : table_rowb(mode, g->lay, g->kp);
  g->el = exact_layout(g->rowb, g->rpad, R, C, nseg);
  return HRF_OK;
}

// ---- classify_screen.hip: (best row, score, runner-up bound) per pixel -------------------------
// the MFMA table of a prepared library (launches only: the caller checks them)
void screen_prepare(const float *ref, int32_t R, int32_t C, const Geometry &g, int32_t mode, void *refx, hipStream_t s);
// the sweep of hrf_classify_pixels (`second`: nullable runner-up bound output)
hrf_status screen_stack(const float *stack, int64_t P, int32_t C, const void *refx, int32_t R, const Geometry &g,
                        int32_t mode, int32_t *best_idx, float *best_dist, float *second, hipStream_t s);
hrf_status pixtable_prepare(const float *stack, int64_t P, int lay, void *table, uint8_t *flags, hipStream_t s);
// the certificate on a screen's output (refine_best_kernel; a launch only)
void refine_best(const RefineArgs &A, int64_t P, int32_t C, const Bounds &bd, const float *second, int32_t *best_idx,
                 float *best_dist, hipStream_t s);
// the pixel-table sweep; fuse (nullable): the sweep runs the certificate itself on its own rows
hrf_status screen_table(const void *table, const uint8_t *flags, int64_t P, const void *refx, int32_t R,
                        const Geometry &g, int32_t *best_idx, float *best_dist, float *second, const RefineArgs *fuse,
                        hipStream_t s);

// ---- classify_exact.hip: a screen's output -> the restated answer ------------------------------
// the exact section of a prepared library (launches only)
void exact_prepare(const float *ref, int32_t R, int32_t C, const Geometry &g, void *refx, hipStream_t s);
ScreenEps eps_of_screen(int screen, const Bounds &bd, int C, int kp);
hrf_status pixsrc_of(const float *const *src_host, const int32_t *channels_host, const int32_t *shifts_dev,
                     int32_t nlaser, int64_t H, int64_t W, int32_t apply_mask, int32_t C, PixSrc *S);
hrf_status refine_args(const PixSrc &S, int64_t P, int32_t C, const void *refx, int32_t R, const Bounds &bd,
                       int32_t screen, void *work, int64_t work_bytes, RefineArgs *A, hipStream_t s);
hrf_status refine_list(const RefineArgs &A, int64_t P, int32_t C, int32_t R, const Bounds &bd, int32_t screen,
                       int32_t *best_idx, float *best_dist, hipStream_t s);
hrf_status refine(const PixSrc &S, int64_t P, int32_t C, const void *refx, int32_t R, const Bounds &bd, int32_t screen,
                  const float *second, int32_t *best_idx, float *best_dist, void *work, int64_t work_bytes,
                  hipStream_t s);

}  // namespace hrf_cls
