// classify.hip -- segmented-cosine barcode classification (a19): the C ABI of the classifier.
//
// Metric (train_reference.py channel_cosine_intensity :223-386 / _7b_v2 :993-1072): per
// excitation segment s, d_s = 1 - <x_s, y_s>/(|x_s||y_s|) (0 if both norms are 0, 1 if one
// is); the spectral distance is the mean over segments (gated variants per cell).
//
// Per pixel (north_star mode, ungated) the answer is the f64 restatement's argmin and distance, bit
// for bit, reached in three steps:
//   * the screen: argmin_r d(x, ref_r) = argmax_r sum_s cos'_s, cos'_s the cosine of the
//     segment-normalised vectors plus 1 where both segments are zero -- one dense GEMM of the pixels
//     against the prepared library table with the argmax over R fused into its epilogue, so the
//     P x R score matrix never exists.  It reports per pixel the best row, its score and an upper
//     bound on every other row's score (the runner-up).  Three generations on a (P, C) stack: mode 0
//     v_mfma_f32_32x32x2_f32 (an exact f32 fmaf chain), mode 1 split-fp16 32x32x16 on any layout,
//     mode 2 split-fp16 on the two reference channel layouts (16x16x32 for E. coli, 32x32x16 for the
//     community); and the table form, the mode-2 16x16x32 sweep on B operands prepared where the
//     registered stack is produced (pixtable.hpp) -- the timed path;
//   * the certificate: the best row rescored in f64 as the restatement does; it is the answer when
//     its distance beats the runner-up bound by the screen's proven error bound (screen_eps);
//   * the list pass: for every pixel the certificate leaves (ties, near-ties, non-finite values)
//     the rows that can be the answer -- from an MFMA sweep of the 16x16x32 library image against a
//     threshold proven from the screen's bound, or from an f32 scoring of all rows with its own
//     bound -- are rescored in f64.
// Per cell (reference semantics, gated by presence flags): f64, exact channel order of the
// restatement, CB cells per workgroup -- bit-identical to oracle_segcos.
//
// Units:  classify_types.hpp   host types, the resolved geometry, the functions the units share
//         classify_refine.hpp  the certificate's device code (refine_pixels64)
//         classify_screen.hip  table builders, the mode 0 / 1 / 2 and table sweeps, the certificate's
//                              two kernels (fused into the table sweep, and on its own), the MFMA probe
//         classify_exact.hip   the exact section, the list pass, screen_eps, the refine's host driver
//         classify_cells.hip   the per-cell path with its entry points
//         classify.hip         the per-pixel entry points: argument checks and calls into the above
#include "classify_types.hpp"
#include "devmem.hpp"

using namespace hrf_cls;

namespace {

int choose_ks(int K) {
  static const int ks[] = {8, 16, 18, 24, 32, 34, 40, 50, 56, 64};
  for (int v : ks)
    if (2 * v >= K) return v;
  return -1;
}

int32_t channel_sum(const int32_t *channels_host, int32_t nlaser) {
  int32_t c = 0;
  for (int q = 0; channels_host && q < nlaser && q < XLMAX; ++q) c += channels_host[q];
  return c;
}

}  // namespace

extern "C" {

hrf_status hrf_classify_geometry(int32_t C, int32_t nseg, int32_t R, int32_t mode, int32_t *kp_host,
                                 int32_t *rpad_host) {
  HRF_REQUIRE(C >= 1 && nseg >= 1 && nseg <= SMAX && R >= 1, "classify_geometry: bad arguments");
  HRF_REQUIRE(mode >= 0 && mode <= 2,
              "classify_geometry: mode must be 0 (f32 MFMA), 1 (split fp16 MFMA) or 2 (split fp16, reference layouts)");
  if (mode == 2) {
    *kp_host = 16 * (int32_t)hrf::cdiv(C + 1, 16);
  } else if (mode == 0) {
    const int ks = choose_ks(C + nseg);
    HRF_REQUIRE(ks > 0, "classify: C + nseg must be <= 128");
    *kp_host = 2 * ks;
  } else {
    const int ks16 = (int)hrf::cdiv(C + nseg + 1, 16);  // + the validity-bias column
    HRF_REQUIRE(ks16 >= 1 && ks16 <= 8, "classify: C + nseg must be <= 127");
    *kp_host = 16 * ks16;
  }
  *rpad_host = (int32_t)(hrf::cdiv(R, RCH) * RCH);
  return HRF_OK;
}

hrf_status hrf_classify_table_row_bytes(int32_t C, const int32_t *bounds_host, int32_t nseg, int32_t mode,
                                        int32_t *row_bytes_host) {
  Geometry g;
  if (hrf_status s = resolve(C, bounds_host, nseg, 1, mode, &g)) return s;
  HRF_REQUIRE(row_bytes_host, "classify_table_row_bytes: null output");
  *row_bytes_host = (int32_t)g.rowb;
  return HRF_OK;
}

hrf_status hrf_classify_prepare_refs(const float *ref, int32_t R, int32_t C, const int32_t *bounds_host, int32_t nseg,
                                     int32_t mode, void *refx, hrf_stream_t stream) {
  Geometry g;
  if (hrf_status s = resolve(C, bounds_host, nseg, R, mode, &g)) return s;
  HRF_REQUIRE(ref && refx, "classify_prepare_refs: null buffer");
  HRF_REQUIRE(mode != 2 || g.lay != 0,
              "classify: mode 2 needs the E. coli (0,32,55,75,89,95) or multispecies (0,23,43,57,63) layout");
  HRF_REQUIRE(C <= 128 && R <= LIST_RMAX, "classify_prepare_refs: C <= 128 and R <= %d required", LIST_RMAX);
  screen_prepare(ref, R, C, g, mode, refx, (hipStream_t)stream);
  exact_prepare(ref, R, C, g, refx, (hipStream_t)stream);
  HRF_LAUNCHED();
  return HRF_OK;
}

int64_t hrf_classify_refx_bytes(int32_t C, const int32_t *bounds_host, int32_t nseg, int32_t R, int32_t mode) {
  Geometry g;
  if (resolve(C, bounds_host, nseg, R, mode, &g) != HRF_OK) return -1;
  return g.el.off + g.el.total;
}

// {listed count (16 B), the list (4 P B)}, then the table sweep's runner-up bounds (4 P B) for
// hrf_classify_pixels_table_exact
int64_t hrf_classify_refine_work_bytes(int64_t P) {
  return P < 0 ? -1 : al256(16 + 4 * (P > 0 ? P : 1)) + 4 * (P > 0 ? P : 1);
}

hrf_status hrf_classify_pixels_screen(const float *stack, int64_t P, int32_t C, const void *refx, int32_t R,
                                      const int32_t *bounds_host, int32_t nseg, int32_t mode, int32_t *best_idx,
                                      float *best_dist, float *second, hrf_stream_t stream) {
  Geometry g;
  if (hrf_status s = resolve(C, bounds_host, nseg, R, mode, &g)) return s;
  return screen_stack(stack, P, C, refx, R, g, mode, best_idx, best_dist, second, (hipStream_t)stream);
}

// (the screen is checked inside refine, after the pixel source: the geometry is resolved there)
hrf_status hrf_classify_pixels_refine(const float *const *src_host, const int32_t *channels_host,
                                      const int32_t *shifts_dev, int32_t nlaser, int64_t H, int64_t W,
                                      int32_t apply_mask, const void *refx, int32_t R, const int32_t *bounds_host,
                                      int32_t nseg, int32_t screen, const float *second, int32_t *best_idx,
                                      float *best_dist, void *work, int64_t work_bytes, hrf_stream_t stream) {
  Bounds bd;
  const int32_t C = channel_sum(channels_host, nlaser);
  if (hrf_status s = make_bounds(bounds_host, nseg, C, &bd)) return s;
  PixSrc S;
  if (hrf_status s = pixsrc_of(src_host, channels_host, shifts_dev, nlaser, H, W, apply_mask, C, &S)) return s;
  return refine(S, H * W, C, refx, R, bd, screen, second, best_idx, best_dist, work, work_bytes, (hipStream_t)stream);
}

hrf_status hrf_classify_screen_eps(int32_t C, const int32_t *bounds_host, int32_t nseg, int32_t R, int32_t screen,
                                   double *eps_host) {
  Geometry g;  // (the bounds are reported before a bad screen, the geometry after it)
  if (hrf_status s = make_bounds(bounds_host, nseg, C, &g.bd)) return s;
  HRF_REQUIRE(screen >= 0 && screen <= 3 && eps_host, "classify_screen_eps: bad arguments");
  if (hrf_status s = resolve(C, bounds_host, nseg, R, screen == 3 ? 2 : screen, &g)) return s;
  const ScreenEps e = eps_of_screen(screen, g.bd, C, g.kp);
  eps_host[0] = e.base;
  eps_host[1] = e.zero;
  eps_host[2] = e.eps32;
  return HRF_OK;
}

hrf_status hrf_classify_pixels(const float *stack, int64_t P, int32_t C, const void *refx, int32_t R,
                               const int32_t *bounds_host, int32_t nseg, int32_t mode, int32_t *best_idx,
                               float *best_dist, hrf_stream_t stream) {
  Geometry g;  // (an empty call checks its bounds only)
  if (P == 0) return make_bounds(bounds_host, nseg, C, &g.bd);
  if (hrf_status s = resolve(C, bounds_host, nseg, R, mode, &g)) return s;
  hipStream_t s = (hipStream_t)stream;
  const int64_t wb = hrf_classify_refine_work_bytes(P);
  hrf::StreamBuf<char> ws;
  HRF_HIP(ws.alloc((size_t)(al256(4 * P) + wb), s));
  char *base = ws;
  float *second = (float *)base;
  HRF_TRY(screen_stack(stack, P, C, refx, R, g, mode, best_idx, best_dist, second, s));
  const float *src[1] = {stack};
  const int32_t ch[1] = {C};
  PixSrc S;
  HRF_TRY(pixsrc_of(src, ch, nullptr, 1, 1, P, 0, C, &S));
  HRF_TRY(refine(S, P, C, refx, R, g.bd, mode, second, best_idx, best_dist, base + al256(4 * P), wb, s));
  HRF_HIP(ws.free());
  return HRF_OK;
}

int64_t hrf_pixtable_bytes(int64_t P, int32_t C, const int32_t *bounds_host, int32_t nseg) {
  Bounds bd;
  if (make_bounds(bounds_host, nseg, C, &bd) != HRF_OK) return -1;
  const int lay = layout_id(bd, C);
  if (lay == 0 || P < 0) return -1;
  const int64_t groups = (P + 255) / 256 * 16;  // whole classifier workgroups
  return groups * (lay == 1 ? hrf_pix::group_entries<LayEcoli>() : hrf_pix::group_entries<LayMulti>()) * 16;
}

hrf_status hrf_pixtable_prepare(const float *stack, int64_t P, int32_t C, const int32_t *bounds_host, int32_t nseg,
                                void *table, uint8_t *flags, hrf_stream_t stream) {
  Bounds bd;
  if (hrf_status s = make_bounds(bounds_host, nseg, C, &bd)) return s;
  const int lay = layout_id(bd, C);
  HRF_REQUIRE(lay != 0, "pixtable: the E. coli or multispecies channel layout only");
  if (P == 0) return HRF_OK;
  HRF_REQUIRE(stack && table && flags, "pixtable: null buffer");
  return pixtable_prepare(stack, P, lay, table, flags, (hipStream_t)stream);
}

hrf_status hrf_classify_pixels_table(const void *table, const uint8_t *flags, int64_t P, int32_t C, const void *refx,
                                     int32_t R, const int32_t *bounds_host, int32_t nseg, int32_t *best_idx,
                                     float *best_dist, float *second, hrf_stream_t stream) {
  Geometry g;
  if (hrf_status s = resolve(C, bounds_host, nseg, R, 2, &g)) return s;
  HRF_REQUIRE(g.lay != 0, "classify_pixels_table: the E. coli or multispecies channel layout only");
  if (P == 0) return HRF_OK;
  HRF_REQUIRE(table && flags && refx && best_idx && best_dist, "classify_pixels_table: null buffer");
  return screen_table(table, flags, P, refx, R, g, best_idx, best_dist, second, nullptr, (hipStream_t)stream);
}

// the table sweep, exact: fused (the sweep certifies its own rows) or the sweep with its runner-up
// bounds, then refine_best_kernel; both followed by the list pass
static hrf_status table_exact(const void *table, const uint8_t *flags, const float *const *src_host,
                              const int32_t *channels_host, const int32_t *shifts_dev, int32_t nlaser, int64_t H,
                              int64_t W, int32_t apply_mask, const void *refx, int32_t R, const int32_t *bounds_host,
                              int32_t nseg, int32_t *best_idx, float *best_dist, void *work, int64_t work_bytes,
                              bool fused, hipStream_t s) {
  const int64_t P = H * W;
  const int32_t C = src_host ? channel_sum(channels_host, nlaser) : 0;
  Geometry g;
  if (hrf_status st = resolve(C, bounds_host, nseg, R, 2, &g)) return st;
  HRF_REQUIRE(g.lay != 0, "classify_pixels_table_exact: the E. coli or multispecies channel layout only");
  if (P == 0) return HRF_OK;
  HRF_REQUIRE(table && flags && refx && best_idx && best_dist, "classify_pixels_table_exact: null buffer");
  PixSrc S;
  if (hrf_status st = pixsrc_of(src_host, channels_host, shifts_dev, nlaser, H, W, apply_mask, C, &S)) return st;
  if (!fused) {
    HRF_REQUIRE(work && work_bytes >= hrf_classify_refine_work_bytes(P), "classify_pixels_table_exact: work buffer too small");
    float *second = (float *)((char *)work + al256(16 + 4 * P));
    if (hrf_status st = screen_table(table, flags, P, refx, R, g, best_idx, best_dist, second, nullptr, s)) return st;
    return refine(S, P, C, refx, R, g.bd, 3, second, best_idx, best_dist, work, work_bytes, s);
  }
  RefineArgs A;
  if (hrf_status st = refine_args(S, P, C, refx, R, g.bd, 3, work, work_bytes, &A, s)) return st;
  if (hrf_status st = screen_table(table, flags, P, refx, R, g, best_idx, best_dist, nullptr, &A, s)) return st;
  return refine_list(A, P, C, R, g.bd, 3, best_idx, best_dist, s);
}

hrf_status hrf_classify_pixels_table_exact(const void *table, const uint8_t *flags, const float *const *src_host,
                                           const int32_t *channels_host, const int32_t *shifts_dev, int32_t nlaser,
                                           int64_t H, int64_t W, int32_t apply_mask, const void *refx, int32_t R,
                                           const int32_t *bounds_host, int32_t nseg, int32_t *best_idx,
                                           float *best_dist, void *work, int64_t work_bytes, hrf_stream_t stream) {
  return table_exact(table, flags, src_host, channels_host, shifts_dev, nlaser, H, W, apply_mask, refx, R, bounds_host,
                     nseg, best_idx, best_dist, work, work_bytes, false, (hipStream_t)stream);
}

// One tile at a time with nothing else on the device: 0.05 ms less than the two-kernel form.  Beside
// concurrent tiles it is slower (826 vs 846 Mpix/s; DESIGN.md "Per-pixel classifier"), so the tile
// pipeline calls the unfused form.
hrf_status hrf_classify_pixels_table_exact_fused(const void *table, const uint8_t *flags,
                                                 const float *const *src_host, const int32_t *channels_host,
                                                 const int32_t *shifts_dev, int32_t nlaser, int64_t H, int64_t W,
                                                 int32_t apply_mask, const void *refx, int32_t R,
                                                 const int32_t *bounds_host, int32_t nseg, int32_t *best_idx,
                                                 float *best_dist, void *work, int64_t work_bytes,
                                                 hrf_stream_t stream) {
  return table_exact(table, flags, src_host, channels_host, shifts_dev, nlaser, H, W, apply_mask, refx, R, bounds_host,
                     nseg, best_idx, best_dist, work, work_bytes, true, (hipStream_t)stream);
}

}  // extern "C"
