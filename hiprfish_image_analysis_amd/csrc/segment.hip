// segment.hip -- native drivers for the two segmentation chains.
//
// The E. coli chain (ecoli measurement.py:44-127) and the synthetic-community chain
// (multispecies measurement.py:102-157) are ~25-30 library calls each, a few of which
// synchronise (KMeans centres, component counts, watershed convergence).  Composed from
// Python, every call pays the interpreter and allocator, and two host threads driving
// concurrent tiles serialise on the GIL.  These drivers run the same calls from C++ with a
// per-context set of device buffers allocated once for the tile size, so one foreign call
// (ctypes drops the GIL for it) does a whole chain.  The composition is the one in
// pipeline.py, step for step; tests check the two give identical label maps.
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "devmem.hpp"

using hrf::DevBuf;
using hrf::PinnedBuf;

struct hrf_seg_ctx {
  int64_t H = 0, W = 0, n = 0;
  int device = 0;
  // f64 images
  DevBuf<double> cn, f1, f2, f3, pad;
  DevBuf<double> scal;  // device scalar (max)
  // u8 masks
  DevBuf<uint8_t> m[6];
  // int32 images / scratch
  DevBuf<int32_t> l[4];
  DevBuf<int32_t> parent, size, blk, dint;
  DevBuf<char> ws_state;
  DevBuf<int32_t> ws_flag;
  // pinned host slots for counts read back at a later synchronisation (.dev(): hrf::zero_publish)
  PinnedBuf hpin;
  DevBuf<char> km;
  int64_t km_bytes = 0;
  DevBuf<char> seed_px;  // erosion seeding's pixel-kernel scratch
  // the last chain's watershed: passes, contested pixels, resolution rounds, decisions between
  // equal-valued markers of different labels (hrf_watershed_ex ties_host) -- hrf_seg_ctx_stats
  int32_t ws_stats[4] = {0, 0, 0, 0};
  // per-label scratch, grown on demand
  int64_t lab_cap = 0;
  DevBuf<int32_t> box, cnt;
  PinnedBuf hbox;  // pinned host copy of box (4 * lab_cap)
  DevBuf<int64_t> mom;
  DevBuf<double> props;
};

namespace {

// Grows the per-label buffers to hold labels 0..maxlab.  The larger set is allocated first and
// moved in (releasing the old one) only when all of it exists; on failure c is unchanged.
hrf_status ensure_labels(hrf_seg_ctx *c, int64_t maxlab, hipStream_t s) {
  if (maxlab + 1 <= c->lab_cap) return HRF_OK;
  HRF_HIP(hipStreamSynchronize(s));  // buffers of the previous size may still be in use
  int64_t cap = 1024;
  while (cap < maxlab + 1) cap *= 2;
  DevBuf<int32_t> box, cnt;
  DevBuf<int64_t> mom;
  DevBuf<double> props;
  PinnedBuf hbox;
  HRF_TRY(box.alloc(4 * cap));
  HRF_TRY(cnt.alloc(cap));
  HRF_TRY(mom.alloc(6 * cap));
  HRF_TRY(props.alloc(8 * cap));
  HRF_TRY(hbox.alloc(4 * cap, "seg_ctx"));
  // the chain clears cnt and mom at the watershed's synchronisation (capacity-wide); buffers
  // allocated after it are cleared here
  HRF_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * cap, s));
  HRF_HIP(hipMemsetAsync(mom, 0, sizeof(int64_t) * 6 * cap, s));
  c->box = std::move(box);
  c->cnt = std::move(cnt);
  c->mom = std::move(mom);
  c->props = std::move(props);
  c->hbox = std::move(hbox);
  c->lab_cap = cap;
  return HRF_OK;
}

hrf_status read_i32(const int32_t *dev, int32_t *host, hipStream_t s) {
  HRF_HIP(hipMemcpyAsync(host, dev, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HRF_HIP(hipStreamSynchronize(s));
  return HRF_OK;
}

// skimage.measure.label(mask, connectivity=2) -> labels, count (host)
hrf_status label_conn2(hrf_seg_ctx *c, const uint8_t *mask, int32_t *labels, int32_t *nlab, hipStream_t s) {
  HRF_TRY(hrf_label(mask, 0, c->H, c->W, 2, labels, c->parent, c->blk, c->dint, s));
  return read_i32(c->dint, nlab, s);
}

// skimage.measure.label(mask, connectivity=2) with the count's read-back only enqueued: it
// lands in c->hpin[0] at the caller's next synchronisation (saves one host round trip)
hrf_status label_conn2_deferred(hrf_seg_ctx *c, const uint8_t *mask, int32_t *labels, hipStream_t s) {
  HRF_TRY(hrf_label(mask, 0, c->H, c->W, 2, labels, c->parent, c->blk, c->dint, s));
  HRF_HIP(hipMemcpyAsync(c->hpin, c->dint, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  return HRF_OK;
}

// KMeans(k) top-cluster mask (rule: see hrf.h); `reuse` when the previous call sorted the same x
hrf_status kmeans_top(hrf_seg_ctx *c, const double *x, int k, int rule, int reuse, uint8_t *top, hipStream_t s) {
  return hrf_kmeans_1d_sorted(x, nullptr, c->n, k, 300, 10, rule, nullptr, top, nullptr, nullptr, c->km, c->km_bytes,
                              reuse, s);
}

}  // namespace

extern "C" {

hrf_status hrf_seg_ctx_create(int64_t H, int64_t W, hrf_seg_ctx **out) {
  HRF_REQUIRE(out && H >= 1 && W >= 1 && H * W < ((int64_t)1 << 31), "seg_ctx: bad size");
  auto c = std::make_unique<hrf_seg_ctx>();
  c->H = H;
  c->W = W;
  c->n = H * W;
  const size_t n = (size_t)c->n;
  HRF_HIP(hipGetDevice(&c->device));
  HRF_TRY(c->cn.alloc(n));
  HRF_TRY(c->f1.alloc(n));
  HRF_TRY(c->f2.alloc(n));
  HRF_TRY(c->f3.alloc(n));
  HRF_TRY(c->pad.alloc((size_t)(H + 10) * (W + 10)));
  HRF_TRY(c->scal.alloc(8));
  for (auto &p : c->m) HRF_TRY(p.alloc(n));
  for (auto &p : c->l) HRF_TRY(p.alloc(n));
  HRF_TRY(c->parent.alloc(n));
  HRF_TRY(c->size.alloc(n));
  HRF_TRY(c->blk.alloc((size_t)::hrf::label_dev_ws_words(c->n)));
  HRF_TRY(c->dint.alloc(16));
  HRF_TRY(c->ws_flag.alloc(8));
  HRF_TRY(c->ws_state.alloc((size_t)hrf_watershed_workspace_bytes(H, W)));
  HRF_TRY(c->hpin.alloc(16, "seg_ctx"));
  c->km_bytes = hrf_kmeans_sorted_workspace_bytes(c->n);
  if (c->km_bytes <= 0) return HRF_EHIP;
  HRF_TRY(c->km.alloc((size_t)c->km_bytes));
  HRF_TRY(c->seed_px.alloc((size_t)::hrf::seed_px_scratch_bytes()));
  *out = c.release();
  return HRF_OK;
}

hrf_status hrf_seg_ctx_destroy(hrf_seg_ctx *c) {
  delete c;
  return HRF_OK;
}

// ecoli :73-127 from image_cn (f64, H x W).  Clears and host read-backs ride on the chain's two
// synchronisations (components + boxes, watershed batch) as ZeroPub launches; `extra` (the
// native tile's per-label buffers) is cleared at the watershed's.
static hrf_status segment_ecoli_from_cn(hrf_seg_ctx *c, const double *cn, int32_t *seg_out, int32_t *maxlab_host,
                                        hipStream_t s, const ::hrf::ZeroPub *extra) {
  const int64_t H = c->H, W = c->W, n = c->n;
  uint8_t *rough = c->m[0], *interior = c->m[1], *a = c->m[2], *b = c->m[3], *d = c->m[4];
  int32_t *lab1 = c->l[0], *seeds = c->l[1], *ws = c->l[2], *lab3 = c->l[3];
  // :73-94; the NaN check (sklearn raises) is read at the component-count synchronisation below
  HRF_TRY(::hrf::kmeans_1d_sorted_pair_deferred(cn, c->n, 2, 3, 300, 10, 2, 0, rough, interior, c->km, c->km_bytes, s,
                                                nullptr));
  const int32_t *km_err = ::hrf::kmeans_error_flag(c->km, c->n);
  HRF_REQUIRE(km_err, "segment_ecoli: kmeans workspace");
  HRF_TRY(hrf_remove_small_holes(interior, H, W, 64, 1, a, c->parent, c->size, s));   // :95
  HRF_TRY(::hrf::binary_opening(a, H, W, 1, d, s));                                 // erosion, dilation
  HRF_TRY(hrf_remove_small_objects_mask(d, H, W, 50, 1, a, c->parent, c->size, s));  // :96 cell_sm = a
  // :97-110.  Components, their count and their boxes come back in ONE synchronisation: the
  // boxes are computed for every label the current capacity holds (labels above it are
  // ignored by the box kernel) and redone in the rare case the count exceeds it.
  HRF_TRY(::hrf::label_dev(a, H, W, 2, lab1, c->parent, c->blk, c->dint, s));
  HRF_TRY(ensure_labels(c, 1, s));
  int32_t guess = (int32_t)(c->lab_cap - 1);
  HRF_TRY(hrf_label_boxes(lab1, H, W, guess, c->box, s));
  {
    ::hrf::ZeroPub zp;
    HRF_REQUIRE(zp.pub(c->dint, c->hpin.dev() + 1, 1) && zp.pub(km_err, c->hpin.dev() + 3, 1) &&
                    zp.pub(c->box, c->hbox.dev(), 4 * (guess + 1)),
                "segment_ecoli: too many read-backs");
    HRF_TRY(::hrf::zero_publish(zp, s));
  }
  HRF_HIP(hipStreamSynchronize(s));
  HRF_REQUIRE(!c->hpin[3], "kmeans_1d_pair: input contains NaN or infinity, or a finite magnitude above 2^1022 (sklearn KMeans raises ValueError)");
  const int32_t ncomp = c->hpin[1];
  HRF_REQUIRE(ncomp >= 0, "segment_ecoli: component numbering failed");
  if (ncomp > guess) {
    HRF_TRY(ensure_labels(c, ncomp, s));
    HRF_TRY(hrf_label_boxes(lab1, H, W, ncomp, c->box, s));
    ::hrf::ZeroPub zp;
    HRF_REQUIRE(zp.pub(c->box, c->hbox.dev(), 4 * (ncomp + 1)), "segment_ecoli: too many read-backs");
    HRF_TRY(::hrf::zero_publish(zp, s));
    HRF_HIP(hipStreamSynchronize(s));
  }
  // Large-box components go to the run kernel too; how many overflowed it lands in hpin[2]
  // at the watershed's synchronisation, and in that (rare) case the seeds and everything
  // after them are redone with those components in the whole-image loop.
  for (int attempt = 0;; ++attempt) {
    HRF_TRY(::hrf::erosion_seeds_hostbox(lab1, H, W, ncomp, c->box, c->hbox, 600, 10, b, s,
                                         attempt == 0 ? c->dint + 8 : nullptr, c->seed_px));
    HRF_TRY(hrf_remove_small_objects_mask(b, H, W, 10, 2, d, c->parent, c->size, s));  // :111
    HRF_TRY(::hrf::label_dev(d, H, W, 2, seeds, c->parent, c->blk, c->dint, s));  // :111-112
    // read back at the watershed's synchronisation: the seed count, the run kernel's overflow
    // count; cleared there: the per-label counts and moments (capacity-wide) and `extra`
    ::hrf::ZeroPub zp = extra ? *extra : ::hrf::ZeroPub();
    HRF_REQUIRE(zp.pub(c->dint, c->hpin.dev() + 0, 1) && (attempt > 0 || zp.pub(c->dint + 8, c->hpin.dev() + 2, 1)) &&
                    zp.zero(c->cnt, sizeof(int32_t) * c->lab_cap) && zp.zero(c->mom, sizeof(int64_t) * 6 * c->lab_cap),
                "segment_ecoli: too many read-backs");
    HRF_TRY(::hrf::watershed_ex_extra(cn, 1, seeds, rough, H, W, ws, c->ws_state, c->ws_flag, 100000, c->ws_stats,
                                      c->ws_stats + 1, s, &zp));  // :113
    if (attempt > 0 || c->hpin[2] == 0) break;
  }
  const int32_t nseeds = c->hpin[0];  // read back by the watershed's synchronisation
  HRF_REQUIRE(nseeds >= 0, "segment_ecoli: seed numbering failed");
  HRF_TRY(ensure_labels(c, nseeds, s));
  HRF_TRY(::hrf::remove_small_objects_labels_zeroed(ws, n, nseeds, 100, lab1, c->cnt, s));    // :114
  HRF_TRY(hrf_clear_border(lab1, H, W, lab3, c->parent, c->size, s));          // :115
  HRF_TRY(::hrf::region_moments_zeroed(lab3, H, W, nseeds, c->mom, s));         // :116
  // the props pass + shape filter (:116-126; the filter straight from the moments -- one launch
  // less, every labelled pixel recomputing its label's eigenvalues -- lost, removed in round 5)
  HRF_TRY(hrf_region_props(c->mom, nseeds, c->props, s));
  HRF_TRY(hrf_shape_filter(lab3, H, W, c->props, nseeds, 15.0, 35.0, seg_out, s));
  *maxlab_host = nseeds;
  return HRF_OK;
}

hrf_status hrf_seg_ctx_stats(const hrf_seg_ctx *c, int32_t *out) {
  HRF_REQUIRE(c && out, "seg_ctx_stats: bad arguments");
  for (int i = 0; i < 4; ++i) out[i] = c->ws_stats[i];
  return HRF_OK;
}

hrf_status hrf_segment_ecoli(hrf_seg_ctx *c, const float *stack, int32_t C, int32_t *seg_out, int32_t *maxlab_host,
                             hrf_stream_t stream) {
  HRF_REQUIRE(c && stack && seg_out && maxlab_host && C >= 1, "segment_ecoli: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  HRF_TRY(hrf_channel_sum(stack, c->n, C, nullptr, 1, 0, c->cn, s));            // :71-72
  return segment_ecoli_from_cn(c, c->cn, seg_out, maxlab_host, s, nullptr);
}

hrf_status hrf_segment_ecoli_cn(hrf_seg_ctx *c, const double *image_cn, int32_t *seg_out, int32_t *maxlab_host,
                                hrf_stream_t stream) {
  HRF_REQUIRE(c && image_cn && seg_out && maxlab_host, "segment_ecoli_cn: bad arguments");
  return segment_ecoli_from_cn(c, image_cn, seg_out, maxlab_host, (hipStream_t)stream, nullptr);
}

}  // extern "C"

// the native tile's entry: hrf_segment_ecoli_cn with the tile's per-label buffers cleared at the
// watershed's synchronisation
hrf_status hrf::segment_ecoli_cn_extra(hrf_seg_ctx *c, const double *image_cn, int32_t *seg_out,
                                       int32_t *maxlab_host, hipStream_t s, const ZeroPub *extra) {
  HRF_REQUIRE(c && image_cn && seg_out && maxlab_host, "segment_ecoli_cn: bad arguments");
  return segment_ecoli_from_cn(c, image_cn, seg_out, maxlab_host, s, extra);
}

extern "C" {

hrf_status hrf_segment_multispecies(hrf_seg_ctx *c, const float *stack, int32_t C, const float *cal, int64_t cal_sp,
                                    int32_t cal_sc, int32_t cal_c0, int32_t cal_c1, int32_t *seg_out,
                                    int32_t *nlab_host, double *image_sum_out, double *final_bkg_out,
                                    hrf_stream_t stream) {
  HRF_REQUIRE(c && stack && seg_out && nlab_host && C >= 1, "segment_multispecies: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const int64_t H = c->H, W = c->W, n = c->n;
  uint8_t *rough = c->m[0], *bkg = c->m[1], *a = c->m[2], *b = c->m[3], *d = c->m[4], *e = c->m[5];
  int32_t *seeds = c->l[0], *seeds_b = c->l[1], *ws = c->l[2], *lab3 = c->l[3];
  // sum: out or cn; norm: f3; nl: f1; final: f2; final_bkg: out or cn (sum is dead by then)
  double *sum = image_sum_out ? image_sum_out : c->cn;
  double *norm = c->f3, *nl = c->f1, *fin = c->f2;
  HRF_TRY(hrf_channel_sum_cal(stack, n, C, cal, cal_sp, cal_sc, cal_c0, cal_c1, 0, sum, s));   // :104-105
  HRF_TRY(hrf_max_f64(sum, n, c->scal, s));                                     // :106
  HRF_TRY(hrf_div_scalar_f64(sum, n, c->scal, norm, s));
  HRF_TRY(hrf_nl_means_2d(norm, H, W, 7, 11, 0.02, 0.0, nl, s));               // :108
  HRF_TRY(hrf_pad_edge_f64(nl, H, W, 5, c->pad, s));                            // :109
  HRF_TRY(hrf_enhance_2d(c->pad, H + 10, W + 10, W + 10, 11, 9, fin, s));      // :110-124
  HRF_TRY(kmeans_top(c, fin, 2, 1, 0, rough, s));                               // :125-135
  HRF_TRY(::hrf::binary_opening(rough, H, W, 1, b, s));                          // :136 erosion, dilation
  HRF_TRY(hrf_remove_small_objects_mask(b, H, W, 10, 1, a, c->parent, c->size, s));  // :137
  HRF_TRY(hrf_fill_holes(a, H, W, b, c->parent, c->size, s));                  // :138
  HRF_TRY(hrf_fill_holes(rough, H, W, d, c->parent, c->size, s));              // :139
  HRF_TRY(hrf_and_u8(b, d, n, e, s));                                          // :140
  HRF_TRY(label_conn2_deferred(c, e, seeds, s));
  HRF_TRY(kmeans_top(c, nl, 2, 1, 0, bkg, s));                                  // :141-149
  const int32_t nseeds = c->hpin[0];  // read back by the KMeans synchronisation
  double *final_bkg = final_bkg_out ? final_bkg_out : c->cn;
  HRF_TRY(hrf_mask_mul_f64(fin, bkg, n, final_bkg, s));                         // :150
  HRF_TRY(hrf_mask_labels(seeds, bkg, n, seeds_b, s));                          // :152
  HRF_TRY(hrf_and_u8(rough, bkg, n, a, s));                                     // :153
  HRF_TRY(hrf_watershed_ex(final_bkg, 1, seeds_b, a, H, W, ws, c->ws_state, c->ws_flag, 100000, c->ws_stats,
                           c->ws_stats + 1, s));  // :154
  HRF_TRY(ensure_labels(c, nseeds, s));
  HRF_TRY(hrf_remove_small_objects_labels(ws, n, nseeds, 60, seeds, c->cnt, s));     // :155
  HRF_TRY(hrf_clear_border(seeds, H, W, lab3, c->parent, c->size, s));         // :156
  HRF_TRY(hrf_relabel_sequential(lab3, n, nseeds, seg_out, c->cnt, c->dint, s));     // :157
  return read_i32(c->dint, nlab_host, s);
}

}  // extern "C"
