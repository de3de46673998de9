"""Device pipelines: the reference's measurement and classification stages, every compute
step a libhrf.so kernel (kernels.py).  Tensors stay resident in HBM from the (H, W, C) stack
to the label map, per-cell spectra, barcode ids and counts.

Each function cites the reference lines it stands in for.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from dataclasses import dataclass, field

import torch

from . import kernels as K

ECOLI_BOUNDS = (0, 32, 55, 75, 89, 95)
MULTI_BOUNDS = (0, 23, 43, 57, 63)


# --------------------------------------------------------------------------------------------
# E. coli / reference-library measurement (hiprfish_imaging_spectral_image_measurement.py)
# --------------------------------------------------------------------------------------------
def erosion_seeds(cell_sm: torch.Tensor, area_max: int = 600, min_obj: int = 10) -> torch.Tensor:
    """ecoli measurement.py:97-110: freeze regions below `area_max` as seeds, erode the rest,
    drop fragments < `min_obj` (4-connected), repeat until nothing is left.  -> seed mask u8
    One launch, one workgroup per 8-connected component (seeds.hip)."""
    return K.erosion_seeds(cell_sm, area_max, min_obj)


def erosion_seeds_global(cell_sm: torch.Tensor, area_max: int = 600, min_obj: int = 10) -> torch.Tensor:
    """The same loop as whole-image passes (one CC / erosion / sieve launch set per iteration);
    kept as a cross-check of the per-component kernel."""
    be = torch.zeros_like(K._u8(cell_sm, "cell_sm"))
    m = K._u8(cell_sm, "cell_sm")
    while K.count_nonzero(m) > 0:                      # markers = regionprops(dist_lab) non-empty
        m = K.split_by_size(m, area_max, be, conn=2)   # :102-106 (dist_lab is 8-connected)
        m = K.binary_erosion(m, 1)                     # :107
        m = K.remove_small_objects(m, min_obj, conn=1)  # :108
    return be


# The segmentation chains run as one native call (segment.hip, same calls in the same order)
# unless intermediates are requested (`keep`) or HRF_NATIVE_SEG=0.
NATIVE_SEG = os.environ.get("HRF_NATIVE_SEG", "1") != "0"
# power-of-two tiles: the registration cross-correlations through xcorr.hip (six launches for all
# lasers) instead of hipFFT; HRF_XCORR=0 keeps hipFFT
XCORR = os.environ.get("HRF_XCORR", "1") != "0"


def segment_ecoli(stack: torch.Tensor, keep: dict | None = None, image_cn: torch.Tensor | None = None):
    """ecoli measurement.py:44-127 on the registered stack.  -> (segmentation int32, max label)
    image_cn: the stack's log(sum + 1e-2) when already computed (register_stack(want_cn=True))"""
    if keep is None and NATIVE_SEG:
        return K.segment_ecoli_native(stack, image_cn)
    if image_cn is None:
        image_cn = K.channel_sum(stack, mode=1)                          # :71-72 log(sum + 1e-2)
    share = {}                                                           # one sort for both fits
    _, rough_mask, _, _ = K.kmeans_1d(image_cn, 2, want_labels=False, share=share, rule=2)  # :73-84 brighter
    _, interior, _, _ = K.kmeans_1d(image_cn, 3, want_labels=False, share=share, rule=0)    # :85-94 brightest
    opened = K.binary_opening(K.remove_small_holes(interior, 64, 1))      # :95
    cell_sm = K.remove_small_objects(opened, 50, conn=1)                 # :96
    be = erosion_seeds(cell_sm)                                          # :97-110
    seeds_mask = K.remove_small_objects(be, 10, conn=2)                  # :111 rso(label(dist_be), 10)
    seeds, nseeds = K.label(seeds_mask, conn=2)                          # :111-112
    seg = K.watershed(image_cn, seeds, rough_mask, negate=True)          # :113 watershed(-image_cn)
    seg = K.remove_small_objects(seg, 100, maxlab=nseeds)                # :114
    seg = K.clear_border(seg)                                            # :115
    props = K.region_props(seg, nseeds)                                  # :116 regionprops
    final = K.shape_filter(seg, props, nseeds, 15.0, 35.0)               # :117-126
    if keep is not None:
        keep.update(image_cn=image_cn, rough_mask=rough_mask, interior=interior, cell_sm=cell_sm, seeds=seeds,
                    watershed=seg)
    return final, nseeds


@dataclass
class Measurement:
    segmentation: torch.Tensor      # (H, W) int32 (labels not re-sequenced, as the reference)
    maxlab: int
    labels: torch.Tensor            # (N,) int32 label of each row (ascending, regionprops order)
    avgint: torch.Tensor            # (N, C) f64 per-cell mean spectrum
    avgint_norm: torch.Tensor       # (N, C) f64 max-normalised
    extras: dict = field(default_factory=dict)


def measure_ecoli(stack: torch.Tensor, calibration: torch.Tensor | None = None, keep: dict | None = None,
                  image_cn: torch.Tensor | None = None):
    """ecoli measurement.py:142-162: segment, flat-field channels 0..31 (load_calibration_images
    :33-38 puts the calibration image on channels 0-31 and 1.0 elsewhere), per-cell means."""
    if isinstance(stack, RegisteredTile):
        seg, maxlab = segment_ecoli(stack, keep, stack.image_cn)
        sums, counts = K.label_sums_lasers(stack.lasers, stack.shifts, seg, maxlab, stack.apply_mask,
                                           cal=calibration, cal_range=(0, 32))                   # :147-155
        _, lor, avgint, avgint_norm = K.cell_table(sums, counts, maxlab)                          # :151-157
        return Measurement(seg, maxlab, lor, avgint, avgint_norm)
    seg, maxlab = segment_ecoli(stack, keep, image_cn)
    sums, counts = K.label_sums(stack, seg, maxlab, cal=calibration,
                                cal_range=(0, 32) if calibration is not None else None)   # :147-155
    _, lor, avgint, avgint_norm = K.cell_table(sums, counts, maxlab)                      # :151-157
    return Measurement(seg, maxlab, lor, avgint, avgint_norm)


# --------------------------------------------------------------------------------------------
# Registration shift estimate
# --------------------------------------------------------------------------------------------
def estimate_shifts(lasers, reduce: str = "max", clamp: int | None = 15, device: bool = False):
    """Integer shift of every laser stack against the first, skimage register_translation
    (upsample 1) on a per-laser projection:
    * reduce "max": np.max(image, axis=2), |shift| > clamp -> 0 (ecoli measurement.py:45-57);
    * reduce "sum": np.sum(image, axis=2), no clamp (multispecies measurement.py:82-84);
    * reduce "logsum": np.log(np.sum(image, axis=2)), the correctly rounded log with no epsilon
      (biofilm :326-327; every channel sum must be positive).
    -> [(0, 0), (dr_1, dc_1), ...] ready for kernels.register_assemble; with `device` an
    (nlaser, 2) int32 device tensor instead (no host synchronisation; register_assemble reads
    it on the device)."""
    H, W = lasers[0].shape[:2]
    if reduce == "max" and len(lasers) <= 8:
        proj = K.channel_max_multi(lasers, stacked=True)                 # one launch for all lasers
        if device and len(lasers) >= 2 and XCORR and K.xcorr_supported(*proj.shape):
            return K.xcorr_shifts_dev(proj, clamp)                      # hand-written FFT pipeline
        proj = list(proj.unbind(0))
    elif reduce == "sum" and device and len(lasers) >= 2 and XCORR and K.xcorr_supported(len(lasers), H, W):
        proj = torch.empty((len(lasers), H, W), dtype=torch.float64, device=lasers[0].device)
        for i, s in enumerate(lasers):
            K.channel_sum(s, out=proj[i])                               # numpy's pairwise order
        return K.xcorr_shifts_dev(proj, clamp)
    elif reduce == "logsum":
        proj = [K.log(K.channel_sum(s)) for s in lasers]                # biofilm :326-327
    else:
        proj = [K.channel_max(s) if reduce == "max" else K.channel_sum(s) for s in lasers]
    if device:
        return K.register_translations_dev(proj[0], proj[1:], clamp)
    shifts = [(0, 0)]
    for img in proj[1:]:
        r, c = K.register_translation(proj[0], img)
        if clamp is not None:
            r = 0 if abs(r) > clamp else r
            c = 0 if abs(c) > clamp else c
        shifts.append((r, c))
    return shifts


def register_stack(lasers, reduce: str = "max", clamp: int | None = 15, apply_mask: bool = True,
                   want_cn: bool = False):
    """ecoli measurement.py:44-70 (-c T: plus load_calibration_images :33-38, applied to the
    per-cell spectra by measure_ecoli): shift estimate on the per-laser projections, then the
    registered, concatenated (H, W, C) stack -- one stream, no synchronisation.  want_cn: also
    image_cn = log(sum + 1e-2) of the registered stack (:71-72) from the assembly pass
    -> (stack, image_cn)."""
    return K.register_assemble(lasers, estimate_shifts(lasers, reduce, clamp, device=True), apply_mask,
                               cn_mode=1 if want_cn else None)


def register_multispecies(lasers, shifts=None):
    """multispecies measurement.py:79-102: the four acquisitions (488, 514, 561, 633) registered on
    their channel sums -- skimage register_translation(sum_0, sum_i), no clamp (:82-84) -- and
    concatenated with zeros outside each shifted frame and NO coverage-mask multiply (:85-102;
    the mask is built but never applied).  shifts: (n, 2) device tensor or host pairs to use
    instead of the estimate.  -> (H, W, C) f32 registered stack (one stream, no synchronisation)"""
    if shifts is None:
        shifts = estimate_shifts(lasers, reduce="sum", clamp=None, device=True)
    return K.register_assemble(lasers, shifts, apply_mask=False)


@dataclass
class RegisteredTile:
    """A registered E. coli tile that is never materialised as an (H, W, C) stack: the per-laser
    acquisitions with their device shifts, image_cn (:71-72) and the per-pixel classifier's
    prepared operands, all written by one assembly pass (register_tile).  process_tile classifies
    its pixels from the table and takes the per-cell spectra from the lasers
    (kernels.label_sums_lasers) -- the same results as register_stack + process_tile."""
    lasers: list
    shifts: torch.Tensor
    image_cn: torch.Tensor
    pixtable: object
    apply_mask: bool = True

    @property
    def shape(self):
        H, W = self.image_cn.shape
        return (H, W, self.pixtable.C)

    @property
    def device(self):
        return self.image_cn.device


def register_tile(lasers, reduce: str = "max", clamp: int | None = 15, apply_mask: bool = True):
    """register_stack(lasers, want_cn=True) without the stack (ecoli measurement.py:44-72): shift
    estimate on the device, then ONE pass over the lasers writing image_cn and the classifier's
    pixel table.  Needs the five E. coli lasers and W a multiple of 16; otherwise returns
    register_stack's (stack, image_cn)."""
    H, W = lasers[0].shape[:2]
    if len(lasers) != 5 or W % 16 or [int(l.shape[2]) for l in lasers] != [32, 23, 20, 14, 6]:
        return register_stack(lasers, reduce, clamp, apply_mask, want_cn=True)
    shifts = estimate_shifts(lasers, reduce, clamp, device=True)
    cn, pt, _ = K.register_assemble_pixtable(lasers, shifts, apply_mask, cn_mode=1, bounds=ECOLI_BOUNDS)
    return RegisteredTile(list(lasers), shifts, cn, pt, apply_mask)


# --------------------------------------------------------------------------------------------
# Biofilm z-stack registration (hiprfish_imaging_biofilm_analysis.py:134-165, :532-559)
# --------------------------------------------------------------------------------------------
# Power-of-two volumes of at least XCORR3_MIN_VOXELS voxels: the registration cross-correlations
# through xcorr.hip's 3-D pipeline instead of hipFFT (not slower in any alternating pair from
# 256 x 256 x 32 up); HRF_XCORR3=0 keeps hipFFT, HRF_XCORR3=1 takes it at every size
XCORR3 = os.environ.get("HRF_XCORR3", "")
XCORR3_MIN_VOXELS = 1 << 21


def estimate_shifts3(vols, clamp: int | None = None, xcorr: bool | None = None):
    """skimage register_translation(vols[0], vols[t]) (upsample_factor 1) for every t >= 1 on an
    (n, X, Y, Z) f64 tensor (or a list of (X, Y, Z) volumes) -> (n, 3) int32 device tensor of
    (sx, sy, sz), row 0 = 0; |component| > clamp -> 0.  xcorr True / False picks the hand-written
    pipeline (power-of-two sizes) / hipFFT; None: the hand-written one where the size is supported
    and the volume has at least XCORR3_MIN_VOXELS voxels."""
    if not isinstance(vols, torch.Tensor):
        vols = torch.stack(list(vols))
    if vols.shape[0] < 2:
        return torch.zeros((vols.shape[0], 3), dtype=torch.int32, device=vols.device)
    if xcorr is None:
        big = vols[0].numel() >= XCORR3_MIN_VOXELS
        xcorr = XCORR3 != "0" and (big or XCORR3 == "1") and K.xcorr3_supported(*vols.shape)
    return K.xcorr3_shifts_dev(vols, clamp) if xcorr else K.register3_translations_dev(vols, clamp)


def t_average_volume(tstack, want_shifts: bool = False, want_sum: str | None = None):
    """biofilm :134-165, get_registered_average_image_from_tstack: tstack a list of T
    (X, Y, Z, C) f32 time points of one laser.  Each is registered to t = 0 on the channel sums
    (np.sum(axis=3), numpy's order; no log, no clamp), shifted with zero fill, added in f64 in t
    order, divided by T and stored f32 -> (X, Y, Z, C) f32; T = 1 returns the time point's values.
    want_shifts: also the (T, 3) device shifts; want_sum "sum" / "log": also np.sum(out, axis=3) /
    log(sum + 1e-8) from the same pass.  Returns out, or (out[, shifts][, sum]).  One stream,
    nothing synchronises."""
    tstack = list(tstack)
    T = len(tstack)
    X, Y, Z, C = tstack[0].shape
    sums = torch.empty((T, X, Y, Z), dtype=torch.float64, device=tstack[0].device)
    if T > 1:
        for i, a in enumerate(tstack):
            K.channel_sum(a.reshape(X * Y, Z, C), out=sums[i].view(X * Y, Z))       # :137, :142
    shifts = estimate_shifts3(sums)                                               # :143
    res = K.volume_taverage(tstack, shifts, want_sum)                             # :144-165
    out, s = res if want_sum else (res, None)
    ret = (out,) + ((shifts,) if want_shifts else ()) + ((s,) if want_sum else ())
    return ret[0] if len(ret) == 1 else ret


def register_volume(lasers, fill: str = "keep", shifts=None, want_sum: bool = False, log_sums=None):
    """biofilm :536-558 (fill "keep", get_t_average_image) or :426-450 (fill "zero"): the averaged
    lasers, (X, Y, Z, C_l) f32 each, registered to the first on log(channel sum + 1e-8) (no clamp),
    shifted and concatenated on C -> (X, Y, Z, sum C_l) f32.  shifts: an (L, 3) device tensor or host
    triples to use instead of the estimate; log_sums: the (L, X, Y, Z) f64 registration images when
    already computed (t_average_volume(want_sum="log")); want_sum: also np.sum(out, axis=3) from
    the assembly pass -> (out, sum).  One stream, nothing synchronises."""
    lasers = list(lasers)
    if shifts is None:
        if log_sums is None:
            X, Y, Z = lasers[0].shape[:3]
            log_sums = torch.empty((len(lasers), X, Y, Z), dtype=torch.float64, device=lasers[0].device)
            for i, v in enumerate(lasers):
                K.volume_channel_sum(v, log=True, out=log_sums[i])                 # :536-537
        shifts = estimate_shifts3(log_sums)                                       # :537-538
    return K.volume_assemble(lasers, shifts, fill, "sum" if want_sum else None)   # :539-558


def register_volume_tstacks(tstacks, fill: str = "keep", want_sum: bool = False):
    """biofilm :532-559, get_t_average_image from raw acquisitions: tstacks[l] the list of time
    points of laser l.  Each laser is t-averaged (t_average_volume), the averages are registered and
    concatenated (register_volume) -> the registered (X, Y, Z, sum C_l) f32 stack (with want_sum
    also its channel sum, for segment_volume_stack(stack_sum=...))."""
    avg, logs = [], []
    for ts in tstacks:
        a, s = t_average_volume(ts, want_sum="log")
        avg.append(a)
        logs.append(s)
    return register_volume(avg, fill, want_sum=want_sum, log_sums=torch.stack(logs))


# --------------------------------------------------------------------------------------------
# Tiled 3-D mosaics (hiprfish_imaging_biofilm_analysis.py:1064-1172)
# --------------------------------------------------------------------------------------------
MOSAIC_MAX_TILES = 64


def tile_tsum(tstack, want_shifts: bool = False):
    """biofilm :203-236 and :1073-1076 on one mosaic tile: tstack a list of T (X, Y, Z, C) f32 time
    points.  The shifts are estimated exactly as t_average_volume does (channel sums in numpy's
    order, estimate_shifts3, no log, no clamp); the time points are shifted with zero fill, added
    in f64 in t order and summed over C -> (sum_filtered (X, Y, Z) f64, mask u8[, shifts]): the
    time sum times its coverage mask, and the mask (K.volume_tsum_masked).  One stream, nothing
    synchronises."""
    tstack = list(tstack)
    T = len(tstack)
    X, Y, Z, C = tstack[0].shape
    sums = torch.empty((T, X, Y, Z), dtype=torch.float64, device=tstack[0].device)
    if T > 1:
        for i, a in enumerate(tstack):
            K.channel_sum(a.reshape(X * Y, Z, C), out=sums[i].view(X * Y, Z))       # :206, :212
    shifts = estimate_shifts3(sums)                                               # :213
    s, m = K.volume_tsum_masked(tstack, shifts)                                   # :214-236, :1073-1076
    return (s, m, shifts) if want_shifts else (s, m)


def estimate_tile_shifts(sum_filtered_list, n: int, overlap: int = 50):
    """biofilm :1077-1087: the shift of every tile of an n x n mosaic against its neighbour on the
    `overlap`-voxel strips -> (n, n, 3) int32 device tensor.  Tile (0, 0): 0.  Column 0 of row
    i > 0: [Tx-ov:Tx, :, :] of tile (i-1, 0) against [0:ov, :, :] of tile (i, 0).  Every other
    tile: [:, Ty-ov:Ty, :] of its left neighbour against its own [:, 0:ov, :].  No clamp.  Strip
    sizes are no powers of two, so every pair goes through K.register3_translations_dev (hipFFT).
    Nothing synchronises."""
    tiles = list(sum_filtered_list)
    if n < 1 or len(tiles) != n * n:
        raise ValueError("estimate_tile_shifts: n * n tiles expected")
    Tx, Ty, Tz = tiles[0].shape
    ov = int(overlap)
    if not (1 <= ov <= min(Tx, Ty)):
        raise ValueError("estimate_tile_shifts: overlap must lie in 1..min(Tx, Ty)")
    out = torch.zeros((n, n, 3), dtype=torch.int32, device=tiles[0].device)         # :1077, :1081
    for i in range(n):
        for j in range(n):
            if i == 0 and j == 0:
                continue
            if j == 0:
                pair = (tiles[(i - 1) * n][Tx - ov:Tx], tiles[i * n][0:ov])         # :1083
            else:
                pair = (tiles[i * n + j - 1][:, Ty - ov:Ty], tiles[i * n + j][:, 0:ov])   # :1086
            out[i, j] = K.register3_translations_dev(torch.stack(pair))[1]
    return out


def mosaic_origins(shifts, tile_shape, overlap: int = 50, margin: int = 10):
    """biofilm :1092-1097 on the host: shifts an (n, n, 3) integer array -> (origins (n * n, 3)
    int32 in tile order k = i * n + j, canvas shape (n Tx + 2 m, n Ty + 2 m, Tz + 2 m)).  The sums
    are the reference's, with its asymmetry -- y and z do not accumulate column 0's shifts of
    earlier rows:
      x0 = i Tx - ov i + sum s[0:i+1, 0, 0] + sum s[i, 1:j+1, 0] + m
      y0 = j Ty - ov j + sum s[i, 0:j+1, 1] + m
      z0 = sum s[i, 0:j+1, 2] + m"""
    import numpy as np
    s = np.asarray(shifts, dtype=np.int64)
    n = s.shape[0]
    if s.shape != (n, n, 3):
        raise ValueError("mosaic_origins: an (n, n, 3) array of shifts expected")
    Tx, Ty, Tz = (int(v) for v in tile_shape)
    ov, m = int(overlap), int(margin)
    org = np.zeros((n * n, 3), dtype=np.int64)
    for i in range(n):
        for j in range(n):
            org[i * n + j] = (i * Tx - ov * i + s[0:i + 1, 0, 0].sum() + s[i, 1:j + 1, 0].sum() + m,
                              j * Ty - ov * j + s[i, 0:j + 1, 1].sum() + m,
                              s[i, 0:j + 1, 2].sum() + m)
    if np.abs(org).max() >= 2 ** 31:
        raise K._lib.HrfValueError("mosaic_origins: origin outside int32")
    return org.astype(np.int32), (n * Tx + 2 * m, n * Ty + 2 * m, Tz + 2 * m)


def stitch_volume_tiles(tile_tstacks, n: int, overlap: int = 50, margin: int = 10):
    """biofilm :1066-1102: tile_tstacks[k], k = i * n + j, the list of (X, Y, Z, C) f32 time
    points of tile (i, j) of an n x n mosaic.  Each tile is summed over time with its coverage mask
    (tile_tsum), registered to its neighbour on the overlap strips (estimate_tile_shifts), placed
    on one canvas (mosaic_origins) and averaged over the overlaps (K.mosaic_accumulate3); the
    canvas is divided by its maximum -> (norm (n Tx + 2 m, n Ty + 2 m, Tz + 2 m) f64, keep) with
    keep a dict of the stages: sum_filtered, masks, t_shifts, shifts, origins, full, count.

    Placement is decided on the host: the (n, n, 3) shifts are copied to the host once, which
    synchronises the stream -- the only synchronisation here.  A tile box that leaves the canvas,
    or more than 64 tiles, raises HrfValueError before the accumulation launches anything."""
    tile_tstacks = list(tile_tstacks)
    if n < 1 or len(tile_tstacks) != n * n:
        raise ValueError("stitch_volume_tiles: n * n tiles expected")
    if n * n > MOSAIC_MAX_TILES:
        raise K._lib.HrfValueError("stitch_volume_tiles: at most %d tiles (got %d)" % (MOSAIC_MAX_TILES, n * n))
    sums, masks, tsh = [], [], []
    for ts in tile_tstacks:
        s, m, sh = tile_tsum(ts, want_shifts=True)                                # :1069-1076
        sums.append(s)
        masks.append(m)
        tsh.append(sh)
    shifts = estimate_tile_shifts(sums, n, overlap)                               # :1077-1087
    origins, canvas = mosaic_origins(shifts.cpu().numpy(), sums[0].shape, overlap, margin)   # the one D2H copy
    full, count = K.mosaic_accumulate3(sums, masks, origins, canvas, want_count=True)        # :1088-1101
    norm = K.div_scalar(full, K.max_f64(full))                                    # :1102
    keep = dict(sum_filtered=sums, masks=masks, t_shifts=tsh, shifts=shifts, origins=origins, full=full, count=count)
    return norm, keep


def enhance_mosaic(norm: torch.Tensor, chunk: int | None = 100) -> torch.Tensor:
    """biofilm :1103-1126: edge pad 5 and the `+ 1e-8` chain in the reference's chunks -> image_final"""
    return K.enhance_3d_eps(K.pad_edge_3d(norm, 5), chunk)


def segment_volume_mosaic(tile_tstacks, n: int, overlap: int = 50, margin: int = 10, chunk: int | None = 100,
                          keep: dict | None = None):
    """biofilm :1064-1172, generate_3d_segmentation_tile_memory_efficient: stitch_volume_tiles,
    enhance_mosaic and segment_volume(background="log10eps_positive")
    -> (segmentation int32 relabelled 1..n_cells, n_cells, final_bkg_filtered f64, norm f64).
    keep: receives the stages of the stitch and of the segmentation, and final."""
    norm, st = stitch_volume_tiles(tile_tstacks, n, overlap, margin)
    final = enhance_mosaic(norm, chunk)
    if keep is not None:
        keep.update(st, norm=norm, final=final)
    seg, ncell, final_bkg = segment_volume(final, norm, keep, background="log10eps_positive")
    return seg, ncell, final_bkg, norm


# --------------------------------------------------------------------------------------------
# Biofilm 3-D enhancement input (hiprfish_imaging_biofilm_analysis.py:808-817)
# --------------------------------------------------------------------------------------------
def enhance_volume(stack: torch.Tensor, v3: bool = False) -> torch.Tensor:
    """biofilm :808-817 on the registered (X, Y, Z, C) volume: channel sum (numpy order),
    / max, edge pad 5, line_profile_memory_efficient_v2 (v3 with `v3`) and the
    average * (1 - quartile coefficient) post-chain -> image_final (X+10, Y+10, Z+10) f64"""
    return _enhance_norm(volume_sum_norm(stack), v3)


def volume_sum_norm(stack: torch.Tensor, stack_sum: torch.Tensor | None = None) -> torch.Tensor:
    """biofilm :808-809: the channel sum of the registered (X, Y, Z, C) volume (numpy order) over
    its maximum -> image_registered_sum (X, Y, Z) f64.  stack_sum: np.sum(stack, axis=3) when the
    registration already wrote it (register_volume(want_sum=True)); the stack is then not read"""
    X, Y, Z, C = stack.shape
    if stack_sum is not None:
        s = K._dev(stack_sum, torch.float64, "stack_sum")
        if tuple(s.shape) != (X, Y, Z):
            raise ValueError("volume_sum_norm: stack_sum must be the (X, Y, Z) channel sum of the stack")
    else:
        s = K.channel_sum(stack.reshape(X * Y, Z, C)).reshape(X, Y, Z)     # :808
    return K.div_scalar(s, K.max_f64(s))                                # :809


def _enhance_norm(s: torch.Tensor, v3: bool = False) -> torch.Tensor:
    pad = K.pad_edge_3d(s, 5)                                           # :810
    return K.enhance_3d_v3(pad) if v3 else K.enhance_3d(pad)            # :811-817


# --------------------------------------------------------------------------------------------
# Biofilm 3-D segmentation (hiprfish_imaging_biofilm_analysis.py:818-859, :489-499)
# --------------------------------------------------------------------------------------------
def segment_volume(final: torch.Tensor, reg_sum: torch.Tensor, keep: dict | None = None, adjacency: bool = False,
                   background: str = "log10p1"):
    """biofilm :818-859 on image_final and the normalised registered sum, both (X, Y, Z) f64.
    -> (segmentation int32 relabelled 1..n, n, final_bkg_filtered f64[, adjacency_seg, n_adj])

    background "log10p1" (the default): the background filter of :845-854 as described below.
    background "log10eps_positive": the mosaic's, :1154-1165 (:1127-1153 are :818-844 again) --
    KMeans k = 2 on log10(reg_sum + 1e-8) (the correctly rounded log10), fitted only where
    reg_sum > 0; the cluster means are taken on reg_sum itself, all of them positive, and 1-D
    clusters are intervals, so the cluster with the larger mean of reg_sum is the one with the
    larger centre in log10 and `i0 < i1` fails only when cluster 1 is empty (a NaN mean): the larger
    cluster when both are non-empty, else cluster 0 -- rule 2.  Both branches of :1161-1165 leave
    the mask false wherever reg_sum <= 0 (the margins and the voxels no tile covers).

    The KMeans cluster choices, read off the reference's comparisons of cluster means:
    :819-828 (k = 2 on final > 0) takes the cluster with the larger mean, sklearn's cluster 0 when
    the comparison is not `i0 < i1` -- every fitted value is positive, so this is rule 2;
    :830-838 (k = 3, same values, the sort shared) takes argmax of the means -- rule 0;
    :846-854 (k = 2 on log10(sum + 1), all voxels) averages the positive sums of each cluster and
    falls to cluster 0 on a NaN mean, log10(sum + 1) > 0 exactly where sum > 0 -- rule 1.
    adjacency: also the flood of :489, :497-499, watershed(-(reg_sum * bkg), seeds * bkg, mask=bkg),
    relabelled -- unlike :858, where the seeds are the label of the very mask passed in and no
    voxel is left to flood, this one does the flood's real work."""
    final = K._dev(final, torch.float64, "final")
    reg_sum = K._dev(reg_sum, torch.float64, "reg_sum")
    if final.dim() != 3 or final.shape != reg_sum.shape:
        raise ValueError("segment_volume: final and reg_sum must be (X, Y, Z) volumes of one shape")
    if background not in ("log10p1", "log10eps_positive"):
        raise ValueError("segment_volume: background must be 'log10p1' or 'log10eps_positive'")
    pos = final > 0
    share: dict = {}
    _, rough, cen2, _ = K.kmeans_1d(final, 2, valid=pos, want_labels=False, share=share, rule=2)    # :818-828
    _, rsf, cen3, _ = K.kmeans_1d(final, 3, valid=pos, want_labels=False, share=share, rule=0)      # :829-838
    opened = K.binary_opening3(rsf, border_value=0)                                 # :839 scipy's opening
    small = K.remove_small_objects3(opened, 10, conn=1)                             # :840
    bfh = K.fill_holes3(small)                                                      # :841
    rough_bfh = K.fill_holes3(rough)                                                # :842
    wmask = K.and_mask(bfh, rough_bfh)                                              # :843
    seeds, nseeds = K.label3(wmask, conn=3)                                         # :844
    if background == "log10p1":
        logsum = K.log10p1(reg_sum)          # :845, the correctly rounded log10 of channel_sum(mode=2)
        _, bkg, cenb, _ = K.kmeans_1d(logsum, 2, want_labels=False, rule=1)         # :846-854
    else:
        logsum = K.log10(reg_sum + 1e-8)                                            # :1154
        _, bkg, cenb, _ = K.kmeans_1d(logsum, 2, valid=reg_sum > 0, want_labels=False, rule=2)   # :1155-1165
    final_bkg = K.mask_mul(final, bkg)                                              # :855
    seeds_bkg = K.mask_labels(seeds, bkg)                                           # :856
    wmask_bkg = K.and_mask(wmask, bkg)                                              # :857
    ties: list = []
    ws = K.watershed3(final_bkg, seeds_bkg, wmask_bkg, negate=True, ties=ties)      # :858
    seg, n = K.relabel_sequential(ws, nseeds)                                       # :859
    out = (seg, n, final_bkg)
    adj = None
    if adjacency:
        ties_adj: list = []
        sum_bkg = K.mask_mul(reg_sum, bkg)                                          # :489
        aws = K.watershed3(sum_bkg, seeds_bkg, bkg, negate=True, ties=ties_adj)     # :497
        adj, n_adj = K.relabel_sequential(aws, nseeds)                              # :499
        out = out + (adj, n_adj)
    if keep is not None:
        keep.update(rough_mask=rough, rsf=rsf, opened=opened, small=small, bfh=bfh, rough_bfh=rough_bfh,
                    watershed_mask=wmask, seeds=seeds, nseeds=nseeds, logsum=logsum, bkg_mask=bkg,
                    final_bkg=final_bkg, seeds_bkg=seeds_bkg, watershed_mask_bkg=wmask_bkg, watershed=ws,
                    centers2=cen2, centers3=cen3, centers_bkg=cenb, ties=ties)
        if adjacency:
            keep.update(adjacency_watershed=aws, adjacency_seg=adj, ties_adjacency=ties_adj)
    return out


def segment_volume_stack(stack: torch.Tensor, keep: dict | None = None, adjacency: bool = False, v3: bool = False,
                         stack_sum: torch.Tensor | None = None):
    """biofilm :808-859 from the registered (X, Y, Z, C) volume: enhance_volume, then
    segment_volume on image_final and the normalised sum it was made from.  stack_sum: the stack's
    channel sum when register_volume(want_sum=True) already wrote it"""
    s = volume_sum_norm(stack, stack_sum)
    final = _enhance_norm(s, v3)
    if keep is not None:
        keep.update(reg_sum=s, final=final)
    return segment_volume(final, s, keep, adjacency)


def measure_volume(stack: torch.Tensor, seg: torch.Tensor, n: int):
    """per-label mean spectra of a segmented (X, Y, Z, C) volume (regionprops mean_intensity per
    channel) and their row-max normalisation, through the flat label_sums / cell_table"""
    X, Y, Z, C = stack.shape
    sums, counts = K.label_sums(stack.reshape(X * Y, Z, C), seg.reshape(X * Y, Z), n)
    _, lor, avgint, avgint_norm = K.cell_table(sums, counts, n)
    return Measurement(seg, n, lor, avgint, avgint_norm)


# --------------------------------------------------------------------------------------------
# Biofilm 2-D registration and segmentation (hiprfish_imaging_biofilm_analysis.py:322-419)
# --------------------------------------------------------------------------------------------
def register_biofilm_2d(lasers, shifts=None):
    """biofilm :323-346: the acquisitions (488, 514, 561, 633) registered against the first on
    log(channel sum) -- skimage register_translation(log(sum_0), log(sum_i)), the correctly rounded
    log, no clamp and no epsilon (:326-327) -- and concatenated with zeros outside each shifted
    frame; the coverage mask is built but never applied (:345), as in register_multispecies.
    shifts: (n, 2) device tensor or host pairs to use instead of the estimate.
    -> (H, W, C) f32 registered stack (one stream, no synchronisation)

    The reference takes shape[0] for both axes (:331), so it is right for square images only; here
    every laser is shifted inside its own (H, W) frame, H != W included.
    Precondition, not checked: every channel sum is positive (a zero gives log -inf, and the
    reference's FFT then yields NaN shifts)."""
    if shifts is None:
        shifts = estimate_shifts(lasers, reduce="logsum", clamp=None, device=True)
    return K.register_assemble(lasers, shifts, apply_mask=False)


def segment_biofilm_2d(stack: torch.Tensor, keep: dict | None = None, epithelial: bool = True,
                       disk_radius: int = 100, bkg_min_size: int = 10000):
    """biofilm :347-418 (generate_2d_segmentation after the registration) on the registered
    (H, W, C) stack.
    -> (segmentation int32 relabelled 1..n, n, adjacency_seg int32 relabelled 1..n_adj, n_adj,
        image_registered_sum f64, image_final_bkg_filtered f64, epithelial area u8 or None)

    Cluster choices.  :367-377 (k = 2 on image_final) keeps the cluster whose positive values have
    the larger mean, sklearn's cluster 0 on a NaN mean: kernels.kmeans_1d rule 1, as in
    segment_multispecies.  :384-392 fits k = 2 on log10(nl) but compares i0, i1 = the means of the
    raw registered sum over each cluster's positive pixels (kernels.cluster_positive_means; NaN for
    a cluster without one) and keeps cluster 1 iff i0 < i1, else cluster 0.  The sums are
    fixed-order tree sums, not numpy's pairwise sum over the boolean-compacted array: i0 and i1 can
    differ from the reference's in the last bits, which matters only if they are equal to ~1e-15.
    image_final_bkg_filtered is nl * mask (:393), not image_final * mask as in the multispecies
    script.  The seeds of :399 / :400 are not multiplied by the flood mask (kernels.watershed floods
    from markers outside it as skimage does).
    An nl value <= 0 makes log10 -inf or NaN and the reference's KMeans raise: ValueError here.
    epithelial: :404-418, the tissue side of the field -- the background of at least bkg_min_size
    pixels, hole-filled, closed and then dilated by disk(disk_radius), the largest object of the
    unmasked flood of -image_registered_sum from label(1 - dilated) taken as the biofilm and
    everything else as epithelium.  Where the reference dies on argmax of an empty list (no
    background component survives, or the dilated background covers the image) ValueError names
    the stage.  False skips :404-418 and returns None.
    keep: receives every intermediate by name, with the [contested, rounds, marker ties] lists of
    the three floods (ties, ties_adjacency, ties_epithelial)."""
    stack = K._dev(stack, torch.float32, "stack")
    if stack.dim() != 3:
        raise ValueError("segment_biofilm_2d: an (H, W, C) registered stack expected")
    s = K.channel_sum(stack)                                                 # :347
    norm = K.div_scalar(s, K.max_f64(s))                                     # :348
    nl = K.nl_means_2d(norm, 7, 11, 0.02, 0.0)                               # :350 (:349 unused)
    nonpos = K.count_nonzero(~(nl > 0))                                      # one count, before any fit
    if nonpos:
        raise ValueError("segment_biofilm_2d: %d pixels of the NL-means image are not positive, log10 is "
                         "not finite there (:383-384)" % nonpos)
    final = K.enhance_2d(K.pad_edge(nl, 5))                                  # :351-366
    _, rough, cen_rough, _ = K.kmeans_1d(final, 2, want_labels=False, rule=1)    # :367-377
    opened = K.binary_opening(rough)                                         # :378
    small = K.remove_small_objects(opened, 10, conn=1)                       # :379
    bfh = K.fill_holes(small)                                                # :380
    rough_bfh = K.fill_holes(rough)                                          # :381
    wmask_rough = K.and_mask(bfh, rough_bfh)                                 # :382
    nl_log = K.log10(nl)                                                     # :383
    blabels, _, cen_bkg, _ = K.kmeans_1d(nl_log, 2, want_labels=True)        # :384
    sums, counts = K.cluster_positive_means(blabels, s, 2)                   # :385-388
    i0, i1 = (sums / counts.double()).tolist()                               # 0 / 0 = NaN
    bkg = (blabels == (1 if i0 < i1 else 0)).to(torch.uint8)                 # :389-392
    final_bkg = K.mask_mul(nl, bkg)                                          # :393
    sum_bkg = K.mask_mul(s, bkg)                                             # :394
    wmask = K.remove_small_objects(K.and_mask(wmask_rough, bkg), 10, conn=1)     # :395-396
    seeds, nseeds = K.label(wmask, conn=2)                                   # :397
    flood_mask = K.and_mask(rough, bkg)                                      # :398
    ties: list = []
    ties_adj: list = []
    ws = K.watershed(final_bkg, seeds, flood_mask, negate=True, ties=ties)   # :399
    aws = K.watershed(sum_bkg, seeds, bkg, negate=True, ties=ties_adj)       # :400
    seg, n = K.relabel_sequential(ws, nseeds)                                # :401
    adj, n_adj = K.relabel_sequential(aws, nseeds)                           # :402
    if keep is not None:
        keep.update(image_sum=s, norm=norm, nl=nl, final=final, rough_mask=rough, opened=opened, small=small,
                    bfh=bfh, rough_bfh=rough_bfh, nl_log=nl_log, bkg_labels=blabels, cluster_means=(i0, i1),
                    bkg_mask=bkg, final_bkg=final_bkg, sum_bkg=sum_bkg, watershed_mask=wmask, seeds=seeds,
                    nseeds=nseeds, flood_mask=flood_mask, watershed=ws, adjacency_watershed=aws, seg=seg,
                    adjacency_seg=adj, centers_rough=cen_rough, centers_bkg=cen_bkg, ties=ties,
                    ties_adjacency=ties_adj)
    epi = None
    if epithelial:
        image_bkg = K.remove_small_objects(bkg == 0, bkg_min_size, conn=1)   # :404-405
        image_bkg_bfh = K.fill_holes(image_bkg)                              # :406
        closed = K.binary_closing_disk(image_bkg_bfh, disk_radius)           # :407-408
        objects, nobj = K.label(closed, conn=2)                              # :409
        big, _ = K.largest_label(objects, nobj)                              # :410-412
        if big == 0:
            raise ValueError("segment_biofilm_2d: no background component of %d pixels or more, the epithelial "
                             "area's background is empty (:405-412)" % bkg_min_size)
        bkg_final = (objects == big).to(torch.uint8)                         # :412
        dilated = K.binary_dilation_disk(bkg_final, disk_radius)             # :413
        overall, nover = K.label(1 - dilated, conn=2)                        # :414
        if nover == 0:
            raise ValueError("segment_biofilm_2d: the background dilated by disk(%d) covers the image, no object "
                             "is left to flood from (:414-418)" % disk_radius)
        ties_epi: list = []
        overall_seg = K.watershed(s, overall, None, negate=True, ties=ties_epi)   # :415
        biggest, _ = K.largest_label(overall_seg, nover)                     # :416-418
        epi = (overall_seg != biggest).to(torch.uint8)                       # :418
        if keep is not None:
            keep.update(image_bkg=image_bkg, image_bkg_bfh=image_bkg_bfh, bkg_closed=closed, bkg_objects=objects,
                        bkg_final=bkg_final, bkg_dilated=dilated, objects_overall=overall,
                        objects_overall_seg=overall_seg, epithelial_area=epi, ties_epithelial=ties_epi)
    return seg, n, adj, n_adj, s, final_bkg, epi


# --------------------------------------------------------------------------------------------
# Synthetic-community measurement (hiprfish_imaging_multispecies_spectral_image_measurement.py)
# --------------------------------------------------------------------------------------------
def segment_multispecies(stack: torch.Tensor, calibration: torch.Tensor | None = None, keep: dict | None = None):
    """multispecies measurement.py:102-157 on the registered (H, W, C) stack.
    -> (segmentation int32 relabelled 1..n, n, registered sum f64, final_bkg_filtered f64)

    The two KMeans(2) cluster choices (:125-135, :141-149) take the cluster whose positive
    values have the larger mean -- for a 1-D partition into intervals the upper one -- and
    sklearn's cluster 0 when one of them holds no positive value (the reference compares a NaN
    mean then): kernels.kmeans_1d rule 1."""
    if keep is None and NATIVE_SEG:
        return K.segment_multispecies_native(stack, calibration)
    s = K.channel_sum(stack, cal=calibration)                    # :104-105 sum(stack / cal)
    norm = K.div_scalar(s, K.max_f64(s))                         # :106
    nl = K.nl_means_2d(norm, 7, 11, 0.02, 0.0)                   # :108 (estimate_sigma :107 unused)
    final = K.enhance_2d(K.pad_edge(nl, 5))                      # :109-124
    _, rough, _, _ = K.kmeans_1d(final, 2, want_labels=False, rule=1)    # :125-135
    opened = K.remove_small_objects(K.binary_opening(rough), 10, conn=1)   # :136-137
    seeds_mask = K.and_mask(K.fill_holes(opened), K.fill_holes(rough))     # :138-140
    seeds, nseeds = K.label(seeds_mask, conn=2)                  # :140 measure.label (8-conn)
    _, bkg, _, _ = K.kmeans_1d(nl, 2, want_labels=False, rule=1)         # :141-149
    final_bkg = K.mask_mul(final, bkg)                           # :150
    seeds_bkg = K.mask_labels(seeds, bkg)                        # :152
    wmask = K.and_mask(rough, bkg)                               # :153
    seg = K.watershed(final_bkg, seeds_bkg, wmask, negate=True)  # :154 watershed(-final_bkg)
    seg = K.remove_small_objects(seg, 60, maxlab=nseeds)         # :155
    seg = K.clear_border(seg)                                    # :156
    seg, n = K.relabel_sequential(seg, nseeds)                   # :157
    if keep is not None:
        keep.update(image_sum=s, nl=nl, final=final, rough_mask=rough, seeds=seeds, bkg_mask=bkg,
                    watershed=seg)
    return seg, n, s, final_bkg


def measure_multispecies(stack: torch.Tensor, calibration: torch.Tensor | None = None, keep: dict | None = None):
    """multispecies measurement.py:161-174: segment, per-cell mean of the calibrated stack
    (regionprops mean_intensity per channel, :167-171), row-max normalisation (:172)."""
    seg, n, s, final_bkg = segment_multispecies(stack, calibration, keep)
    sums, counts = K.label_sums(stack, seg, n, cal=calibration)
    _, lor, avgint, avgint_norm = K.cell_table(sums, counts, n)
    return Measurement(seg, n, lor, avgint, avgint_norm, extras=dict(image_sum=s, final_bkg=final_bkg))


# --------------------------------------------------------------------------------------------
# Classification (segmented cosine against a reference library)
# --------------------------------------------------------------------------------------------
@dataclass
class Library:
    """Reference barcode library: row r is barcode r + 1 (mean spectrum of enc_{r+1},
    train_reference.py:1397), max-normalised."""
    spectra: torch.Tensor        # (R, C) f64
    bounds: tuple
    nbit: int
    _refx: torch.Tensor | None = None
    _refx2: torch.Tensor | None = None
    _flags: dict = field(default_factory=dict)

    @property
    def R(self):
        return self.spectra.shape[0]

    def refx(self):
        """the per-pixel classifier's prepared library.  It is made from spectra ROUNDED TO F32:
        per pixel the answers are exact against spectra.to(float32), not against the f64 rows
        (which the per-cell classifier reads as they are).  R <= 4096, C <= 128; a tile must hold
        H * W * C < 2^31 values (kernels.classify_pixels)."""
        if self._refx is None:
            self._refx = K.classify_prepare(self.spectra.to(torch.float32), self.bounds)
        return self._refx

    def refx_table(self):
        """the mode-2 table the pixel-table classifier (register_tile, process_tile_native) reads,
        whatever mode refx() was prepared in"""
        r = self.refx()
        if K.refx_mode(r, self.spectra.shape[1], self.bounds) == 2:
            return r
        if self._refx2 is None:
            self._refx2 = K.classify_prepare(self.spectra.to(torch.float32), self.bounds, mode=2)
        return self._refx2

    def presence_flags(self, thr: float = 0.1) -> torch.Tensor:
        """per-segment presence of the library rows (max over the segment > thr), computed once
        per threshold"""
        f = self._flags.get(thr)
        if f is None:
            f = self._flags[thr] = segment_flags(self.spectra, self.bounds, thr)
        return f


def segment_flags(x: torch.Tensor, bounds, thr: float = 0.1) -> torch.Tensor:
    """the gated metrics' presence flags on the library path: max over each segment > thr
    (hrf_segment_flags)"""
    return K.segment_flags(x, bounds, thr)


def classify_cells(avgint_norm: torch.Tensor, lib: Library, variant: int = 0, flag_thr: float = 0.1):
    """image_classification.py:43-56 / classify_spectra.py:27-35 restated on the max-normalised
    cell spectra (hrf_cell_table computes avgint / rowmax, :43): argmin of the segmented-cosine
    distance over the library.  variant 0: ungated mean of segment distances; 1:
    channel_cosine_intensity gating (train_reference.py:223-386); 2: _7b_v2 gating
    (:993-1072).  -> (index, distance)"""
    x = avgint_norm
    fx = fr = None
    if variant:
        fx = segment_flags(x, lib.bounds, flag_thr)
        fr = lib.presence_flags(flag_thr)
    return K.classify_cells(x, lib.spectra, lib.bounds, variant, fx, fr)


def classify_pixels(stack: torch.Tensor, lib: Library):
    """north_star per-pixel mode: argmin over the library of the ungated segmented-cosine
    distance for every pixel spectrum (a split-fp16 MFMA screen with a fused argmax, then the f64
    certificate and list pass: the restatement's exact answer)."""
    return K.classify_pixels(stack, lib.refx(), lib.R, lib.bounds)


def barcode_strings(idx, nbit: int):
    """barcode number = library row + 1, written as the reference's binary code string"""
    return [format(int(i) + 1, "0%db" % nbit) for i in idx]


@dataclass
class TileResult:
    meas: Measurement
    cell_idx: torch.Tensor
    cell_dist: torch.Tensor
    counts: torch.Tensor
    identification: torch.Tensor
    pixel_idx: torch.Tensor | None = None
    pixel_dist: torch.Tensor | None = None


_SIDE_STREAMS: "OrderedDict" = OrderedDict()
SIDE_PRIORITY = 0   # stream priority of the classifier side streams (torch convention: lower = higher)
SIDE_STREAMS_MAX = 64


def _side_stream(main: torch.cuda.Stream) -> torch.cuda.Stream:
    """the side stream paired with `main` (one per caller stream, so concurrent tiles on
    different streams do not serialise on a shared one); the least recently used beyond
    SIDE_STREAMS_MAX are dropped (work queued on them is held by the events their callers joined)"""
    key = (main.device, main.cuda_stream, SIDE_PRIORITY)
    s = _SIDE_STREAMS.get(key)
    if s is None:
        s = _SIDE_STREAMS[key] = torch.cuda.Stream(device=main.device, priority=SIDE_PRIORITY)
        while len(_SIDE_STREAMS) > SIDE_STREAMS_MAX:
            _SIDE_STREAMS.popitem(last=False)
    else:
        _SIDE_STREAMS.move_to_end(key)
    return s


@dataclass
class PendingTile:
    """A tile whose per-pixel classification is enqueued (start_tile) and whose measurement is
    not yet (finish_tile)."""
    stack: object
    lib: Library
    main: torch.cuda.Stream
    side: torch.cuda.Stream | None
    pix: tuple | None
    overlap: bool


def process_tile(stack: torch.Tensor, lib: Library, calibration=None, per_pixel: bool = True, variant: int = 0,
                 overlap: bool = True, pixel_events: list | None = None, measure=None, image_cn=None):
    """One tile of the hot path: measure (segment + per-cell spectra) + classify + count.

    The per-pixel classification does not depend on the segmentation, so with `overlap` it
    runs on a side stream concurrently with the segmentation chain (many small, latency-bound
    launches and a few host synchronisations) and fills the compute units that chain leaves
    idle; the caller's stream joins it before returning.  `pixel_events`, if given, receives
    the (start, end) events recorded around the classification on the stream it ran on.
    `measure` selects the measurement chain (default measure_ecoli; measure_multispecies for
    the synthetic-community pipeline); `image_cn` hands measure_ecoli the log-sum image the
    registration pass already produced.  `stack` may be a RegisteredTile (register_tile): the
    pixels are then classified from its prepared table and the per-cell spectra read from its
    lasers.  process_tile = finish_tile(start_tile(...)); a caller driving a sequence of tiles
    may start tile i+1 before finishing tile i, so that tile's classifier is queued while tile
    i's segmentation chain runs."""
    p = start_tile(stack, lib, per_pixel, overlap, pixel_events)
    return finish_tile(p, calibration, variant, measure, image_cn)


def start_tile(stack, lib: Library, per_pixel: bool = True, overlap: bool = True,
               pixel_events: list | None = None) -> PendingTile:
    """first half of process_tile: enqueue the per-pixel classification (side stream with
    `overlap`, after everything the caller's stream holds so far, i.e. the stack / table)"""
    main = torch.cuda.current_stream(stack.device)
    reg = isinstance(stack, RegisteredTile)
    pix = None
    side = None
    if per_pixel:
        refx = lib.refx_table() if reg else lib.refx()        # prepared on the caller's stream
        side = _side_stream(main) if overlap else main
        if overlap:
            side.wait_stream(main)                            # stack (and refx) ready
        with torch.cuda.stream(side):
            e0 = e1 = None
            if pixel_events is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side)
            if reg:                                           # from the assembly's pixel table
                pix = K.classify_pixels_table(stack.pixtable, refx, lib.R)
            else:
                pix = K.classify_pixels(stack, refx, lib.R, lib.bounds)
            if pixel_events is not None:
                e1.record(side)
                pixel_events.append((e0, e1))
        if overlap:
            if reg:
                stack.pixtable.table.record_stream(side)
                stack.pixtable.flags.record_stream(side)
            else:
                stack.record_stream(side)
            refx.record_stream(side)
    return PendingTile(stack, lib, main, side, pix, overlap)


def finish_tile(p: PendingTile, calibration=None, variant: int = 0, measure=None, image_cn=None) -> TileResult:
    """second half of process_tile, on the stream start_tile was called on: measurement,
    per-cell classification, counts, identification map, then the join with the per-pixel
    classification"""
    stack, lib, main, side, pix, overlap = p.stack, p.lib, p.main, p.side, p.pix, p.overlap
    per_pixel = pix is not None
    reg = isinstance(stack, RegisteredTile)
    if reg:
        meas = measure_ecoli(stack, calibration)
    elif image_cn is not None:
        meas = (measure or measure_ecoli)(stack, calibration, image_cn=image_cn)
    else:
        meas = (measure or measure_ecoli)(stack, calibration)
    idx, dist = classify_cells(meas.avgint_norm, lib, variant)
    counts = K.barcode_counts(idx, lib.R)                       # collect_measurement_results.py:92-98
    ident = K.paint_ids(meas.segmentation, idx + 1)             # image_classification.py:65-71
    res = TileResult(meas, idx, dist, counts, ident)
    if per_pixel:
        if overlap:
            main.wait_stream(side)
            for t in pix:
                t.record_stream(main)
        res.pixel_idx, res.pixel_dist = pix
    return res


class NativeTileResult:
    """TileResult of process_tile_native: the per-cell rows are narrowed to the tile's cell count
    on first access (one read of the device-held count); counts, the identification map and
    the per-pixel outputs need no host round trip."""

    def __init__(self, d):
        self._d = d
        self._n = None
        self.counts = d["counts"]
        self.identification = d["ident"]
        self.pixel_idx = d["pixel_idx"]
        self.pixel_dist = d["pixel_dist"]

    @property
    def ncells(self) -> int:
        if self._n is None:
            self._n = int(self._d["ncells"].item())
        return self._n

    @property
    def cell_idx(self):
        return self._d["cell_idx"][:self.ncells]

    @property
    def cell_dist(self):
        return self._d["cell_dist"][:self.ncells]

    @property
    def meas(self) -> Measurement:
        d, n = self._d, self.ncells
        return Measurement(d["seg"], d["maxlab"], d["labels"][:n], d["avgint"][:n], d["avgint_norm"][:n])


def process_tile_native(lasers, lib: Library, calibration=None, per_pixel: bool = True, variant: int = 1,
                        overlap: bool = True, pixel_events: list | None = None) -> NativeTileResult:
    """register_tile(lasers) + process_tile(..., variant) as ONE native call (hrf_tile_ecoli,
    tile.hip): ecoli measurement.py:44-162 (-c T) + image_classification.py:43-71 + collect
    :92-98, the per-pixel classifier on the side stream with `overlap`.  The same results as the
    composed path bit for bit (tests/test_tile_gpu.py).  lasers: the five E. coli acquisitions
    (W a multiple of 16; the registration FFT is xcorr.hip for power-of-two H and W, hipFFT
    otherwise)."""
    main = torch.cuda.current_stream(lasers[0].device)
    side = _side_stream(main) if (per_pixel and overlap) else None
    refx = lib.refx_table() if per_pixel else None
    flags = lib.presence_flags() if variant else None
    d = K.tile_ecoli(lasers, calibration, refx, lib.spectra, flags, variant=variant, per_pixel=per_pixel, side=side,
                     pix_events=pixel_events)
    return NativeTileResult(d)


# --------------------------------------------------------------------------------------------
# Multi-GPU: tiles shard round-robin; the only exchange is the per-barcode count vector
# --------------------------------------------------------------------------------------------
def shard(n_tiles: int, rank: int, world: int):
    """tile indices owned by `rank` (tile_idx % world)"""
    return list(range(rank, n_tiles, world))


def allreduce_counts(counts: torch.Tensor, group=None) -> torch.Tensor:
    """global per-barcode counts = SUM over ranks (collect_measurement_results.py:92-98 across
    FOVs).  RCCL on device tensors; any torch.distributed backend works."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=group)
    return counts


def allreduce_adjacency(adj: torch.Tensor, group=None) -> torch.Tensor:
    """the optional second exchange: the int64 (R, R) barcode adjacency summed over
    ranks, one all-reduce of R*R*8 bytes per job"""
    return allreduce_counts(adj, group)


# --------------------------------------------------------------------------------------------
# Biofilm cell typing and the filtered adjacency (biofilm_analysis.py:1259-1295, row f4)
# --------------------------------------------------------------------------------------------
@dataclass
class CellTyping:
    is_cell: torch.Tensor          # (N,) u8 per cell row: 1 'cell', 0 'debris'
    debris_labels: torch.Tensor    # (maxlab + 1,) u8: labels overlapping the epithelial area
    adjacency: torch.Tensor        # (R, R) int64
    adjacency_filtered: torch.Tensor


def biofilm_typing_and_adjacency(segmentation: torch.Tensor, adjacency_seg: torch.Tensor, bc_idx: torch.Tensor,
                                 R: int, max_probability: torch.Tensor | None = None,
                                 epithelial_area: torch.Tensor | None = None, area_max: float = 10000.0,
                                 prob_min: float = 0.95) -> CellTyping:
    """cell rows = the labels of `segmentation` in ascending order (regionprops), bc_idx their
    barcode index in the (R, R) matrices (-1: not counted).  As the reference, row i stands for
    node i + 1 of the adjacency graph of `adjacency_seg` (:1285-1290 index cell_info by
    node - 1), so the labels are expected to be sequential."""
    seg = segmentation.to(torch.int32).contiguous()
    maxlab = int(seg.max().item()) if seg.numel() else 0
    props = K.region_props(seg, maxlab)
    present = props[1:, 7] > 0
    labels = (torch.nonzero(present).flatten() + 1).to(torch.int32)
    area = props[1:, 0][present].contiguous()
    overlap = None
    if epithelial_area is not None:
        overlap = K.label_overlap(seg, epithelial_area, maxlab)                       # :1259-1262
    is_cell = K.cell_typing(labels, area, max_probability, overlap, maxlab, area_max, prob_min)   # :1263-1269
    aseg = adjacency_seg.to(torch.int32).contiguous()
    amax = int(aseg.max().item()) if aseg.numel() else 0
    edge = K.rag_edges(aseg, amax)                                                    # :1277-1278
    n = labels.numel()
    bc = torch.full((amax + 1,), -1, dtype=torch.int32, device=seg.device)
    keep = torch.zeros(amax + 1, dtype=torch.uint8, device=seg.device)
    m = min(n, amax)
    bc[1:m + 1] = bc_idx[:m].to(torch.int32)
    keep[1:m + 1] = is_cell[:m]
    adj, adjf = K.barcode_adjacency_filtered(edge, bc, keep, R)                       # :1283-1295
    return CellTyping(is_cell, overlap if overlap is not None else torch.zeros(maxlab + 1, dtype=torch.uint8,
                                                                              device=seg.device), adj, adjf)


def biofilm_typing_and_adjacency3(segmentation: torch.Tensor, adjacency_seg: torch.Tensor, bc_idx: torch.Tensor,
                                  R: int, max_probability: torch.Tensor | None = None, area_max: float = 100000.0,
                                  prob_min: float = 0.95, conn: int = 2) -> CellTyping:
    """biofilm_typing_and_adjacency on (X, Y, Z) volumes (measure_biofilm_images_3d, :1359-1417):
    rows = the labels of `segmentation` ascending, row i standing for node i + 1 of the adjacency
    graph of `adjacency_seg`.  The 3-D rule is :1411 -- debris when area > 100000 or max_probability
    <= 0.95; its loop never consults debris_labels (image_epithelial_area is not defined there), so
    debris_labels comes back all zero.  The graph is rag_boundary's with its default connectivity 2
    (conn), held as a sparse edge set: no label limit."""
    seg = segmentation.to(torch.int32).contiguous()
    maxlab = int(seg.max().item()) if seg.numel() else 0
    props = K.region_props3(seg, maxlab)
    present = props[1:, 4] > 0
    labels = (torch.nonzero(present).flatten() + 1).to(torch.int32)
    area = props[1:, 0][present].contiguous()
    is_cell = K.cell_typing(labels, area, max_probability, None, maxlab, area_max, prob_min)      # :1411
    aseg = adjacency_seg.to(torch.int32).contiguous()
    amax = max(int(aseg.max().item()), 0) if aseg.numel() else 0
    keys = K.rag_edges3(aseg, conn)
    n = labels.numel()
    bc = torch.full((amax + 1,), -1, dtype=torch.int32, device=seg.device)
    keep = torch.zeros(amax + 1, dtype=torch.uint8, device=seg.device)
    m = min(n, amax)
    bc[1:m + 1] = bc_idx[:m].to(torch.int32)
    keep[1:m + 1] = is_cell[:m]
    adj, adjf = K.barcode_adjacency_edges(keys, bc, R, keep)
    return CellTyping(is_cell, torch.zeros(maxlab + 1, dtype=torch.uint8, device=seg.device), adj, adjf)
