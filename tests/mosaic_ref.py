"""numpy restatement of the tiled 3-D mosaic (hiprfish_imaging_biofilm_analysis.py:1064-1172,
generate_3d_segmentation_tile_memory_efficient, with :203-236), parametric in the sizes the
reference hard-codes, and the seeded inputs the device tests run on.  tests/test_mosaic_ref.py
checks it against what the reference's own lines computed (tests/golden/mosaic.npz).

Registration is oracle.register_translation, the line profiles are the oracle's line_profile_3d
(neighbor.line_profile_v2), the segmentation stages are tests/volume_ref.py's; KMeans and log10
are passed in, as there."""
import numpy as np

import oracle as O
import volreg_ref as R
import volume_ref as VR

MAX_TILES = 64


# ---- stage 1: per-tile time sum with coverage mask (:203-236, :1073-1076) -------------------------
def tsum_masked(tstack, shifts):
    """-> (sum_filtered (X, Y, Z) f64, mask bool): tstack[0] + the zero-filled shifted later time
    points in f64 in t order, np.sum(axis=3), times the AND of the time points' coverage boxes"""
    a0 = np.asarray(tstack[0], np.float32).astype(np.float64)
    acc = a0.copy()
    mask = np.ones(a0.shape[:3], bool)
    for a, s in zip(tstack[1:], list(shifts)[1:]):
        acc += R.shift_zero(np.asarray(a, np.float32).astype(np.float64), s)
        hold = np.zeros(a0.shape[:3], bool)
        hold[R._box(a0.shape[:3], s)[0]] = True
        mask = mask & hold
    return np.sum(acc, axis=3) * mask, mask


def time_shifts(tstack):
    """:206-213: register_translation on the channel sums, no log, no clamp -> (T, 3) int32"""
    s = [np.sum(np.asarray(a, np.float32).astype(np.float64), axis=3) for a in tstack]
    return np.array([(0, 0, 0)] + [R.register(s[0], b) for b in s[1:]], np.int32)


def tile_tsum(tstack):
    return tsum_masked(tstack, time_shifts(tstack))


# ---- stage 2: neighbour shifts on the overlap strips (:1077-1087) ---------------------------------
def strip_pairs(sum_filtered, n, ov):
    """((i, j), strip of the neighbour, own strip) for every tile but (0, 0)"""
    Tx, Ty, _ = sum_filtered[0].shape
    for i in range(n):
        for j in range(n):
            if i == 0 and j == 0:
                continue
            if j == 0:
                yield (i, j), sum_filtered[(i - 1) * n][Tx - ov:Tx, :, :], sum_filtered[i * n][0:ov, :, :]
            else:
                yield (i, j), sum_filtered[i * n + j - 1][:, Ty - ov:Ty, :], sum_filtered[i * n + j][:, 0:ov, :]


def tile_shifts(sum_filtered, n, ov):
    out = np.zeros((n, n, 3), np.int32)
    for (i, j), a, b in strip_pairs(sum_filtered, n, ov):
        out[i, j] = R.register(a, b)
    return out


def peak_ratio(a, b):
    """the strip correlation's peak over its runner-up"""
    cc = np.sort(R.cc_abs(a, b).ravel())
    return cc[-1] / cc[-2]


# ---- stage 3: placement (:1088-1097) -------------------------------------------------------------
def origins(shifts, tile_shape, ov, m):
    """-> ((n * n, 3) int32 in tile order k = i * n + j, canvas shape).  x accumulates column 0's
    shifts of the rows above and the row's own; y and z only the row's own, column 0 included"""
    s = np.asarray(shifts).astype(np.float64)
    n = s.shape[0]
    Tx, Ty, Tz = tile_shape
    out = np.zeros((n * n, 3), np.int64)
    for i in range(n):
        for j in range(n):
            out[i * n + j] = (int(i * Tx - ov * i + np.sum(s[0:i + 1, 0, 0]) + np.sum(s[i, 1:j + 1, 0])) + m,
                              int(j * Ty - ov * j + np.sum(s[i, 0:j + 1, 1])) + m,
                              int(np.sum(s[i, 0:j + 1, 2])) + m)
    return out.astype(np.int32), (n * Tx + 2 * m, n * Ty + 2 * m, Tz + 2 * m)


def check_boxes(org, tile_shape, canvas):
    """the reference would wrap a negative index or fail to broadcast; here both are errors"""
    org = np.asarray(org).reshape(-1, 3)
    if len(org) > MAX_TILES:
        raise ValueError("more than %d tiles" % MAX_TILES)
    for k, o in enumerate(org):
        for a in range(3):
            if o[a] < 0 or o[a] + tile_shape[a] > canvas[a]:
                raise ValueError("tile %d leaves the canvas on axis %d" % (k, a))


# ---- stage 4: accumulation (:1098-1102) -----------------------------------------------------------
def accumulate(sum_filtered, masks, org, canvas):
    """-> (full / count, count) with count 0 -> 1"""
    tile_shape = sum_filtered[0].shape
    check_boxes(org, tile_shape, canvas)
    full = np.zeros(canvas)
    count = np.zeros(canvas)
    for s, m, o in zip(sum_filtered, masks, np.asarray(org).reshape(-1, 3)):
        box = tuple(slice(int(a), int(a) + t) for a, t in zip(o, tile_shape))
        full[box] += s * m
        count[box][np.asarray(m) > 0] += 1
    count[count == 0] = 1
    return full / count, count.astype(np.int32)


def stitch(tile_tstacks, n, ov, m):
    """:1066-1102 -> dict of the stages"""
    tsh = [time_shifts(ts) for ts in tile_tstacks]
    sm = [tsum_masked(ts, s) for ts, s in zip(tile_tstacks, tsh)]
    sums, masks = [a for a, _ in sm], [b for _, b in sm]
    shifts = tile_shifts(sums, n, ov)
    org, canvas = origins(shifts, sums[0].shape, ov, m)
    full, count = accumulate(sums, masks, org, canvas)
    return dict(t_shifts=tsh, sum_filtered=sums, masks=masks, shifts=shifts, origins=org, full=full, count=count,
                norm=full / np.max(full))


# ---- stage 5: enhancement, the + 1e-8 form (:1103-1126) -------------------------------------------
def enhance_eps(pad, chunk=None):
    """on the edge-padded canvas.  Minimum and maximum are the compare-select recurrences the device
    keeps for special values (`x < mn ? x : mn` from the first tap on), the mean is numpy's
    pairwise sum over 72 (eight accumulators), the quartiles numpy's linear interpolation at
    positions 17.75 and 53.25.  chunk c: only the (X // c) x (Y // c) whole chunks are written"""
    pad = np.ascontiguousarray(pad, np.float64)
    lp = O.line_profile_3d(pad)                                           # (X, Y, Z, 72, 11)
    mn = lp[..., 0].copy()
    mx = lp[..., 0].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(1, 11):
            x = lp[..., l]
            mn = np.where(x < mn, x, mn)
            mx = np.where(x > mx, x, mx)
        v = (lp[..., 5] - mn) / ((mx - mn) + 1e-8)                        # :1116-1119
        acc = v[..., 0:8].copy()
        for i in range(8, 72, 8):
            acc += v[..., i:i + 8]
        avg = (((acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])) +
               ((acc[..., 4] + acc[..., 5]) + (acc[..., 6] + acc[..., 7]))) / 72.0      # :1120
        s = np.sort(v, axis=3)
        lq = s[..., 18] - (s[..., 18] - s[..., 17]) * 0.25                # :1121
        uq = s[..., 53] + (s[..., 54] - s[..., 53]) * 0.25                # :1122
        qcv = (uq - lq) / (uq + lq + 1e-8)                                # :1123
        final = avg * (1 - qcv)                                           # :1125
    if chunk is not None:
        X, Y, _ = final.shape
        final[(X // chunk) * chunk:] = 0
        final[:, (Y // chunk) * chunk:] = 0
    return final


# ---- stage 6: segmentation (:1127-1170) -----------------------------------------------------------
def segment(final, norm, kmeans, log10=np.log10):
    """:1127-1153 are :818-844 (volume_ref.chain); the background filter of :1154-1165 is fitted on
    log10(norm + 1e-8) where norm > 0 and is false wherever norm <= 0 -> dict of the stages"""
    final = np.asarray(final, np.float64)
    norm = np.asarray(norm, np.float64)
    fpos = final > 0
    x = final[fpos]
    l2, _ = kmeans(x, 2)                                                    # :1128
    rough = np.zeros(final.shape, bool)
    rough[fpos] = l2 == VR._top_of_two(x, l2)                               # :1129-1137
    l3, _ = kmeans(x, 3)                                                    # :1139
    with np.errstate(invalid="ignore"):
        means = [x[l3 == c].mean() if (l3 == c).any() else np.nan for c in range(3)]
    rsf = np.zeros(final.shape, bool)
    rsf[fpos] = l3 == int(np.argmax(means))                                 # :1140-1147
    opened = VR.opening(rsf)                                                # :1148
    small = VR.remove_small_objects(opened, 10)                             # :1149
    bfh = VR.fill_holes(small)                                              # :1150
    rough_bfh = VR.fill_holes(rough)                                        # :1151
    wmask = bfh & rough_bfh                                                 # :1152
    seeds, nseeds = VR.label(wmask, final.ndim)                             # :1153
    pos = norm > 0
    lb, cb = kmeans(log10(norm + 1e-8)[pos], 2)                             # :1154-1156
    top = VR._top_of_two(norm[pos], lb)                                     # :1157-1161, every value positive
    bkg = np.zeros(norm.shape, bool)
    bkg[pos] = lb == top                                                    # :1162-1165
    final_bkg = final * bkg                                                 # :1166
    seeds_bkg = (seeds * bkg).astype(np.int32)                              # :1167
    wmask_bkg = wmask & bkg                                                 # :1168
    ws = VR.flood(-final_bkg, seeds_bkg, wmask_bkg)                         # :1169
    seg, n = VR.relabel_sequential(ws)                                      # :1170
    return dict(rough_mask=rough, rsf=rsf, opened=opened, small=small, bfh=bfh, rough_bfh=rough_bfh,
                watershed_mask=wmask, seeds=seeds, nseeds=nseeds, bkg_mask=bkg, final_bkg=final_bkg,
                seeds_bkg=seeds_bkg, watershed_mask_bkg=wmask_bkg, watershed=ws, seg=seg, n=n,
                centers_bkg=np.asarray(cb, np.float64).ravel())


def segment_mosaic(tile_tstacks, n, ov, m, chunk, kmeans, log10=np.log10):
    st = stitch(tile_tstacks, n, ov, m)
    st["final"] = enhance_eps(np.pad(st["norm"], 5, mode="edge"), chunk)
    st.update(segment(st["final"], st["norm"], kmeans, log10))
    return st


# ---- inputs --------------------------------------------------------------------------------------
def cells(shape, rng, density=1 / 150, r0=1.6, r1=2.4):
    """Gaussian cells of radius r0..r1 on a zero floor, maximum 1: what the enhancement and the
    segmentation find objects in (volreg_ref.blobs' spots are too small to survive the opening)"""
    s = np.zeros(shape)
    g = np.meshgrid(*[np.arange(a) for a in shape], indexing="ij")
    for _ in range(max(4, int(np.prod(shape) * density))):
        c = rng.random(3) * np.array(shape)
        r = r0 + (r1 - r0) * rng.random()
        s += (0.4 + 0.6 * rng.random()) * np.exp(-sum((gi - ci) ** 2 for gi, ci in zip(g, c)) / (2 * r * r))
    return s / s.max()


def mosaic_case(n, tile, ov, C, tile_offsets, t_offsets, seed, half=7, amp=150):
    """tile_tstacks[k][t], k = i * n + j: (X, Y, Z, C) f32 integer-valued crops of one scene.  Tile
    (i, j) shows the scene from (i (Tx - ov), j (Ty - ov), 0) + tile_offsets[k] on, time point t from
    t_offsets[t] further, so that the tile's shift against its neighbour is the difference of their
    offsets and its time shifts are t_offsets.  The scene is cells, except within `half` voxels of the
    seams, where it is sparse single-voxel spikes: the unnormalised correlation of two smooth strips
    has a peak barely above its neighbours, that of two spiky ones stands several times above its
    runner-up, so no FFT's rounding moves the neighbour shifts."""
    rng = np.random.default_rng(seed)
    Tx, Ty, Tz = tile
    shape = [v + 2 * R.MARGIN for v in (n * Tx - (n - 1) * ov, n * Ty - (n - 1) * ov, Tz)]
    band = np.zeros(shape, bool)
    for i in range(1, n):
        cx, cy = R.MARGIN + i * (Tx - ov) + ov // 2, R.MARGIN + i * (Ty - ov) + ov // 2
        band[cx - half:cx + half] = True
        band[:, cy - half:cy + half] = True
    spikes = (rng.random(shape) < 0.05) * (0.4 + 0.6 * rng.random(shape))
    scene = np.where(band, spikes, cells(shape, rng))
    w = 0.3 + 0.7 * rng.random(C)
    out = []
    for k in range(n * n):
        i, j = divmod(k, n)
        base = np.array((i * (Tx - ov), j * (Ty - ov), 0)) + np.array(tile_offsets[k])
        out.append([np.floor(amp * R.crop(scene, tile, base + np.array(to))[..., None] * w).astype(np.float32)
                    for to in t_offsets])
    return out


GOLDEN = dict(n=2, tile=(24, 24, 8), ov=8, margin=10, C=3, chunk=23, nchunk=2,
              tile_offsets=[(0, 0, 0), (1, -2, 1), (-2, 1, -1), (0, 2, 1)],
              t_offsets=[(0, 0, 0), (1, -1, 0), (-1, 2, 1)], seed=2)


def golden_case():
    """the inputs of tests/golden/mosaic.npz: 2 x 2 tiles of 24 x 24 x 8, overlap 8, T = 3, C = 3,
    integer valued (the f64 time sums are exact); every neighbour shift axis is non-zero somewhere"""
    g = GOLDEN
    return mosaic_case(g["n"], g["tile"], g["ov"], g["C"], g["tile_offsets"], g["t_offsets"], g["seed"])


def enhance_chunk_case():
    """a free-standing (26, 26, 18) chunk for :1112-1125: random, with an all-zero region (flat
    windows) -> image_chunk"""
    rng = np.random.default_rng(12)
    a = rng.random((26, 26, 18))
    a[:13, 8:, :10] = 0.0
    return a
