"""numpy restatement of the 2-D biofilm chain (hiprfish_imaging_biofilm_analysis.py:322-419) for the
tests of csrc/biofilm2d.hip, pipeline.register_biofilm_2d / segment_biofilm_2d and
biofilm.measure_biofilm_2d.  numpy and the committed oracle module only; the brute-force disk
operators are checked against scipy.ndimage in tests/test_biofilm2d_ref.py."""
import contextlib
import ctypes

import numpy as np

import oracle as O

LASER_CHANNELS = (23, 20, 14, 6)


# ---- disk morphology by brute force ----------------------------------------------------------
def disk(r):
    """skimage.morphology.disk(r): X^2 + Y^2 <= r^2 on [-r, r]^2"""
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return x * x + y * y <= r * r


def dilate_disk(mask, r):
    """scipy.ndimage.binary_dilation(mask, structure=disk(r)): every set pixel stamps the disk"""
    m = np.asarray(mask).astype(bool)
    H, W = m.shape
    d = disk(r)
    out = np.zeros((H + 2 * r, W + 2 * r), bool)
    for y, x in np.argwhere(m):
        out[y:y + 2 * r + 1, x:x + 2 * r + 1] |= d
    return out[r:r + H, r:r + W]


def dilate_disk_rows(mask, r):
    """dilate_disk for large radii and dense masks, where stamping takes too long: the disk is the
    union over dy of the row run |dx| <= floor(sqrt(r^2 - dy^2)), and a run hits iff the row's
    cumulative count differs across it.  (Row runs shifted in y; the device sweeps columns and tests
    along x.)  Checked equal to dilate_disk in tests/test_biofilm2d_ref.py."""
    m = np.asarray(mask).astype(bool)
    H, W = m.shape
    c = np.zeros((H, W + 1), np.int64)
    c[:, 1:] = np.cumsum(m, axis=1)
    xs = np.arange(W)
    out = np.zeros((H, W), bool)
    for dy in range(-r, r + 1):
        w = int(np.floor(np.sqrt(r * r - dy * dy)))
        while w * w > r * r - dy * dy:
            w -= 1
        while (w + 1) * (w + 1) <= r * r - dy * dy:
            w += 1
        hit = (c[:, np.minimum(xs + w + 1, W)] - c[:, np.maximum(xs - w, 0)]) > 0
        y0, y1 = max(0, -dy), min(H, H - dy)
        if y0 < y1:
            out[y0:y1] |= hit[y0 + dy:y1 + dy]
    return out


def erode_disk(mask, r, border_value=1, dilate=dilate_disk):
    """scipy.ndimage.binary_erosion(mask, structure=disk(r), border_value=...): border value 1 is the
    complement of the complement's dilation; border value 0 the same on the mask padded by r zeros"""
    m = np.asarray(mask).astype(bool)
    if border_value:
        return ~dilate(~m, r)
    H, W = m.shape
    p = np.pad(m, r, mode="constant", constant_values=False)
    return (~dilate(~p, r))[r:r + H, r:r + W]


def closing_disk(mask, r, dilate=dilate_disk):
    """skimage.morphology.binary_closing(mask, disk(r))"""
    return erode_disk(dilate(mask, r), r, 1, dilate)


# ---- the two argmax rules --------------------------------------------------------------------
def cluster_rule(labels, reg_sum):
    """:385-392: i_j = the mean of the positive registered sums of cluster j (NaN without one); cluster
    1 iff i0 < i1, else cluster 0 -> (mask, i0, i1)"""
    i = []
    for j in (0, 1):
        v = reg_sum * (labels == j)
        v = v[v > 0]
        i.append(float(np.average(v)) if v.size else float("nan"))
    return (labels == 1 if i[0] < i[1] else labels == 0), i[0], i[1]


def largest_label(lab, maxlab):
    """:410-412, :416-418: the label with the largest area, the first among equals -> (label, area);
    (0, 0) when no label in 1..maxlab occurs"""
    cnt = np.bincount(np.asarray(lab).ravel(), minlength=maxlab + 1)[1:maxlab + 1]
    if cnt.size == 0 or cnt.max() == 0:
        return 0, 0
    k = int(np.argmax(cnt))
    return k + 1, int(cnt[k])


# ---- registration (:323-346) -----------------------------------------------------------------
def register_biofilm_2d_ref(lasers):
    """-> (registered stack in the lasers' dtype, [(dr, dc), ...])"""
    sums = [np.sum(l.astype(np.float64), axis=2) for l in lasers]                     # :326
    ref = O.cr_log(sums[0])
    shifts = [(0, 0)] + [tuple(int(v) for v in O.register_translation(ref, O.cr_log(s))) for s in sums[1:]]   # :327
    H, W = lasers[0].shape[:2]
    reg = []
    for img, (dr, dc) in zip(lasers, shifts):                                          # :332-345
        out = np.zeros(img.shape, img.dtype)
        out[max(0, dr):H + min(0, dr), max(0, dc):W + min(0, dc)] = \
            img[-min(0, dr):H - max(0, dr), -min(0, dc):W - max(0, dc)]
        reg.append(out)
    return np.concatenate(reg, axis=2), shifts                                         # :346


# ---- segmentation (:347-418) -----------------------------------------------------------------
def _brighter_cluster(img, lab):
    mask, _, _ = cluster_rule(lab, img)
    return mask


def segment_biofilm_2d_ref(stack, keep=None, epithelial=True, disk_radius=100, bkg_min_size=10000,
                           dilate=dilate_disk):
    """-> (seg, n, adjacency_seg, n_adj, image_registered_sum, image_final_bkg_filtered, epithelial or None)
    dilate: the disk dilation to use, dilate_disk(mask, r) by default"""
    s = np.sum(stack.astype(np.float64), axis=2)                                       # :347
    norm = s / np.max(s)                                                               # :348
    nl = O.nl_means(norm, 7, 11, 0.02, 0.0)                                            # :350
    final = O.enhance_2d(np.pad(nl, 5, mode="edge"))                                   # :351-366
    l2, _, _ = O.kmeans_sk(final, 2)                                                   # :367
    rough = _brighter_cluster(final, l2)                                               # :368-377
    opened = O.opening(rough)                                                          # :378
    small = O.remove_small_objects_mask(opened, 10, 1)                                 # :379
    bfh = O.fill_holes(small)                                                          # :380
    rough_bfh = O.fill_holes(rough)                                                    # :381
    wmask_rough = bfh & rough_bfh                                                      # :382
    if not (nl > 0).all():
        raise ValueError("Input contains NaN, infinity or a value too large for dtype('float64').")
    nl_log = O.cr_log10(nl)                                                            # :383
    lb, _, _ = O.kmeans_sk(nl_log, 2)                                                  # :384
    bkg, i0, i1 = cluster_rule(lb, s)                                                  # :385-392
    final_bkg = nl * bkg                                                               # :393
    sum_bkg = s * bkg                                                                  # :394
    wmask = O.remove_small_objects_mask(wmask_rough & bkg, 10, 1)                      # :395-396
    seeds, nseeds = O.label(wmask.astype(np.int32), 2)                                 # :397
    flood_mask = rough & bkg                                                           # :398
    ws = O.watershed(-final_bkg, seeds, flood_mask)                                    # :399
    aws = O.watershed(-sum_bkg, seeds, bkg)                                            # :400
    seg, n = O.relabel_sequential(ws)                                                  # :401
    adj, n_adj = O.relabel_sequential(aws)                                             # :402
    if keep is not None:
        keep.update(image_sum=s, norm=norm, nl=nl, final=final, rough_mask=rough, opened=opened, small=small,
                    bfh=bfh, rough_bfh=rough_bfh, nl_log=nl_log, bkg_labels=lb, cluster_means=(i0, i1),
                    bkg_mask=bkg, final_bkg=final_bkg, sum_bkg=sum_bkg, watershed_mask=wmask, seeds=seeds,
                    nseeds=nseeds, flood_mask=flood_mask, watershed=ws, adjacency_watershed=aws, seg=seg,
                    adjacency_seg=adj)
    epi = None
    if epithelial:
        image_bkg = O.remove_small_objects_mask(~bkg, bkg_min_size, 1)                 # :404-405
        image_bkg_bfh = O.fill_holes(image_bkg)                                        # :406
        closed = closing_disk(image_bkg_bfh, disk_radius, dilate)                      # :407-408
        objects, nobj = O.label(closed.astype(np.int32), 2)                            # :409
        big, _ = largest_label(objects, nobj)                                          # :410-412
        if big == 0:
            raise ValueError("argmax of an empty sequence (:412)")
        bkg_final = objects == big                                                     # :412
        dilated = dilate(bkg_final, disk_radius)                                       # :413
        overall, nover = O.label((1 - dilated.astype(np.int32)), 2)                    # :414
        if nover == 0:
            raise ValueError("argmax of an empty sequence (:418)")
        overall_seg = O.watershed(-s, overall, None)                                   # :415
        biggest, _ = largest_label(overall_seg, nover)                                 # :416-418
        epi = overall_seg != biggest                                                   # :418
        if keep is not None:
            keep.update(image_bkg=image_bkg, image_bkg_bfh=image_bkg_bfh, bkg_closed=closed, bkg_objects=objects,
                        bkg_final=bkg_final, bkg_dilated=dilated, objects_overall=overall, nover=nover,
                        objects_overall_seg=overall_seg, epithelial_area=epi)
    return seg, n, adj, n_adj, s, final_bkg, epi


# ---- the synthetic field of view ---------------------------------------------------------------
SCENE_KW = dict(disk_radius=8, bkg_min_size=300)
NKIND = 6


def scene_spectra():
    """six unit-sum spectra over the 63 channels, so the channel sum of a pixel is its intensity"""
    rng = np.random.default_rng(5)
    sp = rng.random((NKIND, sum(LASER_CHANNELS))) ** 2 + 0.05
    return sp / sp.sum(axis=1, keepdims=True)


def scene(quantise=False):
    """A 160 x 160 field as four unshifted acquisitions (23, 20, 14, 6 channels, f32): a dark background
    on the left and below, a glowing biofilm field with 24 bright cells on the upper right,
    and one broad dim tissue blob on the lower border, a dark gap apart from the field.  Continuous,
    seeded values; quantise: the noisy intensity rounded to 255 levels (never 0), so that equal values
    meet in the floods while no neighbourhood is flat (a flat line profile is 0 / 0 at :358).  -> (lasers, intensity image)"""
    H = W = 160
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)

    def step(v, at, width=1.5):
        return 1.0 / (1.0 + np.exp(-(v - at) / width))

    field = step(xx, 62) * step(-yy, -100)            # open to the top and right borders: not a hole
    img = 0.05 + 0.02 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 0.25 * field
    cy, cx = np.meshgrid(np.arange(14, 96, 16), np.arange(72, 152, 14), indexing="ij")
    cy = cy.ravel() + rng.uniform(-2, 2, cy.size)
    cx = cx.ravel() + rng.uniform(-2, 2, cx.size)
    amp = rng.uniform(0.6, 1.0, cy.size)
    sig = rng.uniform(2.6, 3.4, cy.size)
    d2 = (yy[..., None] - cy) ** 2 + (xx[..., None] - cx) ** 2
    img += (amp * np.exp(-d2 / (2 * sig ** 2))).sum(axis=2)
    img += 0.14 * np.exp(-(((yy - 150) / 22.0) ** 4 + ((xx - 112) / 30.0) ** 4))       # the tissue
    kind = (np.argmin(d2, axis=2) % NKIND)
    img = img * (1.0 + 0.02 * rng.standard_normal((H, W)))
    if quantise:
        img = img + 0.004 * rng.standard_normal((H, W))
        img = np.maximum(np.round(img / img.max() * 255), 1.0) / 255.0
    stack = (img[..., None] * scene_spectra()[kind]).astype(np.float32)
    bounds = np.cumsum((0,) + LASER_CHANNELS)
    lasers = [np.ascontiguousarray(stack[:, :, a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
    return lasers, img


@contextlib.contextmanager
def one_openmp_thread():
    """oracle.nl_means is an OpenMP loop.  With several threads libgomp starts its pool in the calling
    process, and a test that forks workers afterwards (tests/test_image_cn_log.py, later in the same
    session) hangs in them; with one thread no pool is started."""
    try:
        gomp = ctypes.CDLL("libgomp.so.1")
    except OSError:
        yield
        return
    n = gomp.omp_get_max_threads()
    gomp.omp_set_num_threads(1)
    try:
        yield
    finally:
        gomp.omp_set_num_threads(n)


_CACHE = {}


def scene_reference(quantise=False):
    """the scene, its registered stack and the restatement's results, computed once per process
    -> dict(lasers, stack, out (the 7-tuple), keep)"""
    if quantise not in _CACHE:
        lasers, img = scene(quantise)
        stack = np.concatenate(lasers, axis=2)
        keep = {}
        with one_openmp_thread():
            out = segment_biofilm_2d_ref(stack, keep=keep, **SCENE_KW)
        _CACHE[quantise] = dict(lasers=lasers, stack=stack, out=out, keep=keep, img=img)
    return _CACHE[quantise]
