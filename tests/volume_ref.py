"""numpy restatements of the 3-D segmentation stages (biofilm_analysis.py:818-859, :489-499), the
yardstick of tests/test_volume_gpu.py.  The committed oracle library is 2-D; these are N-D and are
themselves checked against scipy.ndimage, the 2-D oracle and the recorded fixture
(tests/test_volume_ref.py, tests/golden/make_volume_golden.py).  numpy only."""
import itertools

import numpy as np


def _offsets(shape_padded, conn):
    """flat offsets of the neighbours with at most `conn` non-zero coordinate steps, in raster-offset
    order (most negative first: -X, -Y, -Z, +Z, +Y, +X for conn 1 in 3-D)"""
    nd = len(shape_padded)
    strides = [int(np.prod(shape_padded[k + 1:])) for k in range(nd)]
    offs = []
    for d in itertools.product((-1, 0, 1), repeat=nd):
        nz = sum(1 for v in d if v)
        if 0 < nz <= conn:
            offs.append(sum(v * s for v, s in zip(d, strides)))
    return sorted(offs)


def _crop(a_flat, shape_padded):
    a = np.asarray(a_flat).reshape(shape_padded)
    return a[tuple(slice(1, -1) for _ in shape_padded)]


def label(mask, conn):
    """scipy.ndimage.label / skimage label of a bool array: components by `conn` (1 = faces only ...
    ndim = full), numbered by raster-first appearance -> (labels int32, count)"""
    m = np.pad(np.asarray(mask) != 0, 1)
    offs = _offsets(m.shape, conn)
    mf = m.ravel().tolist()
    lab = [0] * len(mf)
    cur = 0
    for p in np.flatnonzero(m.ravel()).tolist():
        if lab[p]:
            continue
        cur += 1
        lab[p] = cur
        stack = [p]
        while stack:
            q = stack.pop()
            for o in offs:
                r = q + o
                if mf[r] and not lab[r]:
                    lab[r] = cur
                    stack.append(r)
    return np.ascontiguousarray(_crop(np.array(lab, np.int32), m.shape)), cur


def erode(mask, border_value=0):
    """binary erosion by the cross (faces); outside the array reads border_value"""
    m = np.pad(np.asarray(mask) != 0, 1, constant_values=bool(border_value))
    core = tuple(slice(1, -1) for _ in m.shape)
    out = m[core].copy()
    for ax in range(m.ndim):
        for sh in (-1, 1):
            out &= np.roll(m, sh, axis=ax)[core]
    return out


def dilate(mask):
    m = np.pad(np.asarray(mask) != 0, 1)
    core = tuple(slice(1, -1) for _ in m.shape)
    out = m[core].copy()
    for ax in range(m.ndim):
        for sh in (-1, 1):
            out |= np.roll(m, sh, axis=ax)[core]
    return out


def opening(mask, border_value=0):
    """scipy.ndimage.binary_opening: dilation(erosion(border_value=0))"""
    return dilate(erode(mask, border_value))


def fill_holes(mask):
    """scipy.ndimage.binary_fill_holes: everything but the background face-connected to the
    array's boundary"""
    m = np.asarray(mask) != 0
    lab, _ = label(~m, 1)
    outside = set()
    for ax in range(m.ndim):
        for side in (0, -1):
            outside.update(np.unique(np.take(lab, side, axis=ax)).tolist())
    outside.discard(0)
    return ~np.isin(lab, sorted(outside)) if outside else np.ones(m.shape, bool)


def remove_small_objects(mask, min_size, conn=1):
    """skimage.morphology.remove_small_objects on a bool array"""
    lab, n = label(mask, conn)
    size = np.bincount(lab.ravel(), minlength=n + 1)
    keep = size >= min_size
    keep[0] = False
    return keep[lab]


def relabel_sequential(lab):
    """skimage.segmentation.relabel_sequential(lab)[0] -> (labels, count)"""
    lab = np.asarray(lab)
    present = np.unique(lab[lab > 0])
    fw = np.zeros(int(lab.max(initial=0)) + 1, np.int32)
    fw[present] = np.arange(1, present.size + 1, dtype=np.int32)
    return fw[lab].astype(np.int32), int(present.size)


def flood(image, markers, mask=None):
    """skimage.morphology.watershed(image, markers, mask=mask), connectivity 1, on an N-D array:
    the heap flood of oracle/hrf_oracle.c (oracle_watershed) with the neighbours in raster-offset
    order.  The heap is that file's own: parent of c is (c + 1) // 2 - 1, strict (value, age)
    order, markers pushed in raster order with age 0, a voxel labelled when it is pushed.
    (heapq keeps another layout, which shows where equal-valued markers meet.)"""
    image = np.asarray(image, np.float64)
    mk = np.asarray(markers)
    inm = np.ones(image.shape, bool) if mask is None else (np.asarray(mask) != 0)
    mp = np.pad(inm, 1)
    offs = _offsets(mp.shape, 1)
    free = mp.ravel().tolist()                      # in the mask and not yet labelled
    val = np.pad(image, 1).ravel().tolist()
    out = np.pad(np.where(inm, mk, 0).astype(np.int64), 1).ravel().tolist()
    heap = []

    def smaller(a, b):
        return a[0] < b[0] or (a[0] == b[0] and a[1] < b[1])

    def push(e):
        c = len(heap)
        heap.append(e)
        while c > 0:
            p = (c + 1) // 2 - 1
            if smaller(heap[c], heap[p]):
                heap[c], heap[p] = heap[p], heap[c]
                c = p
            else:
                break

    def pop():
        top = heap[0]
        last = heap.pop()
        n = len(heap)
        if n == 0:
            return top
        heap[0] = last
        i = 0
        while True:
            s, l, r = i, 2 * i + 1, 2 * i + 2
            if l >= n:
                break
            if smaller(heap[l], heap[i]):
                s = l
            if r < n and smaller(heap[r], heap[s]):
                s = r
            if s == i:
                break
            heap[i], heap[s] = heap[s], heap[i]
            i = s
        return top

    for p in range(len(out)):
        if out[p]:
            free[p] = False
            push((val[p], 0, p))
    age = 1
    while heap:
        _, _, p = pop()
        lp = out[p]
        for o in offs:
            q = p + o
            if free[q]:
                free[q] = False
                age += 1
                push((val[q], age, q))
                out[q] = lp
    return np.ascontiguousarray(_crop(np.array(out, np.int64), mp.shape).astype(np.int32))


def _top_of_two(values, labels):
    """:822-828, :849-854: the cluster whose positive `values` have the larger mean; cluster 0 when
    the reference's `i0 < i1` is false (a NaN mean included)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        means = []
        for c in (0, 1):
            v = values * (labels == c)
            v = v[v > 0]
            means.append(v.mean() if v.size else np.nan)
    return 1 if means[0] < means[1] else 0


def chain(final, reg_sum, kmeans, log10=np.log10):
    """biofilm :818-859 plus the adjacency flood of :489, :497-499.  kmeans(x_1d, k) -> (labels,
    centres) stands for KMeans(n_clusters=k, random_state=0, n_init=10).fit_predict.
    -> dict of every intermediate"""
    final = np.asarray(final, np.float64)
    reg_sum = np.asarray(reg_sum, np.float64)
    pos = final > 0
    x = final[pos]
    l2, c2 = kmeans(x, 2)                                                   # :819
    rough = np.zeros(final.shape, bool)
    rough[pos] = l2 == _top_of_two(x, l2)                                   # :820-828
    l3, c3 = kmeans(x, 3)                                                   # :830
    with np.errstate(invalid="ignore"):
        means = [x[l3 == c].mean() if (l3 == c).any() else np.nan for c in range(3)]
    rsf = np.zeros(final.shape, bool)
    rsf[pos] = l3 == int(np.argmax(means))                                  # :831-838
    opened = opening(rsf)                                                   # :839
    small = remove_small_objects(opened, 10)                                # :840
    bfh = fill_holes(small)                                                 # :841
    rough_bfh = fill_holes(rough)                                           # :842
    wmask = bfh & rough_bfh                                                 # :843
    seeds, nseeds = label(wmask, final.ndim)                                # :844
    logsum = log10(reg_sum + 1)                                             # :845
    lb, cb = kmeans(logsum.ravel(), 2)                                      # :846
    lb = lb.reshape(final.shape)
    bkg = lb == _top_of_two(reg_sum, lb)                                    # :847-854
    final_bkg = final * bkg                                                 # :855
    seeds_bkg = seeds * bkg                                                 # :856
    wmask_bkg = wmask & bkg                                                 # :857
    ws = flood(-final_bkg, seeds_bkg, wmask_bkg)                            # :858
    seg, n = relabel_sequential(ws)                                         # :859
    aws = flood(-(reg_sum * bkg), seeds_bkg, bkg)                           # :489, :497
    adj, n_adj = relabel_sequential(aws)                                    # :499
    return dict(rough_mask=rough, rsf=rsf, opened=opened, small=small, bfh=bfh, rough_bfh=rough_bfh,
                watershed_mask=wmask, seeds=seeds, nseeds=nseeds, bkg_mask=bkg, final_bkg=final_bkg,
                seeds_bkg=seeds_bkg.astype(np.int32), watershed_mask_bkg=wmask_bkg, watershed=ws, seg=seg, n=n,
                adjacency_watershed=aws, adjacency_seg=adj, n_adj=n_adj,
                centers2=np.asarray(c2, np.float64).ravel(), centers3=np.asarray(c3, np.float64).ravel(),
                centers_bkg=np.asarray(cb, np.float64).ravel(), labels2=l2, labels3=l3, labels_bkg=lb)


def synthetic_volume(shape=(32, 48, 40), seed=11, nblobs=22):
    """Gaussian blobs plus noise for the normalised registered sum; final is a noisy multiple of it
    with about 2 % exact zeros (what nan_to_num and the quartile term leave in image_final).
    Both as float32, to be promoted to float64 by the user."""
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    gx, gy, gz = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    s = np.zeros(shape)
    for _ in range(nblobs):
        c = rng.random(3) * np.array(shape)
        r = 2.5 + 2.5 * rng.random()
        s += (0.5 + rng.random()) * np.exp(-((gx - c[0]) ** 2 + (gy - c[1]) ** 2 + (gz - c[2]) ** 2) / (2 * r * r))
    s += 0.03 * rng.random(shape)
    s /= s.max()
    final = s * (0.8 + 0.4 * rng.random(shape))
    final[rng.random(shape) < 0.02] = 0.0
    return final.astype(np.float32), s.astype(np.float32)
