"""Writes tests/golden/volume3d.npz: scipy.ndimage's and sklearn's answers for the 3-D segmentation
stages (biofilm_analysis.py:818-859, :489-499).  Needs scipy and scikit-learn; run from the
repository root:  python tests/golden/make_volume_golden.py

Primitive masks (`p_*`): scipy.ndimage.label with the cross and with np.ones((3, 3, 3)),
binary_opening, binary_erosion(border_value=0 / 1), binary_dilation, binary_fill_holes.
Chain (`c_*`): a 32 x 48 x 40 synthetic volume (volume_ref.synthetic_volume, inputs stored as
float32) through the reference chain with sklearn KMeans(random_state=0, n_init=10), scipy's
morphology and labelling, remove_small_objects as label + bincount, and the flood of
tests/volume_ref.py for skimage's watershed (checked against the 2-D oracle in
tests/test_volume_ref.py).  Every intermediate mask, the seeds, the segmentation, the adjacency
segmentation, the KMeans labels and centres are recorded."""
import os
import sys

import numpy as np
import scipy.ndimage as ndi
from sklearn.cluster import KMeans

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import volume_ref as VR  # noqa: E402

CROSS = ndi.generate_binary_structure(3, 1)
FULL = np.ones((3, 3, 3), bool)


def primitive_mask():
    """(19, 11, 70): random blobs at mixed density, ones on some faces (border_value 0 vs 1), a
    closed cavity, and thin bridges"""
    rng = np.random.default_rng(3)
    m = ndi.binary_dilation(rng.random((19, 11, 70)) < 0.06, CROSS, iterations=1)
    m |= rng.random(m.shape) < 0.15
    m[0, :, :30] = True
    m[:, -1, 40:] = True
    m[5:12, 3:9, -1] = True
    m[8:13, 2:7, 10:16] = True
    m[10, 4, 12] = False                                   # closed cavity
    return m


def sk_kmeans(x, k):
    km = KMeans(n_clusters=k, random_state=0, n_init=10).fit(np.asarray(x, np.float64).reshape(-1, 1))
    return km.labels_.astype(np.int32), km.cluster_centers_.ravel()


def scipy_chain(final, reg_sum):
    """biofilm :818-859 and :489, :497-499 with scipy / sklearn for every stage they cover"""
    pos = final > 0
    x = final[pos]
    l2, c2 = sk_kmeans(x, 2)
    rough = np.zeros(final.shape, bool)
    rough[pos] = l2 == VR._top_of_two(x, l2)
    l3, c3 = sk_kmeans(x, 3)
    rsf = np.zeros(final.shape, bool)
    rsf[pos] = l3 == int(np.argmax([x[l3 == c].mean() for c in range(3)]))
    opened = ndi.binary_opening(rsf)
    lab, nl = ndi.label(opened, CROSS)
    small = (np.bincount(lab.ravel(), minlength=nl + 1) >= 10)[lab] & opened
    bfh = ndi.binary_fill_holes(small)
    rough_bfh = ndi.binary_fill_holes(rough)
    wmask = bfh & rough_bfh
    seeds, nseeds = ndi.label(wmask, FULL)
    logsum = np.log10(reg_sum + 1)
    lb, cb = sk_kmeans(logsum.ravel(), 2)
    lb = lb.reshape(final.shape)
    bkg = lb == VR._top_of_two(reg_sum, lb)
    final_bkg = final * bkg
    seeds_bkg = (seeds * bkg).astype(np.int32)
    wmask_bkg = wmask & bkg
    ws = VR.flood(-final_bkg, seeds_bkg, wmask_bkg)
    seg, n = VR.relabel_sequential(ws)
    aws = VR.flood(-(reg_sum * bkg), seeds_bkg, bkg)
    adj, n_adj = VR.relabel_sequential(aws)
    u8 = lambda a: a.astype(np.uint8)  # noqa: E731
    return dict(rough_mask=u8(rough), rsf=u8(rsf), opened=u8(opened), small=u8(small), bfh=u8(bfh),
                rough_bfh=u8(rough_bfh), watershed_mask=u8(wmask), seeds=seeds.astype(np.int32),
                nseeds=np.int64(nseeds), bkg_mask=u8(bkg), seeds_bkg=seeds_bkg, watershed_mask_bkg=u8(wmask_bkg),
                watershed=ws, seg=seg, n=np.int64(n), adjacency_watershed=aws, adjacency_seg=adj,
                n_adj=np.int64(n_adj), centers2=c2, centers3=c3, centers_bkg=cb, labels2=u8(l2), labels3=u8(l3),
                labels_bkg=u8(lb))


def main():
    out = {}
    m = primitive_mask()
    out["p_mask"] = m.astype(np.uint8)
    out["p_label6"] = ndi.label(m, CROSS)[0].astype(np.int32)
    out["p_label26"] = ndi.label(m, FULL)[0].astype(np.int32)
    out["p_opening"] = ndi.binary_opening(m).astype(np.uint8)
    out["p_erosion0"] = ndi.binary_erosion(m, border_value=0).astype(np.uint8)
    out["p_erosion1"] = ndi.binary_erosion(m, border_value=1).astype(np.uint8)
    out["p_dilation"] = ndi.binary_dilation(m).astype(np.uint8)
    out["p_fill"] = ndi.binary_fill_holes(m).astype(np.uint8)
    final32, sum32 = VR.synthetic_volume()
    out["c_final"] = final32
    out["c_reg_sum"] = sum32
    c = scipy_chain(final32.astype(np.float64), sum32.astype(np.float64))
    for k, v in c.items():
        out["c_" + k] = v
    path = os.path.join(HERE, "volume3d.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    print("seeds %d  opening removed %d  fills added %d and %d  seg labels %d  adjacency labels %d" % (
        c["nseeds"], int(c["rsf"].sum()) - int(c["opened"].sum()), int(c["bfh"].sum()) - int(c["small"].sum()),
        int(c["rough_bfh"].sum()) - int(c["rough_mask"].sum()), c["n"], c["n_adj"]))
    print("small objects removed %d  bkg voxels %d of %d  zeros in final %d" % (
        int(c["opened"].sum()) - int(c["small"].sum()), int(c["bkg_mask"].sum()), final32.size,
        int((final32 == 0).sum())))


if __name__ == "__main__":
    main()
