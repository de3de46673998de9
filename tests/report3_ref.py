"""numpy / scipy restatements of the 3-D per-cell report's device stages (csrc/report3.hip), the
yardstick of tests/test_report3_gpu.py; themselves checked in tests/test_report3_ref.py against
scipy.ndimage's own measurements, the 2-D oracle and the recorded fixture
(tests/golden/make_report3_golden.py)."""
import numpy as np
from scipy import ndimage as ndi


def pack(a, b):
    return (np.asarray(a, np.int64) << 32) | np.asarray(b, np.int64)


def rag_edges3(lab, conn=2):
    """skimage.future.graph.rag_boundary's edge set (its construction: grey erosion and dilation by
    generate_binary_structure(ndim, connectivity), the two boundary concatenations) as the sorted
    unique keys (a << 32) | b, a < b; a pair with a negative member is dropped"""
    lab = np.asarray(lab, np.int32)
    fp = ndi.generate_binary_structure(lab.ndim, conn)
    eroded = ndi.grey_erosion(lab, footprint=fp)
    dilated = ndi.grey_dilation(lab, footprint=fp)
    b0 = eroded != lab
    b1 = dilated != lab
    small = np.concatenate((eroded[b0], lab[b1])).astype(np.int64)
    large = np.concatenate((lab[b0], dilated[b1])).astype(np.int64)
    ok = small >= 0                                   # small < large, so large > 0 with it
    return np.unique(pack(small[ok], large[ok]))


def keys_of_matrix(edge):
    """the keys of a dense (L, L) edge matrix (oracle.rag_edges / kernels.rag_edges)"""
    a, b = np.nonzero(np.asarray(edge))
    return np.unique(pack(a, b))


def moments3(lab, maxlab):
    """(maxlab + 1, 4) int64: count, sum x, sum y, sum z per label 1..maxlab; everything else zero"""
    lab = np.asarray(lab)
    ok = (lab > 0) & (lab <= maxlab)
    l = lab[ok].astype(np.int64)
    out = np.zeros((maxlab + 1, 4), np.int64)
    out[:, 0] = np.bincount(l, minlength=maxlab + 1)
    for k, c in enumerate(np.nonzero(ok)):
        # bincount's weights are doubles: exact while every partial sum stays below 2^53
        w = np.bincount(l, weights=c.astype(np.float64), minlength=maxlab + 1)
        assert w.max(initial=0.0) < 2.0 ** 53
        out[:, 1 + k] = w.astype(np.int64)
    return out


def props3(mom):
    """(L, 5) f64: area, centroid x, y, z (sum / count, one division), valid"""
    mom = np.asarray(mom, np.int64)
    out = np.zeros((mom.shape[0], 5))
    ok = mom[:, 0] > 0
    out[ok, 0] = mom[ok, 0]
    out[ok, 1:4] = mom[ok, 1:4].astype(np.float64) / mom[ok, 0].astype(np.float64)[:, None]
    out[ok, 4] = 1.0
    return out


def barcode_adjacency_edges(keys, bc, R, keep=None):
    """every key with 1 <= a < b <= max label and both barcodes in 0..R-1: +1 at [ba][bb] and
    [bb][ba]; with keep, only when both flags are set"""
    bc = np.asarray(bc)
    adj = np.zeros((R, R), np.int64)
    for key in np.asarray(keys, np.int64).tolist():
        a, b = key >> 32, key & 0xffffffff
        if not (1 <= a < b < len(bc)):
            continue
        ba, bb = int(bc[a]), int(bc[b])
        if not (0 <= ba < R and 0 <= bb < R):
            continue
        if keep is not None and not (keep[a] and keep[b]):
            continue
        adj[ba, bb] += 1
        adj[bb, ba] += 1
    return adj


def planes(lab, colour):
    """(3, n) f32: image_identification[:, :, :, ch].flatten('F') of the volume painted
    colour[label]; labels outside 0..ncell are background (row 0)"""
    lab = np.asarray(lab)
    colour = np.asarray(colour)
    l = np.where((lab < 0) | (lab >= colour.shape[0]), 0, lab)
    img = colour[l]
    return np.stack([img[..., ch].flatten("F").astype("<f4") for ch in range(3)])


def bvox_bytes(shape, plane):
    """a Blender voxel file: [nx, ny, nz, 1] as <i4, then the plane as <f4"""
    return np.array([shape[0], shape[1], shape[2], 1]).astype("<i4").tobytes() + \
        np.asarray(plane).astype("<f4").tobytes()


def voronoi(shape, ncell, cut, seed):
    """a Voronoi label volume of `ncell` random sites, voxels farther than `cut` from their site
    background, labels renumbered 1..n -> (labels int32, n)"""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0, 1, (ncell, len(shape))) * np.array(shape)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).reshape(-1, len(shape))
    d, i = cKDTree(pts).query(grid.astype(np.float64))
    lab = (i + 1).astype(np.int32)
    lab[d > cut] = 0
    present = np.unique(lab)
    present = present[present > 0]
    remap = np.zeros(ncell + 1, np.int32)
    remap[present] = np.arange(1, len(present) + 1)
    return remap[lab].reshape(shape), len(present)
