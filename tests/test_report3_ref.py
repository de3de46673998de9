"""tests/report3_ref.py -- the checker of tests/test_report3_gpu.py -- against scipy.ndimage's own
measurements, the 2-D oracle on flat placements and the bytes the reference's
save_identification_bvox wrote (tests/golden/report3.npz).  CPU only."""
import os
import sys

import numpy as np
from scipy import ndimage as ndi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import report3_ref as R3  # noqa: E402

BIG = (33, 17, 65)


def test_moments_equal_scipy_measurements():
    rng = np.random.default_rng(3)
    lab = rng.integers(-2, 46, BIG).astype(np.int32)
    lab[lab == 17] = 0                                            # an absent label
    mom = R3.moments3(lab, 40)
    idx = np.arange(1, 41)
    assert np.array_equal(mom[1:, 0], ndi.sum(np.ones(BIG), lab, idx).astype(np.int64))
    assert mom[0].tolist() == [0, 0, 0, 0] and mom[17].tolist() == [0, 0, 0, 0]
    props = R3.props3(mom)
    com = np.array(ndi.center_of_mass(np.ones(BIG), lab, idx[mom[1:, 0] > 0]))
    np.testing.assert_allclose(props[1:][mom[1:, 0] > 0, 1:4], com, rtol=1e-13, atol=0)
    assert props[17].tolist() == [0.0] * 5 and props[1, 4] == 1.0
    # labels above maxlab and negative ones are counted nowhere
    assert mom[:, 0].sum() == np.count_nonzero((lab > 0) & (lab <= 40))


def test_edges_tell_the_footprints_apart():
    lab, n = R3.voronoi(BIG, 150, 6.0, seed=4)
    assert n > 100
    counts = [len(R3.rag_edges3(lab, conn)) for conn in (1, 2, 3)]
    assert counts[0] < counts[1] < counts[2], counts
    k = R3.rag_edges3(lab, 2)
    assert np.all((k >> 32) < (k & 0xffffffff)) and (k >> 32).min() == 0
    # the single pairs of the device tests: an edge diagonal and a corner
    two = np.zeros(BIG, np.int32)
    two[3, 3, 63], two[4, 4, 63] = 1, 2
    assert [int(R3.pack(1, 2)) in R3.rag_edges3(two, c).tolist() for c in (1, 2, 3)] == [False, True, True]
    two[4, 4, 63], two[4, 4, 64] = 0, 2
    assert [int(R3.pack(1, 2)) in R3.rag_edges3(two, c).tolist() for c in (1, 2, 3)] == [False, False, True]


def test_edges_on_flat_placements_equal_the_2d_oracle(orc):
    rng = np.random.default_rng(5)
    lab, n = R3.voronoi((40, 37), 60, 4.0, seed=6)
    lab[rng.random(lab.shape) < 0.02] = 0
    want = R3.keys_of_matrix(orc.rag_edges(lab, n))
    assert len(want) > n
    for shape in ((1, 40, 37), (40, 1, 37), (40, 37, 1)):
        for conn in (2, 3):                                       # the 2-D graph is the 3 x 3 window's
            assert np.array_equal(R3.rag_edges3(lab.reshape(shape), conn), want), (shape, conn)
    assert np.array_equal(R3.rag_edges3(lab, 2), want)


def test_barcode_adjacency_equals_the_2d_oracle(orc):
    rng = np.random.default_rng(8)
    lab, n = R3.voronoi((40, 37), 60, 4.0, seed=6)
    e = orc.rag_edges(lab, n)
    bc = rng.integers(-1, 5, n + 1).astype(np.int32)
    keys = R3.keys_of_matrix(e)
    assert np.array_equal(R3.barcode_adjacency_edges(keys, bc, 5), orc.barcode_adjacency(e, bc, 5))
    keep = rng.random(n + 1) < 0.6
    bcf = np.where(keep, bc, -1).astype(np.int32)
    assert np.array_equal(R3.barcode_adjacency_edges(keys, bc, 5, keep), orc.barcode_adjacency(e, bcf, 5))


def test_planes_and_bvox_equal_the_reference_files(golden):
    g = golden("report3")
    lab, colour, image = g["labels"], g["colour"], g["image"]
    assert image.shape == (3, 4, 5, 3) and np.array_equal(colour[lab], image)
    pl = R3.planes(lab, colour)
    for ch, c in enumerate("rgb"):
        assert np.array_equal(pl[ch], image[:, :, :, ch].flatten("F").astype("<f4"))
        assert R3.bvox_bytes(lab.shape, pl[ch]) == g["bvox_" + c].tobytes(), c
    # x runs fastest in a plane
    assert pl[0].reshape(5, 4, 3)[2, 1, 0] == np.float32(image[0, 1, 2, 0])
    # labels outside the table are background
    far = lab.copy()
    far[0, 0, 0], far[1, 1, 1] = 6, -3
    ref = lab.copy()
    ref[0, 0, 0], ref[1, 1, 1] = 0, 0
    assert np.array_equal(R3.planes(far, colour), R3.planes(ref, colour))
