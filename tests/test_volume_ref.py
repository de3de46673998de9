"""The 3-D yardstick itself (tests/volume_ref.py, numpy only) against scipy.ndimage's recorded
answers, the 2-D oracle and the recorded chain of tests/golden/volume3d.npz.  No device here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import volume_ref as VR  # noqa: E402


@pytest.fixture(scope="module")
def g(golden):
    return golden("volume3d")


def test_primitives_equal_scipy(g):
    m = g["p_mask"].astype(bool)
    assert np.array_equal(VR.label(m, 1)[0], g["p_label6"])
    assert np.array_equal(VR.label(m, 3)[0], g["p_label26"])
    assert int(g["p_label26"].max()) < int(g["p_label6"].max())      # the two connectivities differ here
    assert np.array_equal(VR.erode(m, 0), g["p_erosion0"].astype(bool))
    assert np.array_equal(VR.erode(m, 1), g["p_erosion1"].astype(bool))
    assert not np.array_equal(g["p_erosion0"], g["p_erosion1"])      # ones on the faces tell them apart
    assert np.array_equal(VR.dilate(m), g["p_dilation"].astype(bool))
    assert np.array_equal(VR.opening(m), g["p_opening"].astype(bool))
    assert np.array_equal(VR.fill_holes(m), g["p_fill"].astype(bool))
    assert int(g["p_fill"].sum()) > int(m.sum())


def _field2d(quantise):
    rng = np.random.default_rng(5)
    a = rng.random((40, 37))
    for _ in range(3):                                               # a smooth field
        a = (a + np.roll(a, 1, 0) + np.roll(a, -1, 0) + np.roll(a, 1, 1) + np.roll(a, -1, 1)) / 5
    a = (a - a.min()) / (a.max() - a.min())
    if quantise:
        a = np.floor(a * 6).clip(0, 5)
    mk = np.zeros(a.shape, np.int32)
    pts = rng.choice(a.size, 12, replace=False)
    mk.ravel()[pts] = np.arange(1, 13)
    mask = rng.random(a.shape) < 0.9
    return a, mk, mask


@pytest.mark.parametrize("quantise", [False, True])
@pytest.mark.parametrize("shape", [(1, 40, 37), (40, 1, 37), (40, 37, 1)])
def test_flood_on_degenerate_shapes_equals_the_2d_oracle(orc, shape, quantise):
    a, mk, mask = _field2d(quantise)
    want = orc.watershed(a, mk, mask)
    got = VR.flood(a.reshape(shape), mk.reshape(shape), mask.reshape(shape))
    assert np.array_equal(got.reshape(a.shape), want)
    assert np.array_equal(VR.flood(a, mk, mask), want)               # and as a 2-D array
    assert np.array_equal(VR.flood(a.reshape(shape), mk.reshape(shape)).reshape(a.shape), orc.watershed(a, mk))


def test_oracle_kmeans_reproduces_the_fixture(orc, g):
    final = g["c_final"].astype(np.float64)
    reg = g["c_reg_sum"].astype(np.float64)
    pos = final > 0
    for k, name in ((2, "2"), (3, "3")):
        lab, cen, _ = orc.kmeans_sk(final, k, valid=pos)
        assert np.array_equal(lab[pos], g["c_labels" + name].astype(np.int32))
        assert np.allclose(cen, g["c_centers" + name], rtol=1e-12, atol=0)
    lab, cen, _ = orc.kmeans_sk(np.log10(reg + 1), 2)
    assert np.array_equal(lab, g["c_labels_bkg"].astype(np.int32))
    assert np.allclose(cen, g["c_centers_bkg"], rtol=1e-12, atol=0)


def test_helper_chain_equals_the_fixture(orc, g):
    final = g["c_final"].astype(np.float64)
    reg = g["c_reg_sum"].astype(np.float64)

    def km(x, k):
        lab, cen, _ = orc.kmeans_sk(x, k)
        return lab, cen

    c = VR.chain(final, reg, km)
    for name in ("rough_mask", "rsf", "opened", "small", "bfh", "rough_bfh", "watershed_mask", "seeds", "bkg_mask",
                 "seeds_bkg", "watershed_mask_bkg", "watershed", "seg", "adjacency_watershed", "adjacency_seg"):
        assert np.array_equal(np.asarray(c[name]).astype(np.int64), g["c_" + name].astype(np.int64)), name
    assert c["nseeds"] == int(g["c_nseeds"]) and c["n"] == int(g["c_n"]) and c["n_adj"] == int(g["c_n_adj"])


def test_fixture_chain_is_not_degenerate(g):
    n = lambda k: int(g["c_" + k].astype(bool).sum())  # noqa: E731
    assert n("rsf") - n("opened") > 0                                # the opening removes
    assert n("opened") - n("small") > 0                              # small objects go
    assert n("bfh") - n("small") > 0 and n("rough_bfh") - n("rough_mask") > 0     # both fills add
    assert int(g["c_nseeds"]) >= 8
    assert 0 < n("bkg_mask") < g["c_bkg_mask"].size
    assert int((g["c_final"] == 0).sum()) > 0
    # :858 floods nothing (its seeds are the label of its own mask); the adjacency flood does
    assert np.array_equal(g["c_watershed"], g["c_seeds_bkg"] * g["c_watershed_mask_bkg"])
    assert n("adjacency_watershed") > 2 * n("seeds_bkg")
    for k in ("c_final", "c_reg_sum"):
        assert g[k].dtype == np.float32
