"""tests/biofilm2d_ref.py against scipy.ndimage and numpy, and the conditions the synthetic field of
tests/test_biofilm2d_gpu.py has to meet under the restatement alone.  No device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import biofilm2d_ref as R  # noqa: E402

SHAPES = [(40, 53, 6), (17, 90, 20), (64, 7, 9), (50, 50, 1), (33, 41, 13)]


@pytest.mark.parametrize("density", [0.002, 0.1, 0.97])
@pytest.mark.parametrize("shape", SHAPES)
def test_disk_operators_equal_scipy(shape, density):
    ndi = pytest.importorskip("scipy.ndimage")
    H, W, r = shape
    rng = np.random.default_rng(H * 1000 + W * 10 + int(density * 1000))
    m = rng.random((H, W)) < density
    d = R.disk(r)
    assert d.shape == (2 * r + 1, 2 * r + 1) and d[r, 0] and d[0, r] and not d[0, 0]
    assert np.array_equal(R.dilate_disk(m, r), ndi.binary_dilation(m, structure=d))
    assert np.array_equal(R.erode_disk(m, r, 1), ndi.binary_erosion(m, structure=d, border_value=True))
    assert np.array_equal(R.erode_disk(m, r, 0), ndi.binary_erosion(m, structure=d, border_value=0))
    closed = ndi.binary_erosion(ndi.binary_dilation(m, structure=d), structure=d, border_value=True)
    assert np.array_equal(R.closing_disk(m, r), closed)


@pytest.mark.parametrize("shape", SHAPES + [(30, 30, 100), (60, 70, 40)])
def test_row_run_dilation_equals_brute_force_and_scipy(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    H, W, r = shape
    rng = np.random.default_rng(H + W + r)
    for density in (0.002, 0.1, 0.97):
        m = rng.random((H, W)) < density
        want = R.dilate_disk(m, r)
        assert np.array_equal(R.dilate_disk_rows(m, r), want)
        assert np.array_equal(want, ndi.binary_dilation(m, structure=R.disk(r)))
        for bv in (0, 1):
            assert np.array_equal(R.erode_disk(m, r, bv, R.dilate_disk_rows), R.erode_disk(m, r, bv))


def test_largest_label_is_argmax_of_bincount():
    rng = np.random.default_rng(3)
    lab = rng.integers(0, 9, (37, 41)).astype(np.int32)
    lab[lab == 4] = 0                                           # a label missing in the middle
    cnt = np.bincount(lab.ravel(), minlength=9)[1:]
    assert R.largest_label(lab, 8) == (int(np.argmax(cnt)) + 1, int(cnt.max()))
    tie = np.zeros((4, 6), np.int32)
    tie[0, :3] = 5
    tie[1, :3] = 2
    tie[2, :2] = 7
    assert R.largest_label(tie, 7) == (2, 3)                    # np.argmax keeps the first maximum
    assert R.largest_label(np.zeros((3, 3), np.int32), 6) == (0, 0)
    assert R.largest_label(np.zeros((3, 3), np.int32), 0) == (0, 0)


def test_cluster_rule():
    lab = np.array([[0, 0, 1], [1, 1, 0]], np.int32)
    s = np.array([[1.0, 3.0, 5.0], [0.0, 7.0, -2.0]])
    mask, i0, i1 = R.cluster_rule(lab, s)
    assert (i0, i1) == (2.0, 6.0) and np.array_equal(mask, lab == 1)
    mask, i0, i1 = R.cluster_rule(1 - lab, s)
    assert (i0, i1) == (6.0, 2.0) and np.array_equal(mask, lab == 1)
    mask, i0, i1 = R.cluster_rule(np.zeros((2, 3), np.int32), s)   # an empty cluster: NaN, cluster 0
    assert i0 == 4.0 and np.isnan(i1) and mask.all()


@pytest.mark.parametrize("quantise", [False, True])
def test_scene_meets_its_conditions(orc, quantise):
    ref = R.scene_reference(quantise)
    seg, n, adj, n_adj, s, final_bkg, epi = ref["out"]
    k = ref["keep"]
    assert (k["nl"] > 0).all()
    assert k["nover"] >= 2                                      # label(1 - bd) has a biofilm and a tissue
    assert 0 < epi.sum() < epi.size
    assert n >= 8 and n_adj >= 8
    i0, i1 = k["cluster_means"]
    assert abs(i0 - i1) > 1e-9 * max(i0, i1)                    # summation order cannot decide :389
    assert all(a.shape == (160, 160) for a in (seg, adj, s, final_bkg, epi))
    assert sum(l.shape[2] for l in ref["lasers"]) == 63


def test_quantised_scene_has_equal_values():
    s = R.scene_reference(True)["out"][4]
    eq = (s[:, 1:] == s[:, :-1]).sum() + (s[1:] == s[:-1]).sum()
    assert eq > 1000                                            # the floods of :400 and :415 meet ties
