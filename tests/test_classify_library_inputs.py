"""The inputs of tests/test_classify_library_gpu.py, checked against the restatement alone (no
GPU): the conditions without which those tests would pass vacuously -- near ties the screens
cannot decide at every row count, every extreme library row actually chosen by some pixels, no
row holding NaN / inf chosen by a non-zero pixel, finite best distances.  A builder seed that
fails one of these is changed; the thresholds are not."""
import numpy as np
import pytest

import test_classify_library_gpu as L

NEAR = 2e-5      # test_kernels_gpu.NEAR: restated best and runner-up a screen alone cannot separate


def top2(orc, x, ref, bounds):
    """orc.classify_top2 on ONE OpenMP thread.  The restatement's loop over pixels is an OpenMP
    parallel region; run with more threads it would leave libgomp's worker pool in the pytest
    process, and a later unmarked test that forks workers (tests/test_image_cn_log.py, a fork-based
    process pool whose children use OpenMP through torch) then hangs on the pool the fork did not
    copy.  One thread runs the region inline and starts no workers; the setting is put back after
    the call.  These are the first unmarked tests to call an OpenMP function of the restatement."""
    import ctypes
    orc.lib()                                         # liboracle.so, and with it libgomp, is loaded
    gomp = ctypes.CDLL("libgomp.so.1")                # the handle of the copy already loaded
    n = gomp.omp_get_max_threads()
    gomp.omp_set_num_threads(1)
    try:
        return orc.classify_top2(x, ref, bounds)
    finally:
        gomp.omp_set_num_threads(n)


@pytest.mark.parametrize("bounds,R", L.ROW_COUNTS, ids=L.ROW_IDS)
def test_row_count_inputs(orc, bounds, R):
    ref, pairs = L.sweep_library(bounds, R)
    x = L.sweep_pixels(ref, pairs, bounds)
    assert ref.shape == (R, bounds[-1]) and ref.dtype == np.float32 and np.isfinite(ref).all()
    assert x.shape == (L.SWEEP_P, bounds[-1]) and x.dtype == np.float32
    ra, d1, d2 = top2(orc, x.astype(np.float64), ref.astype(np.float64), bounds)
    assert np.isfinite(d1).all()
    kinds = {k for _, _, k in pairs}
    if R >= 2:
        assert (0, R - 1, "near") in pairs
        assert R < 65 or (63, 64, "near") in pairs            # across the first chunk boundary
        assert R < 4 or (R - 2, R - 1, "near") in pairs       # (R = 3: rows 0, 1, 2 are one triple)
        assert ("dup" in kinds) == (R >= 8 or R == 3)
        near = int(((d2 - d1) <= NEAR).sum())
        print("R = %d: %d of %d pixels are near ties" % (R, near, L.SWEEP_P))
        assert near >= L.SWEEP_P // 4
        for a, b, k in pairs:
            if k == "dup":                       # an exact tie: the lower row, and it is exercised
                assert np.array_equal(ref[a], ref[b]) and not (ra == b).any() and (ra == a).sum() >= 8
            else:
                assert not np.array_equal(ref[a], ref[b])
    else:
        assert not pairs and (ra == 0).all() and np.isinf(d2).all()
    # the negated pixels: every non-zero segment's restated cosine is <= 0 for every row, so no
    # row scores above the pixel's count of all-zero segments
    nb = L.SWEEP_P // 2 if pairs else 0
    ng = x[nb:nb + 64]
    nseg = len(bounds) - 1
    nz = sum((ng[:, bounds[s]:bounds[s + 1]] == 0).all(1).astype(int) for s in range(nseg))
    assert (ng <= 0).all() and (nz < nseg).all() and (d1[nb:nb + 64] >= (nseg - nz) / nseg - 1e-12).all()
    assert R < 16 or (nz == 0).sum() >= 8          # (a library of one or two rows may have none)
    assert (x[nb + 64:nb + 80] == 0).all()


@pytest.mark.parametrize("kind", L.VALUE_KINDS)
def test_value_inputs(orc, kind):
    ref, shapes, special = L.values_library(kind)
    x = L.values_pixels(ref, shapes, special, kind)
    assert ref.shape == (L.VALUES_R, 95) and ref.dtype == np.float32 and x.dtype == np.float32
    ra, d1, d2 = top2(orc, x.astype(np.float64), ref.astype(np.float64), L.ECOLI)
    assert np.isfinite(x).all() and np.isfinite(d1).all()         # no pixel holds NaN or inf
    counts = np.bincount(ra, minlength=L.VALUES_R)
    print({name: int(counts[row]) for name, row in special.items()})
    nonzero = np.abs(x).sum(1) > 0
    if kind != "nonfinite":
        assert np.isfinite(ref).all()
        for name, row in special.items():
            assert counts[row] >= 8, "special row %s (%d) is the argmin of %d pixels" % (name, row, counts[row])
        ny = np.stack([(ref[:, L.ECOLI[s]:L.ECOLI[s + 1]].astype(np.float64) ** 2).sum(1) for s in range(5)], 1)
        # "huge" has no segment the parent's tiny route (0 < ny < 1e-30) would catch; "tiny" does
        assert ((ny > 0) & (ny < 1e-30)).any() == (kind == "tiny") and (ny > 1e30).any()
    if kind == "huge":
        # the overflow case: pixels of the 1e25 row at scale 1e14 -- sums of squares under the list
        # pass's 1e30 gate, products with the row past the f32 maximum -- that are near ties
        r = special["e25"]
        big = np.abs(x).max(1) > 1e13
        nx = max(float((x[big, L.ECOLI[s]:L.ECOLI[s + 1]].astype(np.float64) ** 2).sum(1).max()) for s in range(5))
        assert big.sum() == 256 and nx < 1e30
        prod = np.abs(x[big].astype(np.float64) * ref[r].astype(np.float64)).max(1)
        assert (prod > L.F32_MAX).all()
        assert (((d2 - d1) <= NEAR) & big).sum() >= 128
        assert np.isin(ra[big], [r, special["e25_twin"]]).all()
    elif kind == "nonfinite":
        bad = ~np.isfinite(ref).all(1)
        assert sorted(np.nonzero(bad)[0]) == sorted(special.values())
        assert not bad[ra[nonzero]].any()
        # rows holding NaN / inf do compete where the pixel's segment is all zero: their restated
        # distance there is finite
        for name in ("one_nan", "one_inf"):
            row = ref[[special[name]]].astype(np.float64)
            dn = top2(orc, x.astype(np.float64), row, L.ECOLI)[1]     # inf where the distance is NaN
            assert np.isfinite(dn[nonzero]).sum() >= 4, name
    assert (((d2 - d1) <= NEAR).sum()) >= 64
