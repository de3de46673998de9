"""Tiled 3-D mosaics on the device (hiprfish_imaging_biofilm_analysis.py:1064-1172): the per-tile
time sum with its coverage mask, the neighbour shifts, placement and accumulation, the `+ 1e-8`
enhancement and the segmentation with the mosaic's background filter, against
tests/golden/mosaic.npz (the reference's own lines) and tests/mosaic_ref.py (equal to it,
tests/test_mosaic_ref.py).  Every comparison is exact: f64 arrays bit for bit, masks, counts and
labels with array_equal."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mosaic_ref as MR  # noqa: E402

G = MR.GOLDEN


@pytest.fixture(scope="module")
def K():
    from hiprfish_image_analysis_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def P():
    from hiprfish_image_analysis_amd import pipeline
    return pipeline


@pytest.fixture(scope="module")
def g(golden):
    return golden("mosaic")


@pytest.fixture(scope="module")
def km(orc):
    def f(x, k):
        lab, cen, _ = orc.kmeans_sk(x, k)
        return lab, cen
    return f


@pytest.fixture(scope="module")
def gseg(g, km, orc):
    """the restatement's segmentation of the fixture's final and norm, computed once"""
    return MR.segment(g["final"], g["norm"], km, orc.cr_log10)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def host(t):
    return t.cpu().numpy()


def tiles_of(g):
    n2 = G["n"] ** 2
    return [g["sum_filtered_k%d" % k] for k in range(n2)], [g["mask_k%d" % k] for k in range(n2)]


# ---- stage 1: time sum with coverage mask ----------------------------------------------------------
TSUM_SHIFTS = [(0, 0, 0), (2, -1, 3), (-3, 2, -2), (0, 0, 0)]      # both signs on every axis, and a zero shift


@functools.lru_cache(maxsize=None)
def tsum_case(shape, C, T):
    """f32 values over twelve decades, so that the f64 order of the t and of the channel sums shows"""
    rng = np.random.default_rng(C * 100 + T + shape[2])
    ts = [(rng.random(shape + (C,)) * 10.0 ** rng.uniform(-6, 6, shape + (C,))).astype(np.float32) for _ in range(T)]
    sh = np.array(TSUM_SHIFTS[:T], np.int32)
    s, m = MR.tsum_masked(ts, sh)
    for a in ts + [s, m, sh]:
        a.setflags(write=False)
    return ts, sh, s, m


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("C", [1, 3, 14, 20, 128])      # chunks of 512, 512, 128, 96 and 32 voxels
@pytest.mark.parametrize("shape", [(9, 7, 70), (16, 12, 8)], ids=str)
def test_tsum_masked_equals_restatement(K, shape, C, T):
    ts, sh, want, wmask = tsum_case(shape, C, T)
    got, mask = K.volume_tsum_masked([dev(a) for a in ts], dev(sh))
    assert mask.dtype == torch.uint8 and np.array_equal(host(mask), wmask.astype(np.uint8))
    assert got.dtype == torch.float64 and np.array_equal(host(got), want)
    if T == 1:
        assert wmask.all() and np.array_equal(want, np.sum(ts[0].astype(np.float64), axis=3))
    else:
        assert 0 < wmask.sum() < wmask.size and (want[~wmask] == 0).all()
        got2, mask2 = K.volume_tsum_masked([dev(a) for a in ts], [tuple(s) for s in sh])      # host triples
        assert np.array_equal(host(got2), want) and np.array_equal(host(mask2), host(mask))


def test_tsum_shift_of_the_extent_leaves_no_coverage(K):
    ts, _, _, _ = tsum_case((16, 12, 8), 3, 4)
    sh = np.array([(0, 0, 0), (1, 0, 0), (0, -12, 2), (0, 1, 0)], np.int32)      # -12: the whole of Y
    want, wmask = MR.tsum_masked(ts, sh)
    assert not wmask.any() and not want.any()
    got, mask = K.volume_tsum_masked([dev(a) for a in ts], dev(sh))
    assert not host(mask).any() and np.array_equal(host(got), want)


def test_tile_tsum_equals_the_fixture(P, g):
    for k, ts in enumerate(MR.golden_case()):
        s, m, sh = P.tile_tsum([dev(a) for a in ts], want_shifts=True)
        assert np.array_equal(host(sh), g["t_shifts_k%d" % k]) and sh.dtype == torch.int32
        assert np.array_equal(host(m), g["mask_k%d" % k])
        assert np.array_equal(host(s), g["sum_filtered_k%d" % k])
    s1, m1 = P.tile_tsum([dev(MR.golden_case()[0][0])])                    # T = 1
    assert host(m1).all() and np.array_equal(host(s1), np.sum(MR.golden_case()[0][0].astype(np.float64), axis=3))


def test_tsum_rejects_bad_arguments(K):
    a = dev(MR.golden_case()[0][0])
    with pytest.raises(ValueError):
        K.volume_tsum_masked([a, a[:8]], [(0, 0, 0)] * 2)
    with pytest.raises(ValueError):
        K.volume_tsum_masked([a, a], [(0, 0, 0)])
    with pytest.raises(ValueError):
        K.volume_tsum_masked([a.repeat(1, 1, 1, 43)], [(0, 0, 0)])         # 129 channels
    with pytest.raises(ValueError):
        K.volume_tsum_masked([a] * 17, [(0, 0, 0)] * 17)


# ---- stage 2: neighbour shifts ---------------------------------------------------------------------
def test_tile_shifts_equal_the_fixture(P, g):
    sums, _ = tiles_of(g)
    got = P.estimate_tile_shifts([dev(s) for s in sums], G["n"], G["ov"])
    assert got.dtype == torch.int32 and tuple(got.shape) == (2, 2, 3)
    assert np.array_equal(host(got), g["shifts"])


# ---- stages 3 and 4: placement and accumulation ----------------------------------------------------
def random_tiles(n, tile, seed):
    """sums over twelve decades (the order of the four-tile `+=` shows) and masks with holes"""
    rng = np.random.default_rng(seed)
    sums = [rng.random(tile) * 10.0 ** rng.uniform(-6, 6, tile) for _ in range(n * n)]
    masks = [(rng.random(tile) < 0.85) for _ in range(n * n)]
    return [s * m for s, m in zip(sums, masks)], masks


def accumulate_both(K, sums, masks, org, canvas):
    want, wcount = MR.accumulate(sums, masks, org, canvas)
    full, count = K.mosaic_accumulate3([dev(s) for s in sums], [dev(m.astype(np.uint8)) for m in masks], org, canvas,
                                       want_count=True)
    assert full.dtype == torch.float64 and count.dtype == torch.int32 and tuple(full.shape) == tuple(canvas)
    assert np.array_equal(host(count), wcount)
    assert np.array_equal(host(full), want)
    only = K.mosaic_accumulate3([dev(s) for s in sums], [dev(m) for m in masks], org, canvas)       # bool masks, no count
    assert np.array_equal(host(only), want)
    return want, wcount


def test_accumulate_one_tile(K):
    sums, masks = random_tiles(1, (9, 7, 70), 1)
    org, canvas = MR.origins(np.zeros((1, 1, 3), np.int32), (9, 7, 70), 4, 10)
    want, wcount = accumulate_both(K, sums, masks, org, canvas)
    assert np.array_equal(want[10:19, 10:17, 10:80], sums[0] * masks[0]) and wcount.max() == 1
    assert not want[:10].any() and not want[:, :, 80:].any()             # voxels under no tile


def test_accumulate_the_fixture(K, g):
    sums, masks = tiles_of(g)
    want, wcount = accumulate_both(K, sums, [m.astype(bool) for m in masks], g["origins"], g["full"].shape)
    assert np.array_equal(want, g["full"]) and np.array_equal(wcount, g["count"])
    assert sorted(np.unique(wcount).tolist()) == [1, 2, 3, 4]            # a corner under all four tiles


def test_accumulate_three_by_three_with_distinct_shifts(K):
    n, tile, ov, m = 3, (12, 10, 6), 4, 10
    rng = np.random.default_rng(33)
    shifts = rng.integers(-1, 2, (n, n, 3)).astype(np.int32)
    shifts[0, 0] = 0
    shifts[1, 0] = (1, -1, 1)
    shifts[2, 0] = (-1, 1, -1)
    org, canvas = MR.origins(shifts, tile, ov, m)
    # both prefix rules: x carries column 0 of the rows above, y and z do not
    assert org[2 * n + 1][0] == 2 * tile[0] - 2 * ov + (1 - 1) + shifts[2, 1, 0] + m
    assert org[2 * n + 1][1] == tile[1] - ov + shifts[2, 0, 1] + shifts[2, 1, 1] + m
    assert org[2 * n + 1][2] == shifts[2, 0, 2] + shifts[2, 1, 2] + m
    sums, masks = random_tiles(n, tile, 34)
    want, wcount = accumulate_both(K, sums, masks, org, canvas)
    boxes = np.zeros(canvas, np.int32)
    for o in org:
        boxes[tuple(slice(int(a), int(a) + t) for a, t in zip(o, tile))] += 1
    assert boxes.max() == 4 and wcount.max() == 4                         # a corner under four tiles
    assert ((boxes >= 2) & (wcount < boxes) & (wcount >= 1)).any()        # the count follows the mask, not the box
    assert ((boxes >= 1) & (np.maximum(wcount, 1) == 1) & (want == 0)).any()
    assert (boxes == 0).any() and not want[boxes == 0].any()


def test_accumulate_boxes_at_and_past_the_canvas_faces(K):
    tile, canvas = (5, 4, 3), (9, 8, 7)
    sums, masks = random_tiles(1, tile, 5)
    for org in ([(4, 4, 4)], [(0, 0, 0)]):                                # flush with the faces: allowed
        want, _ = accumulate_both(K, sums, masks, np.array(org, np.int32), canvas)
        assert want.any()
    s, mk = dev(sums[0]), dev(masks[0].astype(np.uint8))
    for org in ([(5, 4, 4)], [(4, 5, 4)], [(4, 4, 5)], [(-1, 0, 0)], [(0, -1, 0)], [(0, 0, -1)]):
        from hiprfish_image_analysis_amd import _lib
        with pytest.raises(_lib.HrfValueError, match="leaves the canvas"):
            K.mosaic_accumulate3([s], [mk], org, canvas)
        # nothing was launched: a buffer handed to the entry point keeps its contents
        full = torch.full(canvas, 7.0, dtype=torch.float64, device="cuda")
        sp, mp = (ctypes.c_void_p * 1)(s.data_ptr()), (ctypes.c_void_p * 1)(mk.data_ptr())
        o = np.array(org, np.int32).reshape(-1)
        with pytest.raises(_lib.HrfValueError):
            _lib.call("hrf_mosaic_accumulate3", ctypes.cast(sp, ctypes.c_void_p), ctypes.cast(mp, ctypes.c_void_p),
                      o.ctypes.data, 1, *tile, *canvas, full.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool((full == 7.0).all())
    with pytest.raises(_lib.HrfValueError, match="64 tiles"):
        K.mosaic_accumulate3([s] * 65, [mk] * 65, [(0, 0, 0)] * 65, canvas)
    with pytest.raises(ValueError):
        K.mosaic_accumulate3([s], [mk], [(0, 0, 0)] * 2, canvas)


def test_stitch_equals_the_fixture(P, g):
    tiles = [[dev(a) for a in ts] for ts in MR.golden_case()]
    norm, keep = P.stitch_volume_tiles(tiles, G["n"], overlap=G["ov"], margin=G["margin"])
    assert np.array_equal(host(keep["shifts"]), g["shifts"])
    assert np.array_equal(keep["origins"], g["origins"])
    assert np.array_equal(host(keep["full"]), g["full"])
    assert np.array_equal(host(keep["count"]), g["count"])
    assert np.array_equal(host(norm), g["norm"]) and float(norm.max()) == 1.0
    from hiprfish_image_analysis_amd import _lib
    with pytest.raises(_lib.HrfValueError):                               # a margin the shifts do not fit in
        P.stitch_volume_tiles(tiles, G["n"], overlap=G["ov"], margin=0)
    with pytest.raises(_lib.HrfValueError):
        P.stitch_volume_tiles([tiles[0][:1]] * 81, 9, overlap=G["ov"])    # more than 64 tiles


# ---- stage 5: enhancement, the + 1e-8 form ---------------------------------------------------------
def test_enhance_eps_equals_the_fragment(K, g):
    got = K.enhance_3d_eps(dev(g["e_chunk"]))
    assert got.dtype == torch.float64 and np.array_equal(host(got), g["e_final"])


def test_enhance_eps_on_a_pad_that_is_no_multiple_of_the_kernel_tile(K):
    rng = np.random.default_rng(21)
    pad = rng.random((17, 19, 47)) ** 3                                   # outputs 7 x 9 x 37: tiles of 4 x 4 x 32
    pad[4:9, :, 20:] = 0.0
    assert np.array_equal(host(K.enhance_3d_eps(dev(pad))), MR.enhance_eps(pad))


def test_enhance_eps_chunks_leave_the_reference_s_zero_tail(K, g):
    pad = np.pad(g["norm"], 5, mode="edge")
    c = G["chunk"] * G["nchunk"]
    got = host(K.enhance_3d_eps(dev(pad), chunk=G["chunk"]))
    assert np.array_equal(got, g["final"])
    assert not got[c:].any() and not got[:, c:].any()
    whole = host(K.enhance_3d_eps(dev(pad)))
    assert np.array_equal(whole[:c, :c], g["final"][:c, :c])
    assert whole[c:].any() and whole[:, c:].any()                         # real data the chunks do not reach
    assert not host(K.enhance_3d_eps(dev(pad), chunk=100)).any()          # no whole chunk at all
    with pytest.raises(ValueError):
        K.enhance_3d_eps(dev(pad), chunk=0)


def test_enhance_eps_special_values_take_the_compare_select_path(K):
    """a kernel tile holding -0.0 and magnitudes of 2^1023 (of both signs: a window's range overflows
    and (c - mn) / inf or inf / inf follow) equals the restatement's compare-select recurrences"""
    rng = np.random.default_rng(22)
    pad = rng.random((18, 18, 50))
    pad[3:6, 3:9, 5:12] = -0.0
    pad[5, 5, 8] = 0.0
    pad[9, 7, 20] = 2.0 ** 1023
    pad[12, 10, 40] = 2.0 ** 1023
    pad[12, 10, 41] = -(2.0 ** 1023)
    want = MR.enhance_eps(pad)
    assert np.isnan(want).any() and np.isfinite(want).any()
    got = host(K.enhance_3d_eps(dev(pad)))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got, want, equal_nan=True)


# ---- stage 6: segmentation -------------------------------------------------------------------------
NAMES = ["rough_mask", "rsf", "opened", "small", "bfh", "rough_bfh", "watershed_mask", "seeds", "bkg_mask", "seeds_bkg",
         "watershed_mask_bkg", "watershed"]


def test_segment_volume_with_the_mosaic_background(P, g, gseg):
    norm = g["norm"]
    assert (norm[:10] == 0).all() and (norm > 0).any()                    # zero margins
    keep: dict = {}
    seg, n, final_bkg = P.segment_volume(dev(g["final"]), dev(norm), keep, background="log10eps_positive")
    for name in NAMES:
        assert np.array_equal(host(keep[name]).astype(np.int64), np.asarray(gseg[name]).astype(np.int64)), name
    assert not host(keep["bkg_mask"])[norm <= 0].any()
    assert np.array_equal(host(seg), gseg["seg"]) and n == gseg["n"] and n >= 2
    assert np.array_equal(host(final_bkg), gseg["final_bkg"])
    assert np.allclose(sorted(keep["centers_bkg"]), sorted(gseg["centers_bkg"]), rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        P.segment_volume(dev(g["final"]), dev(norm), background="log10")


def test_segment_volume_default_background_still_equals_volume3d(P, golden):
    v = golden("volume3d")
    keep: dict = {}
    seg, n, final_bkg = P.segment_volume(dev(v["c_final"].astype(np.float64)), dev(v["c_reg_sum"].astype(np.float64)),
                                         keep)
    assert np.array_equal(host(seg), v["c_seg"]) and n == int(v["c_n"])
    assert np.array_equal(host(keep["bkg_mask"]), v["c_bkg_mask"])
    assert np.array_equal(host(final_bkg), v["c_final"].astype(np.float64) * v["c_bkg_mask"])


def test_segment_volume_mosaic_end_to_end(P, g, gseg):
    tiles = [[dev(a) for a in ts] for ts in MR.golden_case()]
    keep: dict = {}
    seg, n, final_bkg, norm = P.segment_volume_mosaic(tiles, G["n"], overlap=G["ov"], margin=G["margin"],
                                                      chunk=G["chunk"], keep=keep)
    assert np.array_equal(host(keep["shifts"]), g["shifts"])
    assert np.array_equal(keep["origins"], g["origins"])
    assert np.array_equal(host(keep["full"]), g["full"])
    assert np.array_equal(host(keep["count"]), g["count"])
    assert np.array_equal(host(norm), g["norm"])
    assert np.array_equal(host(keep["final"]), g["final"])
    assert np.array_equal(host(seg), gseg["seg"]) and n == gseg["n"] and seg.dtype == torch.int32
    assert np.array_equal(host(final_bkg), gseg["final_bkg"])
