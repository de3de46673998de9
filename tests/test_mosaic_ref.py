"""The mosaic yardstick itself (tests/mosaic_ref.py) against what the reference's own lines
computed (tests/golden/mosaic.npz, tests/golden/make_mosaic_golden.py), the placement's error
cases, the mosaic CZI loader and the exported ABI.  No device here."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mosaic_ref as MR  # noqa: E402
from czi_writer import write_czi  # noqa: E402

from hiprfish_image_analysis_amd import _lib, czi  # noqa: E402

G = MR.GOLDEN
NAMES = ["hrf_volume_tsum_masked_dev", "hrf_mosaic_accumulate3", "hrf_enhance_3d_eps"]


@pytest.fixture(scope="module")
def g(golden):
    return golden("mosaic")


@pytest.fixture(scope="module")
def st(orc):
    """the restatement's stitch and enhancement of the golden case, computed once"""
    s = MR.stitch(MR.golden_case(), G["n"], G["ov"], G["margin"])
    s["pad"] = np.pad(s["norm"], 5, mode="edge")
    s["final"] = MR.enhance_eps(s["pad"], G["chunk"])
    return s


def test_inputs_are_the_recorded_ones(g):
    for k, ts in enumerate(MR.golden_case()):
        for t, a in enumerate(ts):
            assert a.dtype == np.float32 and np.array_equal(a, g["in_k%d_t%d" % (k, t)])


def test_stitch_equals_the_fragments_at_every_stage(g, st):
    n = G["n"]
    for k in range(n * n):
        assert np.array_equal(st["t_shifts"][k], g["t_shifts_k%d" % k]), k
        assert np.array_equal(st["t_shifts"][k], np.array(G["t_offsets"])), k      # the planted time shifts
        assert np.array_equal(st["masks"][k], g["mask_k%d" % k].astype(bool)), k
        assert np.array_equal(st["sum_filtered"][k], g["sum_filtered_k%d" % k]), k
        assert 0 < st["masks"][k].sum() < st["masks"][k].size
    assert np.array_equal(st["shifts"], g["shifts"])
    assert np.array_equal(st["origins"], g["origins"])
    assert np.array_equal(st["full"], g["full"]) and st["full"].dtype == np.float64
    assert np.array_equal(st["count"], g["count"])
    assert np.array_equal(st["norm"], g["norm"])
    assert st["full"].shape == (68, 68, 28)


def test_golden_case_is_not_degenerate(g):
    off = np.array(G["tile_offsets"])
    assert np.array_equal(g["shifts"].reshape(-1, 3)[1:], [off[1] - off[0], off[2] - off[0], off[3] - off[2]])
    assert all(np.abs(g["shifts"][..., a]).max() > 0 for a in range(3))
    ratios = [MR.peak_ratio(a, b) for _, a, b in
              MR.strip_pairs([g["sum_filtered_k%d" % k] for k in range(4)], G["n"], G["ov"])]
    assert min(ratios) >= 1.05
    assert sorted(np.unique(g["count"]).tolist()) == [1, 2, 3, 4]      # a corner under all four tiles
    # mask holes inside an overlap: a voxel under two boxes that only one mask covers
    boxes = np.zeros(g["count"].shape, np.int32)
    for o in g["origins"]:
        boxes[tuple(slice(int(a), int(a) + t) for a, t in zip(o, G["tile"]))] += 1
    assert ((boxes >= 2) & (g["count"] < boxes)).any() and ((boxes == 0) & (g["full"] == 0)).any()
    # y and z do not accumulate column 0's shifts of the row above: tile (1, 1) against a placement that did
    s = g["shifts"].astype(np.int64)
    assert s[1, 0, 1] != 0 and s[1, 0, 2] != 0


def test_enhancement_equals_the_fragments(g, st):
    assert np.array_equal(st["final"], g["final"])
    c = G["chunk"] * G["nchunk"]
    assert not g["final"][c:].any() and not g["final"][:, c:].any()
    whole = MR.enhance_eps(st["pad"])
    assert np.array_equal(whole[:c, :c], g["final"][:c, :c])          # the chunking itself changes nothing
    assert whole[c:].any() and whole[:, c:].any()                     # real data beyond the whole chunks
    assert np.array_equal(MR.enhance_eps(g["e_chunk"]), g["e_final"])
    assert (g["e_final"] == 0).any() and (g["e_final"] > 0).any()     # flat windows and live ones


def test_placement_formulas_and_errors():
    s = np.zeros((3, 3, 3), np.int32)
    s[1, 0] = (2, -3, 1)
    s[2, 0] = (-1, 2, -2)
    s[1, 1] = (1, 1, 1)
    s[2, 2] = (0, -1, 3)
    org, canvas = MR.origins(s, (20, 16, 6), 4, 10)
    assert canvas == (80, 68, 26)
    assert org[2 * 3 + 2].tolist() == [2 * 20 - 8 + (2 - 1) + 0 + 10, 2 * 16 - 8 + (2 - 1) + 10, (-2 + 3) + 10]
    assert org[1 * 3 + 1].tolist() == [20 - 4 + 2 + 1 + 10, 16 - 4 + (-3 + 1) + 10, (1 + 1) + 10]
    MR.check_boxes(org, (20, 16, 6), canvas)
    from hiprfish_image_analysis_amd import pipeline as P
    org_p, canvas_p = P.mosaic_origins(s, (20, 16, 6), 4, 10)
    assert np.array_equal(org_p, org) and org_p.dtype == np.int32 and tuple(canvas_p) == canvas
    flush = np.array([[0, 0, 0], [60, 52, 20]])
    MR.check_boxes(flush, (20, 16, 6), canvas)                        # flush with both faces: allowed
    for bad in ([[61, 0, 0]], [[0, 53, 0]], [[0, 0, 21]], [[-1, 0, 0]], [[0, 0, -1]]):
        with pytest.raises(ValueError):
            MR.check_boxes(np.array(bad), (20, 16, 6), canvas)
    with pytest.raises(ValueError):
        MR.check_boxes(np.zeros((65, 3), np.int32), (1, 1, 1), (4, 4, 4))
    with pytest.raises(ValueError):
        MR.accumulate([np.ones((2, 2, 2))], [np.ones((2, 2, 2), bool)], [[3, 0, 0]], (4, 4, 4))


def test_load_mosaic_tstacks(tmp_path):
    rng = np.random.default_rng(9)
    n, T, Z, C, H, W = 2, 2, 3, 2, 6, 5
    data = rng.integers(0, 65536, (n * n, T, H, W, Z, C), dtype=np.uint16)
    blocks = []
    for k in range(n * n):
        i, j = divmod(k, n)
        for t in range(T):
            for z in range(Z):
                for c in range(C):
                    blocks.append((data[k, t, :, :, z, c], {"X": 100 + j * 4, "Y": 50 + i * 5, "C": c, "M": k, "Z": z,
                                                            "T": t}))
    p = str(tmp_path / "mosaic.czi")
    write_czi(p, blocks)
    assert czi.get_tile_size(p) == n and czi.get_t_range(p) == T
    got = czi.load_mosaic_tstacks(p, rescale=False)
    assert len(got) == n * n and all(len(ts) == T for ts in got)
    for k in range(n * n):
        for t in range(T):
            assert got[k][t].shape == (H, W, Z, C) and np.array_equal(got[k][t], data[k, t])
    scaled = czi.load_mosaic_tstacks(p)
    assert scaled[3][1].dtype == np.float32
    assert np.array_equal(scaled[3][1], data[3, 1].astype(np.float32) / np.float32(65535.0))


def test_mosaic_symbols_declared_and_exported():
    decl = _lib.declared_functions()
    assert not [n for n in NAMES if n not in decl]
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert not [n for n in NAMES if not hasattr(L, n)]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert set(NAMES) <= exported


def test_bad_arguments_answer_without_a_device():
    """the host-side checks run before anything touches the device"""
    one = (ctypes.c_void_p * 1)(8)
    org = np.array([0, 0, 0], np.int32)
    for o, canvas in (((3, 0, 0), (4, 4, 4)), ((-1, 0, 0), (4, 4, 4)), ((0, 0, 3), (4, 4, 4))):
        org[:] = o
        with pytest.raises(_lib.HrfValueError, match="leaves the canvas"):
            _lib.call("hrf_mosaic_accumulate3", ctypes.cast(one, ctypes.c_void_p), ctypes.cast(one, ctypes.c_void_p),
                      org.ctypes.data, 1, 2, 2, 2, *canvas, 16, None, None)
    many = (ctypes.c_void_p * 65)(*([8] * 65))
    with pytest.raises(_lib.HrfValueError, match="64 tiles"):
        _lib.call("hrf_mosaic_accumulate3", ctypes.cast(many, ctypes.c_void_p), ctypes.cast(many, ctypes.c_void_p),
                  np.zeros(195, np.int32).ctypes.data, 65, 1, 1, 1, 4, 4, 4, 16, None, None)
    with pytest.raises(ValueError):
        _lib.call("hrf_volume_tsum_masked_dev", None, 0, None, 4, 4, 4, 1, None, None, None)
    with pytest.raises(ValueError):
        _lib.call("hrf_volume_tsum_masked_dev", ctypes.cast(one, ctypes.c_void_p), 1, None, 4, 4, 4, 129, 16, 16, None)
    with pytest.raises(ValueError):
        _lib.call("hrf_enhance_3d_eps", 16, 20, 20, 20, 11, 9, 9, -1, 16, None)
