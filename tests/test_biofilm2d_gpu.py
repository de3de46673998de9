"""The 2-D biofilm path on the device (csrc/biofilm2d.hip, kernels.*_disk / log / log10 /
cluster_positive_means / largest_label, pipeline.register_biofilm_2d / segment_biofilm_2d,
biofilm.measure_biofilm_2d) against tests/biofilm2d_ref.py, itself checked against scipy.ndimage in
tests/test_biofilm2d_ref.py.

Disk shapes: the five of the restatement's own check, a radius close to H (128, 300, 100), a radius
beyond both sides (30, 30, 100), and (257, 65, 3): W off a wave multiple, nine row bands of 32."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import biofilm2d_ref as R  # noqa: E402

SMALL = [(40, 53, 6), (17, 90, 20), (64, 7, 9), (50, 50, 1), (33, 41, 13)]
LARGE = [(128, 300, 100), (30, 30, 100), (257, 65, 3)]


@pytest.fixture(scope="module")
def K():
    from hiprfish_image_analysis_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def P():
    from hiprfish_image_analysis_amd import pipeline
    return pipeline


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def live():
    from hiprfish_image_analysis_amd import _lib
    return _lib.lib().hrf_live_allocations()


# ---- disk morphology ---------------------------------------------------------------------------
def check_disk(K, m, r, dilate):
    d = dev(m.astype(np.uint8))
    got = host(K.binary_dilation_disk(d, r))
    assert got.dtype == np.uint8 and np.array_equal(got.astype(bool), dilate(m, r)), "dilation"
    for bv in (1, 0):
        got = host(K.binary_erosion_disk(d, r, border_value=bv))
        assert np.array_equal(got.astype(bool), R.erode_disk(m, r, bv, dilate)), ("erosion", bv)
    closed = host(K.binary_closing_disk(d, r))
    assert np.array_equal(closed.astype(bool), R.closing_disk(m, r, dilate)), "closing"
    two = host(K.binary_erosion_disk(K.binary_dilation_disk(d, r), r, border_value=1))
    assert np.array_equal(closed, two), "closing is dilation then erosion"


def special_masks(H, W):
    yield "zeros", np.zeros((H, W), bool)
    yield "ones", np.ones((H, W), bool)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        m = np.zeros((H, W), bool)
        m[y, x] = True
        yield "corner %d %d" % (y, x), m
    m = np.ones((H, W), bool)
    m[H // 2, W // 3] = False
    yield "all but one", m


@pytest.mark.parametrize("density", [0.002, 0.1, 0.97])
@pytest.mark.parametrize("shape", SMALL)
def test_disk_random_masks(K, shape, density):
    H, W, r = shape
    rng = np.random.default_rng(H * 1000 + W * 10 + int(density * 1000))
    check_disk(K, rng.random((H, W)) < density, r, R.dilate_disk)


@pytest.mark.parametrize("shape", SMALL)
def test_disk_special_masks(K, shape):
    H, W, r = shape
    for name, m in special_masks(H, W):
        check_disk(K, m, r, R.dilate_disk)


@pytest.mark.parametrize("shape", LARGE)
def test_disk_large_radius_and_row_bands(K, shape):
    H, W, r = shape
    rng = np.random.default_rng(H + W + r)
    check_disk(K, rng.random((H, W)) < 0.002, r, R.dilate_disk_rows)
    check_disk(K, rng.random((H, W)) < 0.3, r, R.dilate_disk_rows)
    for name, m in special_masks(H, W):
        check_disk(K, m, r, R.dilate_disk_rows)


def test_disk_rejects_bad_arguments_and_leaks_nothing(K):
    from hiprfish_image_analysis_amd import _lib
    m = dev(np.ones((20, 30), np.uint8))
    torch.cuda.synchronize()
    before = live()
    for r in (0, 1024, -3):
        with pytest.raises(_lib.HrfError):
            K.binary_dilation_disk(m, r)
        with pytest.raises(_lib.HrfError):
            K.binary_erosion_disk(m, r)
        with pytest.raises(_lib.HrfError):
            K.binary_closing_disk(m, r)
    need = int(_lib.lib().hrf_disk_workspace_bytes(20, 30, 5))
    assert need >= 2 * 20 * 30
    small = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.HrfError):
        K.binary_dilation_disk(m, 5, work=small)
    with pytest.raises(_lib.HrfError):
        K.binary_erosion_disk(m, 5, work=small)
    with pytest.raises(_lib.HrfError):
        K.binary_erosion_disk(m, 5, border_value=2)
    assert int(_lib.lib().hrf_disk_workspace_bytes(20, 30, 0)) < 0
    assert int(_lib.lib().hrf_disk_workspace_bytes(20, 30, 1024)) < 0
    assert int(_lib.lib().hrf_disk_workspace_bytes(1 << 16, 1 << 15, 5)) < 0        # H * W = 2^31
    torch.cuda.synchronize()
    assert live() == before
    ok = torch.empty(need, dtype=torch.uint8, device="cuda")                          # the exact size serves
    assert host(K.binary_dilation_disk(m, 5, work=ok)).all()


# ---- log, log10 --------------------------------------------------------------------------------
def test_log_and_log10_are_the_correctly_rounded_ones(K, orc):
    rng = np.random.default_rng(8)
    x = np.concatenate([rng.random(3000), 10.0 ** rng.uniform(-300, 300, 3000), rng.uniform(0.5, 2.0, 3000),
                        [5e-324, 1e-310, 2.2250738585072014e-308, 1.0, 10.0, 1e22, 0.0, np.inf]])
    with np.errstate(divide="ignore"):
        want10, want = orc.cr_log10(x), orc.cr_log(x)
    got10, got = host(K.log10(dev(x))), host(K.log(dev(x)))
    assert np.array_equal(got10.view(np.int64), want10.view(np.int64))
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    assert got10[-2] == -np.inf and got10[-1] == np.inf and got[-2] == -np.inf and got[-1] == np.inf
    assert got10[-4] == 1.0 and got10[-5] == 0.0
    img = rng.random((5, 7))
    assert K.log10(dev(img)).shape == (5, 7)


# ---- cluster_positive_means --------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 70001, 600 * 512 + 17])        # one thread, one block, many, past the grid
def test_cluster_positive_means(K, n):
    rng = np.random.default_rng(n)
    lab = rng.integers(0, 3, n).astype(np.int32)
    val = rng.random(n) * 10.0 ** rng.uniform(-3, 3, n)
    val[rng.random(n) < 0.2] = 0.0
    val[rng.random(n) < 0.1] *= -1.0
    val[lab == 2] = -np.abs(val[lab == 2])                                # cluster 2: no positive value
    if n > 10:
        val[5] = np.nan
    sums, counts = K.cluster_positive_means(dev(lab), dev(val), 4)
    sums2, counts2 = K.cluster_positive_means(dev(lab), dev(val), 4)
    s, c = host(sums), host(counts)
    assert c.dtype == np.int64 and s.dtype == np.float64
    assert np.array_equal(s.view(np.int64), host(sums2).view(np.int64)) and np.array_equal(c, host(counts2))
    for j in range(4):
        sel = (lab == j) & (val > 0)
        assert c[j] == sel.sum()
        want = math.fsum(val[sel].tolist())
        assert abs(s[j] - want) <= 1e-12 * want, (j, s[j], want)
    assert c[2] == 0 and s[2] == 0.0 and c[3] == 0 and s[3] == 0.0
    with np.errstate(invalid="ignore"):
        assert np.isnan((s / c)[3])                                       # the chain's NaN mean


def test_cluster_positive_means_rejects_k(K):
    lab, val = dev(np.zeros(4, np.int32)), dev(np.ones(4))
    for k in (0, 65):
        with pytest.raises(ValueError):
            K.cluster_positive_means(lab, val, k)


# ---- largest_label -----------------------------------------------------------------------------
def test_largest_label(K):
    rng = np.random.default_rng(2)
    lab = rng.integers(0, 40, (97, 131)).astype(np.int32)
    lab[lab == 17] = 0                                                    # a label missing in the middle
    lab[:30, :50] = 23
    assert K.largest_label(dev(lab), 39) == R.largest_label(lab, 39) == (23, int((lab == 23).sum()))
    assert K.largest_label(dev(lab), 20) == R.largest_label(lab, 20)      # labels above maxlab do not count
    tie = np.zeros((40, 70), np.int32)
    tie[3, :60] = 9
    tie[20, :60] = 4
    tie[30, :59] = 2
    tie[35, :60] = 300
    assert K.largest_label(dev(tie), 300) == (4, 60) == R.largest_label(tie, 300)
    assert K.largest_label(dev(np.zeros((9, 9), np.int32)), 12) == (0, 0)
    assert K.largest_label(dev(np.zeros((9, 9), np.int32)), 0) == (0, 0)
    big = np.full((600, 700), 3, np.int32)                                # one label, many waves
    big[0, 0] = 1
    assert K.largest_label(dev(big), 3) == (3, 600 * 700 - 1)
    out = K.largest_label(dev(tie), 300, sync=False)
    assert out.dtype == torch.int32 and out.tolist() == [4, 60]


# ---- registration ------------------------------------------------------------------------------
def smooth_lasers():
    """four acquisitions (23, 20, 14, 6 channels) cut from one smooth positive image at known offsets"""
    H, W, m = 96, 128, 12
    rng = np.random.default_rng(40)
    yy, xx = np.mgrid[0:H + 2 * m, 0:W + 2 * m].astype(np.float64)
    big = np.full(yy.shape, 0.2)
    for _ in range(30):
        cy, cx, sg = rng.uniform(0, H + 2 * m), rng.uniform(0, W + 2 * m), rng.uniform(3, 9)
        big += rng.uniform(0.3, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sg * sg))
    moves = [(0, 0), (3, -5), (-7, 2), (4, 6)]
    lasers = []
    for (dr, dc), C in zip(moves, R.LASER_CHANNELS):
        w = rng.uniform(0.5, 1.5, C)
        lasers.append((big[m - dr:m - dr + H, m - dc:m - dc + W, None] * w).astype(np.float32))
    return lasers, moves


def test_register_biofilm_2d(K, P, orc):
    lasers, moves = smooth_lasers()
    want, shifts = R.register_biofilm_2d_ref(lasers)
    # register_translation undoes the move, to a pixel: the crops differ at their borders
    assert all(abs(sr + dr) <= 1 and abs(sc + dc) <= 1 for (sr, sc), (dr, dc) in zip(shifts, moves))
    assert all(abs(sr) + abs(sc) >= 5 for sr, sc in shifts[1:])
    dl = [dev(l) for l in lasers]
    got = P.estimate_shifts(dl, reduce="logsum", clamp=None, device=True)
    assert [tuple(v) for v in host(got).tolist()] == shifts
    assert P.estimate_shifts(dl, reduce="logsum", clamp=None) == shifts
    reg = P.register_biofilm_2d(dl)
    assert reg.dtype == torch.float32 and tuple(reg.shape) == (96, 128, 63)
    assert np.array_equal(host(reg), want)
    lo = 0
    for (sr, sc), C in zip(shifts, R.LASER_CHANNELS):                     # zeros outside each shifted frame only
        frame = np.zeros((96, 128), bool)
        frame[max(0, sr):96 + min(0, sr), max(0, sc):128 + min(0, sc)] = True
        assert (want[:, :, lo:lo + C][~frame] == 0).all() and (want[:, :, lo:lo + C][frame] > 0).all()
        lo += C
    assert np.array_equal(host(P.register_biofilm_2d(dl, shifts=shifts)), want)


# ---- the whole chain ---------------------------------------------------------------------------
MASKS = ["rough_mask", "opened", "small", "bfh", "rough_bfh", "bkg_mask", "watershed_mask", "flood_mask", "image_bkg",
         "image_bkg_bfh", "bkg_closed", "bkg_final", "bkg_dilated", "epithelial_area"]
LABELS = ["bkg_labels", "seeds", "watershed", "adjacency_watershed", "seg", "adjacency_seg", "bkg_objects",
          "objects_overall", "objects_overall_seg"]
IMAGES = ["image_sum", "norm", "nl", "final", "nl_log", "final_bkg", "sum_bkg"]


def check_chain(P, quantise):
    ref = R.scene_reference(quantise)
    keep = {}
    out = P.segment_biofilm_2d(dev(ref["stack"]), keep=keep, **R.SCENE_KW)
    rk = ref["keep"]
    for name in IMAGES:
        assert np.array_equal(host(keep[name]), rk[name]), name
    for name in MASKS:
        assert np.array_equal(host(keep[name]).astype(bool), rk[name]), name
    for name in LABELS:
        assert np.array_equal(host(keep[name]), rk[name]), name
    assert keep["nseeds"] == rk["nseeds"]
    seg, n, adj, n_adj, s, final_bkg, epi = out
    rseg, rn, radj, rn_adj, rs, rfinal_bkg, repi = ref["out"]
    assert (n, n_adj) == (rn, rn_adj) and n >= 8
    assert np.array_equal(host(seg), rseg) and np.array_equal(host(adj), radj)
    assert np.array_equal(host(s), rs) and np.array_equal(host(final_bkg), rfinal_bkg)
    assert epi.dtype == torch.uint8 and np.array_equal(host(epi).astype(bool), repi)
    i0, i1 = keep["cluster_means"]
    assert abs(i0 - rk["cluster_means"][0]) <= 1e-12 * i0 and abs(i1 - rk["cluster_means"][1]) <= 1e-12 * i1
    print("ties [contested, rounds, marker ties]: cells %s, adjacency %s, epithelial %s"
          % (keep["ties"], keep["ties_adjacency"], keep["ties_epithelial"]))
    assert all(len(keep[k]) == 3 for k in ("ties", "ties_adjacency", "ties_epithelial"))
    return out, keep


def test_segment_biofilm_2d(P, orc):
    check_chain(P, False)


def test_segment_biofilm_2d_quantised(P, orc):
    check_chain(P, True)


def test_segment_biofilm_2d_without_epithelial(P, orc):
    ref = R.scene_reference(False)
    keep = {}
    seg, n, adj, n_adj, s, final_bkg, epi = P.segment_biofilm_2d(dev(ref["stack"]), keep=keep, epithelial=False)
    assert epi is None and "epithelial_area" not in keep and "bkg_closed" not in keep
    assert n == ref["out"][1] and np.array_equal(host(seg), ref["out"][0])
    assert n_adj == ref["out"][3] and np.array_equal(host(adj), ref["out"][2])


def test_segment_biofilm_2d_empty_stages_raise(P, orc):
    ref = R.scene_reference(False)
    stack = dev(ref["stack"])
    with pytest.raises(ValueError, match="background"):                   # nothing survives bkg_min_size
        P.segment_biofilm_2d(stack, disk_radius=8, bkg_min_size=160 * 160 + 1)
    with pytest.raises(ValueError, match="covers the image"):             # 1 - bd is empty
        P.segment_biofilm_2d(stack, disk_radius=150, bkg_min_size=300)
    with pytest.raises(ValueError):
        R.segment_biofilm_2d_ref(ref["stack"], disk_radius=8, bkg_min_size=160 * 160 + 1)
    dark = ref["stack"].copy()
    dark[:48, :48] = 0.0                                                  # NL-means of an all-zero window is 0
    with pytest.raises(ValueError, match="not positive"):
        P.segment_biofilm_2d(dev(dark), **R.SCENE_KW)
    with pytest.raises(ValueError):
        R.segment_biofilm_2d_ref(dark, **R.SCENE_KW)


# ---- the report --------------------------------------------------------------------------------
def classifier_bundle(tmp_path):
    """the stand-in bundle of tests/test_biofilm_gpu.py, fitted on the scene's six spectra"""
    from types import SimpleNamespace

    from sklearn.preprocessing import StandardScaler
    from sklearn.svm import SVC
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools.export_classifier import export_bundle
    from hiprfish_image_analysis_amd import backend as B
    rng = np.random.default_rng(31)
    spectra = R.scene_spectra()
    y = np.repeat(np.arange(6), 30)
    xt = spectra[y] * rng.uniform(0.8, 1.2, (len(y), 1)) + rng.normal(0, 0.02 * spectra.max(), (len(y), 63))
    xt /= xt.max(axis=1, keepdims=True)
    sc = StandardScaler().fit(xt)
    xs = sc.transform(xt)
    feats = np.zeros((len(y), 67))
    feats[:, :63] = xt
    checks = []
    for k, (lo, hi) in enumerate(B.MULTI_SEGMENTS):
        seg_max = xt[:, lo:hi].max(axis=1)
        lab = np.zeros(len(y))
        lab[np.argsort(seg_max, kind="stable")[len(y) // 2:]] = 1.0
        checks.append(SVC(kernel="linear", C=1.0).fit(xs[:, lo:hi], lab))
        feats[:, 63 + k] = checks[-1].predict(xs[:, lo:hi])
    emb = (rng.normal(0, 5, (6, 2))[y] + rng.normal(0, 0.4, (len(y), 2))).astype(np.float32)
    codes = np.array([format(v + 1, "07b") for v in y])
    clf_umap = SVC(kernel="rbf", gamma=0.5, C=10.0, probability=True, random_state=0).fit(emb.astype(float), codes)
    um = SimpleNamespace(_raw_data=feats, embedding_=emb, n_neighbors=15, local_connectivity=1.0,
                         metric=SimpleNamespace(__name__="channel_cosine_intensity_7b_v2"), _a=1.577, _b=0.8951,
                         repulsion_strength=1.0, negative_sample_rate=5, n_epochs=None, _initial_alpha=1.0)
    path = str(tmp_path / "bundle.npz")
    export_bundle(path, um, clf_umap, checks, sc)
    return B.ClassifierModel.load(path)


def test_measure_biofilm_2d(tmp_path, orc):
    import pandas as pd
    from hiprfish_image_analysis_amd import biofilm
    model = classifier_bundle(tmp_path)
    taxon_codes = [format(v + 1, "07b") for v in range(5)]
    ref = R.scene_reference(False)
    rseg, rn, radj, rn_adj, rs, rfinal_bkg, repi = ref["out"]
    sample = str(tmp_path / "fov")
    out = biofilm.measure_biofilm_2d(sample, [dev(l) for l in ref["lasers"]], model, taxon_codes, **R.SCENE_KW)
    # the scene's acquisitions are unshifted, so the registered stack is their concatenation
    saved = {k: np.load("{}_{}.npy".format(sample, k)) for k in ("registered", "seg", "adjacency_seg",
                                                                 "epithelial_area")}
    assert saved["registered"].dtype == np.float64 and np.array_equal(saved["registered"], ref["stack"])
    assert np.array_equal(saved["seg"], rseg) and np.array_equal(saved["adjacency_seg"], radj)
    assert saved["epithelial_area"].dtype == bool and np.array_equal(saved["epithelial_area"], repi)
    assert np.array_equal(host(out["segmentation"]), rseg) and np.array_equal(host(out["image_registered_sum"]), rs)
    for suffix in ("_cell_information.csv", "_cell_information_filtered.csv", "_avgint.csv", "_avgint_filtered.csv",
                   "_adjacency_matrix.csv", "_adjacency_matrix_filtered.csv"):
        assert os.path.exists(sample + suffix)
    want = biofilm.cell_report(sample, dev(ref["stack"]), dev(rseg), dev(radj), model, taxon_codes,
                               epithelial_area=dev(repi.astype(np.uint8)), write=False)
    # the same arrays in, so the same frames out -- up to the order of label_sums' f64 atomic adds,
    # which differs between two runs in the last bits (~1e-16 relative) of a cell's mean spectrum
    for name in ("cell_info", "cell_info_filtered", "avgint", "avgint_filtered", "adjacency", "adjacency_filtered"):
        pd.testing.assert_frame_equal(out[name], want[name], check_exact=False, rtol=1e-9, atol=1e-12)
    assert len(out["cell_info"]) == rn
    with pytest.raises(ValueError):
        biofilm.measure_biofilm_2d(sample, [dev(l) for l in ref["lasers"]], model, taxon_codes, epithelial=False)
