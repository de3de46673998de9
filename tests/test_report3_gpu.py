"""The 3-D per-cell report on the device (csrc/report3.hip, kernels.region_props3 / rag_edges3 /
barcode_adjacency_edges / paint_planes3, pipeline.biofilm_typing_and_adjacency3,
biofilm.volume_report) against tests/report3_ref.py -- itself checked against scipy.ndimage, the
2-D oracle and the reference's recorded bvox bytes in tests/test_report3_ref.py.

Shapes cross the 4 x 4 x 64 brick on every axis and degenerate to 2-D and to a single voxel."""
import colorsys
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import report3_ref as R3  # noqa: E402
import volume_ref as VR  # noqa: E402

SHAPES = [(1, 1, 1), (1, 40, 37), (40, 1, 37), (40, 37, 1), (33, 17, 65), (5, 70, 3), (32, 48, 40)]
FLAT = [(1, 40, 37), (40, 1, 37), (40, 37, 1)]
BIG = (33, 17, 65)


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


@pytest.fixture(scope="module")
def voro():
    """the Voronoi volume the edge tests share, with its restated keys per footprint"""
    lab, n = R3.voronoi(BIG, 150, 6.0, seed=4)
    return lab, n, {conn: R3.rag_edges3(lab, conn) for conn in (1, 2, 3)}


@pytest.fixture(scope="module")
def flat2d():
    rng = np.random.default_rng(5)
    lab, n = R3.voronoi((40, 37), 60, 4.0, seed=6)
    lab[rng.random(lab.shape) < 0.02] = 0
    return lab, n


# ---- moments and props --------------------------------------------------------------------------
def check_moments(K, lab, maxlab):
    mom = R3.moments3(lab, maxlab)
    got = host(K.region_moments3(dev(lab), maxlab))
    assert got.dtype == np.int64 and np.array_equal(got, mom)
    props = host(K.region_props3(dev(lab), maxlab))
    assert props.shape == (maxlab + 1, 5)
    assert np.array_equal(props.view(np.uint64), R3.props3(mom).view(np.uint64))     # bitwise
    return mom


@pytest.mark.parametrize("shape", SHAPES)
def test_moments_random_labels(K, shape):
    rng = np.random.default_rng(hash(shape) % 2 ** 32)
    lab = rng.integers(-2, 46, shape).astype(np.int32)      # negative values, labels above maxlab = 40
    lab[lab == 17] = 0                                        # an absent label
    mom = check_moments(K, lab, 40)
    assert mom[17, 0] == 0 and mom[0].tolist() == [0, 0, 0, 0]


def test_moments_runs_of_labels(K, voro):
    lab, n, _ = voro                                          # runs along Z, several labels per wave
    check_moments(K, lab, n)


def test_moments_one_label_fills_the_volume(K):
    mom = check_moments(K, np.ones(BIG, np.int32), 1)
    assert mom[1, 0] == 33 * 17 * 65


def test_moments_sum_past_32_bits(K):
    shape = (2, 2, 1048576)
    mom = check_moments(K, np.ones(shape, np.int32), 3)
    assert mom[1].tolist() == [4 * 1048576, 2 * 1048576, 2 * 1048576, 4 * (1048575 * 1048576 // 2)]
    assert mom[1, 3] > 2e12 > 2 ** 32                         # past 32 bits


# ---- edge keys ------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [1, 2, 3])
def test_edges_voronoi(K, voro, conn):
    lab, n, want = voro
    got = K.rag_edges3(dev(lab), conn=conn)
    assert got.dtype == torch.int64 and np.array_equal(host(got), want[conn])
    assert len(want[1]) < len(want[2]) < len(want[3])         # the input tells the footprints apart


@pytest.mark.parametrize("conn", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_edges_random_labels(K, shape, conn):
    rng = np.random.default_rng(hash((shape, conn)) % 2 ** 32)
    lab = rng.integers(-1, 9, shape).astype(np.int32)        # a negative member drops the pair
    lab = np.repeat(lab, 2, axis=2)[:, :, :shape[2]]         # runs of two along Z
    assert np.array_equal(host(K.rag_edges3(dev(lab), conn=conn)), R3.rag_edges3(lab, conn))


@pytest.mark.parametrize("shape", FLAT)
def test_edges_flat_placements_equal_the_2d_kernel(K, flat2d, shape):
    lab, n = flat2d
    dense = R3.keys_of_matrix(host(K.rag_edges(dev(lab), n)))
    vol = lab.reshape(shape)
    for conn in (1, 2, 3):
        got = host(K.rag_edges3(dev(vol), conn=conn))
        assert np.array_equal(got, R3.rag_edges3(vol, conn)), conn
        if conn >= 2:                                         # the 3 x 3 window of the 2-D graph
            assert np.array_equal(got, dense), conn


def test_edges_across_a_brick_boundary(K):
    k12 = int(R3.pack(1, 2))
    two = np.zeros(BIG, np.int32)
    two[3, 3, 63], two[4, 4, 63] = 1, 2                       # an edge diagonal, across the x and y bricks
    for conn, there in ((1, False), (2, True), (3, True)):
        got = host(K.rag_edges3(dev(two), conn=conn))
        assert np.array_equal(got, R3.rag_edges3(two, conn)) and (k12 in got.tolist()) == there, conn
    two[4, 4, 63], two[4, 4, 64] = 0, 2                       # a corner, across all three
    for conn, there in ((1, False), (2, False), (3, True)):
        got = host(K.rag_edges3(dev(two), conn=conn))
        assert np.array_equal(got, R3.rag_edges3(two, conn)) and (k12 in got.tolist()) == there, conn


def test_edges_past_the_dense_limit(K):
    shape = (48, 48, 40)
    lab = np.arange(1, 48 * 48 * 40 + 1, dtype=np.int32).reshape(shape)     # 92160 labels
    from hiprfish_image_analysis_amd import _lib
    dlab = dev(lab)
    with pytest.raises(ValueError):                           # the dense matrix refuses, before it is touched
        _lib.call("hrf_rag_edges", dlab.data_ptr(), 48, 48 * 40, 92160, dlab.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    for conn in (1, 2, 3):
        got = host(K.rag_edges3(dlab, conn=conn))
        assert np.array_equal(got, R3.rag_edges3(lab, conn)), conn
        assert (got & 0xffffffff).max() == 92160 and len(got) > 92160


def test_edges_do_not_depend_on_the_capacity(K, voro):
    lab, n, want = voro
    first, small = [], []
    a = K.rag_edges3(dev(lab), attempts=first)
    b = K.rag_edges3(dev(lab), capacity=64, attempts=small)
    assert torch.equal(a, b) and np.array_equal(host(b), want[2])
    assert first == [(1 << (32 * (n + 1) - 1).bit_length(), len(want[2]), 0)]
    assert small[0][0] == 64 and small[0][2] == 1             # the first attempt overflowed
    assert [c for c, _, _ in small] == [64 * 4 ** i for i in range(len(small))]
    assert small[-1][1:] == (len(want[2]), 0)
    with pytest.raises(ValueError):
        K.rag_edges3(dev(lab), capacity=100)


# ---- adjacency from keys --------------------------------------------------------------------------
def test_adjacency_from_keys(K, voro):
    lab, n, want = voro
    rng = np.random.default_rng(12)
    bc = rng.integers(-1, 5, n + 1).astype(np.int32)          # some barcodes -1
    bc[0] = 2                                                 # a background pair would count here
    keep = (rng.random(n + 1) < 0.6).astype(np.uint8)
    keep[0] = 1
    keys = K.rag_edges3(dev(lab))
    assert int((keys >> 32).min()) == 0                       # the set holds background pairs
    adj, adjf = K.barcode_adjacency_edges(keys, dev(bc), 5, dev(keep))
    assert np.array_equal(host(adj), R3.barcode_adjacency_edges(want[2], bc, 5))
    assert np.array_equal(host(adjf), R3.barcode_adjacency_edges(want[2], bc, 5, keep))
    assert np.array_equal(host(K.barcode_adjacency_edges(keys, dev(bc), 5)), host(adj))
    fg = want[2][(want[2] >> 32) >= 1]
    assert np.array_equal(host(adj), R3.barcode_adjacency_edges(fg, bc, 5)) and host(adj).sum() > 0
    assert 0 < host(adjf).sum() < host(adj).sum()


def test_adjacency_from_keys_equals_the_dense_path(K, flat2d):
    lab, n = flat2d
    rng = np.random.default_rng(13)
    bc = rng.integers(-1, 5, n + 1).astype(np.int32)
    keep = (rng.random(n + 1) < 0.6).astype(np.uint8)
    want = K.barcode_adjacency_filtered(K.rag_edges(dev(lab), n), dev(bc), dev(keep), 5)
    got = K.barcode_adjacency_edges(K.rag_edges3(dev(lab.reshape(40, 1, 37))), dev(bc), 5, dev(keep))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and int(want[1].sum()) > 0


# ---- planes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + [(70, 3, 130)])
def test_planes(K, shape):
    rng = np.random.default_rng(hash(shape) % 2 ** 32)
    ncell = 12
    seg = rng.integers(-1, ncell + 3, shape).astype(np.int32)    # labels above ncell and below 0
    colour = rng.random((ncell + 1, 3)).astype(np.float32)
    got = host(K.paint_planes3(dev(seg), dev(colour)))
    assert got.shape == (3,) + shape[::-1] and got.dtype == np.float32
    inside = np.where((seg < 0) | (seg > ncell), 0, seg)
    for ch in range(3):
        assert np.array_equal(got[ch].ravel(), colour[inside][..., ch].flatten("F"))
    assert np.array_equal(got.reshape(3, -1), R3.planes(seg, colour))


# ---- the report -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bundle(tmp_path_factory):
    """a classifier bundle fitted as tests/test_biofilm_gpu.py fits its own (tools/time_volume_report.py)"""
    from types import SimpleNamespace
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools.time_volume_report import synthetic_bundle
    model, clf, spectra = synthetic_bundle(str(tmp_path_factory.mktemp("bundle3") / "bundle.npz"))
    taxon_codes = [format(v + 1, "07b") for v in range(5)]       # one class missing from the lookup
    return SimpleNamespace(model=model, clf=clf, spectra=spectra, taxon_codes=taxon_codes)


COLUMNS_TAIL = ["sample", "label", "centroid_x", "centroid_y", "centroid_z", "area", "type"]
SUFFIXES = ["_avgint.csv", "_cell_information.csv", "_cell_information_filtered.csv", "_avgint_filtered.csv",
            "_adjacency_matrix.csv", "_adjacency_matrix_filtered.csv"] + \
    ["_identification%s_%s.bvox" % (f, c) for f in ("", "_filtered") for c in "rgb"]


def test_volume_report(tmp_path, K, bundle):
    from hiprfish_image_analysis_amd import biofilm
    rng = np.random.default_rng(41)
    shape = (40, 36, 32)
    seg, N = R3.voronoi(shape, 64, 7.0, seed=9)
    assert 50 <= N <= 64 and (seg == 0).any()
    kind = rng.integers(0, 6, N + 1)
    stack = (bundle.spectra[kind[seg]] * (seg > 0)[..., None] + 0.01 * rng.random(shape + (63,))).astype(np.float32)
    dstack, dseg = dev(stack), dev(seg)
    sample = str(tmp_path / "bf3")
    first = biofilm.volume_report(sample, dstack, dseg, dseg, bundle.model, bundle.taxon_codes, write=False)
    assert not any(os.path.exists(sample + s) for s in SUFFIXES)
    # the reference's cuts (0.95, 100000) moved to this input's medians, so both clauses fire
    prob_min = float(np.median(first["cell_info"].max_probability))
    area_max = float(np.median(first["cell_info"].area))
    out = biofilm.volume_report(sample, dstack, dseg, dseg, bundle.model, bundle.taxon_codes, prob_min=prob_min,
                                area_max=area_max)
    ci = out["cell_info"]
    classes = list(bundle.clf.classes_)
    assert list(ci.columns) == ["channel_{}".format(i) for i in range(63)] + \
        ["intensity_classification_{}".format(i) for i in range(4)] + ["cell_barcode", "max_probability"] + \
        [c + "_prob" for c in classes] + COLUMNS_TAIL
    assert len(ci) == N and list(ci.label) == list(range(1, N + 1))
    mom = R3.moments3(seg, N)
    assert np.array_equal(ci.area.values, mom[1:, 0])
    assert np.array_equal(ci[["centroid_x", "centroid_y", "centroid_z"]].values, R3.props3(mom)[1:, 1:4])
    # predict_proba of the device embedding, by sklearn itself
    feats = bundle.model.features(K.cell_table(*K.label_sums(dstack.reshape(-1, shape[2], 63),
                                                             dseg.reshape(-1, shape[2]), N), N)[3])
    e = host(bundle.model.umap.transform(feats).double())
    np.testing.assert_allclose(ci[[c + "_prob" for c in classes]].values, bundle.clf.predict_proba(e), rtol=0,
                               atol=1e-12)
    # typing (:1411): both clauses decide rows, both types occur
    by_area = ci.area.values > area_max
    by_prob = ci.max_probability.values <= prob_min
    want = ~(by_area | by_prob)
    assert (by_area & ~by_prob).any() and (by_prob & ~by_area).any()
    assert np.array_equal(ci.type.values == "cell", want) and 0 < want.sum() < N
    assert set(ci.type) == {"cell", "debris"}
    assert list(out["cell_info_filtered"].label) == [i + 1 for i in range(N) if want[i]]
    assert len(out["avgint"]) == N and len(out["avgint_filtered"]) == want.sum()
    # both adjacency matrices, connectivity 2
    idx = {c: i for i, c in enumerate(bundle.taxon_codes)}
    bc = np.array([-1] + [idx.get(c, -1) for c in ci.cell_barcode], np.int32)
    keys = R3.rag_edges3(seg, 2)
    keep = np.concatenate([[False], want])
    assert np.array_equal(out["adjacency"].values.astype(np.int64), R3.barcode_adjacency_edges(keys, bc, 5))
    assert np.array_equal(out["adjacency_filtered"].values.astype(np.int64),
                          R3.barcode_adjacency_edges(keys, bc, 5, keep))
    assert out["adjacency"].values.sum() > out["adjacency_filtered"].values.sum() > 0
    assert list(out["adjacency"].columns) == bundle.taxon_codes
    # the barcode-valued volumes
    value = np.array([0] + [int(c, 2) for c in ci.cell_barcode], np.int32)
    assert np.array_equal(host(out["identification_barcode"]), value[seg])
    assert np.array_equal(host(out["identification_barcode_filtered"]), np.where(keep, value, 0)[seg])
    # files
    for s in SUFFIXES:
        assert os.path.exists(sample + s), s
    rows = open(sample + "_cell_information.csv").read().splitlines()
    assert len(rows) == N and "channel_0" not in rows[0]      # no header row
    assert float(rows[0].split(",")[0]) == ci.channel_0[0]
    assert open(sample + "_cell_information_filtered.csv").readline().startswith("channel_0,")
    # the bvox files: a taxon's hue, white outside the lookup, grey debris in the filtered set
    colour = np.zeros((N + 1, 3), np.float32)
    for i, c in enumerate(ci.cell_barcode):
        colour[i + 1] = colorsys.hsv_to_rgb(idx[c] / 5, 1, 1) if c in idx else (1, 1, 1)
    assert (bc[1:] == -1).any() and (bc[1:] >= 0).any()
    colour_f = colour.copy()
    colour_f[1:][~want] = 0.5
    for table, stem in ((colour, "_identification_"), (colour_f, "_identification_filtered_")):
        pl = R3.planes(seg, table)
        for ch, c in enumerate("rgb"):
            assert open(sample + stem + c + ".bvox", "rb").read() == R3.bvox_bytes(shape, pl[ch]), stem + c


def test_report_follows_the_segmentation_chain(tmp_path, P, bundle):
    """segment_volume_stack's two label volumes number the same bodies: the row <-> node
    correspondence the report relies on"""
    from hiprfish_image_analysis_amd import biofilm
    rng = np.random.default_rng(21)
    _, s = VR.synthetic_volume()
    vol = (s[..., None] * (0.2 + rng.random(63)) * (0.9 + 0.2 * rng.random(s.shape + (63,)))).astype(np.float32)
    dvol = dev(vol)
    seg, n, _, adj, n_adj = P.segment_volume_stack(dvol, adjacency=True)
    hs, ha = host(seg), host(adj)
    assert n > 1 and n_adj == n
    assert np.array_equal(ha[hs > 0], hs[hs > 0])
    assert np.array_equal(np.unique(hs[hs > 0]), np.arange(1, n + 1))
    assert np.array_equal(np.unique(ha[ha > 0]), np.arange(1, n + 1))
    out = biofilm.volume_report(str(tmp_path / "chain"), dvol, seg, adj, bundle.model, bundle.taxon_codes)
    assert list(out["cell_info"].label) == list(range(1, n + 1))
    assert np.array_equal(out["cell_info"].area.values, np.bincount(hs.ravel(), minlength=n + 1)[1:])
    idx = {c: i for i, c in enumerate(bundle.taxon_codes)}
    bc = np.array([-1] + [idx.get(c, -1) for c in out["cell_info"].cell_barcode], np.int32)
    assert np.array_equal(out["adjacency"].values.astype(np.int64),
                          R3.barcode_adjacency_edges(R3.rag_edges3(ha, 2), bc, 5))


def test_report_calls_leave_no_allocation(K, P, voro):
    lab, n, _ = voro
    colour = torch.rand((n + 1, 3), device="cuda")
    bc = torch.zeros(n, dtype=torch.int32, device="cuda")

    def calls():
        K.region_props3(dev(lab), n)
        keys = K.rag_edges3(dev(lab), capacity=64)
        K.barcode_adjacency_edges(keys, torch.zeros(n + 1, dtype=torch.int32, device="cuda"), 3)
        K.paint_planes3(dev(lab), colour)
        P.biofilm_typing_and_adjacency3(dev(lab), dev(lab), bc, 3)
        torch.cuda.synchronize()

    calls()
    before = live()
    calls()
    assert live() == before
