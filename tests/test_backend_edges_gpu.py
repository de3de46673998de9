"""The classifier back-end kernels (backend.hip) at real class counts and at their own limits,
against the oracle (oracle/backend.c), the plain restatements (tests/backend_ref.py) and sklearn's
recorded outputs (tests/golden/backend_edges.npz, make_backend_edges_golden.py).

The contract is tests/test_backend_gpu.py's: class decisions, kNN indices and UMAP outputs
bit-equal to the oracle; decision values within 1e-12 of sklearn (and of the oracle, rtol = atol);
probabilities within 1e-13 of the oracle and 1e-12 of sklearn; kNN distances within 1e-13.  The
oracle and the restatements are pinned to sklearn and to each other, at these class counts and
sizes, by tests/test_backend_ref.py on the CPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import backend_cases as C  # noqa: E402
import backend_ref as R  # noqa: E402
from hiprfish_image_analysis_amd import backend as B  # noqa: E402
from hiprfish_image_analysis_amd import kernels as K  # noqa: E402

AB = dict(a=1.577, b=0.8951)


def dev(a, dt=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def devmodel(m):
    """a model dict (sklearn's attribute layout) on the device"""
    f64 = lambda k: None if k not in m else np.asarray(m[k], np.float64)  # noqa: E731
    return B.SvcModel.from_arrays(m["sv"], f64("dual_coef"), f64("intercept"), m["n_support"], m["classes"],
                                  int(m["kernel"]), float(m["gamma"]), float(m["coef0"]), int(m["degree"]),
                                  probA=f64("probA"), probB=f64("probB"))


def predict(m, x, **kw):
    pred, dec = K.svc_predict(dev(x), devmodel(m), want_dec=True, **kw)
    return pred.cpu().numpy(), dec.cpu().numpy()


def proba_o(orc, m, x):
    return orc.svc_proba(x, *C.libsvm(m), np.asarray(m["probA"], np.float64), np.asarray(m["probB"], np.float64))


def check_predict(orc, m, x, helper_rows=None):
    """device == oracle (decisions exactly, values at the contract's tolerance) and the helper"""
    pred, dec = predict(m, x)
    opred, odec = orc.svc_predict(x, *C.libsvm(m), want_dec=True)
    assert np.array_equal(pred, opred)
    np.testing.assert_allclose(dec, odec, rtol=1e-12, atol=1e-12, equal_nan=True)
    h = slice(0, helper_rows)
    hpred, hdec, _ = R.svc_decision(x[h], *C.libsvm(m))
    assert np.array_equal(pred[h], hpred)
    np.testing.assert_allclose(dec[h], hdec, rtol=1e-12, atol=1e-12, equal_nan=True)
    return pred, dec


# ---- SVC predict -----------------------------------------------------------------------------------
def test_predict_130_classes_fixture_and_strided_column(golden, orc):
    """8385 pairs: 33 strides of the 256-thread pair loop, every row boundary of the decode.
    Every row and pair is compared with the oracle; the comparison with sklearn's recorded decision
    values here is a sample (the fixture's size limit leaves room for one row, every second pair).
    The oracle is held to live sklearn on all rows and pairs at 130 classes by
    tests/test_backend_ref.py::test_svc_predict_against_sklearn."""
    m = C.from_fixture(golden("backend_edges"), "pred130")
    x = m["x"]
    pred, dec = check_predict(orc, m, x)
    assert np.array_equal(m["classes"][pred], m["pred"])
    np.testing.assert_allclose(dec[:len(m["dec"]), ::2], m["dec"], rtol=1e-12, atol=1e-12)   # sklearn, every 2nd pair
    table = torch.full((len(x), 7), -1.0, dtype=torch.float64, device="cuda")
    table[:, 1:4] = dev(x)
    p2 = devmodel(m).predict(table[:, 1:4], out_column=table[:, 5])
    t = table.cpu().numpy()
    assert np.array_equal(t[:, 5], m["pred"]) and np.array_equal(p2.cpu().numpy(), pred)
    assert np.array_equal(t[:, 1:4], x) and np.all(t[:, [0, 4, 6]] == -1.0)


@pytest.mark.parametrize("name", ["poly1", "poly2", "poly4", "poly5"])
def test_predict_poly_degrees(golden, orc, name):
    """libsvm's square-and-multiply powi: degrees 1 (one multiply), 2 (square), 4 (two squares),
    5 (odd, even, odd bits)"""
    m = C.from_fixture(golden("backend_edges"), name)
    pred, dec = check_predict(orc, m, m["x"])
    assert np.array_equal(m["classes"][pred], m["pred"])
    np.testing.assert_allclose(dec, m["dec"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("ncls,kernel", [(2, "rbf"), (24, "sigmoid"), (24, "rbf"), (1023, "rbf")])
def test_predict_class_counts(orc, ncls, kernel):
    """2 classes (one pair), 24 (276 pairs: the first count past one 256-thread stride), 1023
    (522,753 pairs: the sqrt decode and its fix-up loops at every row boundary).  A decode off by
    one anywhere moves a decision value to the wrong column."""
    rng = np.random.default_rng(ncls)
    m, centres = C.random_svc(rng, ncls, 3, kernel, per_class=2, gamma=0.5 if kernel == "rbf" else 0.05, coef0=0.1)
    x = centres[rng.integers(0, ncls, 64)] + 0.3 * rng.normal(size=(64, 3))
    if kernel == "sigmoid":
        # tanh is the device libm's against glibc's, so the values are held at the tolerance only,
        # and that bound decides which votes it fixes: |dec - odec| <= 1e-12 (1 + |odec|), asserted
        # here, gives a pair with |odec| > 2e-12 the oracle's sign.  Rows where every pair is that
        # clear must decide as the oracle does (derived from the tolerance, not from a measurement)
        pred, dec = predict(m, x)
        opred, odec = orc.svc_predict(x, *C.libsvm(m), want_dec=True)
        np.testing.assert_allclose(dec, odec, rtol=1e-12, atol=1e-12)
        safe = np.abs(odec).min(axis=1) > 2e-12
        assert safe.sum() > 32 and np.array_equal(pred[safe], opred[safe])
        return
    check_predict(orc, m, x, helper_rows=8 if ncls > 100 else None)


@pytest.mark.parametrize("nsv,ncls", [(8200, 2), (8200, 5), (20000, 2)])
def test_predict_lds_above_64k(orc, nsv, ncls):
    """dynamic LDS past 64 KiB (8,192 support vectors) and at 160,024 of the 163,840 bytes"""
    rng = np.random.default_rng(nsv + ncls)
    m, _ = C.random_svc(rng, ncls, 2, "rbf", per_class=nsv // ncls, gamma=0.7)
    x = rng.normal(size=(5, 2))
    pred, dec = predict(m, x)
    opred, odec = orc.svc_predict(x, *C.libsvm(m), want_dec=True)
    assert np.array_equal(pred, opred)
    np.testing.assert_allclose(dec, odec, rtol=1e-12, atol=1e-12)


def test_predict_lds_budget_refused():
    rng = np.random.default_rng(3)
    m, _ = C.random_svc(rng, 2, 2, "rbf", per_class=10239)       # 20,478 support vectors: 163,848 bytes
    with pytest.raises(ValueError, match="LDS budget"):
        K.svc_predict(dev(rng.normal(size=(2, 2))), devmodel(m))


def test_predict_vote_tie_zero_sums_and_one_cell(orc):
    """a three-class cycle (one vote each: the first maximum, class 0, wins), and an all-zero
    model (every sum exactly 0 votes b: the last class); n = 1"""
    pred, dec = predict(C.cycle_model(), np.ones((3, 1)))
    assert np.array_equal(pred, [0, 0, 0]) and np.array_equal(dec, np.tile([1.0, -1.0, 1.0], (3, 1)))
    x = np.random.default_rng(1).random((1, 3))
    pred, dec = predict(C.zero_model(), x)
    assert np.array_equal(pred, [4]) and not dec.any() and not np.signbit(dec).any()
    assert np.array_equal(orc.svc_predict(x, *C.libsvm(C.zero_model())), pred)


def test_predict_rbf_underflow_bit_equal(orc):
    """gamma d^2 from 707 (the smallest normal) past 745 (0): the decision value of the probe model
    IS the kernel value -- subnormal, then exactly 0, bit for bit the oracle's"""
    m = C.probe_model(1.0)
    x = np.array([[26.6], [27.0], [27.25], [27.29], [27.295], [27.3], [28.0], [1e200]])
    _, dec = predict(m, x)
    _, odec = orc.svc_predict(x, *C.libsvm(m), want_dec=True)
    assert np.array_equal(dec.view(np.uint64), odec.view(np.uint64))
    assert 0 < dec[1, 0] < 2.3e-308 and dec[6, 0] == 0.0 and dec[7, 0] == 0.0


@pytest.mark.parametrize("kernel", ["rbf", "linear"])
def test_predict_nan_and_inf_rows(orc, kernel):
    rng = np.random.default_rng(8)
    m, centres = C.random_svc(rng, 5, 3, kernel, per_class=3)
    x = centres[rng.integers(0, 5, 12)] + 0.3 * rng.normal(size=(12, 3))
    clean_pred, clean_dec = predict(m, x)
    bad = x.copy()
    bad[3, 1] = np.nan
    bad[7, 2] = np.inf
    bad[9, 0] = -np.inf
    pred, dec = predict(m, bad)
    opred, odec = orc.svc_predict(bad, *C.libsvm(m), want_dec=True)
    assert np.array_equal(pred, opred)
    np.testing.assert_allclose(dec, odec, rtol=1e-12, atol=1e-12, equal_nan=True)
    assert np.isnan(dec[3]).all() and pred[3] == 4              # a NaN sum is not > 0: every pair votes b
    keep = [i for i in range(12) if i not in (3, 7, 9)]
    assert np.array_equal(pred[keep], clean_pred[keep]) and np.array_equal(dec[keep], clean_dec[keep])


# ---- SVC predict_proba -----------------------------------------------------------------------------
def check_proba(orc, m, x):
    prob = devmodel(m).predict_proba(dev(x)).cpu().numpy()
    np.testing.assert_allclose(prob, proba_o(orc, m, x), rtol=0, atol=1e-13)
    np.testing.assert_allclose(prob.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    return prob


@pytest.mark.parametrize("name", ["proba65", "proba101", "proba127"])
def test_proba_fixture_second_slot(golden, orc, name):
    """65 classes: one class in the second register slot; 101: past the max_iter switch (which no
    output shows: these rows converge long before 100 sweeps); 127: a 7-bit community.  Slot 1 of
    Qp read from the wrong lane, or a class >= 64 left out of a sum, moves every probability."""
    m = C.from_fixture(golden("backend_edges"), name)
    prob = check_proba(orc, m, m["x"])
    np.testing.assert_allclose(prob, m["proba"], rtol=0, atol=1e-12)
    pred, _ = predict(m, m["x"])
    assert np.array_equal(m["classes"][pred], m["pred"])
    # information only: libsvm does not promise that the two agree
    print("%s: argmax(prob) == predict on %d of %d rows" % (name, int((prob.argmax(axis=1) == pred).sum()), len(pred)))


@pytest.mark.parametrize("ncls,kernel", [(64, "linear"), (100, "rbf"), (128, "linear"), (128, "rbf")])
def test_proba_random_models_and_clamps(orc, ncls, kernel):
    """64: the first slot full, the second empty; 100: the last count with max_iter = 100; 128: both
    slots full.  Rows 50x further out than any class clamp a linear model's pairs at both ends."""
    rng = np.random.default_rng(ncls + len(kernel))
    m, centres = C.random_svc(rng, ncls, 3, kernel, per_class=2, proba=True, spread=2.0)
    x = np.vstack([centres[rng.integers(0, ncls, 20)] + 0.3 * rng.normal(size=(20, 3)), 50.0 * centres[:6]])
    prob = check_proba(orc, m, x)
    info = {}
    ref = R.svc_proba(x[16:], *C.libsvm(m), m["probA"], m["probB"], info=info)
    np.testing.assert_allclose(prob[16:], ref, rtol=0, atol=1e-12)
    if kernel == "linear":
        assert min(info["r_min"][4:]) == 1e-7 and max(info["r_max"][4:]) == 1 - 1e-7


@pytest.mark.parametrize("k", [101, 128])
def test_proba_coupling_stops_first_and_runs_long(orc, k):
    """pairs all 1/2 pass the first check: exactly uniform.  The longest coupling known for clamped
    pairs (two tied classes that beat all others: 48 sweeps at 101 classes, 60 at 128; none of
    the inputs tried reaches max_iter, see tests/test_backend_ref.py, so max_iter = k against a
    fixed 100 is not observable).  A row holding a NaN has every pair clamped to 1e-7, as in
    libsvm (test_backend_ref.py::test_proba_nan_row_against_sklearn): nearly all probability on
    the last class."""
    rng = np.random.default_rng(k)
    m, centres = C.random_svc(rng, k, 3, "rbf", proba=True)
    x = centres[:5] + 0.1
    flat = dict(m, probA=0 * m["probA"], probB=0 * m["probB"])
    assert np.array_equal(devmodel(flat).predict_proba(dev(x)).cpu().numpy(), np.full((5, k), 1.0 / k))
    slow = C.slow_coupling_model(k)
    info = {}
    ref = R.svc_proba(np.ones((1, 1)), *C.libsvm(slow), slow["probA"], slow["probB"], info=info)
    assert 40 < info["sweeps"][0] < k
    prob = check_proba(orc, slow, np.ones((3, 1)))
    np.testing.assert_allclose(prob[0], ref[0], rtol=0, atol=1e-12)
    assert abs(prob[0, 0] - prob[0, 1]) < 1e-6 and prob[0, :2].sum() > 0.99
    x[2, 1] = np.nan
    prob = devmodel(m).predict_proba(dev(x)).cpu().numpy()
    want = proba_o(orc, m, x)
    np.testing.assert_allclose(prob, want, rtol=0, atol=1e-13)
    assert prob[2, -1] > 1 - 1e-9 and np.isfinite(prob).all()


def test_proba_129_classes_refused():
    rng = np.random.default_rng(2)
    m, centres = C.random_svc(rng, 129, 3, "rbf", proba=True)
    with pytest.raises(ValueError, match="classes"):
        devmodel(m).predict_proba(dev(centres[:2]))


# ---- kNN ---------------------------------------------------------------------------------------------
def check_knn(orc, q, tr, metric, k, helper=True):
    idx, dist = K.knn(dev(q), dev(tr.T), metric, k)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    oi, od = orc.knn(q, tr, metric, k)
    assert np.array_equal(idx, oi)
    np.testing.assert_allclose(dist, od, rtol=0, atol=1e-13, equal_nan=True)
    assert np.array_equal(np.isinf(dist), np.isinf(od)) and np.all((idx < 0) == (np.arange(k)[None, :] >= len(tr)))
    if helper:
        ri, rd = R.knn(q, tr, metric, k)
        assert np.array_equal(idx, ri)
        np.testing.assert_allclose(dist, rd, rtol=0, atol=1e-13)
    return idx, dist


@pytest.mark.parametrize("nt", [1, 255, 256, 257, 513])
def test_knn_chunk_boundaries(orc, nt):
    """the table ends one row before, on and one row after a 256-row chunk, and two chunks + 1;
    k = 1, 15 and 64 (k = 64 > nt = 1: -1 / inf slots)"""
    rng = np.random.default_rng(nt)
    tr, q = rng.random((nt, 20)), rng.random((7, 20))
    for k in (1, 15, 64):
        check_knn(orc, q, tr, 0, k)


def test_knn_widest_row_and_column_slice(orc):
    rng = np.random.default_rng(160)
    tr, wide = rng.random((300, 160)), rng.random((5, 170))
    idx, dist = K.knn(dev(wide)[:, 4:164], dev(tr.T), 0, 15)          # ldq = 170 > f = 160
    oi, od = orc.knn(wide[:, 4:164], tr, 0, 15)
    assert np.array_equal(idx.cpu().numpy(), oi)
    np.testing.assert_allclose(dist.cpu().numpy(), od, rtol=0, atol=1e-13)
    with pytest.raises(ValueError):
        K.knn(dev(rng.random((2, 161))), dev(rng.random((161, 10))), 0, 3)
    with pytest.raises(ValueError):
        K.knn(dev(wide[:, :160]), dev(tr.T), 0, 65)


@pytest.mark.parametrize("descending", [True, False])
def test_knn_monotone_distances(orc, descending):
    """descending with the row: every row of every chunk beats the current k-th, 256 candidates
    per merge, the best list rewritten each time; ascending: nothing after the first k rows"""
    q, tr = C.knn_line(600, descending)
    for k in (1, 15, 64):
        idx, _ = check_knn(orc, q, tr, 0, k)
        want = np.arange(599, 599 - k, -1) if descending else np.arange(k)
        assert np.array_equal(idx[0], want)


def test_knn_ties_keep_row_order(orc):
    """all rows identical: 0 .. k-1; identical rows across 255|256 and 511|512: the lower row
    first, and alone for k = 1.  A merge that is not in row order, or `<=` for `<`, swaps them."""
    rng = np.random.default_rng(42)
    row = rng.random(4)
    for k in (1, 15, 64):
        idx, _ = check_knn(orc, rng.random((3, 4)), np.tile(row, (520, 1)), 0, k)
        assert np.array_equal(idx, np.tile(np.arange(k), (3, 1)))
    q, tr = C.knn_boundary_pairs(rng)
    for k in (1, 2, 15):
        idx, dist = check_knn(orc, q, tr, 0, k)
        assert list(idx[:4, 0]) == [255, 511, 255, 511]
        if k > 1:
            assert list(idx[:4, 1]) == [256, 512, 256, 512] and np.array_equal(dist[:4, 0], dist[:4, 1])


@pytest.mark.parametrize("metric", [1, 2])
def test_knn_metric_branches(orc, metric):
    """zero-norm segments (query only, training row only, both), a query flag of 0, flags differing
    by 0.009 (equal) and 0.011 (mismatch) in total"""
    rng = np.random.default_rng(43)
    q, tr = C.knn_metric_edges(rng, metric)
    idx, dist = check_knn(orc, q, tr, metric, 48)
    d = np.empty((len(q), len(tr)))
    np.put_along_axis(d, idx, dist, axis=1)                         # back to row order
    np.testing.assert_allclose(d, R.knn_distances(q, tr, metric), rtol=0, atol=1e-13)
    if metric == 1:
        assert np.all(d[0, 22:28] < 0.5) and np.all(d[0, 28:40] == 1.0)
        assert np.all(d[1, 0:6] < d[1, 40:].min())       # both zero: that segment costs 0, query-only: 1
    else:
        assert np.all(d[0, 22:28] < 0.5) and np.all(d[0, 28:40] > 1 / 6)


def test_knn_nan_query_row(orc):
    """a NaN distance is never `<` anything: the NaN query keeps the first k rows in row order"""
    rng = np.random.default_rng(44)
    tr, q = rng.random((300, 6)), rng.random((4, 6))
    q[1, 2] = np.nan
    idx, dist = check_knn(orc, q, tr, 0, 15, helper=False)
    assert np.array_equal(idx[1], np.arange(15)) and np.isnan(dist[1]).all()


# ---- UMAP initial embedding ------------------------------------------------------------------------
def check_init(orc, idx, dist, emb, nn, lc, helper=True):
    out, memb = K.umap_init_transform(dev(idx, np.int32), dev(dist), dev(emb, np.float32), nn, lc, want_memb=True)
    out, memb = out.cpu().numpy(), memb.cpu().numpy()
    want, wmemb = orc.umap_init(idx, dist, emb, nn, lc, want_memb=True)
    assert np.array_equal(memb, wmemb) and np.array_equal(out, want)
    info = {}
    if helper:
        href, hmemb = R.umap_init(idx, dist, emb, nn, lc, want_memb=True, info=info)
        assert np.array_equal(memb, hmemb) and np.array_equal(out, href)
    return out, memb, info


@pytest.mark.parametrize("name", list(C.umap_families()))
def test_umap_init_families(orc, name):
    """the four rho branches (lc index, interpolated, lc 0, fewer non-zero distances than lc: their
    maximum, or none), zero distances (a query equal to training rows), k = 1 and 64, d = 2, 3, 8,
    -1 / inf slots"""
    f = C.umap_families()[name]
    _, _, info = check_init(orc, f["idx"], f["dist"], f["emb"], f["n_neighbors"], f["lc"])
    want = {"zeros_lc3": {"index", "max", "none"}, "lc1.5_d3": {"interp"}, "zeros_lc0": {"zero"}}.get(name)
    assert want is None or want <= set(info["rho_branch"])


def test_umap_init_block_edges_and_dims(orc):
    rng = np.random.default_rng(50)
    for nq in (1, 63, 64, 65, 129):
        for d in (1, 2, 3, 8):
            idx, dist = C.graph(rng, nq, 15, 100)
            check_init(orc, idx, dist, (rng.normal(size=(100, d)) * 3).astype(np.float32), 15.0, 1.0, helper=nq == 65)


def test_umap_init_sigma_floor_from_the_batch_mean(orc):
    """rows of zero and tiny distances among ordinary ones: sigma is floored at 1e-3 x the mean of
    ALL distances, and the tiny distances weigh exp(-d / floor) -- taken per row, or not at all,
    the floor would leave them a weight of 0.
    The wrapper takes that mean with torch's mean(), a tree reduction on the device; the oracle and
    the helper add in row-major order.  The two f64 means can differ in their last bits (~1e-16
    relative); sigma is stored as float32 (6e-8), which absorbs that unless 1e-3 x the mean falls
    within 1e-16 of a float32 rounding boundary.  If a change of these inputs makes this test miss
    by one float32 ulp of sigma, that is the cause: give both sides one summation order then."""
    idx, dist, emb = C.sigma_floor_case()
    _, memb, info = check_init(orc, idx, dist, emb, 15.0, 0.0)
    assert info["floor"].count("all") == len(idx) // 2 and info["floor"][1] is None
    assert np.all(memb[0::2, :6] == 1.0) and np.all((memb[0::2, 6:] > 0) & (memb[0::2, 6:] < 1))


# ---- UMAP refinement -------------------------------------------------------------------------------
def refine_cases(orc):
    out = {}
    for name, f in C.umap_families().items():
        init, memb = orc.umap_init(f["idx"], f["dist"], f["emb"], f["n_neighbors"], f["lc"], want_memb=True)
        for ne in (30, 100):
            out["%s-%d" % (name, ne)] = (f["idx"], memb, init, f["emb"], ne)
    out.update(C.refine_edge_cases())
    return out


REFINE_NAMES = ["%s-%d" % (n, e) for n in C.umap_families() for e in (30, 100)] + list(C.refine_edge_cases())


def run_refine(idx, memb, init, tail, ne, seed=5):
    return K.umap_refine(dev(idx, np.int32), dev(memb, np.float32), dev(init, np.float32), dev(tail, np.float32), ne,
                         AB["a"], AB["b"], 1.0, 0.25, 5.0, seed=seed).cpu().numpy()


@pytest.mark.parametrize("name", REFINE_NAMES)
def test_umap_refine_cases(orc, name):
    """the families at 30 and 100 epochs (d = 2, 3, 8, k = 1 and 64, -1 slots, coincident training
    points), queries that start ON their neighbour (d2 == 0; dn == 0 with the drawn row equal to
    the query's number -- skipped -- and not -- pushed by +4 alpha), rows whose every edge falls
    below wmax / n_epochs (unchanged), one training row, d = 1 across the 64-thread block"""
    idx, memb, init, tail, ne = refine_cases(orc)[name]
    got = run_refine(idx, memb, init, tail, ne)
    want = orc.umap_refine(idx, memb, init, tail, ne, AB["a"], AB["b"], 1.0, 0.25, 5.0, seed=5)
    assert np.array_equal(got, want)
    moved = np.any(got != np.asarray(init, np.float32), axis=1)
    assert moved.any()
    if name.startswith(("coincident", "dropped")):
        info = {}
        assert np.array_equal(R.umap_refine(idx, memb, init, tail, ne, AB["a"], AB["b"], 1.0, 0.25, 5.0, seed=5,
                                            info=info), got)
        if name.startswith("coincident"):
            assert info["zero_same"] > 0 and info["zero_other"] > 0 and info["d2_zero"] > 0
        else:
            assert not any(info["edges"][0::2]) and all(info["edges"][1::2])
            assert not moved[0::2].any() and moved[1::2].all()


def test_umap_refine_seeds_input_and_limits(orc):
    f = C.umap_families()["plain"]
    init, memb = orc.umap_init(f["idx"], f["dist"], f["emb"], 15.0, 0.0, want_memb=True)
    init_dev = dev(init, np.float32)
    args = (dev(f["idx"], np.int32), dev(memb, np.float32), init_dev, dev(f["emb"], np.float32), 30, AB["a"], AB["b"])
    r1, r1b, r2 = (K.umap_refine(*args, seed=s).cpu().numpy() for s in (1, 1, 2))
    assert np.array_equal(r1, r1b) and not np.array_equal(r1, r2)
    assert np.array_equal(init_dev.cpu().numpy(), init)                 # refined in a copy
    emb9 = np.zeros((200, 9), np.float32)
    with pytest.raises(ValueError):
        K.umap_refine(args[0], args[1], dev(np.zeros((len(init), 9)), np.float32), dev(emb9, np.float32), 30,
                      AB["a"], AB["b"])


# ---- the chain -------------------------------------------------------------------------------------
def oracle_chain(orc, feats, tr, metric, emb, um, svc):
    oi, od = orc.knn(feats, tr, metric, um.n_neighbors)
    e, memb = orc.umap_init(oi, od, emb, float(um.n_neighbors), 0.0, want_memb=True)
    e = orc.umap_refine(oi, memb, e, emb, 100, um.a, um.b, 1.0, 0.25, 5.0, seed=0).astype(np.float64)
    return e, orc.svc_predict(e, *C.libsvm(svc))


def test_chain_community_127_classes_with_probabilities(orc):
    """ClassifierModel.classify on the community layout (63 channels + 4 check flags from the
    scaled segments) with a 127-barcode SVC, each stage against the oracle, then predict_proba and
    biofilm.py's debris rule max_probability <= 0.95"""
    rng = np.random.default_rng(127)
    n = 200
    avg = rng.random((n, 63))
    avg /= avg.max(axis=1, keepdims=True)
    mean, scale = rng.random(63), rng.uniform(0.5, 2, 63)
    chk = [C.random_svc(rng, 2, hi - lo, "linear", per_class=3)[0] for lo, hi in B.MULTI_SEGMENTS]
    sc = (avg - mean) / scale
    feats = np.zeros((n, 67))
    feats[:, :63] = avg
    for k, (lo, hi) in enumerate(B.MULTI_SEGMENTS):
        feats[:, 63 + k] = orc.svc_predict(sc[:, lo:hi], *C.libsvm(chk[k]))
    assert 0 < feats[:, 63:].mean() < 1
    tr = np.vstack([feats[:150] * rng.uniform(0.9, 1.1, (150, 67)), feats[50:200]])
    tr[:, 63:] = np.vstack([feats[:150, 63:], feats[50:200, 63:]])
    emb = (rng.normal(size=(300, 2)) * 4).astype(np.float32)
    svc = C.nearest_centre_svc(emb[:127], 2.0, -50.0)        # barcodes centred on training points
    um = B.UmapModel(dev(tr.T), dev(emb, np.float32), 15, 1.0, "channel_cosine_intensity_7b_v2")
    bundle = B.ClassifierModel([devmodel(c) for c in chk], um, devmodel(svc), dev(mean), dev(scale))
    cls, _, f2 = bundle.classify(dev(avg))
    assert np.array_equal(f2.cpu().numpy(), feats)
    e, want = oracle_chain(orc, feats, tr, 1, emb, um, svc)
    assert np.array_equal(cls.cpu().numpy(), want) and len(np.unique(want)) > 10
    got_e = um.transform(f2)
    assert np.array_equal(got_e.cpu().numpy().astype(np.float64), e)
    prob = bundle.svc.predict_proba(got_e.double()).cpu().numpy()
    oprob = proba_o(orc, svc, e)
    np.testing.assert_allclose(prob, oprob, rtol=0, atol=1e-13)
    mp, omp = prob.max(axis=1), oprob.max(axis=1)
    clear = np.abs(omp - 0.95) > 1e-12
    assert np.array_equal((mp <= 0.95)[clear], (omp <= 0.95)[clear]) and clear.sum() >= n - 1
    assert 10 < (mp <= 0.95).sum() < n - 10                   # both answers of the rule occur
    print("127 classes: %d of %d cells are debris by max_probability <= 0.95; argmax(prob) == predict on %d" %
          (int((mp <= 0.95).sum()), n, int((prob.argmax(axis=1) == want).sum())))


def test_chain_ecoli_130_classes(orc):
    """the E. coli layout (95 channels, 31 differences, 6 check flags) with a 130-barcode SVC"""
    rng = np.random.default_rng(130)
    n = 200
    avg = rng.random((n, 95))
    avg /= avg.max(axis=1, keepdims=True)
    chk = [C.random_svc(rng, 2, hi - lo, "rbf", per_class=3)[0] for lo, hi in B.ECOLI_SEGMENTS]
    feats = np.zeros((n, 132))
    feats[:, :95] = avg
    feats[:, 95:126] = np.diff(avg[:, :32], axis=1)
    for k, (lo, hi) in enumerate(B.ECOLI_SEGMENTS):
        feats[:, 126 + k] = orc.svc_predict(feats[:, lo:hi], *C.libsvm(chk[k]))
    tr = np.vstack([feats[:150], rng.random((150, 132))])
    tr[150:, 126:] = rng.random((150, 6)) < 0.5
    emb = (rng.normal(size=(300, 2)) * 4).astype(np.float32)
    svc, _ = C.random_svc(rng, 130, 2, "rbf", per_class=2, gamma=0.3, spread=4.0)
    um = B.UmapModel(dev(tr.T), dev(emb, np.float32), 15, 1.0, "channel_cosine_intensity_violet_derivative_v2")
    bundle = B.ClassifierModel([devmodel(c) for c in chk], um, devmodel(svc))
    cls, _, f2 = bundle.classify(dev(avg))
    assert np.array_equal(f2.cpu().numpy(), feats)
    e, want = oracle_chain(orc, feats, tr, 2, emb, um, svc)
    assert np.array_equal(um.transform(f2).cpu().numpy().astype(np.float64), e)
    assert np.array_equal(cls.cpu().numpy(), want) and len(np.unique(want)) > 10
