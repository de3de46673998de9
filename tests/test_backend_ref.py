"""tests/backend_ref.py (the plain restatements) and oracle/backend.c pinned to each other and to
sklearn at the class counts, kernel branches and table sizes the device tests
(tests/test_backend_edges_gpu.py) use.  Models are fitted live.  CPU only.

Tolerances are the existing contract's (tests/test_backend_oracle.py): decision values rtol =
atol = 1e-12, probabilities 1e-12 to sklearn and 1e-13 between oracle and helper, kNN distances
1e-14; UMAP outputs bit for bit."""
import os
import sys

import numpy as np
import pytest

pytest.importorskip("sklearn")

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import backend_cases as C  # noqa: E402
import backend_ref as R  # noqa: E402
from make_golden import metric_7b_v2, metric_violet_v2  # noqa: E402
from test_backend_oracle import assert_same_neighbours  # noqa: E402


def blobs(rng, ncls, per_class, f=3, spread=4.0, noise=0.5):
    centres = rng.normal(0, spread, (ncls, f))
    y = np.repeat(np.arange(ncls), per_class)
    return centres, centres[y] + rng.normal(0, noise, (len(y), f)), y


def queries(rng, centres, n_near, n_far):
    near = centres[rng.integers(0, len(centres), n_near)] + rng.normal(0, 0.8, (n_near, centres.shape[1]))
    return np.vstack([near, 50.0 * centres[rng.integers(0, len(centres), n_far)]])


PREDICT = [(ncls, kw) for ncls in (2, 3, 24, 130)
           for kw in (dict(kernel="linear"), dict(kernel="rbf", gamma=0.05), dict(kernel="sigmoid", gamma=0.01, coef0=0.1),
                      dict(kernel="poly", degree=1, gamma=0.3, coef0=0.7), dict(kernel="poly", degree=2, gamma=0.3, coef0=0.7),
                      dict(kernel="poly", degree=4, gamma=0.1, coef0=0.7), dict(kernel="poly", degree=5, gamma=0.1, coef0=0.7))]


@pytest.mark.parametrize("ncls,kw", PREDICT, ids=lambda v: str(v) if isinstance(v, int) else
                         v["kernel"] + str(v.get("degree", "")))
def test_svc_predict_against_sklearn(orc, ncls, kw):
    from sklearn.svm import SVC
    rng = np.random.default_rng(ncls * 11 + len(str(kw)))
    centres, x, y = blobs(rng, ncls, 12 if ncls < 100 else 4, spread=2.0 if kw["kernel"] == "poly" else 4.0)
    clf = SVC(decision_function_shape="ovo", C=2.0, **kw).fit(x, y)
    xt = queries(rng, centres, 40, 0)
    want_pred, want_dec = clf.predict(xt), clf.decision_function(xt)
    if ncls == 2:
        want_dec = -want_dec.reshape(-1, 1)       # sklearn reports the binary decision with the flipped sign
    m = C.libsvm(C.sk_model(clf))
    for name, (pred, dec) in (("oracle", orc.svc_predict(xt, *m, want_dec=True)), ("helper", R.svc_decision(xt, *m)[:2])):
        assert np.array_equal(clf.classes_[pred], want_pred), name
        np.testing.assert_allclose(dec, want_dec, rtol=1e-12, atol=1e-12, err_msg=name)


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
@pytest.mark.parametrize("ncls", [2, 64, 65, 100, 101, 127, 128])
def test_svc_proba_against_sklearn(orc, ncls, kernel):
    from sklearn.svm import SVC
    rng = np.random.default_rng(500 + ncls)
    centres, x, y = blobs(rng, ncls, 12)
    kw = dict(kernel="rbf", gamma=0.05, C=10.0) if kernel == "rbf" else dict(kernel="linear", C=1.0)
    clf = SVC(probability=True, random_state=0, **kw).fit(x, y)
    xt = queries(rng, centres, 12, 6)
    want = clf.predict_proba(xt)
    sk = C.sk_model(clf)
    m = C.libsvm(sk)
    info = {}
    got_o = orc.svc_proba(xt, *m, sk["probA"], sk["probB"])
    got_r = R.svc_proba(xt, *m, sk["probA"], sk["probB"], info=info)
    np.testing.assert_allclose(got_o, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got_r, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got_r, got_o, rtol=0, atol=1e-13)
    # the far rows drive a linear model's pair probabilities into both clamps (every rbf kernel
    # value is 0 out there: the decision values are the intercepts)
    if kernel == "linear":
        lo, hi = min(info["r_min"][12:]) == 1e-7, max(info["r_max"][12:]) == 1 - 1e-7
        assert (lo and hi) if ncls > 2 else (lo or hi)        # two classes have one pair


def test_proba_coupling_stops_first_and_last(orc):
    """Platt parameters of 0 make every pair 1/2: the first check passes and p stays uniform.
    The other end, a run of all max(100, k) sweeps, was not reached by any input tried: pair
    probabilities clamped to [1e-7, 1 - 1e-7] converged within 0.48 k sweeps (k = 101, 128;
    random and cyclic tournaments, hierarchies of tied pairs and triples, chains; the slowest:
    two tied classes that beat all others, below)."""
    rng = np.random.default_rng(9)
    m, centres = C.random_svc(rng, 101, 3, proba=True)
    x = centres[:6] + 0.1
    info = {}
    p = R.svc_proba(x, *C.libsvm(m), 0 * m["probA"], 0 * m["probB"], info=info)
    assert info["sweeps"] == [0] * 6 and np.array_equal(p, np.full((6, 101), 1.0 / 101))
    assert np.array_equal(orc.svc_proba(x, *C.libsvm(m), 0 * m["probA"], 0 * m["probB"]), p)
    r, info = C.two_tied_dominant(101), {}
    R.couple(r, info)
    assert 40 < info["sweeps"][0] < 101


@pytest.mark.parametrize("ncls", [5, 65])
def test_proba_nan_row_against_sklearn(orc, ncls):
    """libsvm clamps with its own max(x, y) = (x > y) ? x : y, which turns a NaN pair probability
    into 1e-7: every pair of a row holding a NaN votes for its second class, and nearly all
    probability lands on the LAST class.  predict_proba refuses a NaN at its input check, so
    sklearn's libsvm is asked through _dense_predict_proba, which has none."""
    from sklearn.svm import SVC
    rng = np.random.default_rng(700 + ncls)
    centres, x, y = blobs(rng, ncls, 12)
    clf = SVC(probability=True, random_state=0, kernel="rbf", gamma=0.05, C=10.0).fit(x, y)
    xt = queries(rng, centres, 6, 0)
    xt[2, 1] = np.nan
    want = clf._dense_predict_proba(np.ascontiguousarray(xt))
    assert want[2, -1] > 1 - 1e-9 and np.isfinite(want).all()
    sk = C.sk_model(clf)
    got_o = orc.svc_proba(xt, *C.libsvm(sk), sk["probA"], sk["probB"])
    got_r = R.svc_proba(xt, *C.libsvm(sk), sk["probA"], sk["probB"])
    np.testing.assert_allclose(got_o, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got_r, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got_r, got_o, rtol=0, atol=1e-13)


def test_constructed_models(orc):
    for m, x, want in ((C.cycle_model(), np.ones((2, 1)), 0), (C.zero_model(), np.random.default_rng(1).random((3, 3)), 4)):
        pred, dec, votes = R.svc_decision(x, *C.libsvm(m))
        assert np.all(pred == want) and np.array_equal(orc.svc_predict(x, *C.libsvm(m)), pred)
    assert np.array_equal(votes[0], [0, 1, 2, 3, 4]) and not dec.any()
    pm = C.probe_model(1.0)
    x = np.array([[26.6], [27.0], [27.25], [27.29], [27.3], [28.0]])
    _, dec = orc.svc_predict(x, *C.libsvm(pm), want_dec=True)
    assert 0 < dec[1, 0] < 2.3e-308 and dec[5, 0] == 0.0     # subnormal, then exactly 0


def _euclidean(x, y):
    return np.sqrt(np.sum((x - y) ** 2))


@pytest.mark.parametrize("nt", [255, 256, 257])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_knn_against_sklearn_brute(orc, nt, metric):
    from sklearn.neighbors import NearestNeighbors
    rng = np.random.default_rng(40 + nt + metric)
    f = (20, 67, 132)[metric]
    tr, q = rng.random((nt, f)), rng.random((6, f))
    if metric:
        for a in (tr, q):
            a[:, (63, 126)[metric - 1]:] = rng.random((len(a), f - (63, 126)[metric - 1])) < 0.85
    # euclidean as a Python callable too, so that all three metrics take sklearn's same
    # one-pair-at-a-time path (its built-in euclidean is a threaded BLAS / OpenMP reduction, whose
    # pool would also outlive this test in a process that later tests fork workers from)
    nn = NearestNeighbors(n_neighbors=15, algorithm="brute",
                          metric=(_euclidean, metric_7b_v2, metric_violet_v2)[metric]).fit(tr)
    wd, wi = nn.kneighbors(q)
    oi, od = orc.knn(q, tr, metric, 15)
    ri, rd = R.knn(q, tr, metric, 15)
    for i, d in ((oi, od), (ri, rd)):
        np.testing.assert_allclose(d, wd, rtol=0, atol=1e-14)
        assert_same_neighbours(i, d, wi)
    assert np.array_equal(oi, ri)


def test_knn_edge_tables_oracle_equals_helper(orc):
    rng = np.random.default_rng(41)
    cases = [C.knn_line(600, True) + (0,), C.knn_line(600, False) + (0,), C.knn_boundary_pairs(rng) + (0,),
             (rng.random((3, 4)), np.tile(rng.random(4), (520, 1)), 0), C.knn_metric_edges(rng, 1) + (1,),
             C.knn_metric_edges(rng, 2) + (2,), (rng.random((4, 5)), rng.random((3, 5)), 0)]
    for q, tr, metric in cases:
        for k in (1, 15, 64):
            oi, od = orc.knn(q, tr, metric, k)
            ri, rd = R.knn(q, tr, metric, k)
            assert np.array_equal(oi, ri) and np.array_equal(od, rd)
    q, tr = C.knn_metric_edges(rng, 1)
    d = R.knn_distances(q, tr, 1)
    assert np.all(d[0, 22:28] < 0.5) and np.all(d[0, 28:40] == 1.0)     # 0.009 agrees, 0.011 does not


def refine_cases():
    """name -> (idx, memb, init, tail, n_epochs): the refinement cases of the device tests"""
    fam = C.umap_families()
    out = {}
    for name, f in fam.items():
        init, memb = R.umap_init(f["idx"], f["dist"], f["emb"], f["n_neighbors"], f["lc"], want_memb=True)
        for ne in (30, 100):
            out["%s-%d" % (name, ne)] = (f["idx"], memb, init, f["emb"], ne)
    out.update(C.refine_edge_cases())
    return out


@pytest.mark.parametrize("name", list(C.umap_families()))
def test_umap_init_oracle_equals_helper(orc, name):
    f = C.umap_families()[name]
    info = {}
    got, memb = R.umap_init(f["idx"], f["dist"], f["emb"], f["n_neighbors"], f["lc"], want_memb=True, info=info)
    want, wmemb = orc.umap_init(f["idx"], f["dist"], f["emb"], f["n_neighbors"], f["lc"], want_memb=True)
    assert np.array_equal(memb, wmemb) and np.array_equal(got, want)
    if name == "zeros_lc3":
        assert {"index", "max", "none"} <= set(info["rho_branch"])
    if name == "lc1.5_d3":
        assert set(info["rho_branch"]) == {"interp"}
    if name == "zeros_lc0":
        assert set(info["rho_branch"]) == {"zero"}


def test_umap_sigma_floor_is_taken(orc):
    idx, dist, emb = C.sigma_floor_case()
    info = {}
    got, memb = R.umap_init(idx, dist, emb, 15.0, 0.0, want_memb=True, info=info)
    assert info["floor"].count("all") == len(idx) // 2 and info["floor"][1] is None
    # the floor decides the weights of the tiny distances: strictly between 0 and 1
    assert np.all(memb[0::2, :6] == 1.0) and np.all((memb[0::2, 6:] > 0) & (memb[0::2, 6:] < 1))
    want, wmemb = orc.umap_init(idx, dist, emb, 15.0, 0.0, want_memb=True)
    assert np.array_equal(got, want) and np.array_equal(memb, wmemb)


@pytest.mark.parametrize("name", list(refine_cases()))
def test_umap_refine_oracle_equals_helper(orc, name):
    idx, memb, init, tail, ne = refine_cases()[name]
    info = {}
    got = R.umap_refine(idx, memb, init, tail, ne, 1.577, 0.8951, 1.0, 0.25, 5.0, seed=5, info=info)
    want = orc.umap_refine(idx, memb, init, tail, ne, 1.577, 0.8951, 1.0, 0.25, 5.0, seed=5)
    assert np.array_equal(got, want)
    moved = np.any(got != np.asarray(init, np.float32), axis=1)
    has_edges = np.array(info["edges"]) > 0
    # rows without an edge come back unchanged; the others moved (an edge whose weight equals the
    # threshold exactly would first fire at epoch n_epochs, hence "nearly all")
    assert not moved[~has_edges].any() and moved[has_edges].mean() > 0.9
    if name.startswith("coincident"):
        assert info["zero_same"] > 0 and info["zero_other"] > 0 and info["d2_zero"] > 0
    if name.startswith("dropped"):
        assert not has_edges[::2].any() and has_edges[1::2].all()


def test_one_epoch_moves_nothing(orc):
    """the first edge fires at epoch >= 1: n_epochs = 1 is no coverage of the update loop"""
    f = C.umap_families()["plain"]
    init, memb = orc.umap_init(f["idx"], f["dist"], f["emb"], 15.0, 0.0, want_memb=True)
    assert np.array_equal(orc.umap_refine(f["idx"], memb, init, f["emb"], 1, 1.577, 0.8951), init)
    assert np.array_equal(R.umap_refine(f["idx"], memb, init, f["emb"], 1, 1.577, 0.8951), init)


def test_fixture_is_current_and_small(golden, orc):
    """backend_edges.npz: arrays only, no larger than volume3d.npz, and the oracle reproduces the
    recorded sklearn outputs from the recorded (float32-rounded) models"""
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert os.path.getsize(os.path.join(here, "backend_edges.npz")) <= 516513
    g = golden("backend_edges")
    for name in ("proba65", "proba101", "proba127"):
        m = C.from_fixture(g, name)
        got = orc.svc_proba(m["x"], *C.libsvm(m), m["probA"].astype(np.float64), m["probB"].astype(np.float64))
        np.testing.assert_allclose(got, m["proba"], rtol=0, atol=1e-12)
    for name in ("pred130", "poly1", "poly2", "poly4", "poly5"):
        m = C.from_fixture(g, name)
        pred, dec = orc.svc_predict(m["x"], *C.libsvm(m), want_dec=True)
        assert np.array_equal(m["classes"][pred], m["pred"])
        step = 2 if name == "pred130" else 1        # the fixture keeps every second pair at 130 classes
        np.testing.assert_allclose(dec[:len(m["dec"]), ::step], m["dec"], rtol=1e-12, atol=1e-12)
