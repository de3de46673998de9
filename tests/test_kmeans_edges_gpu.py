"""kmeans.hip against the CPU restatement (oracle/kmeans_sk.c) on every case of the table in
tests/kmeans_inputs.py -- the sizes, populations and arguments at which the sort, the k-means++
pick, the Lloyd search and the stopping rules change path (tests/test_kmeans_inputs.py proves
each case reaches its path and pins the restatement to sklearn).  The unit is exact by design:
labels, centres (bitwise), iterations, the top mask and every run's record must be equal."""
import numpy as np
import pytest

import kmeans_inputs as KI

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from hiprfish_image_analysis_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def fits(orc):
    """restatement fits.  A fit with a key (a table case's name) is computed once and shared by
    the tests that use that case; its arrays are read-only.  The top rule is no part of a fit:
    it is applied to the fit's labels and centres (KI.top_mask)."""
    done = {}

    def fit(x, valid, k, n_init=10, max_iter=300, key=None):
        if key is None or key not in done:
            out = orc.kmeans_sk_runs(x, k, valid, n_init, max_iter)
            for a in out:
                a.setflags(write=False)
            if key is None:
                return out
            done[key] = out
        return done[key]

    return fit


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()       # a copy: the table's arrays are read-only


def host(t):
    return t.cpu().numpy()


def check_fit(K, got, x, valid, ref, rule, n_init):
    """labels, centres (bitwise), iterations, top mask, and the record of every run"""
    lab, top, cen, it = got
    rl, rc, info, runs = ref
    assert np.array_equal(host(lab), rl.reshape(x.shape))
    assert np.array_equal(np.array(cen).view(np.uint64), rc.view(np.uint64))
    assert it == info[1]
    assert np.array_equal(host(top).astype(bool), KI.top_mask(x, valid, rl.reshape(x.shape), rc, rule))
    iters, reloc, strict = K.kmeans_last_runs(n_init)
    assert iters.tolist() == runs[:, 0].tolist()
    assert strict.tolist() == runs[:, 1].tolist()
    assert reloc.tolist() == runs[:, 2].tolist()


@pytest.mark.parametrize("case", KI.DEVICE_CASES, ids=lambda c: c.name)
def test_case_equals_restatement(K, fits, case):
    """every case of the table, those sklearn differs on and the reported defect included"""
    x, valid = KI.build(case)
    ref = fits(x, valid, case.k, case.n_init, case.max_iter, key=case.name)
    got = K.kmeans_1d(dev(x), case.k, valid=dev(valid), max_iter=case.max_iter, rule=case.rule, n_init=case.n_init)
    check_fit(K, got, x, valid, ref, case.rule, case.n_init)


def test_last_runs_needs_a_fit_and_bounds_n(K):
    K.kmeans_1d(dev(np.arange(8.0)), 2, n_init=3)
    assert all(len(a) == 3 for a in K.kmeans_last_runs(3))
    with pytest.raises(ValueError):
        K.kmeans_last_runs(11)
    with pytest.raises(ValueError):
        K.kmeans_last_runs(0)
    # a refused call leaves no records: not the previous fit's
    with pytest.raises(ValueError):
        K.kmeans_1d(dev(np.array([0.7, 0.1])), 3)
    with pytest.raises(ValueError, match="did not complete"):
        K.kmeans_last_runs(3)
    with pytest.raises(ValueError):
        K.kmeans_1d(dev(np.array([0.7, np.inf, 0.1])), 2)
    with pytest.raises(ValueError, match="did not complete"):
        K.kmeans_last_runs(3)


# ---- refused inputs -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", KI.REFUSED, ids=lambda c: c.name)
def test_refused_inputs_raise_and_leave_the_stream_usable(K, fits, case):
    """sklearn raises ValueError for infinity and for fewer samples than clusters; so do kmeans_1d
    and kmeans_1d_pair, and the next valid call -- same stream, same share dict -- is a plain fit"""
    x, valid = case.gen()
    d, v = dev(x), dev(valid)
    nv = KI.valid_values(x, valid).size
    what = "NaN or infinity" if case.why == "infinity" else "n_samples=%d .*n_clusters=%d" % (nv, case.k)
    share = {}
    with pytest.raises(ValueError, match=what):
        K.kmeans_1d(d, case.k, valid=v, share=share)
    other = max(1, case.k - 1)
    with pytest.raises(ValueError, match=what):
        K.kmeans_1d_pair(d, case.k, other, valid=v, rules=(0, 0))
    with pytest.raises(ValueError, match=what):
        K.kmeans_1d_pair(d, other, case.k, valid=v, rules=(0, 0))
    if case.why != "infinity":
        # the same samples fit with as many clusters as there are samples, on the sort the
        # refused call left in the share dict
        got = K.kmeans_1d(d, nv, valid=v, share=share)
        check_fit(K, got, x, valid, fits(x, valid, nv), 0, 10)
    good = KI.BY_NAME["n_init_9_k3"]
    gx, gvalid = KI.build(good)
    got = K.kmeans_1d(dev(gx), 3, valid=dev(gvalid), share=share, n_init=9)
    check_fit(K, got, gx, gvalid, fits(gx, gvalid, 3, 9, key=good.name), 0, 9)


def test_nan_and_infinity_say_so(K, orc, fits):
    for bad in (np.nan, np.inf, -np.inf, 1e308, -1e308):
        x = np.linspace(0.0, 1.0, 5000)
        x[4097] = bad
        # one message for all three, and it names the bound a finite value can break
        with pytest.raises(ValueError, match="NaN or infinity, or a finite magnitude above 2\\^1022"):
            K.kmeans_1d(dev(x), 2)
        with pytest.raises(ValueError, match="NaN or infinity, or a finite magnitude above 2\\^1022"):
            K.kmeans_1d_pair(dev(x), 2, 3)
        with pytest.raises(ValueError, match="NaN or infinity, or a finite magnitude above 2\\^1022"):
            orc.kmeans_sk(x, 2)
    x[4097] = -2.0 ** 1022                   # the largest magnitude accepted; its square overflows
    x[11] = 2.0 ** 1022
    for k in (2, 3):
        check_fit(K, K.kmeans_1d(dev(x), k), x, None, fits(x, None, k), 0, 10)


@pytest.mark.parametrize("edge", [2.0 ** -481, 2.0 ** 512])
def test_value_domain_edges(K, fits, edge):
    """a range just inside and just outside either end of the value domain: inside,
    an ordinary fit; outside, every sample in cluster 0.  sklearn is no reference between 2^-511
    and 2^-481, so these ranges are not in the table"""
    base = KI.smooth(5000, 90)
    base = (base - base.min()) / (base.max() - base.min())
    for factor in (0.99, 1.01):
        x = base * (edge * factor)
        inside = KI.in_value_domain(x)
        assert inside == ((factor > 1) == (edge < 1))
        ref = fits(x, None, 3)
        assert ref[0].any() == inside
        check_fit(K, K.kmeans_1d(dev(x), 3), x, None, ref, 0, 10)


# ---- the pair, and a shared sort ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mask_rule2", "mask_blocks", "mask_bad_values"])
def test_pair_with_a_mask_equals_two_fits(K, fits, name):
    case = KI.BY_NAME[name]
    x, valid = KI.build(case)
    d, v = dev(x), dev(valid)
    t1, t2 = K.kmeans_1d_pair(d, 2, 3, valid=v)                         # rules (2, 0)
    a = K.kmeans_1d(d, 2, valid=v, rule=2)
    b = K.kmeans_1d(d, 3, valid=v, rule=0)
    assert torch.equal(t1, a[1]) and torch.equal(t2, b[1])
    r2, r3 = fits(x, valid, 2), fits(x, valid, 3)
    assert np.array_equal(host(t1).astype(bool), KI.top_mask(x, valid, r2[0], r2[1], 2))
    assert np.array_equal(host(t2).astype(bool), KI.top_mask(x, valid, r3[0], r3[1], 0))
    u1, u2 = K.kmeans_1d_pair(d, 3, 2, valid=v, rules=(0, 1), n_init=3, max_iter=2)
    r3, r2 = fits(x, valid, 3, 3, 2), fits(x, valid, 2, 3, 2)
    assert np.array_equal(host(u1).astype(bool), KI.top_mask(x, valid, r3[0], r3[1], 0))
    assert np.array_equal(host(u2).astype(bool), KI.top_mask(x, valid, r2[0], r2[1], 1))


@pytest.mark.parametrize("name", ["mask_rule1", "rule1_zero_bucket", "five_levels_k8"])
def test_shared_sort_with_k_and_rule_changed_equals_fresh_fits(K, fits, name):
    case = KI.BY_NAME[name]
    x, valid = KI.build(case)
    d, v = dev(x), dev(valid)
    share = {}
    for k, rule, n_init, max_iter in [(2, 1, 10, 300), (3, 0, 10, 300), (2, 2, 3, 300), (8, 0, 10, 2), (1, 0, 1, 300),
                                      (2, 1, 10, 300)]:
        got = K.kmeans_1d(d, k, valid=v, share=share, rule=rule, n_init=n_init, max_iter=max_iter)
        fresh = K.kmeans_1d(d, k, valid=v, rule=rule, n_init=n_init, max_iter=max_iter)
        assert torch.equal(got[0], fresh[0]) and torch.equal(got[1], fresh[1]) and got[2:] == fresh[2:]
        check_fit(K, fresh, x, valid, fits(x, valid, k, n_init, max_iter), rule, n_init)
    assert share["ident"][0] == d.data_ptr()
