"""The k-means case table (tests/kmeans_inputs.py) on the CPU alone: every case reaches the branch
of kmeans.hip it is built for (proved from the input by the numpy geometry), and the CPU
restatement (oracle/kmeans_sk.c) returns sklearn 1.7.2's labels_ and n_iter_ on every case --
but those flagged sklearn_differs, which must belong to one of three classes and must indeed
differ (k-means thresholds and value domain, records what differs in each)."""
import warnings

import numpy as np
import pytest

import kmeans_inputs as KI

CASES = KI.CASES
GROUP = {}
for _c in CASES:
    GROUP.setdefault(_c.group, []).append(_c)


@pytest.fixture(scope="module")
def fits(orc):
    """restatement fits, one per case, shared by the tests below"""
    done = {}

    def fit(case):
        if case.name not in done:
            x, valid = KI.build(case)
            done[case.name] = orc.kmeans_sk_runs(x, case.k, valid, case.n_init, case.max_iter)
        return done[case.name]

    return fit


def values(case):
    return KI.valid_values(*KI.build(case))


def lloyd_bracket(v, c_lo, c_hi):
    """km_bucket_step's first bracket for the step between two neighbouring centres: the buckets
    of midpoint -+ (|c| + |c'| + range) 2^-40 -> (populations of those buckets)"""
    mn, mx = v.min(), v.max()
    m = 0.5 * c_lo + 0.5 * c_hi
    delta = (abs(c_lo) + abs(c_hi) + (mx - mn)) * 2.0 ** -40
    b = KI.buckets(np.array([mn, mx, m - delta, m + delta]))[2:]
    return KI.bucket_counts(v)[b[0]:b[1] + 1]


# ---- preconditions ----------------------------------------------------------------------------
def test_table_is_complete():
    """the groups and sizes the table promises"""
    assert [len(KI.build(c)[0]) for c in GROUP["sizes"]] == [4095, 4096, 4097, 8192, 8193, 16385]
    assert {(c.k, c.n_init) for c in GROUP["n_init"]} == {(k, ni) for k in (2, 3, 8) for ni in (1, 3, 9)}
    assert {(c.k, c.max_iter) for c in GROUP["max_iter"]} == {(k, mi) for k in (3, 8) for mi in (1, 2)}
    for g in ("crowded1", "crowded63", "crowded_bracket"):
        assert {2, 3} <= {c.k for c in GROUP[g]}
    # one coarse digit: the same one-sided input at k = 2 (table) and k = 3 (reported defect)
    k2, (k3,) = KI.BY_NAME["one_coarse_digit_k2"], KI.REPORTED
    assert (k2.k, k3.k) == (2, 3) and np.array_equal(KI.build(k2)[0], KI.build(k3)[0])
    assert k3.sklearn_differs == KI.REPORTED_DEFECT and KI.DEVICE_CASES == CASES + KI.REPORTED
    assert max(len(KI.build(c)[0]) for c in CASES) == (1 << 20) + 1
    assert all(c.sklearn_differs in (None, KI.TIES, KI.K_ABOVE_VALUES, KI.FAR_OUTLIERS) for c in CASES)
    flagged = {c.name: c.sklearn_differs for c in CASES if c.sklearn_differs}
    assert flagged == {"crowded_levels_k3": KI.TIES, "five_levels_jitter_k8": KI.K_ABOVE_VALUES,
                       "far_outliers_k4": KI.FAR_OUTLIERS}


def test_sizes_cross_the_chunk_and_scan_blocks():
    blocks = {len(KI.build(c)[0]): KI.potential_blocks(len(KI.build(c)[0])) for c in GROUP["sizes"]}
    assert blocks == {4095: 1, 4096: 1, 4097: 2, 8192: 2, 8193: 3, 16385: 5}
    assert KI.pass_a_scan_blocks(16384) == 1 and KI.pass_a_scan_blocks(16385) == 2
    assert all(KI.pass_a_scan_blocks(n) == 1 for n in blocks if n < 16385)


def test_pick_above_2p20_gives_two_blocks_per_thread():
    (case,) = GROUP["pick"]
    n = values(case).size
    assert n == (1 << 20) + 1 and KI.pick_blocks_per_thread(n) == 2 and KI.pick_blocks_per_thread(n - 1) == 1
    assert all(KI.pick_blocks_per_thread(values(c).size) == 1 for c in CASES if c.group not in ("pick",))


def test_early_stop_without_strict_convergence(fits):
    hit = 0
    for case in GROUP["max_iter"]:
        runs = fits(case)[3]
        hit += int(np.any((runs[:, 0] == case.max_iter) & (runs[:, 1] == 0)))
    assert hit >= 1
    # and the default max_iter is never what stops a run of the other cases
    assert all(fits(c)[3][:, 0].max() < c.max_iter for c in KI.DEVICE_CASES if c.group != "max_iter")


def test_fewer_runs_can_change_the_winner(fits):
    """the winner over n_init runs is a run index below n_init, and the per-run records of a
    shorter fit are a prefix of the longer one's only where the stream allows: the first run is"""
    for case in GROUP["n_init"]:
        lab, cen, info, runs = fits(case)
        assert runs.shape == (case.n_init, 3) and 0 <= info[0] < case.n_init
    assert len({int(fits(c)[2][0]) for c in GROUP["n_init"]}) > 1      # not always run 0


@pytest.mark.parametrize("case", GROUP["crowded1"] + GROUP["crowded63"], ids=lambda c: c.name)
def test_crowded_buckets(case):
    counts = KI.bucket_counts(values(case))
    crowded = int(np.sum(counts > KI.CHUNK))
    assert crowded >= (1 if case.group == "crowded1" else 2)
    if case.group == "crowded1":
        assert np.count_nonzero(counts) == 9 and crowded == 8          # eight buckets 1/8 wide and the outlier's
    else:
        assert np.count_nonzero(counts) == 63 and crowded == 63


@pytest.mark.parametrize("case", GROUP["crowded_bracket"] + [c for c in GROUP["crowded1"] if c.k == 3] +
                         [KI.BY_NAME["far_outliers_k4"]] + KI.REPORTED,
                         ids=lambda c: c.name)
def test_lloyd_bracket_holds_crowded_buckets(case, fits):
    """the probing loop below the exhaustive count runs when a bracket holds more than 4096
    samples; in the crowded_bracket cases several crowded buckets share one bracket"""
    v = values(case)
    cen = np.sort(fits(case)[1])
    pops = [lloyd_bracket(v, a, b) for a, b in zip(cen[:-1], cen[1:])]
    assert any(p.sum() > KI.CHUNK for p in pops)
    if case.group == "crowded_bracket":
        assert any(p.sum() > KI.CHUNK and np.sum(p > KI.CHUNK) >= 2 for p in pops)


@pytest.mark.parametrize("case", GROUP["coarse"] + KI.REPORTED, ids=lambda c: c.name)
def test_one_coarse_digit_needs_many_chunks(case):
    v = values(case)
    coarse = KI.coarse_counts(v)
    outliers = int(np.sum(np.abs(v) >= 2.0 ** 30))
    assert 0 < outliers <= 6 and coarse.max() == v.size - outliers
    assert KI.pass_b_chunks(v).max() >= 5
    assert np.count_nonzero(coarse) == 1 + len({float(s) for s in np.sign(v[np.abs(v) >= 2.0 ** 30])})


def test_k_above_the_distinct_values_relocates_in_every_run(fits):
    case = KI.BY_NAME["five_levels_k8"]
    v = values(case)
    lev, count = np.unique(v, return_counts=True)
    assert lev.size == 5 and count.min() > 8                            # the farthest samples tie among equals
    assert np.all(fits(case)[3][:, 2] > 0)
    assert fits(KI.BY_NAME["five_levels_k3"])[3][:, 2].sum() == 0


def test_value_domain_cases():
    inside = {c.name: KI.in_value_domain(values(c)) for c in GROUP["domain"]}
    for name, ok in inside.items():
        outside = any(t in name for t in ("1e-300", "1e-170", "1e160", "1e300"))
        assert ok != outside, name
    v = values(KI.BY_NAME["negatives_zeros_k3"])
    assert v.max() == 0.0 and np.any(np.signbit(v[v == 0.0])) and not np.all(np.signbit(v[v == 0.0]))
    v = values(KI.BY_NAME["one_subnormal_k3"])
    assert 0.0 < v.min() < np.finfo(np.float64).tiny and np.sort(v)[1] > 0.4


def test_valid_mask_cases():
    for case, nv in zip(GROUP["mask_count"], (1, 4095, 4096, 4097)):
        x, valid = KI.build(case)
        assert x.size == 20000 and int(valid.sum()) == nv
    x, valid = KI.build(KI.BY_NAME["mask_blocks"])
    per_block = valid.reshape(5, KI.CHUNK).sum(axis=1)
    assert per_block.tolist() == [KI.CHUNK, 0, KI.CHUNK, 0, KI.CHUNK]
    x, valid = KI.build(KI.BY_NAME["mask_bad_values"])
    bad = ~np.isfinite(x)
    assert np.isnan(x).any() and (x == np.inf).any() and (x == -np.inf).any() and not np.any(bad & (valid != 0))
    x, valid = KI.build(KI.BY_NAME["mask_scan_carry"])
    assert -(-x.size // KI.CHUNK) > KI.PT                                # more block counts than one scan round
    assert {c.rule for c in GROUP["mask_rules"]} == {1, 2} and all(KI.build(c)[1] is not None for c in GROUP["mask_rules"])


def test_rule1_counts_inside_a_bucket(fits):
    case = KI.BY_NAME["rule1_zero_bucket"]
    x, _ = KI.build(case)
    b = KI.buckets(x)
    b0 = b[np.flatnonzero(x == 0.0)[0]]
    assert np.all(b[x == 0.0] == b0)
    inside = x[b == b0]
    assert np.any(inside > 0.0) and np.sum(inside == 0.0) == 500 and np.any(x < 0.0)
    # the lower cluster's only positives are those: a count of the whole bucket as <= 0 would
    # flip the rule, and the flip shows in the mask because the upper cluster is not id 0
    lab, cen, _, _ = fits(case)
    hi = int(np.argmax(cen))
    assert hi != 0 and np.all(b[(lab == 1 - hi) & (x > 0.0)] == b0)
    assert KI.top_mask(x, None, lab, cen, 1).sum() == np.sum(lab == hi)
    case = KI.BY_NAME["mask_rule1_no_positive"]
    x, valid = KI.build(case)
    lab, cen, _, _ = fits(case)
    assert np.array_equal(KI.top_mask(x, valid, lab, cen, 1), lab == 0)


# ---- the restatement against sklearn ----------------------------------------------------------
def sk_fit(case):
    from sklearn.cluster import KMeans
    x, valid = KI.build(case)
    v = KI.valid_values(x, valid)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")           # ConvergenceWarning: fewer distinct points than clusters
        with np.errstate(all="ignore"):
            return KMeans(n_clusters=case.k, random_state=0, n_init=case.n_init,
                          max_iter=case.max_iter).fit(v.reshape(-1, 1))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_restatement_equals_sklearn(case, fits):
    """labels_ (cluster ids, not only the partition) and n_iter_.  A flagged case must differ:
    a flag that no longer holds is removed, not kept"""
    x, valid = KI.build(case)
    lab, cen, info, runs = fits(case)
    sk = sk_fit(case)
    ours = lab.ravel() if valid is None else lab.ravel()[valid.astype(bool)]
    if valid is not None:
        assert np.all(lab.ravel()[~valid.astype(bool)] == -1)
    same = np.array_equal(ours, sk.labels_) and int(info[1]) == sk.n_iter_
    if case.sklearn_differs:
        assert not same, "flag %r no longer needed" % case.sklearn_differs
    else:
        assert np.array_equal(ours, sk.labels_)
        assert int(info[1]) == sk.n_iter_
    assert runs[info[0], 0] == info[1] and runs[info[0], 1] == info[2] and runs[:, 2].sum() == info[3]


def test_reported_defect_one_sided_outliers_k3(fits):
    """NOT excused, reported: 20000 samples in [0, 1) plus three at 2^30, k = 3.  Once the outlier
    level holds a centre every bulk potential is floor(d^2 * 2^S) = 0 (S = 0: the fixed point
    resolves 2^-61 of the largest squared distance, 2^60 here), so all trials of the third centre
    pick the first sample, x[0], where sklearn draws by distance.  Every run stops after one
    iteration (tol = 1e-4 var is ~1.7e10), so the seeds decide the fit.  Figures, pinned so that
    the discrepancy cannot drift unseen: restatement run 8, sizes 10025 / 3 / 9975, inertia
    417.1816; sklearn sizes 9607 / 3 / 10393, inertia 421.7547; 418 labels differ.  A fix needs
    potentials finer than 2^-61 of the range squared, in kernel and restatement alike."""
    (case,) = KI.REPORTED
    x, _ = KI.build(case)
    lab, cen, info, runs = fits(case)
    sk = sk_fit(case)
    assert info.tolist() == [8, 1, 0, 0] and runs.tolist() == [[1, 0, 0]] * 10 and sk.n_iter_ == 1
    assert np.bincount(lab).tolist() == [10025, 3, 9975] and np.bincount(sk.labels_).tolist() == [9607, 3, 10393]
    assert int(np.sum(lab != sk.labels_)) == 418
    assert np.array_equal(lab == 1, x == 2.0 ** 30) and np.array_equal(sk.labels_ == 1, x == 2.0 ** 30)
    ours = sum(((x[lab == j] - cen[j]) ** 2).sum() for j in range(3))
    assert abs(ours - 417.1816378962) < 1e-6 and abs(sk.inertia_ - 421.7547323318) < 1e-6
    # the blind seed: with n_init = 1 and one iteration, the third centre is the mean of the
    # bulk samples nearer to x[0] than to the first centre
    l1, c1, i1, _ = __import__("oracle").kmeans_sk_runs(x, 3, n_init=1)
    first = x[__import__("oracle").kmeans_draws(x.size, 3, 1)[0][0]]
    bulk = x < 2.0
    near0 = bulk & (np.abs(x - x[0]) < np.abs(x - first))
    assert i1[1] == 1 and abs(c1[2] - x[near0].mean()) < 1e-6 and abs(c1[0] - x[bulk & ~near0].mean()) < 1e-6


@pytest.mark.parametrize("case", KI.REFUSED, ids=lambda c: c.name)
def test_refused_inputs_raise_as_sklearn_does(case, orc):
    from sklearn.cluster import KMeans
    x, valid = case.gen()
    v = KI.valid_values(x, valid)
    with pytest.raises(ValueError):
        KMeans(n_clusters=case.k, random_state=0, n_init=10).fit(v.reshape(-1, 1))
    with pytest.raises(ValueError, match="infinity" if case.why == "infinity" else "n_samples=%d .* n_clusters=%d"
                       % (v.size, case.k)):
        orc.kmeans_sk(x, case.k, valid)


def test_empty_inputs_stay_as_they_were(orc):
    """no valid sample at all is not refused (test_kmeans_quantised_and_degenerate pins the device)"""
    lab, cen, info = orc.kmeans_sk(np.zeros(0), 2)
    assert lab.size == 0
    lab, cen, info = orc.kmeans_sk(np.arange(5.0), 2, np.zeros(5, np.uint8))
    assert np.all(lab == -1) and np.all(cen == 0)


def test_tolerance_and_inertia_survive_a_large_mean(fits):
    """tol = 1e-4 var(x) and the inertia that picks the winning run: the large_mean values have
    var / mean^2 ~ 2^-60, below the 2^-53 an f64 difference of squares about zero resolves (that
    gave a tolerance and inertias of rounding noise: other iteration counts, another winner).
    sklearn centres the data first; the restatement takes n sum(q^2) - sum(q)^2 in integers"""
    winners = set()
    for case in GROUP["tol"]:
        x, _ = KI.build(case)
        assert x.var() / x.mean() ** 2 < 2.0 ** -55
        lab, cen, info, runs = fits(case)
        sk = sk_fit(case)
        assert info[1] == sk.n_iter_ and np.array_equal(lab, sk.labels_)
        assert np.all(runs[:, 1] == 0)            # every run stopped by the tolerance, not by equal labels
        winners.add(int(info[0]))
    assert winners != {0}                          # and the inertia contest is not won by default
