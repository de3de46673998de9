"""Inputs shared by tests/test_backend_ref.py (CPU) and tests/test_backend_edges_gpu.py: random
and constructed SVC models, kNN tables and UMAP graphs at the class counts, sizes and edges the
back-end kernels branch on.  numpy only; models are dicts with sklearn's attribute names."""
import numpy as np

KERNEL_ID = {"linear": 0, "poly": 1, "rbf": 2, "sigmoid": 3}


# ---- SVC -------------------------------------------------------------------------------------------
def sk_model(clf):
    """the public attributes of a fitted sklearn SVC as arrays"""
    m = dict(sv=clf.support_vectors_, dual_coef=clf.dual_coef_, intercept=clf.intercept_,
             n_support=clf.n_support_.astype(np.int32), classes=clf.classes_.astype(np.float64),
             kernel=np.int32(KERNEL_ID[clf.kernel]), gamma=np.float64(clf._gamma), coef0=np.float64(clf.coef0),
             degree=np.int32(clf.degree))
    if clf.probability:
        m["probA"], m["probB"] = clf.probA_, clf.probB_
    return m


def from_fixture(g, name):
    keys = [k[len(name) + 1:] for k in g.files if k.startswith(name + "_")]
    return {k: g[name + "_" + k] for k in keys}


def libsvm(m):
    """-> (sv, coef, intercept, start, kernel, gamma, coef0, degree) in libsvm's signs (sklearn
    negates dual_coef_ and intercept_ of a two-class model)"""
    dual, inter = np.asarray(m["dual_coef"], np.float64), np.asarray(m["intercept"], np.float64).ravel()
    ns = np.asarray(m["n_support"], np.int64)
    if len(ns) == 2:
        dual, inter = -dual, -inter
    start = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    return (np.asarray(m["sv"], np.float64), dual, inter, start, int(m["kernel"]), float(m["gamma"]),
            float(m["coef0"]), int(m["degree"]))


def random_svc(rng, ncls, f, kernel="rbf", per_class=2, gamma=0.5, coef0=0.0, degree=3, proba=False, spread=1.0):
    """a random model in sklearn's layout: per_class support vectors around one centre per class"""
    ns = np.full(ncls, per_class, np.int32)
    nsv = int(ns.sum())
    centres = rng.normal(0, spread, (ncls, f))
    sv = np.repeat(centres, per_class, axis=0) + 0.2 * rng.normal(size=(nsv, f))
    npair = ncls * (ncls - 1) // 2
    m = dict(sv=sv, dual_coef=rng.normal(size=(ncls - 1, nsv)), intercept=0.1 * rng.normal(size=npair), n_support=ns,
             classes=np.arange(ncls, dtype=np.float64), kernel=np.int32(KERNEL_ID[kernel]), gamma=np.float64(gamma),
             coef0=np.float64(coef0), degree=np.int32(degree))
    if proba:
        m["probA"] = -rng.uniform(0.5, 3.0, npair)
        m["probB"] = 0.2 * rng.normal(size=npair)
    return m, centres


def cycle_model():
    """three classes, one support vector each, linear kernel on one feature, x = 1: kernel values
    are the support vectors themselves (1, 1, 1).  Pair sums: (0,1) = +1 -> 0, (0,2) = -1 -> 2,
    (1,2) = +1 -> 1: one vote each, the first maximum is class 0."""
    # pair (a, b): coef[b-1][sv of a] kv + coef[a][sv of b] kv + intercept
    dual = np.zeros((2, 3))
    inter = np.array([1.0, -1.0, 1.0])
    return dict(sv=np.ones((3, 1)), dual_coef=dual, intercept=inter, n_support=np.ones(3, np.int32),
                classes=np.arange(3.0), kernel=np.int32(0), gamma=np.float64(1.0), coef0=np.float64(0.0),
                degree=np.int32(3))


def zero_model(ncls=5, f=3):
    """every coefficient and intercept 0: every pair sum is exactly 0 and votes b, so the last
    class collects ncls - 1 votes"""
    return dict(sv=np.ones((ncls, f)), dual_coef=np.zeros((ncls - 1, ncls)), intercept=np.zeros(ncls * (ncls - 1) // 2),
                n_support=np.ones(ncls, np.int32), classes=np.arange(float(ncls)), kernel=np.int32(0),
                gamma=np.float64(1.0), coef0=np.float64(0.0), degree=np.int32(3))


def nearest_centre_svc(centres, gamma, A):
    """an rbf model that votes for the nearer centre in every pair: one support vector per class,
    coefficient +1 where its class is the pair's first and -1 where it is the second, intercepts
    0; Platt slope A (negative), offset 0 -- confident near a centre, flat between centres"""
    k = len(centres)
    dual = np.where(np.arange(k - 1)[:, None] >= np.arange(k)[None, :], 1.0, -1.0)
    npair = k * (k - 1) // 2
    return dict(sv=np.asarray(centres, np.float64), dual_coef=dual, intercept=np.zeros(npair),
                n_support=np.ones(k, np.int32), classes=np.arange(float(k)), kernel=np.int32(2), gamma=np.float64(gamma),
                coef0=np.float64(0.0), degree=np.int32(3), probA=np.full(npair, float(A)), probB=np.zeros(npair))


def two_tied_dominant(k):
    """pairwise probabilities of the slowest coupling found: classes 0 and 1 beat every other
    class at the clamp and tie with each other; all other pairs tie"""
    r = np.full((k, k), 0.5)
    r[:2, 2:] = 1 - 1e-7
    r[2:, :2] = 1e-7
    np.fill_diagonal(r, 0.0)
    return r


def slow_coupling_model(k):
    """a model whose pair probabilities are two_tied_dominant(k) for x = 1: one support vector
    per class, zero coefficients, the intercepts as decision values (+40 -> clamped, 0 -> 1/2),
    probA = -1, probB = 0"""
    a, b = np.triu_indices(k, 1)
    inter = np.where((a < 2) & (b >= 2), 40.0, 0.0)
    return dict(sv=np.ones((k, 1)), dual_coef=np.zeros((k - 1, k)), intercept=inter, n_support=np.ones(k, np.int32),
                classes=np.arange(float(k)), kernel=np.int32(0), gamma=np.float64(1.0), coef0=np.float64(0.0),
                degree=np.int32(3), probA=-np.ones(len(a)), probB=np.zeros(len(a)))


def probe_model(gamma):
    """two classes, two support vectors, coefficients (1, 0), intercept 0 (libsvm signs): the one
    decision value IS the rbf kernel value of the first support vector (0 * kv + kv + 0)"""
    return dict(sv=np.array([[0.0], [1.0]]), dual_coef=-np.array([[1.0, 0.0]]), intercept=-np.array([0.0]),
                n_support=np.ones(2, np.int32), classes=np.arange(2.0), kernel=np.int32(2), gamma=np.float64(gamma),
                coef0=np.float64(0.0), degree=np.int32(3))


# ---- kNN ---------------------------------------------------------------------------------------------
def knn_line(nt, descending, f=3):
    """rows on a line so that the distance to the query at the origin strictly descends (or
    ascends) with the row index: with descending every row of every 256-row chunk beats the
    current k-th and is a candidate"""
    r = np.arange(nt, dtype=np.float64)
    t = (nt - r) if descending else (r + 1.0)
    tr = np.zeros((nt, f))
    tr[:, 0] = t
    tr[:, 1] = 0.5 * t
    return np.zeros((3, f)), tr


def knn_boundary_pairs(rng, nt=600, f=6):
    """identical rows on either side of the chunk boundaries 255|256 and 511|512, and queries
    next to them: the lower row must come first although it is merged a chunk earlier"""
    tr = rng.random((nt, f))
    tr[256] = tr[255]
    tr[512] = tr[511]
    q = np.vstack([tr[255] + 1e-3, tr[511] - 1e-3, tr[255], tr[511], rng.random((4, f))])
    return q, tr


def knn_metric_edges(rng, metric):
    """rows that reach every branch of the segmented-cosine metrics: a segment all zero in the
    query only, in the training row only, in both; a query flag of 0; flags differing by 0.009 and
    by 0.011 in total"""
    f, f0, nf, b = (67, 63, 4, (0, 23, 43, 57, 63)) if metric == 1 else (132, 126, 6, (0, 32, 55, 75, 89, 95))
    tr = rng.random((48, f))
    tr[:, f0:] = 1.0
    q = rng.random((10, f))
    q[:, f0:] = 1.0
    tr[0:6, b[0]:b[1]] = 0.0                 # training rows with segment 0 zero
    tr[6:12, b[2]:b[3]] = 0.0                # ... segment 2 zero
    q[1, b[0]:b[1]] = 0.0                    # both zero against rows 0..5, query-only against the rest
    q[2, b[1]:b[2]] = 0.0                    # query-only zero segment
    q[3, f0 + 2] = 0.0                       # flag 0: segment 2 skipped (rows 12..17 agree on the flag)
    tr[12:18, f0 + 2] = 0.0
    q[4, b[0]:b[1]] = 0.0                    # zero segment AND its flag 0
    q[4, f0] = 0.0
    tr[18:22, f0] = 0.0
    tr[22:28, f0:f0 + 3] += 0.003            # total 0.009: still "equal flags"
    tr[28:34, f0:f0 + 2] += 0.004            # total 0.011: mismatch
    tr[28:34, f0 + 2] += 0.003
    tr[34:40, f0 + 1] = 0.0                  # plain mismatch
    return q, tr


# ---- UMAP ------------------------------------------------------------------------------------------
def graph(rng, nq, k, nt):
    """a kNN-like graph: k distinct training rows per query, distances ascending in (0.05, 1)"""
    idx = np.stack([rng.permutation(nt)[:k] if nt >= k else np.concatenate([rng.permutation(nt), -np.ones(k - nt)])
                    for _ in range(nq)]).astype(np.int32)
    dist = np.sort(rng.uniform(0.05, 1.0, (nq, k)), axis=1)
    dist[idx < 0] = np.inf
    return idx, dist


def zero_runs(rng, dist):
    """the first 0..k distances of each row set to 0 (query equal to training rows); row 0 keeps
    none, row 1 all"""
    d = dist.copy()
    nq, k = d.shape
    runs = rng.integers(0, k + 1, nq)
    runs[0], runs[min(1, nq - 1)] = 0, k
    if nq > 2:
        runs[2] = min(2, k)
    for i, r in enumerate(runs):
        d[i, :r] = 0.0
    return d


def three_point_embedding(d=2):
    """six training rows on three distinct points (row j and row j + 3 coincide)"""
    pts = np.zeros((3, d), np.float32)
    pts[0, 0], pts[1, 0], pts[2, 0] = 1.5, -2.0, 0.25
    pts[:, -1] += np.float32([0.5, 1.0, -3.0])
    return np.vstack([pts, pts])


def umap_families():
    """name -> dict(idx, dist, emb, n_neighbors, lc): the eight input families"""
    rng = np.random.default_rng(31)
    fam = {}

    def add(name, nq, k, nt, d, lc, zeros=False, emb=None):
        idx, dist = graph(rng, nq, k, nt)
        if zeros:
            dist = zero_runs(rng, dist)
        e = (rng.normal(size=(nt, d)) * 3).astype(np.float32) if emb is None else emb
        fam[name] = dict(idx=idx, dist=dist, emb=e, n_neighbors=float(max(k, 2)), lc=lc)

    add("plain", 24, 15, 200, 2, 0.0)
    add("lc1.5_d3", 24, 15, 200, 3, 1.5)
    add("zeros_lc0", 24, 15, 200, 2, 0.0, zeros=True)
    add("zeros_lc3", 24, 15, 200, 2, 3.0, zeros=True)
    add("k1", 24, 1, 50, 2, 0.0)
    add("k64_d8", 8, 64, 300, 8, 1.0)
    add("nt5_k8", 24, 8, 5, 2, 0.0)
    add("three_points", 24, 4, 6, 2, 0.0, emb=three_point_embedding(2))
    return fam


def sigma_floor_case(nq=70, k=15, nt=120):
    """even rows: six zero distances, then distances of 1e-4 .. 2e-3.  With local_connectivity 0
    rho is 0; five ones in the sum exceed log2(15) whatever sigma is, so the bisection halves it
    64 times, and it is floored at 1e-3 x the mean of ALL distances (~2.6e-4: the odd rows are
    ordinary).  The small distances then weigh exp(-d / floor), between 0 and 1 -- without the
    floor, or with the row's own mean (~6e-7), they would weigh 0.  70 rows cross the 64-thread
    block."""
    rng = np.random.default_rng(33)
    idx, dist = graph(rng, nq, k, nt)
    dist[0::2, :6] = 0.0
    dist[0::2, 6:] = np.sort(rng.uniform(1e-4, 2e-3, (len(dist[0::2]), k - 6)), axis=1)
    return idx, dist, (rng.normal(size=(nt, 2)) * 3).astype(np.float32)


def refine_edge_cases():
    """name -> (idx, memb, init, tail, n_epochs) beyond the eight families"""
    rng = np.random.default_rng(34)
    out = {}
    for d, ne in ((1, 30), (2, 100), (8, 30)):
        out["coincident_d%d-%d" % (d, ne)] = coincident_refine_case(d) + (ne,)
    # every edge of the even rows below wmax / n_epochs = 1 / 30
    idx, _ = graph(rng, 20, 6, 40)
    memb = np.ones((20, 6), np.float32)
    memb[0::2] = np.float32(1e-3) * rng.uniform(0.1, 1.0, (10, 6)).astype(np.float32)
    tail = (rng.normal(size=(40, 2)) * 3).astype(np.float32)
    out["dropped-30"] = (idx, memb, tail[idx[:, 0]] + np.float32(0.5), tail, 30)
    # one training row: every negative sample is row 0
    idx1 = np.zeros((9, 3), np.int32)
    idx1[:, 1:] = -1
    memb1 = np.zeros((9, 3), np.float32)
    memb1[:, 0] = rng.uniform(0.3, 1.0, 9)
    out["ntrain1-30"] = (idx1, memb1, rng.normal(size=(9, 2)).astype(np.float32), np.float32([[0.5, -0.25]]), 30)
    # one dimension, rows across the 64-thread block
    idx, dist = graph(rng, 65, 5, 30)
    memb = np.exp(-dist).astype(np.float32)
    tail = (rng.normal(size=(30, 1)) * 3).astype(np.float32)
    out["d1_nq65-30"] = (idx, memb, tail[idx[:, 0]] + np.float32(0.25), tail, 30)
    return out


def coincident_refine_case(d=2, nq=30):
    """queries that START on a training point whose twin row is their second neighbour: the
    attractive step sees d2 == 0; a negative sample of the query's own row number at distance 0 is
    skipped, one of the twin row pushes by +4 alpha -> (idx, memb, init, tail)"""
    tail = three_point_embedding(d)
    idx = np.array([[i % 6, (i % 6 + 3) % 6] for i in range(nq)], np.int32)
    memb = np.ones((nq, 2), np.float32)
    init = tail[idx[:, 0]].copy()
    return idx, memb, init, tail
