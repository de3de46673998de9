"""Plain restatements of the per-cell classifier back-end (backend.py's stages), the second
yardstick of tests/test_backend_edges_gpu.py beside oracle/backend.c.  Written from the module
docs of backend.py, include/hrf.h and the documented behaviour of libsvm / sklearn / umap-learn
0.4, as array code (SVC, kNN) and scalar Python (the coupling iteration, the UMAP transform);
themselves pinned to sklearn and to the oracle by tests/test_backend_ref.py.  numpy + math only.

Arithmetic: f64 everywhere except where umap keeps float32 (rho, sigma, memberships, the
embedding).  A float32 value is carried as a Python float that is exactly representable in
float32; rounding an f64 result of one +, -, * or / of two such values to float32 equals the
float32 operation (53 >= 2 * 24 + 2 bits), so `_f32(a * b)` is the float32 product.  exp / pow are
the C library's (math.exp, math.pow), not csrc/detmath.h's: the two agree to an ulp of f64, which
the float32 stores absorb."""
import math
import struct

import numpy as np

_F = struct.Struct("f")


def _f32(v):
    """round an f64 to the nearest float32 (returned as a Python float)"""
    return _F.unpack(_F.pack(v))[0]


# ---- SVC (libsvm one-vs-one) ---------------------------------------------------------------------
def svc_kernel_matrix(x, sv, kernel, gamma=1.0, coef0=0.0, degree=3):
    """K[i, s] = k(x_i, sv_s): 0 linear <x, s>; 1 poly (gamma <x, s> + coef0)^degree; 2 rbf
    exp(-gamma |x - s|^2); 3 sigmoid tanh(gamma <x, s> + coef0)"""
    x = np.asarray(x, np.float64)
    sv = np.asarray(sv, np.float64)
    with np.errstate(all="ignore"):
        if kernel == 2:
            d2 = np.zeros((len(x), len(sv)))
            for c in range(x.shape[1]):
                d2 += (x[:, c, None] - sv[None, :, c]) ** 2
            return np.exp(-gamma * d2)
        s = np.zeros((len(x), len(sv)))
        for c in range(x.shape[1]):
            s += x[:, c, None] * sv[None, :, c]
        if kernel == 0:
            return s
        if kernel == 1:
            base = gamma * s + coef0
            out = np.ones_like(base)
            for _ in range(int(degree)):
                out = out * base
            return out
        return np.tanh(gamma * s + coef0)


def pair_table(k):
    """libsvm's pair order: (0,1), (0,2) .. (0,k-1), (1,2) .. -> two int arrays"""
    a, b = np.triu_indices(k, 1)
    return a, b


def svc_decision(x, sv, coef, intercept, start, kernel, gamma=1.0, coef0=0.0, degree=3):
    """-> (first-maximum class (int32, n), pair decision values (n, pairs), votes (n, k)).
    coef (k - 1, nsv) / intercept (pairs) in libsvm's signs: pair (a, b) sums the class-a support
    vectors with coef[b - 1] and the class-b ones with coef[a], adds intercept, votes a when the
    sum is > 0 and b otherwise (a NaN sum therefore votes b)."""
    coef = np.asarray(coef, np.float64)
    intercept = np.asarray(intercept, np.float64)
    start = np.asarray(start, np.int64)
    k = len(start) - 1
    K = svc_kernel_matrix(x, sv, kernel, gamma, coef0, degree)
    n = len(K)
    dec = np.empty((n, k * (k - 1) // 2))
    assert np.all(np.diff(start) > 0), "every class owns a support vector (sklearn's models do)"
    p = 0
    with np.errstate(all="ignore"):
        for a in range(k - 1):
            sa = slice(start[a], start[a + 1])
            first = K[:, sa] @ coef[a:k - 1, sa].T            # (n, k-1-a): b = a+1 .. k-1
            second = np.add.reduceat(K * coef[a], start[:-1], axis=1)   # per-class sums (n, k)
            m = k - 1 - a
            dec[:, p:p + m] = first + second[:, a + 1:] + intercept[p:p + m]
            p += m
    pa, pb = pair_table(k)
    winner = np.where(dec > 0, pa[None, :], pb[None, :])
    votes = np.zeros((n, k), np.int64)
    for i in range(n):
        votes[i] = np.bincount(winner[i], minlength=k)
    return votes.argmax(axis=1).astype(np.int32), dec, votes


def platt(dec, A, B):
    """libsvm sigmoid_predict: 1 / (1 + exp(dec A + B)) written so that exp never overflows"""
    f = dec * A + B
    with np.errstate(all="ignore"):
        e = np.exp(-np.abs(f))
        return np.where(f >= 0, e / (1.0 + e), 1.0 / (1.0 + e))


def couple(r, info=None):
    """libsvm multiclass_probability (Wu, Lin & Weng, second method) on one k x k matrix of
    pairwise probabilities: p starts uniform; Q[t][t] = sum_{j != t} r[j][t]^2, Q[t][j] =
    -r[j][t] r[t][j]; up to max(100, k) sweeps, stopping when max_t |(Qp)_t - p'Qp| < 0.005 / k;
    a sweep updates one p[t] at a time and renormalises.  The maximum is libsvm's running
    `if (error > max) max = error`, which a NaN never enters (svc_proba's clamp hands it none)."""
    k = len(r)
    Q = -(r.T * r)
    sq = r * r
    for t in range(k):
        Q[t, t] = sq[:t, t].sum() + sq[t + 1:, t].sum()
    p = np.full(k, 1.0 / k)
    max_iter = max(100, k)
    eps = 0.005 / k
    sweeps = 0
    for _ in range(max_iter):
        Qp = Q @ p
        pQp = float(p @ Qp)
        if np.fmax.reduce(np.abs(Qp - pQp), initial=0.0) < eps:   # libsvm's running maximum skips a NaN
            break
        for t in range(k):
            diff = (-Qp[t] + pQp) / Q[t, t]
            p[t] += diff
            pQp = (pQp + diff * (diff * Q[t, t] + 2 * Qp[t])) / (1 + diff) / (1 + diff)
            Qp = (Qp + diff * Q[t]) / (1 + diff)
            p /= (1 + diff)
        sweeps += 1
    if info is not None:
        info.setdefault("sweeps", []).append(sweeps)  # 0: stopped at the first check; max_iter: never converged
    return p


def svc_proba(x, sv, coef, intercept, start, kernel, gamma, coef0, degree, probA, probB, info=None):
    """libsvm svm_predict_probability: Platt sigmoid per pair clamped to [1e-7, 1 - 1e-7], then
    the coupling (two classes are coupled too, as sklearn's libsvm does) -> (n, k).  A row holding
    a NaN has every pair clamped to 1e-7: nearly all probability on the last class, as sklearn gives.
    info (a dict) receives "sweeps" per row and "r_min" / "r_max" per row (the clamps)."""
    _, dec, _ = svc_decision(x, sv, coef, intercept, start, kernel, gamma, coef0, degree)
    k = len(start) - 1
    pa, pb = pair_table(k)
    rr = platt(dec, np.asarray(probA, np.float64)[None, :], np.asarray(probB, np.float64)[None, :])
    # libsvm's own max(x, y) = (x > y) ? x : y and min(x, y) = (x < y) ? x : y: a NaN fails the first
    # comparison and becomes 1e-7, a confident vote for the pair's second class
    rr = np.where(rr > 1e-7, rr, 1e-7)
    rr = np.where(rr < 1 - 1e-7, rr, 1 - 1e-7)
    out = np.empty((len(dec), k))
    for i in range(len(dec)):
        r = np.zeros((k, k))
        r[pa, pb] = rr[i]
        r[pb, pa] = 1 - rr[i]
        out[i] = couple(r, info)
        if info is not None:
            info.setdefault("r_min", []).append(rr[i].min())
            info.setdefault("r_max", []).append(rr[i].max())
    return out


# ---- kNN under the reference metrics ----------------------------------------------------------------
def _seg_cos(q, tr, lo, hi):
    """1 - cosine over columns lo..hi for every (query, row): 0 when both are all zero, 1 when
    one is; sums in column order"""
    r = np.zeros((len(q), len(tr)))
    nx = np.zeros((len(q), 1))
    ny = np.zeros((1, len(tr)))
    for c in range(lo, hi):
        r += q[:, c, None] * tr[None, :, c]
        nx += q[:, c, None] ** 2
        ny += tr[None, :, c] ** 2
    with np.errstate(all="ignore"):
        v = 1.0 - r / np.sqrt(nx * ny)
    v = np.where((nx == 0) | (ny == 0), 1.0, v)
    return np.where((nx == 0) & (ny == 0), 0.0, v)


def knn_distances(q, tr, metric):
    """all (nq, nt) distances.  metric 0 euclidean; 1 channel_cosine_intensity_7b_v2 (67 columns:
    four laser segments 0/23/43/57/63 and four flags; flags differing by 0.01 or more in total ->
    1.0, else half the mean of the segment cosines with a segment skipped when the QUERY's flag
    is 0); 2 the scalar of ..._violet_derivative_v2 (132 columns: five segments 0/32/55/75/89/95,
    six flags from 126; (d + c1 + .. + c5) / 6 with d = 0 and flag-skipped segments when the flags
    agree within 0.01, else d = 1 and every segment counted)"""
    q = np.asarray(q, np.float64)
    tr = np.asarray(tr, np.float64)
    if metric == 0:
        s = np.zeros((len(q), len(tr)))
        for c in range(q.shape[1]):
            s += (q[:, c, None] - tr[None, :, c]) ** 2
        return np.sqrt(s)
    f0, nf, b = (63, 4, (0, 23, 43, 57, 63)) if metric == 1 else (126, 6, (0, 32, 55, 75, 89, 95))
    check = np.zeros((len(q), len(tr)))
    for c in range(f0, f0 + nf):
        check += np.abs(q[:, c, None] - tr[None, :, c])
    agree = check < 0.01
    cs = []
    for s in range(len(b) - 1):
        c = _seg_cos(q, tr, b[s], b[s + 1])
        skipped = np.where((q[:, f0 + s] == 0)[:, None], 0.0, c)
        cs.append(skipped if metric == 1 else np.where(agree, skipped, c))
    if metric == 1:
        return np.where(agree, 0.5 * (cs[0] + cs[1] + cs[2] + cs[3]) / 4, 1.0)
    d = np.where(agree, 0.0, 1.0)
    return (d + cs[0] + cs[1] + cs[2] + cs[3] + cs[4]) / 6


def knn(q, tr, metric, k):
    """the k nearest rows by (distance, row index): a stable sort of all distances; slots past
    the table's size hold -1 / inf.  (NaN distances sort last here; the device keeps arrival
    order for them -- compared with the oracle only.)"""
    d = knn_distances(q, tr, metric)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    idx = np.full((len(d), k), -1, np.int32)
    dist = np.full((len(d), k), np.inf)
    idx[:, :order.shape[1]] = order
    dist[:, :order.shape[1]] = np.take_along_axis(d, order, axis=1)
    return idx, dist


# ---- umap-learn 0.4 transform ---------------------------------------------------------------------
def umap_init(idx, dist, emb, n_neighbors, local_connectivity=0.0, want_memb=False, info=None):
    """transform()'s initial embedding.  Per query: smooth_knn_dist (rho from the non-zero
    distances by local_connectivity, interpolated; sigma by 64 bisection steps towards
    sum_{j >= 1} exp(-(d_j - rho) / sigma) = log2(n_neighbors), tolerance 1e-5; floor 1e-3 x the
    row mean when rho > 0, else 1e-3 x the mean of ALL distances, summed in row-major order);
    memberships exp(-(d - rho) / sigma) (1 at or below rho) as float32; the row sorted by
    training index (CSR), l1-normalised (f64 sum, float32 store); float32 weighted sum of the
    training embedding.  Slots with idx < 0 carry no edge.
    info receives per row "rho_branch" ('index', 'interp', 'zero', 'max', 'none') and
    "floor" ('row', 'all' or None)."""
    idx = np.asarray(idx)
    dist = np.asarray(dist, np.float64)
    emb = np.asarray(emb, np.float32)
    nq, k = idx.shape
    d = emb.shape[1]
    total = 0.0
    for v in dist.ravel().tolist():
        total += v
    mean_all = total / float(nq * k) if nq * k else 0.0
    target = math.log2(n_neighbors)
    out = np.zeros((nq, d), np.float32)
    memb = np.zeros((nq, k), np.float32)
    embl = emb.astype(np.float64)
    for i in range(nq):
        di = dist[i].tolist()
        ii = idx[i].tolist()
        nz = [v for v in di if v > 0.0]
        rho, branch = 0.0, "none"
        if len(nz) >= local_connectivity:
            index = int(math.floor(local_connectivity))
            interp = local_connectivity - index
            if index > 0:
                rho, branch = _f32(nz[index - 1]), "index"
                if interp > 1e-5:
                    rho, branch = _f32(rho + interp * (nz[index] - nz[index - 1])), "interp"
            else:
                rho, branch = _f32(interp * (nz[0] if nz else 0.0)), "zero"
        elif nz:
            rho, branch = _f32(max(nz)), "max"
        lo, hi, mid = 0.0, math.inf, 1.0
        for _ in range(64):
            psum = 0.0
            for j in range(1, k):
                dd = di[j] - rho
                psum += math.exp(-(dd / mid)) if dd > 0 else 1.0
            if abs(psum - target) < 1e-5:
                break
            if psum > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2 if hi == math.inf else (lo + hi) / 2.0
        sigma, floor = _f32(mid), None
        if rho > 0.0:
            m = 0.0
            for v in di:
                m += v
            m /= k
            if sigma < 1e-3 * m:
                sigma, floor = _f32(1e-3 * m), "row"
        elif sigma < 1e-3 * mean_all:
            sigma, floor = _f32(1e-3 * mean_all), "all"
        edges = []
        for j in range(k):
            if ii[j] < 0:
                continue
            dd = di[j] - rho
            w = 1.0 if (dd <= 0.0 or sigma == 0.0) else _f32(math.exp(-(dd / sigma)))
            memb[i, j] = w
            edges.append((ii[j], w))
        edges.sort(key=lambda e: e[0])            # stable: equal training rows keep knn order
        s = 0.0
        for _, w in edges:
            s += abs(w)
        acc = [0.0] * d
        for t, w in edges:
            wn = _f32(w / s) if s != 0.0 else w
            row = embl[t]
            for c in range(d):
                acc[c] = _f32(acc[c] + _f32(wn * row[c]))
        out[i] = acc
        if info is not None:
            info.setdefault("rho_branch", []).append(branch)
            info.setdefault("floor", []).append(floor)
    return (out, memb) if want_memb else out


_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF


def _splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) & _M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return state, z ^ (z >> 31)


def query_stream(seed, row):
    """the three Tausworthe states of query `row`: successive splitmix64 outputs of
    seed ^ (0xD1B54A32D192ED03 (row + 1)), low 32 bits, with bits 1 / 3 / 4 set"""
    sm = (seed ^ (0xD1B54A32D192ED03 * (row + 1))) & _M64
    st = []
    for bit in (2, 8, 16):
        sm, z = _splitmix64(sm)
        st.append((z & _M32) | bit)
    return st


def _tau(st):
    """umap's tau_rand_int on unsigned 32-bit states"""
    st[0] = (((st[0] & 4294967294) << 12) & _M32) ^ ((((st[0] << 13) & _M32) ^ st[0]) >> 19)
    st[1] = (((st[1] & 4294967288) << 4) & _M32) ^ ((((st[1] << 2) & _M32) ^ st[1]) >> 25)
    st[2] = (((st[2] & 4294967280) << 17) & _M32) ^ ((((st[2] << 3) & _M32) ^ st[2]) >> 11)
    return st[0] ^ st[1] ^ st[2]


def _clip(v):
    return 4.0 if v > 4.0 else (-4.0 if v < -4.0 else v)


def _rdist(cur, o):
    r = 0.0
    for c in range(len(cur)):
        df = _f32(cur[c] - o[c])
        r += _f32(df * df)
    return r


def _pow(x, y):
    return math.pow(x, y)


def umap_refine(idx, memb, init, tail, n_epochs, a, b, gamma=1.0, alpha0=0.25, neg_rate=5.0, seed=0, info=None):
    """transform()'s refinement of `init` against the fixed training embedding `tail`.
    Edges: slot j of row i is kept when idx >= 0 and its float32 membership w is non-zero and
    >= float32(max(memb) / n_epochs); epochs_per_sample = n_epochs / (n_epochs w / wmax) in
    float32.  Epoch n (alpha = alpha0 for epochs 0 and 1, then alpha0 (1 - (n - 1) / n_epochs):
    it is recomputed at the END of an epoch) visits the row's due edges in knn order: the
    attractive step (gradient coefficient -2ab d2^(b-1) / (a d2^b + 1), 0 when d2 == 0, each
    component clipped to +-4), then int((n - next_negative) / per_negative) negative samples
    drawn from the row's own stream (training row = draw mod ntrain): repulsive coefficient
    2 gamma b / ((0.001 + dn)(a dn^b + 1)); at dn == 0 the sample is skipped when the drawn row
    number equals the query's row number and pushes +4 on every component otherwise.  The state
    is float32, the gradients f64.
    info receives "zero_same" / "zero_other" (counts of the two dn == 0 cases), "d2_zero" and
    "edges" (kept edges per row)."""
    idx = np.asarray(idx)
    memb = np.asarray(memb, np.float32)
    tail = np.asarray(tail, np.float32)
    out = np.array(init, np.float32, copy=True)
    nq, k = idx.shape
    d = tail.shape[1]
    ntrain = len(tail)
    taill = tail.astype(np.float64).tolist()
    wmax = float(memb.max()) if memb.size else 0.0
    if not wmax > 0.0:
        wmax = 0.0
    thr = _f32(wmax / float(n_epochs))
    ne32 = _f32(float(n_epochs))
    stats = {"zero_same": 0, "zero_other": 0, "d2_zero": 0, "edges": []}
    for i in range(nq):
        eps, nxt, nneg_nxt, tl = [], [], [], []
        for j in range(k):
            w = float(memb[i, j])
            if idx[i, j] < 0 or not (w >= thr) or w == 0.0:
                continue
            ns = _f32(ne32 * _f32(w / wmax))
            e = _f32(ne32 / ns) if ns > 0.0 else -1.0
            eps.append(e)
            nxt.append(e)
            nneg_nxt.append(e / neg_rate)
            tl.append(int(idx[i, j]))
        stats["edges"].append(len(tl))
        cur = out[i].astype(np.float64).tolist()
        st = query_stream(seed, i)
        alpha = alpha0
        for n in range(n_epochs):
            for e in range(len(tl)):
                if not (nxt[e] <= n):
                    continue
                o = taill[tl[e]]
                d2 = _rdist(cur, o)
                gc = 0.0
                if d2 > 0.0:
                    gc = -2.0 * a * b * _pow(d2, b - 1.0)
                    gc /= a * _pow(d2, b) + 1.0
                else:
                    stats["d2_zero"] += 1
                for c in range(d):
                    g = _clip(gc * _f32(cur[c] - o[c]))
                    cur[c] = _f32(cur[c] + g * alpha)
                nxt[e] += eps[e]
                per_neg = eps[e] / neg_rate
                nneg = int((n - nneg_nxt[e]) / per_neg)
                for _ in range(nneg):
                    kk = _tau(st) % ntrain
                    on = taill[kk]
                    dn = _rdist(cur, on)
                    if dn > 0.0:
                        gn = 2.0 * gamma * b
                        gn /= (0.001 + dn) * (a * _pow(dn, b) + 1.0)
                    elif kk == i:
                        stats["zero_same"] += 1
                        continue
                    else:
                        stats["zero_other"] += 1
                        gn = 0.0
                    for c in range(d):
                        g = _clip(gn * _f32(cur[c] - on[c])) if gn > 0.0 else 4.0
                        cur[c] = _f32(cur[c] + g * alpha)
                nneg_nxt[e] += nneg * per_neg
            alpha = alpha0 * (1.0 - float(n) / float(n_epochs))
        out[i] = cur
    if info is not None:
        info.update(stats)
    return out
