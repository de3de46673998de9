"""Write tests/golden/backend_edges.npz: sklearn SVC models and their outputs at the class counts
and kernel branches tests/test_backend_edges_gpu.py cannot refit on the device side --
predict_proba at 65, 101 and 127 classes (the second register slot of the coupling kernel, and
max_iter = k past 100 classes), predict / decision_function at 130 classes, and polynomial
kernels of degree 1, 2, 4 and 5.  Arrays only.

Size: a model of k classes carries k (k - 1) / 2 intercepts, probA and probB -- 53,778 numbers
for the four large models -- besides its dual coefficients, which no choice of samples shrinks.
To stay below the largest committed fixture (volume3d.npz, 516,513 bytes) the large models use 2
samples per class, 3 features and wide kernels (few support vectors per pair, so dual_coef_ is
mostly zeros), their parameters are rounded to float32 inside the estimator BEFORE sklearn
computes the recorded outputs (round32), and every second pair of one decision_function row is
kept at 130 classes; every row's decision values are compared with sklearn live in tests/test_backend_ref.py.

Usage: python tests/golden/make_backend_edges_golden.py   (needs scikit-learn; ~5 s)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from backend_cases import sk_model  # noqa: E402

PROBA = [("proba65", 65, dict(kernel="rbf", gamma=0.05, C=10.0)), ("proba101", 101, dict(kernel="linear", C=1.0)),
         ("proba127", 127, dict(kernel="rbf", gamma=0.005, C=100.0))]
POLY = [("poly1", 1), ("poly2", 2), ("poly4", 4), ("poly5", 5)]
DEC_ROWS = 1      # decision_function rows kept at 130 classes (8385 pairs each) ...
DEC_STEP = 2      # ... and of those every second pair (pairs 0, 2, 4 ...)


def blobs(rng, ncls, per_class, f=3, spread=4.0, noise=0.5):
    centres = rng.normal(0, spread, (ncls, f))
    y = np.repeat(np.arange(ncls), per_class)
    return centres, centres[y] + rng.normal(0, noise, (len(y), f)), y


def round32(clf):
    """round the fitted coefficients, intercepts and Platt parameters to float32 values IN the
    estimator, so that sklearn's outputs below are those of the rounded model: still a valid
    libsvm model next to the fit, and the arrays take half the room (stored as float32, exact)"""
    for name in ("_dual_coef_", "dual_coef_", "_intercept_", "intercept_", "_probA", "_probB"):
        a = getattr(clf, name)
        setattr(clf, name, np.ascontiguousarray(a.astype(np.float32).astype(np.float64)))
    return clf


def model32(clf):
    m = sk_model(clf)
    for k in ("dual_coef", "intercept", "probA", "probB"):
        if k in m:
            assert np.array_equal(m[k], m[k].astype(np.float32)), k
            m[k] = m[k].astype(np.float32)
    return m


def queries(rng, centres, n_near, n_far):
    """cells near the classes, and cells 50x further out than any class (the Platt clamps)"""
    near = centres[rng.integers(0, len(centres), n_near)] + rng.normal(0, 0.8, (n_near, centres.shape[1]))
    far = 50.0 * centres[rng.integers(0, len(centres), n_far)]
    return np.vstack([near, far])


def main():
    from sklearn.svm import SVC
    rng = np.random.default_rng(20)
    out = {}

    def put(name, m, **extra):
        for k, v in {**m, **extra}.items():
            out[name + "_" + k] = v

    for name, ncls, kw in PROBA:
        centres, x, y = blobs(rng, ncls, 2)
        clf = round32(SVC(probability=True, random_state=0, **kw).fit(x, y))
        xt = queries(rng, centres, 6, 4)
        put(name, model32(clf), x=xt, proba=clf.predict_proba(xt), pred=clf.predict(xt).astype(np.float64))
    centres, x, y = blobs(rng, 130, 2)
    clf = round32(SVC(decision_function_shape="ovo", kernel="rbf", gamma=0.01, C=50.0).fit(x, y))
    xt = queries(rng, centres, 40, 8)
    put("pred130", model32(clf), x=xt, pred=clf.predict(xt).astype(np.float64),
        dec=clf.decision_function(xt[:DEC_ROWS])[:, ::DEC_STEP])
    for name, degree in POLY:
        centres, x, y = blobs(rng, 4, 30, f=5, spread=1.5, noise=1.0)
        clf = SVC(decision_function_shape="ovo", kernel="poly", degree=degree, gamma=0.3, coef0=0.7, C=2.0).fit(x, y)
        xt = queries(rng, centres, 40, 0)
        put(name, sk_model(clf), x=xt, pred=clf.predict(xt).astype(np.float64), dec=clf.decision_function(xt))
    path = os.path.join(HERE, "backend_edges.npz")
    np.savez_compressed(path, **out)
    print("backend_edges.npz written: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
