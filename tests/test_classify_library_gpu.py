"""The per-pixel classifier's LIBRARY side (classify.hip: the MFMA screens' prepared tables, the
f64 certificate, the list pass) and the cell classifier at library sizes and values the other
modules never reach.  tests/test_classify_exact_gpu.py and tests/test_kernels_gpu.py vary the
pixels; every library there is synthetic.reference_library(nbit): R = 31, 127, 1023 or 4095 rows
(one padding row in a 64-row chunk, or none of the sizes below) of ordinary values in [0, 1].

Here:
  * A. row counts with 0, 1, 8, 62 and 63 padding rows, one and many 64-row chunks, R = 1 (no
       runner-up) and R = 4096 (the list pass's limit), with duplicate and near-duplicate rows
       planted at the first / last rows and across a chunk boundary, on every surface;
  * B. library rows that are huge, tiny, subnormal, all zero, partly zero, mixed in scale,
       negated, or hold NaN / inf -- the restatement's answer (oracle_classify_top2's `d < best`
       loop: a row whose distance is NaN never wins; against an all-zero pixel segment a
       non-finite row segment scores 1.0 like any other non-zero one);
  * C. the f64 cell classifier at ragged row and cell counts on a library that f32 cannot hold;
  * D. one native tile on such a library: the per-cell answers against the f64 library, the
       per-pixel answers against the library ROUNDED TO F32 (the per-pixel contract), and the
       tile context's listed-pixel count.

The builders below need numpy only: tests/test_classify_library_inputs.py runs them through the
restatement on the CPU and asserts the conditions that keep these tests from passing vacuously.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ECOLI = (0, 32, 55, 75, 89, 95)
MULTI = (0, 23, 43, 57, 63)

ROW_COUNTS = [(ECOLI, R) for R in (1, 2, 3, 16, 63, 64, 65, 120, 128, 129, 1000, 1024, 1025, 4096)] + \
             [(MULTI, R) for R in (1, 65, 120)]
ROW_IDS = ["%s-R%d" % ("ecoli" if b is ECOLI else "multi", R) for b, R in ROW_COUNTS]
SWEEP_P = 1024            # one 32 x 32 stack
VALUE_KINDS = ("huge", "tiny", "nonfinite")


@functools.lru_cache(maxsize=None)
def _base_library(nbit, bounds):
    from hiprfish_image_analysis_amd import synthetic
    lib = synthetic.reference_library(nbit, bounds).astype(np.float32)
    lib.setflags(write=False)
    return lib


def _perturbed(row, rng):
    """a copy ~3e-7 relative away in every channel: far below any MFMA screen's resolution"""
    return (row * (1 + rng.normal(0, 3e-7, row.shape[0]))).astype(np.float32)


# ---- A: row counts ------------------------------------------------------------------------------
def sweep_library(bounds, R):
    """-> (ref (R, C) f32, pairs): a fixed-seed selection of R rows of the 12-bit E. coli library
    (R = 4096: all 4095 and a blend of two of them), or the 7-bit multispecies library's first R;
    planted in it, where the rows exist: an exact duplicate pair and near-duplicate pairs at
    (0, R - 1), (R - 2, R - 1) and across the first chunk boundary (63, 64).  Pairs that share a row
    chain into near-duplicate triples (R = 3, 65, 66).  pairs: [(a, b, "dup" | "near")], a < b."""
    rng = np.random.default_rng(7000 + R)
    if tuple(bounds) == ECOLI:
        base = _base_library(12, ECOLI)
        ref = base[rng.permutation(base.shape[0])[:min(R, base.shape[0])]].copy()
        if R > ref.shape[0]:
            assert R == ref.shape[0] + 1
            ref = np.concatenate([ref, (0.5 * (ref[100].astype(np.float64) + ref[2000]))[None].astype(np.float32)])
    else:
        ref = _base_library(7, MULTI)[:R].copy()
    assert ref.shape[0] == R
    pairs = []
    planted = set()
    if R >= 8:
        a, b = 2, R // 3 + 5                     # never one of 0, 63, 64, R - 2, R - 1
        ref[b] = ref[a]
        pairs.append((a, b, "dup"))
    elif R == 3:
        ref[1] = ref[0]
        pairs.append((0, 1, "dup"))
        planted.add(1)
    for a, b in ((0, R - 1), (R - 2, R - 1), (63, 64)):
        if not (0 <= a < b < R) or (a, b, "near") in pairs or (a in planted and b in planted):
            continue
        if b in planted:
            ref[a] = _perturbed(ref[b], rng)
        else:
            ref[b] = _perturbed(ref[a], rng)
        planted.update((a, b))
        pairs.append((a, b, "near"))
    return ref, pairs


def _noisy_rows(ref, n, rng, noise=0.02):
    x = ref[rng.integers(0, ref.shape[0], n)] * rng.uniform(0.5, 1, (n, 1)) + rng.normal(0, noise, (n, ref.shape[1]))
    return np.clip(x, 0, None)


def _blends(ref, pairs, n, rng):
    out = np.empty((n, ref.shape[1]))
    for i in range(n):
        a, b = pairs[i % len(pairs)][:2]
        x = 0.5 * (ref[a].astype(np.float64) + ref[b]) * rng.uniform(0.5, 1.0)
        out[i] = x * (1 + rng.normal(0, 1e-3, ref.shape[1]))
    return out


def sweep_pixels(ref, pairs, bounds, P=SWEEP_P):
    """(P, C) f32: half of them blends of the planted pairs (both rows about equally close), 64
    negated library rows (every real row scores below 0: the padding rows' -1024 bias must still
    lose), 16 all-zero pixels (answered from the library alone, ExactHdr.idx0), 16 with one zero
    segment, and noisy multiples of random rows"""
    R, C = ref.shape
    rng = np.random.default_rng(9000 + R)
    nblend = P // 2 if pairs else 0
    parts = []
    if nblend:
        parts.append(_blends(ref, pairs, nblend, rng))
    neg = -ref[rng.integers(0, R, 64)].astype(np.float64) * rng.uniform(0.5, 1, (64, 1))
    parts.append(neg * (1 + rng.normal(0, 0.02, (64, C))))
    parts.append(np.zeros((16, C)))
    zs = _noisy_rows(ref, 16, rng)
    for i in range(16):
        s = i % (len(bounds) - 1)
        zs[i, bounds[s]:bounds[s + 1]] = 0.0
    parts.append(zs)
    parts.append(_noisy_rows(ref, P - nblend - 96, rng))
    x = np.concatenate(parts).astype(np.float32)
    assert x.shape == (P, C)
    return x


# ---- B: extreme library rows ----------------------------------------------------------------------
VALUES_R = 120
F32_MAX = float(np.finfo(np.float32).max)


def values_library(kind):
    """-> (ref (120, 95) f32, shapes, special): R = 120 rows of the 12-bit E. coli library with a
    near-duplicate pairs (20, 90) and (40, 41) and the special rows of `kind` written over ordinary ones.
    shapes: the (R, C) f64 ordinary-scale spectra whose multiples are CLOSEST to each row (the
    segmented cosine does not see a segment's scale; zero where the row is zero, negated where it
    is); special: {name: row}.  "huge": a row x 1e25 (with a near-duplicate at scale 1), a row whose
    first segment reaches the f32 maximum, an all-zero row and a row zero in two segments; "tiny": a
    row x 1e-20, a row of f32 subnormals, a row with segments x 1e20 and x 1e-20, and the negation
    of another row (with it the mode-2 sweeps take their compare-and-select argmax); "nonfinite":
    rows holding one NaN, one +inf, only inf.  The tiny rows are kept out of "huge": one segment sum
    of squares below 1e-30 already sends every listed pixel of the library to full scoring
    (ExactHdr.tiny), which would hide what the huge rows do to the list pass's f32 scores."""
    assert kind in VALUE_KINDS
    rng = np.random.default_rng(31)
    base = _base_library(12, ECOLI)
    full = np.all([base[:, ECOLI[s]:ECOLI[s + 1]].max(1) > 0.05 for s in range(5)], axis=0)
    ref = base[rng.permutation(np.nonzero(full)[0])[:VALUES_R]].copy()     # every segment present
    ref[90] = _perturbed(ref[20], rng)
    ref[41] = _perturbed(ref[40], rng)         # two of the four rows one lane of a 16-row MFMA block holds
    shapes = ref.astype(np.float64)
    r64 = ref.astype(np.float64)
    special = {}
    if kind == "huge":
        special = dict(e25=5, e25_twin=6, fmax=11, zero=31, zero2=37)
        ref[5] = (r64[5] * 1e25).astype(np.float32)
        ref[6] = _perturbed(r64[5].astype(np.float32), rng)    # the 1e25 row's near-duplicate at scale 1: its
        shapes[6] = shapes[5]                                  # pixels are near ties, so the list pass scores them
        ref[11, 0:32] = (r64[11, 0:32] / r64[11, 0:32].max() * (F32_MAX * (1 - 1e-6))).astype(np.float32)
        ref[31] = 0.0
        shapes[31] = 0.0
        ref[37, 32:55] = 0.0
        ref[37, 75:89] = 0.0
        shapes[37] = ref[37]
        assert np.isfinite(ref).all()
    elif kind == "tiny":
        special = dict(e_20=17, subnormal=23, mixed=44, negated=52)
        ref[17] = (r64[17] * 1e-20).astype(np.float32)         # ny ~ 1e-40
        ref[23] = (r64[23] * 1e-40).astype(np.float32)         # f32 subnormals
        assert 0 < np.abs(ref[23]).max() < np.finfo(np.float32).tiny
        shapes[23] = ref[23].astype(np.float64) * 1e40         # (what survived the subnormal rounding)
        ref[44, 0:32] = (r64[44, 0:32] * 1e20).astype(np.float32)
        ref[44, 32:55] = (r64[44, 32:55] * 1e-20).astype(np.float32)
        ref[52] = -ref[60]
        shapes[52] = -shapes[60]
        assert np.isfinite(ref).all()
    else:
        special = dict(one_nan=9, one_inf=14, all_inf=27)
        ref[9, 40] = np.nan
        ref[14, 3] = np.inf
        ref[27] = np.inf
    return ref, shapes, special


def values_pixels(ref, shapes, special, kind):
    """(1408, 95) f32 pixels for values_library(kind): noisy multiples (multiplicative noise: zero
    segments stay zero, signs stay) of every special row's shape at scale 1; for "huge" also of the
    1e25 row at scale 1e12 and at scale 1e14 -- there the pixel's segment sums of squares stay
    under 1e30 while every product with the 1e25 row is past the f32 maximum --; blends of the
    near-duplicate pairs; ordinary pixels, all-zero pixels and pixels with one zero segment (for
    "nonfinite": some zero exactly where a row holds its NaN / inf, so that row's distance is
    finite there and it must still lose)"""
    R, C = ref.shape
    rng = np.random.default_rng(77 + VALUE_KINDS.index(kind))

    def multiples(row, n, scale):
        return shapes[row] * scale * rng.uniform(0.5, 1, (n, 1)) * (1 + rng.normal(0, 0.02, (n, C)))

    parts = []
    for name, row in special.items():
        if name not in ("zero", "e25_twin"):
            parts.append(multiples(row, 64, 1.0))
    if kind == "huge":
        parts.append(multiples(special["e25"], 128, 1e12))
        parts.append(multiples(special["e25"], 256, 1e14))
    parts.append(_blends(ref, [(20, 90), (40, 41)], 64, rng))
    parts.append(np.zeros((16, C)))
    plain = np.setdiff1d(np.arange(R), list(special.values()))
    zs = shapes[rng.choice(plain, 32)] * rng.uniform(0.5, 1, (32, 1)) + rng.normal(0, 0.02, (32, C))
    zs = np.clip(zs, 0, None)
    for i in range(32):
        s = i % 5
        zs[i, ECOLI[s]:ECOLI[s + 1]] = 0.0
    parts.append(zs)
    n = 1408 - sum(p.shape[0] for p in parts)
    x = shapes[rng.choice(plain, n)] * rng.uniform(0.5, 1, (n, 1)) + rng.normal(0, 0.02, (n, C))
    parts.append(np.clip(x, 0, None))
    x = np.concatenate(parts).astype(np.float32)
    assert x.shape == (1408, C) and np.isfinite(x).all()
    return x


# ---- C: cells ---------------------------------------------------------------------------------------
CELL_ROW_COUNTS = (1, 2, 120, 1025)
CELLS_N = 37


def cells_library(R):
    """(R, 95) f64 rows that f32 cannot hold -- row k = f32 row * (1 + 1e-12 k) -- with rows that
    differ only below f32 resolution: (0, R - 1) and, where they exist, (63, 64)"""
    rng = np.random.default_rng(500 + R)
    base = _base_library(12, ECOLI)
    ref = base[rng.permutation(base.shape[0])[:R]].astype(np.float64)
    ref *= 1 + 1e-12 * np.arange(1, R + 1)[:, None]
    pairs = [(a, b) for a, b in ((0, R - 1), (63, 64)) if 0 <= a < b < R]
    for a, b in pairs:
        ref[b] = ref[a] * (1 + 1e-10 * rng.uniform(-1, 1, ref.shape[1]))
        assert np.array_equal(ref[a].astype(np.float32), ref[b].astype(np.float32)) and not np.array_equal(ref[a], ref[b])
    assert not np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    return ref, pairs


def cells_spectra(ref, pairs, N=CELLS_N):
    """N max-normalised cell spectra: noisy multiples of random rows, every third one of a paired row"""
    rng = np.random.default_rng(600 + ref.shape[0])
    rows = rng.integers(0, ref.shape[0], N)
    if pairs:
        rows[::3] = [pairs[i % len(pairs)][i % 2] for i in range(len(rows[::3]))]
    x = ref[rows] * rng.uniform(0.5, 1, (N, 1)) + rng.normal(0, 0.01, (N, ref.shape[1]))
    x = np.clip(x, 0, None)
    return x / x.max(axis=1, keepdims=True)


def presence_flags(x, bounds, thr=0.1):
    return np.stack([x[:, bounds[k]:bounds[k + 1]].max(axis=1) > thr for k in range(len(bounds) - 1)], 1).astype(np.float64)


# ---- D: an f64 library ----------------------------------------------------------------------------
def tile_library(R=120):
    """(R, 95) f64 library of a real probe design's shape: f64 means (the reference writes them as
    %.18e text), each within about half an f32 ulp of an f32 value but not one itself"""
    rng = np.random.default_rng(120)
    base = _base_library(12, ECOLI)
    ref32 = base[rng.permutation(base.shape[0])[:R]]
    ref = ref32.astype(np.float64) * (1 + 2e-8 * rng.uniform(-1, 1, ref32.shape))
    assert not np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    return ref


# ---- the GPU tests --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def K(torch):
    from hiprfish_image_analysis_amd import kernels
    return kernels


def host(t):
    return t.detach().cpu().numpy()


def all_surfaces(torch, K, ref, x, bounds, shape):
    """every per-pixel surface on one library and one stack: classify_pixels on the three screens,
    the pixel-table classifier plain, fused and composed -> ({name: (idx, dist)}, pixels the
    table's certificate listed)"""
    R, C = ref.shape
    refd = torch.from_numpy(np.ascontiguousarray(ref)).cuda()
    st = torch.from_numpy(np.ascontiguousarray(x.reshape(tuple(shape) + (C,)))).cuda()
    out = {}
    refx = None

    def real_row(name, idx):
        # a screen's own argmax is a library row: the refine would list a padding row's win and
        # still answer exactly, so a padding row that wins shows here only
        lo, hi = int(idx.min()), int(idx.max())
        assert 0 <= lo and hi < R, "%s screen: argmax rows %d..%d with R = %d" % (name, lo, hi, R)

    for mode in (0, 1, 2):
        refx = K.classify_prepare(refd, bounds, mode=mode)
        out["mode %d" % mode] = K.classify_pixels(st, refx, R, bounds, mode=mode)
        real_row("mode %d" % mode, K.classify_pixels_screen(st, refx, R, bounds, mode=mode)[0])
    pt = K.pixtable_prepare(st, bounds)
    real_row("table", K.classify_pixels_table_screen(pt, refx, R)[0])
    gi, gd, listed = K.classify_pixels_table(pt, refx, R, want_listed=True)
    out["table"] = (gi, gd)
    out["table fused"] = K.classify_pixels_table(pt, refx, R, fused=True)
    out["table composed"] = K.classify_pixels_table(pt, refx, R, composed=True)
    return out, listed


def check_surfaces(torch, orc, out, x, ref, bounds):
    """every surface equals the restatement on every pixel (argmin, and the distance bit for bit),
    so they equal one another; the restatement is checked first, surface by surface, so a failure
    names the surface"""
    from test_kernels_gpu import check_pixel_argmin
    x64, ref64 = x.astype(np.float64), ref.astype(np.float64)
    first = None
    near = 0
    for name, (gi, gd) in out.items():
        print("surface %s:" % name)
        near, _ = check_pixel_argmin(orc, host(gi).ravel(), host(gd).ravel(), x64, ref64, bounds)
        if first is None:
            first = (gi, gd)
        assert torch.equal(gi, first[0]) and torch.equal(gd, first[1]), "surface %s differs from mode 0" % name
    return near


@pytest.mark.parametrize("bounds,R", ROW_COUNTS, ids=ROW_IDS)
def test_library_row_counts_exact(torch, K, orc, bounds, R):
    """Rpad - R = 63, 62, 61, 48, 1, 0, 63, 8, 0, 63, 24, 0, 63, 0 padding rows (the -1024 validity
    bias of the f16 tables, the r < R guards of the f32 sweep and the list pass, exact_layout's RT
    pitch, one to 64 chunks): every surface gives the restatement's argmin -- the lower row of an
    exact duplicate pair -- and its distance bit for bit; the list pass ran (R >= 2); R = 1 answers
    row 0 everywhere; R = LIST_RMAX = 4096 runs and one row more is refused"""
    ref, pairs = sweep_library(bounds, R)
    x = sweep_pixels(ref, pairs, bounds)
    out, listed = all_surfaces(torch, K, ref, x, bounds, (32, 32))
    near = check_surfaces(torch, orc, out, x, ref, bounds)
    if R >= 2:
        assert listed > 0, "no pixel reached the list pass at R = %d" % R
        assert near >= SWEEP_P // 4
    else:
        assert int(out["table"][0].abs().max()) == 0          # (the restated distance: check_surfaces)
    if R == 4096:
        big = torch.from_numpy(np.concatenate([ref, ref[:1]])).cuda()
        for mode in (0, 1, 2):
            with pytest.raises(ValueError, match="R <= 4096"):
                K.classify_prepare(big, bounds, mode=mode)


@pytest.mark.parametrize("kind", VALUE_KINDS)
def test_library_values_exact(torch, K, orc, kind):
    """library rows x 1e25, up to the f32 maximum, all zero, zero in two segments ("huge"); x 1e-20,
    subnormal, mixed 1e20 / 1e-20, negated ("tiny"); rows holding one NaN, one +inf, or only inf
    ("nonfinite"): the restatement's argmin and distance on every pixel and every surface.  The
    pixels at scale 1e14 near the 1e25 row are the case the list pass's f32 scores overflow on:
    it must fall back to scoring every row exactly (the library header's range flag, the
    non-finite threshold test), not answer row 0 at distance inf."""
    ref, shapes, special = values_library(kind)
    x = values_pixels(ref, shapes, special, kind)
    out, listed = all_surfaces(torch, K, ref, x, ECOLI, (32, 44))
    check_surfaces(torch, orc, out, x, ref, ECOLI)
    assert listed > 0


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("R", CELL_ROW_COUNTS)
def test_classify_cells_row_counts(torch, K, orc, R, variant):
    """hrf_classify_cells at R = 1, 2, 120 and 1025 (one more row than the workgroup has threads)
    and 37 cells (ragged against the 4 cells of a workgroup), on f64 rows that f32 cannot hold,
    two of them equal in f32: the restatement's argmin and f64 distance bit for bit"""
    ref, pairs = cells_library(R)
    x = cells_spectra(ref, pairs)
    fx, fr = presence_flags(x, ECOLI), presence_flags(ref, ECOLI)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    a, dist = K.classify_cells(d(x), d(ref), ECOLI, variant, d(fx) if variant else None, d(fr) if variant else None)
    ra, rd = orc.classify(x, ref, ECOLI, variant, fx if variant else None, fr if variant else None)
    assert np.array_equal(host(a), ra)
    assert np.array_equal(host(dist), rd)


def test_tile_f64_library_contract(torch, K, orc):
    """One 256 x 256 E. coli tile on a library of 120 f64 rows that are not f32 values, through
    process_tile_native and the composed process_tile.

    THE PER-PIXEL F32-LIBRARY CONTRACT (pinned here; a refine that carries f64 library rows
    tightens this one test): the per-CELL classifier reads the f64 library as given, so cell_idx /
    cell_dist equal the restatement on the f64 rows; the per-PIXEL classifier reads
    Library.spectra.to(float32) (Library.refx), so pixel_idx / pixel_dist equal the restatement on
    spectra.to(f32).to(f64), NOT on the f64 rows.  How many pixels' argmin that rounding moves is
    printed, not asserted.

    Then hrf_tile_ctx_pixel_listed: after the native tile it is the certificate's listed count of
    the same registered tile, and 0 after a native tile without the per-pixel pass."""
    from hiprfish_image_analysis_amd import pipeline as P
    from hiprfish_image_analysis_amd import synthetic as S
    from test_kernels_gpu import check_pixel_argmin
    H = W = 256
    ref = tile_library()
    R = ref.shape[0]
    ref32 = ref.astype(np.float32)
    lay = S.cell_layout(H, W, S.default_ncells(H, W), R, 20190120)
    truth, prof = S.render_truth(H, W, lay, with_profile=True)
    stack = S.render_stack(truth, lay, ref32, seed=20190120, device="cuda", profile=prof)
    lasers = S.laser_split(stack)
    lib = P.Library(torch.from_numpy(ref).cuda(), ECOLI, 7)
    dev = lasers[0].device

    nat = P.process_tile_native(lasers, lib, variant=1)
    listed_native = K.tile_pixel_listed(dev, H, W)
    rt = P.register_tile(lasers)
    comp = P.process_tile(rt, lib, per_pixel=True, variant=1)
    listed_table = K.classify_pixels_table(rt.pixtable, lib.refx_table(), R, want_listed=True)[2]
    torch.cuda.synchronize()
    assert nat.ncells > 5

    # per cell: the f64 library
    fr = presence_flags(ref, ECOLI)
    for res in (nat, comp):
        xc = host(res.meas.avgint_norm)
        ra, rd = orc.classify(xc, ref, ECOLI, 1, presence_flags(xc, ECOLI), fr)
        assert np.array_equal(host(res.cell_idx), ra)
        assert np.array_equal(host(res.cell_dist), rd)

    # per pixel: the library rounded to f32
    reg, _ = K.register_assemble(lasers, rt.shifts, True, cn_mode=1)
    x64 = host(reg).reshape(H * W, -1).astype(np.float64)
    for res in (nat, comp):
        check_pixel_argmin(orc, host(res.pixel_idx).ravel(), host(res.pixel_dist).ravel(), x64,
                           ref32.astype(np.float64), ECOLI)
    assert torch.equal(nat.pixel_idx, comp.pixel_idx) and torch.equal(nat.pixel_dist, comp.pixel_dist)
    true_idx = orc.classify_top2(x64, ref, ECOLI)[0]
    print("f32-library contract: %d of %d pixels' argmin differs from the restatement on the f64 library"
          % (int((host(nat.pixel_idx).ravel() != true_idx).sum()), H * W))

    # the tile context's listed count
    assert listed_native == listed_table
    assert listed_table > 0
    P.process_tile_native(lasers, lib, variant=1, per_pixel=False)
    assert K.tile_pixel_listed(dev, H, W) == 0
