"""The list pass's MFMA candidate sweep (E. coli layout, the 16x16x32 library image).

A listed pixel's candidate rows come from one sweep of the library image against a threshold
proven from the screen's error bound; the candidates are rescored in f64.  Every case here forces
its listed pixels by construction -- a pixel equal to a library row that exists twice has an exact
tie no certificate settles, every other pixel is a clean copy of a unique row -- asserts the listed
count it expects (so it cannot pass without the sweep), and checks argmin and distance on every
pixel against the restatement (oracle.classify_top2 through check_pixel_argmin) on both entry
points: the plain stack in mode 2, and the pixel table refined from the five lasers.

Statistics (classify_refine(..., want_listed="stats")): listed pixels, sparse candidates, pixels
scored on every row in f64.  A sparse-path answer is a member of the emitted candidate set, so
"no pixel scored in full and every answer the oracle's" is the premise itself: the oracle's argmin
was among the emitted candidates of every listed pixel.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ECOLI = (0, 32, 55, 75, 89, 95)
C = 95
NSEG = 5


@pytest.fixture(scope="module")
def K():
    from hiprfish_image_analysis_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def base_library():
    """R = 1023 E. coli barcodes, f32 (read-only: every case copies it)"""
    from hiprfish_image_analysis_amd import synthetic
    ref = synthetic.reference_library(10, ECOLI).astype(np.float32)
    ref.setflags(write=False)
    return ref


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def library_of(base, R, seed=0):
    """the first R base rows, past 1023 rows random positive spectra"""
    ref = base[:min(R, base.shape[0])].copy()
    if R > base.shape[0]:
        extra = np.random.default_rng(seed).uniform(0.05, 1.0, (R - base.shape[0], C)).astype(np.float32)
        ref = np.concatenate([ref, extra])
    return ref


def run_both(K, orc, x, ref, listed, full=None):
    """x (P, C) f32 against ref on both entry points; asserts the listed count (and the pixels scored
    in full) and the restatement's answer on every pixel -> (listed, candidates, full) of the stack run"""
    from test_kernels_gpu import check_pixel_argmin
    P, R = x.shape[0], ref.shape[0]
    x64, ref64 = x.astype(np.float64), ref.astype(np.float64)
    refx = K.classify_prepare(dev(ref), ECOLI, mode=2)
    st = dev(x.reshape(1, P, C))
    # stack, mode 2: hrf_classify_pixels, and its screen + refine with the statistics
    gi, gd = K.classify_pixels(st, refx, R, ECOLI, mode=2)
    check_pixel_argmin(orc, host(gi).ravel(), host(gd).ravel(), x64, ref64, ECOLI)
    si, sd, sec = K.classify_pixels_screen(st, refx, R, ECOLI, mode=2)
    stats = K.classify_refine(K.StackSource(st), refx, R, ECOLI, 2, si, sd, sec, want_listed="stats")
    assert torch.equal(si, gi) and torch.equal(sd.view(torch.int32), gd.view(torch.int32))
    # pixel table + lasers: hrf_classify_pixels_table_exact reading the five acquisitions
    pt = K.pixtable_prepare(st, ECOLI)
    lasers = [st[:, :, ECOLI[k]:ECOLI[k + 1]].contiguous() for k in range(NSEG)]
    pt.source = K.LaserSource(lasers, torch.zeros((NSEG, 2), dtype=torch.int32, device="cuda"), True)
    ti, td, tlisted = K.classify_pixels_table(pt, refx, R, want_listed=True)
    check_pixel_argmin(orc, host(ti).ravel(), host(td).ravel(), x64, ref64, ECOLI)
    ci, cd, csec = K.classify_pixels_table_screen(pt, refx, R)
    tstats = K.classify_refine(pt.source, refx, R, ECOLI, 3, ci, cd, csec, want_listed="stats")
    assert torch.equal(ci, ti) and torch.equal(cd.view(torch.int32), td.view(torch.int32))
    print("stack (listed, candidates, full) = %s, table = %s" % (stats, tstats))
    assert int(host(gi).max()) < R and int(host(ti).max()) < R
    assert stats[0] == listed and tlisted == listed and tstats[0] == listed
    if full is not None:
        assert stats[2] == full and tstats[2] == full
    return stats


def clean_rows(orc, ref, avoid, n, rng):
    """n rows of ref outside `avoid` whose own pixel no other row comes near (restated runner-up more
    than 1e-3 away, 40 times the certificate's margin): pixels made from them are certified"""
    rows = np.array([r for r in range(ref.shape[0]) if r not in avoid])
    if rows.size == 0:
        return rows
    if ref.shape[0] == 1:
        return rows[:1]
    _, d1, d2 = orc.classify_top2(ref[rows].astype(np.float64), ref.astype(np.float64), ECOLI)
    rows = rows[(d2 - d1) > 1e-3]
    return rows[rng.integers(0, rows.size, n)]


def tie_mix(orc, ref, tie_row, P, tie_at, rng, avoid=()):
    """P pixels: power-of-two multiples of ref[tie_row] at the positions tie_at, clean copies of
    unique rows elsewhere.  Checks on the CPU that the restatement alone reports the ties."""
    tie_at = np.asarray(tie_at, dtype=np.int64)
    rows = clean_rows(orc, ref, set(avoid) | {tie_row}, P, rng)
    x = np.zeros((P, C), dtype=np.float32)
    if rows.size:
        x[:] = ref[rows] * np.float32(0.5)
    scale = np.float32(2.0) ** rng.integers(-3, 2, tie_at.size)
    x[tie_at] = ref[tie_row][None, :] * scale[:, None].astype(np.float32)
    ra, d1, d2 = orc.classify_top2(x.astype(np.float64), ref.astype(np.float64), ECOLI)
    tied = d1 == d2
    assert tied[tie_at].all() and int(tied.sum()) == tie_at.size, "the ties are not exactly the constructed ones"
    return x


def copy_positions(R):
    """>= 40 positions over every 32-row chunk of the image, every 16-row block position (hence all
    four lane quarters) and the last chunk; position 3 is the lowest (the source row)"""
    pos = {32 * c + (5 * c + 3) % 32 for c in range((R + 31) // 32)}
    pos |= {32 * c + (5 * c + 19) % 32 for c in range(10)}
    pos |= {R - 1, R - 2}
    pos = sorted(p for p in pos if p < R)
    assert pos[0] == 3 and len(pos) >= 40 and {p % 16 for p in pos} == set(range(16))
    assert {p // 32 for p in pos} == set(range((R + 31) // 32))
    return pos


@pytest.mark.parametrize("R", [1023, 1040])
def test_many_ties(K, orc, base_library, R):
    """one row at >= 40 positions: every pixel drawn from it answers the lowest copy, through the
    sparse path (20 such pixels in one batch keep the candidate list below its capacity)"""
    ref = library_of(base_library, R)
    pos = copy_positions(R)
    ref[pos] = ref[3]
    rng = np.random.default_rng(R)
    P = 2048
    tie_at = rng.choice(P, 20, replace=False)
    x = tie_mix(orc, ref, 3, P, tie_at, rng, avoid=pos)
    stats = run_both(K, orc, x, ref, listed=20, full=0)
    assert stats[1] == 20 * len(pos)   # b1 and every other copy, each once


def test_candidate_list_overflow(K, orc, base_library):
    """whole batches of such pixels exceed the LDS candidate list: those pixels are scored on every
    row instead, and the answers stay the restatement's"""
    ref = library_of(base_library, 1023)
    pos = copy_positions(1023)
    ref[pos] = ref[3]
    rng = np.random.default_rng(7)
    P = 2048
    tie_at = rng.choice(P, 640, replace=False)
    x = tie_mix(orc, ref, 3, P, tie_at, rng, avoid=pos)
    stats = run_both(K, orc, x, ref, listed=640)
    assert stats[2] > 0


@pytest.mark.parametrize("R", [1, 17, 1000])
def test_padding_rows_never_answer(K, orc, base_library, R):
    """negative pixels (every cosine against a real row negative, so an image padding row's zero
    would beat them all) whose best rows are duplicates: no answer >= R, the index the oracle's"""
    # rows without an all-zero segment only (a one-zero segment's cosine term is 0, not negative)
    whole = np.all([np.abs(base_library[:, ECOLI[s]:ECOLI[s + 1]]).sum(1) > 0 for s in range(NSEG)], 0)
    ref = library_of(base_library[whole], R)
    assert ref.shape[0] == R and ref.min() >= 0
    rng = np.random.default_rng(R)
    P = 256
    if R == 1:
        x = -ref[np.zeros(P, dtype=np.int64)] * rng.uniform(0.5, 1.0, (P, 1)).astype(np.float32)
        run_both(K, orc, x.astype(np.float32), ref, listed=0, full=0)
        return
    # the best row of the pixel -ref[c], duplicated at a row no pixel of the case is made from
    src = list(range(4))
    ra, _, _ = orc.classify_top2(-ref[src].astype(np.float64), ref.astype(np.float64), ECOLI)
    dst = [r for r in range(R - 1, -1, -1) if r not in set(src) | set(int(a) for a in ra)][:len(src)]
    for a, b in zip(ra, dst):
        ref[b] = ref[a]
    avoid = set(dst) | set(int(a) for a in ra)
    rows = clean_rows(orc, ref, avoid, P, rng)
    x = (ref[rows] * np.float32(0.5)).astype(np.float32)
    neg_at = rng.choice(P, 100, replace=False)
    x[neg_at] = -ref[np.array(src)[np.arange(100) % len(src)]] * np.float32(0.5)
    _, d1, d2 = orc.classify_top2(x.astype(np.float64), ref.astype(np.float64), ECOLI)
    assert (d1[neg_at] == d2[neg_at]).all() and int((d1 == d2).sum()) == 100
    assert (d1[neg_at] > 1.0).all()   # every cosine negative
    run_both(K, orc, x, ref, listed=100, full=0)


def test_zero_segments(K, orc, base_library):
    """listed pixels with one to four all-zero segments (the indicator step, eps_zero per segment).
    For k = 1..4 the library holds a row with its first k segments zeroed, an exact copy of it (the
    tie that forces the listing), a copy perturbed by ~3e-7 in the other segments only (a near tie),
    and a copy that differs only inside the pixel's zero segments (they are filled)"""
    ref = library_of(base_library, 1023)
    rng = np.random.default_rng(11)
    nonzero = np.all([np.abs(ref[:, ECOLI[s]:ECOLI[s + 1]]).sum(1) > 0 for s in range(NSEG)], 0)
    a = int(np.nonzero(nonzero)[0][40])
    fam = set()
    for k in range(1, 5):
        row = ref[a].copy()
        row[0:ECOLI[k]] = 0.0
        near = row.copy()
        near[ECOLI[k]:] *= (1 + rng.normal(0, 3e-7, C - ECOLI[k])).astype(np.float32)
        ref[100 + k], ref[600 + k], ref[300 + k], ref[400 + k] = row, row, near, ref[a]
        ref[400 + k, ECOLI[k - 1]:ECOLI[k]] = 0.0 if k > 1 else ref[a, 0:32]
        fam |= {100 + k, 600 + k, 300 + k, 400 + k}
    P = 512
    rows = clean_rows(orc, ref, fam | {a}, P, rng)
    x = (ref[rows] * np.float32(0.5)).astype(np.float32)
    z_at = rng.choice(P, 80, replace=False)
    for i, p in enumerate(z_at):
        x[p] = ref[100 + 1 + i % 4] * np.float32(2.0 ** (i % 3 - 1))
    ra, d1, d2 = orc.classify_top2(x.astype(np.float64), ref.astype(np.float64), ECOLI)
    assert (d1[z_at] == d2[z_at]).all() and int((d1 == d2).sum()) == 80
    assert (ra[z_at] <= 101 + np.arange(80) % 4).all()   # (a base row may equal a zeroed row: then it is the lowest)
    run_both(K, orc, x, ref, listed=80, full=0)


@pytest.mark.parametrize("P,listed", [(1, 0), (1, 1), (16, 0), (16, 15), (4099, 17), (4099, 37)])
def test_ragged_lists(K, orc, base_library, P, listed):
    """listed counts that are empty, end inside a 16-pixel MFMA group, or leave a batch ragged"""
    ref = library_of(base_library, 1023)
    ref[800] = ref[5]
    rng = np.random.default_rng(P + listed)
    tie_at = rng.choice(P, listed, replace=False)
    x = tie_mix(orc, ref, 5, P, tie_at, rng, avoid={800})
    stats = run_both(K, orc, x, ref, listed=listed, full=0)
    assert stats[1] == 2 * listed


def test_bypass_classes(K, orc, base_library):
    """NaN, inf and 1e20-scaled pixels (outside the bound's premises: scored on every row) in the
    same batches as ordinary and 1e-25-scaled ties, which stay on the sparse path"""
    ref = library_of(base_library, 1023)
    ref[800] = ref[5]
    rng = np.random.default_rng(3)
    P = 512
    tie_at = rng.choice(P, 90, replace=False)
    x = tie_mix(orc, ref, 5, P, tie_at[:60], rng, avoid={800})
    x[tie_at[60:70]] = ref[5] * np.float32(1e-25)      # f32-underflowing sums of squares: the f64 redo
    x[tie_at[70:76]] = ref[5] * np.float32(1e20)       # f32-overflowing sums of squares
    x[tie_at[76:80]] = ref[5] * np.float32(1e20)
    x[tie_at[80:84], 40] = np.nan
    x[tie_at[84:87], 7] = np.inf
    x[tie_at[87:90], 90] = -np.inf
    run_both(K, orc, x, ref, listed=90, full=20)


@pytest.mark.parametrize("lib", ["near", "dup"])
def test_argmin_among_candidates(K, orc, lib):
    """the premise on the near-duplicate libraries of test_classify_exact_gpu.py: no pixel leaves
    the sparse path and every answer is the oracle's, so the oracle's argmin was in the emitted
    candidate set of every listed pixel"""
    from hiprfish_image_analysis_amd import synthetic as S
    from test_classify_exact_gpu import _library, _pixels
    from test_kernels_gpu import check_pixel_argmin
    ref, pairs = _library(S, 10, ECOLI, near=lib == "near", dup=lib == "dup")
    x = _pixels(ref, pairs, 4096, np.random.default_rng(23))
    R = ref.shape[0]
    refx = K.classify_prepare(dev(ref), ECOLI, mode=2)
    st = dev(x.reshape(1, -1, C))
    for screen in (2, 3):
        if screen == 2:
            idx, dist, sec = K.classify_pixels_screen(st, refx, R, ECOLI, mode=2)
        else:
            idx, dist, sec = K.classify_pixels_table_screen(K.pixtable_prepare(st, ECOLI), refx, R)
        stats = K.classify_refine(K.StackSource(st), refx, R, ECOLI, screen, idx, dist, sec, want_listed="stats")
        print("screen %d: listed %d, candidates %d, full %d" % ((screen,) + stats))
        assert stats[0] > 4096 // 4 and stats[2] == 0
        assert stats[1] >= stats[0]
        check_pixel_argmin(orc, host(idx).ravel(), host(dist).ravel(), x.astype(np.float64),
                           ref.astype(np.float64), ECOLI)
