"""tests/volreg_ref.py, the numpy restatement of the biofilm z-stack registration, against what the
reference's own lines computed (tests/golden/volreg.npz, written by
tests/golden/make_volreg_golden.py), the wrap rule at its edges, and the peak-margin condition
that lets the device tests demand equal shifts from any correct FFT."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import volreg_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def g(golden):
    return golden("volreg")


def test_golden_inputs_are_the_generated_case(g):
    ts = R.golden_case()
    for l, lst in enumerate(ts):
        for t, a in enumerate(lst):
            assert np.array_equal(g["in_l%d_t%d" % (l, t)], a)
            assert a.dtype == np.float32 and np.array_equal(a, np.floor(a))


def test_t_average_equals_reference_lines(g):
    for l, ts in enumerate(R.golden_case()):
        out, shifts = R.t_average(ts, want_shifts=True)
        assert out.dtype == np.float32
        assert np.array_equal(shifts, g["tshifts_l%d" % l])
        assert np.array_equal(out.astype(np.float64), g["avg_l%d" % l])
        assert np.abs(shifts).max() > 0


@pytest.mark.parametrize("fill", ["keep", "zero"])
def test_laser_registration_equals_reference_lines(g, fill):
    avg = [R.t_average(ts) for ts in R.golden_case()]
    out, shifts = R.register_lasers(avg, fill)
    assert np.array_equal(shifts, g["lshifts"])
    assert out.dtype == np.float32 and np.array_equal(out.astype(np.float64), g[fill])
    assert all(np.abs(s).max() > 0 for s in shifts[1:])
    assert not np.array_equal(g["keep"], g["zero"])


def test_shift_fills():
    a = np.arange(1, 1 + 4 * 3 * 2 * 1, dtype=np.float32).reshape(4, 3, 2, 1)
    z = R.shift_zero(a, (1, -1, 0))
    k = R.shift_keep(a, (1, -1, 0))
    assert np.array_equal(z[1:, :2], a[:3, 1:]) and np.array_equal(k[1:, :2], a[:3, 1:])
    assert not z[0].any() and not z[:, 2].any()
    assert np.array_equal(k[0], a[0]) and np.array_equal(k[:, 2], a[:, 2])
    for s in ((4, 0, 0), (0, -3, 0), (4, 3, -2)):                   # a shift of a whole axis: empty slices
        assert not R.shift_zero(a, s).any() and np.array_equal(R.shift_keep(a, s), a)
    assert np.array_equal(R.shift_zero(a, (0, 0, 0)), a)


@pytest.mark.parametrize("n", [4, 5, 6, 7, 16])
def test_wrap_at_half_and_past_it(n):
    rng = np.random.default_rng(n)
    v = rng.random((n, 3, 2))
    half = n // 2
    assert R.wrap(half, n) == half and R.wrap(half + 1, n) == half + 1 - n
    # the roll that puts the peak at index k is reported as wrap(k)
    for k in (half, half + 1):
        assert R.register(v, np.roll(v, -k, 0))[0] == R.wrap(k, n)


def test_roll_cases_sit_on_the_wrap_edges():
    for shape in R.ROLL_SHAPES:
        v, sh = R.roll_volumes(shape)
        assert sh[1] == tuple(n // 2 for n in shape) and sh[2] == tuple(-(n // 2 - 1) for n in shape)
        for t in (1, 2):
            assert R.register(v[0], v[t]) == sh[t]


def test_peak_margin_of_every_device_registration():
    """The device surfaces are pinned to numpy's within 1e-13 of the peak (test_volreg_gpu.py), so a
    runner-up 1e-9 of the peak below it cannot win on any correct FFT.  Smallest margin over the
    92 registrations, measured with numpy: 2.0e-5."""
    worst = 1.0
    n = 0
    for name, a, b in R.all_registrations():
        cc = np.sort(R.cc_abs(a, b), axis=None)
        margin = (cc[-1] - cc[-2]) / cc[-1]
        assert margin >= 1e-9, (name, margin)
        worst = min(worst, margin)
        n += 1
    print("registrations %d, smallest margin %.3g" % (n, worst))
    assert n >= 60


def test_planted_offsets_are_mostly_recovered():
    """the shift tests are about nonzero shifts of both signs on every axis: what the restatement
    finds on the generated crops must cover them (a crop is not a roll, a planted offset need not
    be recovered exactly)"""
    found = []
    for shape, offs in R.POW2_SHIFT_CASES + R.OTHER_SHIFT_CASES:
        v = R.volumes(shape, offs, seed=sum(shape))
        found += [R.register(v[0], v[t]) for t in range(1, len(offs))]
    f = np.array(found)
    assert (f > 0).any(0).all() and (f < 0).any(0).all() and (f == 0).any(0).all()
