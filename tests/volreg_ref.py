"""numpy restatement of the biofilm z-stack registration (hiprfish_imaging_biofilm_analysis.py
:134-165 t-average, :536-558 laser registration with the keep fill, :428-450 with zero fill), and
the seeded inputs the device tests run on.  tests/test_volreg_ref.py checks the restatement
against what the reference's own lines computed (tests/golden/volreg.npz).

Shift s on an axis of length n: dst[max(0, s) : n + min(0, s)] = src[-min(0, s) : n - max(0, s)].
"""
import numpy as np

import oracle as O

MARGIN = 6          # the scene is this much larger than a crop on every side


# ---- semantics -----------------------------------------------------------------------------------
def wrap(k, n):
    """register_translation's wrap of a peak index: k > fix(n / 2) -> k - n"""
    return k - n if k > np.fix(n / 2) else k


def _box(shape3, s):
    dst = tuple(slice(max(0, int(v)), n + min(0, int(v))) for v, n in zip(s, shape3))
    src = tuple(slice(-min(0, int(v)), n - max(0, int(v))) for v, n in zip(s, shape3))
    return dst, src


def shift_zero(a, s):
    out = np.zeros_like(a)
    dst, src = _box(a.shape[:3], s)
    out[dst] = a[src]
    return out


def shift_keep(a, s):
    """the reference assigns the shifted box of a volume onto the volume itself; numpy copies an
    overlapping source first, so everything outside the destination box keeps its value"""
    out = a.copy()
    dst, src = _box(a.shape[:3], s)
    out[dst] = a[src]
    return out


def cc_abs(a, b):
    """|ifftn(fftn(a) conj(fftn(b)))|, the surface register_translation takes its maximum of"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.abs(np.fft.ifftn(np.fft.fftn(a) * np.fft.fftn(b).conj()))


def register(a, b):
    return tuple(int(v) for v in O.register_translation(a, b))


def t_average(tstack, want_shifts=False):
    """:134-165: sums in f64 in t order, / T, stored f32"""
    a0 = np.asarray(tstack[0], np.float32)
    T = len(tstack)
    acc = a0.astype(np.float64)
    s0 = np.sum(a0.astype(np.float64), axis=3)
    shifts = [(0, 0, 0)]
    for a in tstack[1:]:
        a = np.asarray(a, np.float32)
        s = register(s0, np.sum(a.astype(np.float64), axis=3))
        shifts.append(s)
        acc = acc + shift_zero(a.astype(np.float64), s)
    out = (acc / T).astype(np.float32)
    return (out, np.array(shifts, np.int32)) if want_shifts else out


def laser_shifts(lasers):
    """:536-538: register_translation(log(S_0 + 1e-8), log(S_l + 1e-8))"""
    sums = [np.sum(np.asarray(v, np.float32).astype(np.float64), axis=3) for v in lasers]
    return np.array([(0, 0, 0)] + [register(np.log(sums[0] + 1e-8), np.log(s + 1e-8)) for s in sums[1:]], np.int32)


def register_lasers(lasers, fill="keep", shifts=None):
    """:539-558 (keep) / :428-450 (zero): shift every laser, concatenate on C"""
    if shifts is None:
        shifts = laser_shifts(lasers)
    f = shift_keep if fill == "keep" else shift_zero
    return np.concatenate([f(np.asarray(v, np.float32), s) for v, s in zip(lasers, shifts)], axis=3), shifts


# ---- inputs --------------------------------------------------------------------------------------
def blobs(shape, rng, density=1 / 40):
    """a positive scene, maximum 1: many small Gaussian spots of varied brightness on a dark floor.
    Sharp, sparse features keep the peak of the (unnormalised) cross-correlation of two crops at
    their planted offset; a smooth bright scene would put it at zero."""
    shape = tuple(shape)
    s = np.zeros(shape)
    for _ in range(max(8, int(np.prod(shape) * density))):
        c = rng.random(3) * np.array(shape)
        r = 0.7 + 0.6 * rng.random()
        amp = 0.2 + rng.random()
        lo = [max(0, int(ci) - 6) for ci in c]                     # exp(-6^2 / (2 * 1.3^2)) < 3e-5
        hi = [min(n, int(ci) + 7) for ci, n in zip(c, shape)]
        g = np.meshgrid(*[np.arange(a, b) for a, b in zip(lo, hi)], indexing="ij")
        s[tuple(slice(a, b) for a, b in zip(lo, hi))] += amp * np.exp(
            -sum((gi - ci) ** 2 for gi, ci in zip(g, c)) / (2 * r * r))
    return 0.002 + s / s.max()


def crop(scene, shape, off):
    """the crop whose content sits at offset `off`: crop(off)(p) = crop(0)(p + off), so shifting
    it by +off registers it to crop(0)"""
    sl = tuple(slice(MARGIN + int(o), MARGIN + int(o) + n) for o, n in zip(off, shape))
    return scene[sl]


def volumes(shape, offsets, seed):
    """(X, Y, Z) f64 integer-valued crops of one scene at the planted offsets (first 0)"""
    rng = np.random.default_rng(seed)
    scene = np.floor(1 + 900 * blobs([n + 2 * MARGIN for n in shape], rng))
    return np.stack([crop(scene, shape, o) for o in offsets])


def acquisitions(shape, channels, offsets, seed, noise=3):
    """per offset an (X, Y, Z, C) f32 crop of one scene seen through C channel weights, integer
    valued (at most about 200 per channel), with a few counts of independent noise per crop"""
    rng = np.random.default_rng(seed)
    scene = blobs([n + 2 * MARGIN for n in shape], rng)
    w = 0.3 + 0.7 * rng.random(channels)
    out = []
    for o in offsets:
        a = np.floor(1 + 190 * crop(scene, shape, o)[..., None] * w)
        a += rng.integers(0, noise + 1, a.shape)
        out.append(a.astype(np.float32))
    return out


POW2_SHIFT_CASES = [((16, 16, 4), [(0, 0, 0), (2, -3, 1), (-1, 0, -1), (0, 4, 0)]),
                    ((32, 16, 8), [(0, 0, 0), (-3, 2, -2), (4, 0, 1)]),
                    ((64, 32, 16), [(0, 0, 0), (3, -4, 2), (-4, 1, 0), (0, 0, -3), (1, 1, 1)])]
OTHER_SHIFT_CASES = [((12, 10, 6), [(0, 0, 0), (2, -1, 1), (-2, 3, 0)]),
                     ((20, 17, 5), [(0, 0, 0), (-3, 2, -1), (1, 0, 1)]),
                     ((33, 16, 7), [(0, 0, 0), (4, -2, 1), (0, 3, -2)])]
ROLL_SHAPES = [(16, 16, 4), (32, 16, 8), (12, 10, 6)]


def roll_volumes(shape, seed=3):
    """np.roll copies of one volume at +n/2 and at -(n/2 - 1) on every axis: the wrap's two edges"""
    rng = np.random.default_rng(seed)
    v = np.floor(1 + 900 * blobs(shape, rng))
    hi = tuple(n // 2 for n in shape)
    lo = tuple(-(n // 2 - 1) for n in shape)
    # register(v, roll(v, -s)) = s
    return np.stack([v, np.roll(v, tuple(-h for h in hi), (0, 1, 2)), np.roll(v, tuple(-l for l in lo), (0, 1, 2))]), \
        [(0, 0, 0), hi, lo]


TAVG_T = (1, 2, 3, 5)
TAVG_C = (1, 6, 23)
TAVG_SHAPES = ((16, 16, 8), (16, 12, 8))
TAVG_OFFSETS = [(0, 0, 0), (2, -1, 1), (-1, 3, 0), (0, -2, -2), (3, 0, 1)]


def taverage_case(shape, C, T):
    return acquisitions(shape, C, TAVG_OFFSETS[:T], seed=1000 + 37 * C + T + shape[1])


LASER_CHANNELS = (3, 2, 2, 1)
LASER_SHAPE = (16, 12, 8)
LASER_OFFSETS = [(0, 0, 0), (1, -2, 1), (-2, 0, 0), (0, 3, -1)]


def laser_case(shape=LASER_SHAPE, channels=LASER_CHANNELS, offsets=LASER_OFFSETS, seed=77):
    """one averaged volume per laser: the same scene at the laser's offset and its own weights"""
    rng = np.random.default_rng(seed)
    scene = blobs([n + 2 * MARGIN for n in shape], rng)
    out = []
    for c, o in zip(channels, offsets):
        w = 0.3 + 0.7 * rng.random(c)
        out.append(np.floor(1 + 190 * crop(scene, shape, o)[..., None] * w).astype(np.float32))
    return out


CHAIN_SHAPE = (32, 32, 16)
CHAIN_CHANNELS = (6, 5, 4, 2)
CHAIN_T = 3
CHAIN_LASER_OFFSETS = [(0, 0, 0), (2, -1, 1), (-1, 2, 0), (0, -2, -1)]
CHAIN_T_OFFSETS = [(0, 0, 0), (1, 1, 0), (-1, 0, 1)]


def tstack_case(shape, channels, laser_offsets, t_offsets, seed):
    """tstacks[l][t]: laser l at time t is the scene at laser_offsets[l] + t_offsets[t]"""
    rng = np.random.default_rng(seed)
    scene = blobs([n + 2 * MARGIN for n in shape], rng)
    out = []
    for c, lo in zip(channels, laser_offsets):
        w = 0.3 + 0.7 * rng.random(c)
        ts = []
        for to in t_offsets:
            a = np.floor(1 + 190 * crop(scene, shape, np.add(lo, to))[..., None] * w)
            a += rng.integers(0, 3, a.shape)
            ts.append(a.astype(np.float32))
        out.append(ts)
    return out


def chain_case():
    return tstack_case(CHAIN_SHAPE, CHAIN_CHANNELS, CHAIN_LASER_OFFSETS, CHAIN_T_OFFSETS, seed=5)


GOLDEN_T = 4
GOLDEN_T_OFFSETS = [(0, 0, 0), (1, -1, 0), (0, 2, 1), (-2, 0, -1)]


def golden_case():
    """the inputs of tests/golden/volreg.npz: 16 x 12 x 8, C = (3, 2, 2, 1), T = 4, integer valued,
    so that the reference's f64 result is exactly representable in f32"""
    return tstack_case(LASER_SHAPE, LASER_CHANNELS, LASER_OFFSETS, GOLDEN_T_OFFSETS, seed=2019)


def all_registrations():
    """(name, reference volume, target volume) of every registration the device tests run"""
    for shape, offs in POW2_SHIFT_CASES + OTHER_SHIFT_CASES:
        v = volumes(shape, offs, seed=sum(shape))
        for t in range(1, len(offs)):
            yield "shift %s %d" % (shape, t), v[0], v[t]
    for shape in ROLL_SHAPES:
        v, _ = roll_volumes(shape)
        for t in (1, 2):
            yield "roll %s %d" % (shape, t), v[0], v[t]
    for shape in TAVG_SHAPES:
        for C in TAVG_C:
            for T in TAVG_T:
                ts = taverage_case(shape, C, T)
                s = [np.sum(a.astype(np.float64), axis=3) for a in ts]
                for t in range(1, T):
                    yield "tavg %s C%d T%d %d" % (shape, C, T, t), s[0], s[t]
    for name, tstacks in (("chain", chain_case()), ("golden", golden_case())):
        avg = []
        for l, ts in enumerate(tstacks):
            s = [np.sum(a.astype(np.float64), axis=3) for a in ts]
            for t in range(1, len(ts)):
                yield "%s laser %d t %d" % (name, l, t), s[0], s[t]
            avg.append(t_average(ts))
        s = [np.log(np.sum(a.astype(np.float64), axis=3) + 1e-8) for a in avg]
        for l in range(1, len(avg)):
            yield "%s laser %d" % (name, l), s[0], s[l]
    s = [np.log(np.sum(a.astype(np.float64), axis=3) + 1e-8) for a in laser_case()]
    for l in range(1, len(s)):
        yield "lasers %d" % l, s[0], s[l]
