"""Biofilm z-stack registration on the device (hiprfish_imaging_biofilm_analysis.py :134-165,
:532-559, :428-450): the 3-D correlation surfaces against numpy's FFT, the shifts of both
correlation paths against the numpy restatement (oracle.register_translation), the t-average
and laser assembly kernels and their pipeline entries against tests/volreg_ref.py (itself equal
to the reference's own lines, tests/test_volreg_ref.py) bit for bit, the chain into the 3-D
segmentation, and both assembly kernels past 2^31 elements.

Equal shifts are demanded because every registration here has a peak margin of at least 1e-9
(test_volreg_ref.py::test_peak_margin_of_every_device_registration) while the surfaces are pinned
to 1e-13 of the peak."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import volreg_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def K():
    from hiprfish_image_analysis_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def P():
    from hiprfish_image_analysis_amd import pipeline
    return pipeline


@pytest.fixture(scope="module")
def g(golden):
    return golden("volreg")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the cached references are read-only


def host(t):
    return t.cpu().numpy()


def rows(t):
    return [tuple(int(v) for v in r) for r in host(t)]


# ---- correlation surfaces ----------------------------------------------------------------------
@pytest.mark.parametrize("n,X,Y,Z", [(2, 16, 16, 4), (3, 16, 32, 8), (4, 64, 16, 16), (2, 32, 32, 32),
                                     (3, 128, 64, 16), (2, 256, 256, 32)])
def test_surfaces_equal_numpy(K, n, X, Y, Z):
    rng = np.random.default_rng(X * 7 + Y * 3 + Z + n)
    vols = rng.random((n, X, Y, Z))
    vols[1:] += 0.5 * vols[:1]
    got = host(K.xcorr3_surfaces(dev(vols)))
    F = np.fft.fftn(vols, axes=(1, 2, 3))
    for t in range(1, n):
        want = np.fft.ifftn(F[0] * F[t].conj()).real * (X * Y * Z // 2)
        scale = np.abs(want).max()
        err = np.abs(got[t - 1] - want).max()
        print("surface %s t=%d: max error %.3g of the peak" % ((n, X, Y, Z), t, err / scale))
        np.testing.assert_allclose(got[t - 1], want, rtol=0, atol=scale * 1e-13)


# ---- shifts --------------------------------------------------------------------------------------
def want_shifts(v):
    return [(0, 0, 0)] + [R.register(v[0], v[t]) for t in range(1, len(v))]


@pytest.mark.parametrize("shape,offs", R.POW2_SHIFT_CASES, ids=lambda c: str(c) if isinstance(c, tuple) else "")
def test_shifts_power_of_two_both_paths(K, P, shape, offs):
    v = R.volumes(shape, offs, seed=sum(shape))
    want = want_shifts(v)
    assert K.xcorr3_supported(*v.shape)
    a = rows(K.xcorr3_shifts_dev(dev(v)))
    b = rows(K.register3_translations_dev(dev(v)))
    assert a == want and b == want
    assert rows(P.estimate_shifts3(dev(v), xcorr=True)) == want
    assert rows(P.estimate_shifts3(list(dev(v)), xcorr=False)) == want
    assert rows(P.estimate_shifts3(dev(v))) == want
    for cl in (0, 2):
        wc = [tuple(0 if abs(c) > cl else c for c in s) for s in want]
        assert rows(K.xcorr3_shifts_dev(dev(v), clamp=cl)) == wc
        assert rows(K.register3_translations_dev(dev(v), clamp=cl)) == wc
        assert rows(P.estimate_shifts3(dev(v), clamp=cl)) == wc


@pytest.mark.parametrize("shape,offs", R.OTHER_SHIFT_CASES, ids=lambda c: str(c) if isinstance(c, tuple) else "")
def test_shifts_other_sizes_through_hipfft(K, P, shape, offs):
    v = R.volumes(shape, offs, seed=sum(shape))
    want = want_shifts(v)
    assert not K.xcorr3_supported(*v.shape)
    assert rows(K.register3_translations_dev(dev(v))) == want
    assert rows(P.estimate_shifts3(dev(v))) == want
    wc = [tuple(0 if abs(c) > 1 else c for c in s) for s in want]
    assert rows(P.estimate_shifts3(dev(v), clamp=1)) == wc
    with pytest.raises(ValueError):
        K.xcorr3_shifts_dev(dev(v))


@pytest.mark.parametrize("shape", R.ROLL_SHAPES, ids=str)
def test_shifts_at_the_wrap_edges(K, shape):
    """np.roll volumes at +n/2 (kept) and at -(n/2 - 1) (index n/2 + 1, wrapped)"""
    v, sh = R.roll_volumes(shape)
    assert want_shifts(v) == [tuple(s) for s in sh]
    assert rows(K.register3_translations_dev(dev(v))) == [tuple(s) for s in sh]
    if K.xcorr3_supported(*v.shape):
        assert rows(K.xcorr3_shifts_dev(dev(v))) == [tuple(s) for s in sh]


def test_shifts_of_identical_volumes_are_zero(K):
    v = R.volumes((16, 16, 8), [(0, 0, 0)] * 3, seed=1)
    assert rows(K.xcorr3_shifts_dev(dev(v))) == [(0, 0, 0)] * 3
    assert rows(K.register3_translations_dev(dev(v))) == [(0, 0, 0)] * 3


def test_estimate_shifts3_default_route(K, P, monkeypatch):
    """supported volumes of at least XCORR3_MIN_VOXELS voxels go through the hand-written pipeline,
    smaller ones and other sizes through hipFFT; both give the rolled volume's shift"""
    used = []
    real = K.xcorr3_shifts_dev
    monkeypatch.setattr(K, "xcorr3_shifts_dev", lambda v, clamp=None: used.append(tuple(v.shape)) or real(v, clamp))
    g = torch.Generator(device="cuda").manual_seed(4)
    assert P.XCORR3_MIN_VOXELS == 256 * 256 * 32
    # at the threshold; below it; above it but no power of two
    for shape, hand in (((256, 256, 32), True), ((128, 128, 32), False), ((264, 256, 32), False)):
        v = torch.rand(shape, generator=g, device="cuda", dtype=torch.float64) ** 8
        vols = torch.stack([v, torch.roll(v, (-5, 3, -2), (0, 1, 2))])
        del used[:]
        assert rows(P.estimate_shifts3(vols)) == [(0, 0, 0), (5, -3, 2)]
        assert bool(used) == hand, shape
        assert rows(P.estimate_shifts3(vols, xcorr=False)) == [(0, 0, 0), (5, -3, 2)]


# ---- t-average -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tavg_ref(shape, C, T):
    ts = R.taverage_case(shape, C, T)
    out, shifts = R.t_average(ts, want_shifts=True)
    for a in ts + [out, shifts]:
        a.setflags(write=False)
    return ts, out, shifts


@pytest.mark.parametrize("T", R.TAVG_T)
@pytest.mark.parametrize("C", R.TAVG_C)
@pytest.mark.parametrize("shape", R.TAVG_SHAPES, ids=str)
def test_t_average_equals_restatement(K, P, orc, shape, C, T):
    ts, want, wshifts = tavg_ref(shape, C, T)
    d = [dev(a) for a in ts]
    got = K.volume_taverage(d, dev(wshifts))
    assert got.dtype == torch.float32 and np.array_equal(host(got), want)
    assert np.array_equal(host(K.volume_taverage(d, [tuple(s) for s in wshifts])), want)   # host triples
    out, shifts = P.t_average_volume(d, want_shifts=True)
    assert np.array_equal(host(shifts), wshifts) and shifts.dtype == torch.int32
    assert np.array_equal(host(out), want)
    assert np.array_equal(host(P.t_average_volume(d)), want)
    if T == 1:
        assert np.array_equal(want, ts[0])
    # the fused channel sum of the result, in both modes
    X, Y, Z = shape
    cs = host(K.channel_sum(got.reshape(X * Y, Z, C))).reshape(X, Y, Z)
    assert np.array_equal(cs, np.sum(want.astype(np.float64), axis=3))
    o2, s_raw = K.volume_taverage(d, dev(wshifts), want_sum="sum")
    o3, s_log = P.t_average_volume(d, want_sum="log")
    assert np.array_equal(host(o2), want) and np.array_equal(host(o3), want)
    assert np.array_equal(host(s_raw), cs)
    assert np.array_equal(host(s_log), orc.cr_log(cs + 1e-8))
    assert np.array_equal(host(K.volume_channel_sum(got, log=True)), host(s_log))
    assert np.array_equal(host(K.volume_channel_sum(got)), cs)


def test_t_average_shift_past_the_volume(K):
    """a shift of a whole axis leaves nothing of that time point (the slices are empty; past the axis
    length the reference's own slice arithmetic no longer holds, and no estimate exceeds n / 2)"""
    ts, _, _ = tavg_ref((16, 12, 8), 6, 3)
    sh = np.array([(0, 0, 0), (16, 0, 0), (0, -12, 2)], np.int32)
    want = ((ts[0].astype(np.float64) + R.shift_zero(ts[1].astype(np.float64), sh[1])
             + R.shift_zero(ts[2].astype(np.float64), sh[2])) / 3).astype(np.float32)
    assert np.array_equal(want, (ts[0].astype(np.float64) / 3).astype(np.float32))
    assert np.array_equal(host(K.volume_taverage([dev(a) for a in ts], dev(sh))), want)


# ---- laser registration --------------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["keep", "zero"])
def test_register_volume_equals_restatement_and_golden(K, P, g, fill):
    avg = [R.t_average(ts) for ts in R.golden_case()]
    want, wshifts = R.register_lasers(avg, fill)
    assert np.array_equal(want.astype(np.float64), g[fill]) and np.array_equal(wshifts, g["lshifts"])
    d = [dev(a) for a in avg]
    got = P.register_volume(d, fill)                                      # shifts estimated
    assert got.dtype == torch.float32 and np.array_equal(host(got), want)
    assert np.array_equal(host(P.register_volume(d, fill, shifts=dev(wshifts))), want)   # shifts passed in
    assert np.array_equal(host(P.register_volume(d, fill, shifts=[tuple(s) for s in wshifts])), want)
    assert np.array_equal(host(K.volume_assemble(d, dev(wshifts), fill)), want)
    out, s = P.register_volume(d, fill, want_sum=True)
    X, Y, Z, C = want.shape
    assert np.array_equal(host(out), want)
    assert np.array_equal(host(s), host(K.channel_sum(out.reshape(X * Y, Z, C))).reshape(X, Y, Z))
    assert np.array_equal(host(s), np.sum(want.astype(np.float64), axis=3))


@pytest.mark.parametrize("fill", ["keep", "zero"])
def test_register_volume_generated_lasers(P, fill):
    lasers = R.laser_case()
    want, wshifts = R.register_lasers(lasers, fill)
    assert np.abs(wshifts).max() > 0
    assert np.array_equal(host(P.register_volume([dev(a) for a in lasers], fill)), want)


@pytest.mark.parametrize("fill", ["keep", "zero"])
def test_register_volume_tstacks_equals_golden(P, g, fill):
    ts = [[dev(a) for a in lst] for lst in R.golden_case()]
    got = host(P.register_volume_tstacks(ts, fill))
    assert np.array_equal(got.astype(np.float64), g[fill])


def test_volume_assemble_rejects_bad_arguments(K):
    a = dev(R.laser_case()[0])
    with pytest.raises(ValueError):
        K.volume_assemble([a], [(0, 0, 0)], fill="mask")
    with pytest.raises(ValueError):
        K.volume_assemble([a, a[:8]], [(0, 0, 0)] * 2)
    with pytest.raises(ValueError):
        K.volume_assemble([a], [(0, 0, 0)] * 2)
    with pytest.raises(ValueError):
        K.volume_taverage([a.repeat(1, 1, 1, 43)], [(0, 0, 0)])            # 129 channels


# ---- chain ---------------------------------------------------------------------------------------
def test_chain_tstacks_to_segmentation(K, P):
    tstacks = R.chain_case()
    avg = [R.t_average(ts) for ts in tstacks]
    want, wshifts = R.register_lasers(avg, "keep")
    assert np.abs(wshifts[1:]).max(axis=1).min() > 0
    d = [[dev(a) for a in ts] for ts in tstacks]
    stack, ssum = P.register_volume_tstacks(d, "keep", want_sum=True)
    assert np.array_equal(host(stack), want)
    seg, n, _ = P.segment_volume_stack(stack, stack_sum=ssum)
    seg_w, n_w, _ = P.segment_volume_stack(dev(want))
    assert n == n_w and n >= 2 and np.array_equal(host(seg), host(seg_w))
    m = P.measure_volume(stack, seg, n)
    lab = host(seg_w)
    spectra = np.stack([want[lab == l].astype(np.float64).mean(axis=0) for l in range(1, n + 1)])
    assert np.allclose(host(m.avgint), spectra, rtol=1e-12, atol=0)


# ---- past 2^31 elements --------------------------------------------------------------------------
BIG = (512, 512, 129, 64)          # 2.16e9 elements, 8.7 GB of f32 per tensor
BIG_SHIFT = (3, -2, 1)


def big_volume(seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 200, BIG, dtype=torch.uint8, device="cuda", generator=gen).to(torch.float32)


def shifted_zero_(a, s):
    """shift_zero on the device, by slices"""
    out = torch.zeros_like(a)
    dst, src = R._box(a.shape[:3], s)
    out[dst] = a[src]
    return out


def test_t_average_past_2g_elements(K):
    assert np.prod(BIG) > 2 ** 31
    a0, a1 = big_volume(1), big_volume(2)
    sh = torch.tensor([(0, 0, 0), BIG_SHIFT], dtype=torch.int32, device="cuda")
    out = K.volume_taverage([a0, a1], sh)
    want = shifted_zero_(a1, BIG_SHIFT).add_(a0).mul_(0.5)      # exact in f32: integers below 400, halved
    assert torch.equal(out, want)
    assert float(out[-1, 0, -1, -1]) == float(a0[-1, 0, -1, -1] + a1[-4, 2, -2, -1]) / 2


def test_assemble_past_2g_elements(K):
    a = big_volume(3)
    sh = torch.tensor([BIG_SHIFT], dtype=torch.int32, device="cuda")
    out, s = K.volume_assemble([a], sh, fill="zero", want_sum="sum")
    want = shifted_zero_(a, BIG_SHIFT)
    assert torch.equal(out, want)
    X, Y, Z, C = BIG
    assert torch.equal(s, K.channel_sum(want.reshape(X * Y, Z, C)).reshape(X, Y, Z))
    del out, s
    dst, src = R._box(BIG[:3], BIG_SHIFT)
    want.copy_(a)
    want[dst] = a[src].clone()
    assert torch.equal(K.volume_assemble([a], sh, fill="keep"), want)
