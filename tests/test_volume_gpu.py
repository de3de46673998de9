"""The 3-D segmentation stages on the device (csrc/volume.hip, kernels.*3, pipeline.segment_volume)
against tests/volume_ref.py -- itself checked against scipy.ndimage, the 2-D oracle and the recorded
fixture in tests/test_volume_ref.py -- and against tests/golden/volume3d.npz.

Shapes cross the 4 x 4 x 64 brick on every axis and degenerate to 2-D and to a single voxel."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import volume_ref as VR  # noqa: E402

SHAPES = [(1, 1, 1), (1, 40, 37), (40, 1, 37), (40, 37, 1), (33, 17, 65), (5, 70, 3), (32, 48, 40)]
FLAT = [(1, 40, 37), (40, 1, 37), (40, 37, 1)]
BIG = (33, 17, 65)


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
    return golden("volume3d")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def live():
    from hiprfish_image_analysis_amd import _lib
    return _lib.lib().hrf_live_allocations()


# ---- components ------------------------------------------------------------------------------
def check_label(K, m):
    for conn in (1, 3):
        want, n = VR.label(m, conn)
        got, gn = K.label3(dev(m), conn=conn)
        assert gn == n, (conn, gn, n)
        assert np.array_equal(host(got), want), conn
    return True


@pytest.mark.parametrize("density", [0.2, 0.5, 0.8])
@pytest.mark.parametrize("shape", SHAPES)
def test_label3_random_masks(K, shape, density):
    rng = np.random.default_rng(hash((shape, int(density * 10))) % 2 ** 32)
    assert check_label(K, rng.random(shape) < density)


def serpentine(shape):
    """one voxel-wide path through the whole volume: every even x plane is a boustrophedon of full z
    lines on even y joined at alternating ends, planes joined through one voxel of the odd x planes"""
    X, Y, Z = shape
    m = np.zeros(shape, bool)
    ys = list(range(0, Y, 2))
    zcur = 0                                                  # where the path enters the current row
    for x in range(0, X, 2):
        for i, y in enumerate(ys):
            m[x, y, :] = True
            zcur = Z - 1 - zcur                               # the row is walked to its other end
            if i + 1 < len(ys):
                m[x, (y + ys[i + 1]) // 2, zcur] = True
        if x + 2 < X:
            m[x + 1, ys[-1], zcur] = True
        ys = ys[::-1]
    return m


def test_label3_serpentine_is_one_component(K):
    m = serpentine(BIG)
    want, n = VR.label(m, 1)
    assert n == 1 and m.sum() > BIG[0] * BIG[2] * 4          # one path, through every brick
    assert all(m[x0:x0 + 4, y0:y0 + 4, z0:z0 + 64].any()
               for x0 in range(0, 33, 4) for y0 in range(0, 17, 4) for z0 in (0, 64))
    for conn in (1, 3):
        got, gn = K.label3(dev(m), conn=conn)
        assert gn == 1 and np.array_equal(host(got), m.astype(np.int32))


def test_label3_bodies_touching_at_a_corner(K):
    m = np.zeros(BIG, bool)
    m[2:4, 2:4, 62:64] = True                                 # the corner (3,3,63)-(4,4,64) crosses a
    m[4:6, 4:6, 64:65] = True                                 # brick boundary on all three axes
    got3, n3 = K.label3(dev(m), conn=3)
    got2, n2 = K.label3(dev(m), conn=2)
    got1, n1 = K.label3(dev(m), conn=1)
    assert (n3, n2, n1) == (1, 2, 2)
    assert np.array_equal(host(got3), VR.label(m, 3)[0]) and np.array_equal(host(got1), VR.label(m, 1)[0])
    assert np.array_equal(host(got2), VR.label(m, 2)[0])
    lab = dev(np.where(m, 7, 0).astype(np.int32))             # an int32 label image: equal values connect
    assert K.label3(lab, conn=3)[1] == 1


def test_primitives_equal_scipy_fixture(K, g):
    m = dev(g["p_mask"])
    assert np.array_equal(host(K.label3(m, conn=1)[0]), g["p_label6"])
    assert np.array_equal(host(K.label3(m, conn=3)[0]), g["p_label26"])
    assert np.array_equal(host(K.binary_erosion3(m, 0)), g["p_erosion0"])
    assert np.array_equal(host(K.binary_erosion3(m, 1)), g["p_erosion1"])
    assert np.array_equal(host(K.binary_dilation3(m)), g["p_dilation"])
    assert np.array_equal(host(K.binary_opening3(m)), g["p_opening"])
    assert np.array_equal(host(K.fill_holes3(m)), g["p_fill"])


# ---- morphology ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_morphology3(K, shape):
    rng = np.random.default_rng(sum(shape))
    m = rng.random(shape) < 0.75
    m[0] = True                                               # ones on the faces tell border 0 from 1
    m[:, -1] = True
    m[:, :, 0] = True
    d = dev(m)
    e0, e1 = host(K.binary_erosion3(d, 0)).astype(bool), host(K.binary_erosion3(d, 1)).astype(bool)
    assert np.array_equal(e0, VR.erode(m, 0)) and np.array_equal(e1, VR.erode(m, 1))
    assert not e0.any() or min(shape) > 2                     # border 0 empties anything one or two thick
    assert e1.sum() > e0.sum()
    assert np.array_equal(host(K.binary_dilation3(d)).astype(bool), VR.dilate(m))
    assert np.array_equal(host(K.binary_opening3(d)).astype(bool), VR.opening(m))
    assert np.array_equal(host(K.binary_opening3(d, border_value=1)).astype(bool), VR.opening(m, 1))


# ---- fill holes ------------------------------------------------------------------------------
def test_fill_holes3_cavities(K):
    m = np.zeros(BIG, bool)
    m[2:9, 2:9, 2:9] = True
    m[4:7, 4:7, 4:7] = False                                  # closed cavity: filled
    m[12:17, 2:7, 2:7] = True
    m[13:16, 3:6, 3:6] = False
    m[12, 2, 4] = False                                       # open only across an edge: filled
    m[20:25, 2:7, 2:7] = True
    m[21:24, 3:6, 3:6] = False
    m[20, 4, 4] = False                                       # open through a face: not filled
    m[26:31, 9:14, 60:65] = True
    m[27:30, 10:13, 61:64] = False
    m[28, 11, 64] = False                                     # a tunnel to the volume's face: not filled
    got = host(K.fill_holes3(dev(m))).astype(bool)
    assert np.array_equal(got, VR.fill_holes(m))
    assert got[4:7, 4:7, 4:7].all()
    assert got[13:16, 3:6, 3:6].all() and not got[12, 2, 4]
    assert not got[21:24, 3:6, 3:6].any() and not got[20, 4, 4]
    assert not got[27:30, 10:13, 61:64].any() and not got[28, 11, 64]
    assert np.array_equal(got & m, m)


@pytest.mark.parametrize("shape", SHAPES)
def test_fill_holes3_random(K, shape):
    rng = np.random.default_rng(sum(shape) + 1)
    m = rng.random(shape) < 0.7
    assert np.array_equal(host(K.fill_holes3(dev(m))).astype(bool), VR.fill_holes(m))
    assert host(K.fill_holes3(dev(np.ones(shape, bool)))).all()
    assert not host(K.fill_holes3(dev(np.zeros(shape, bool)))).any()


# ---- remove small objects --------------------------------------------------------------------
def test_remove_small_objects3(K):
    m = np.zeros(BIG, bool)
    m[1, 3:12, 5] = True                                      # 9 voxels: removed
    m[3, 3:13, 5] = True                                      # 10 voxels, across bricks in y: kept
    m[6:9, 0:3, 10] = True                                    # two 9-voxel plates touching at a corner:
    m[9:12, 3:6, 11] = True                                   # both removed at conn 1, one body of 18 at conn 3
    m[20, 8, 60:65] = True                                    # 5 + 5 across the brick edge in z and ...
    m[20, 3:8, 64] = True                                     # ... y: one body of 10
    got1 = host(K.remove_small_objects3(dev(m), 10, conn=1)).astype(bool)
    got3 = host(K.remove_small_objects3(dev(m), 10, conn=3)).astype(bool)
    assert np.array_equal(got1, VR.remove_small_objects(m, 10, 1))
    assert np.array_equal(got3, VR.remove_small_objects(m, 10, 3))
    assert not got1[1].any() and got1[3, 3:13, 5].all() and not got1[6:12, :, 10:12].any()
    assert got1[20].sum() == 10 and got3[6:12, :, 10:12].sum() == 18
    rng = np.random.default_rng(2)
    r = rng.random((5, 70, 3)) < 0.3
    assert np.array_equal(host(K.remove_small_objects3(dev(r), 10)).astype(bool), VR.remove_small_objects(r, 10))


# ---- watershed -------------------------------------------------------------------------------
def ws_case(shape, seed=0):
    """a smooth noise field as ranks / n (all values distinct), about 12 markers and a mask"""
    rng = np.random.default_rng(seed + sum(shape))
    a = rng.random(shape)
    for _ in range(3):
        a = sum(np.roll(a, s, ax) for ax in range(3) for s in (-1, 1)) / 6 + a / 6
    n = a.size
    ranks = np.empty(n, np.float64)
    ranks[np.argsort(a.ravel(), kind="stable")] = np.arange(n)
    f = (ranks / n).reshape(shape)
    mk = np.zeros(shape, np.int32)
    k = min(12, max(1, n // 4))
    mk.ravel()[rng.choice(n, k, replace=False)] = np.arange(1, k + 1)
    mask = rng.random(shape) < 0.9
    return f, mk, mask


@pytest.fixture(scope="module")
def ws_refs():
    """the helper floods the watershed tests share, computed once per (shape, quantised)"""
    cache = {}

    def get(shape, quantised):
        key = (shape, quantised)
        if key not in cache:
            f, mk, mask = ws_case(shape)
            if quantised:
                f = np.floor(f * 6).clip(0, 5)
            cache[key] = (f, mk, mask, VR.flood(f, mk, mask))
        return cache[key]

    return get


@pytest.mark.parametrize("shape", SHAPES)
def test_watershed3_distinct_values(K, ws_refs, shape):
    f, mk, mask, want = ws_refs(shape, False)
    ties = []
    got = host(K.watershed3(dev(f), dev(mk), dev(mask), False, ties=ties))
    assert np.array_equal(got, want)
    relaxable = bool((mask & (mk == 0)).any())
    assert ties[0] == 0 and ties[1] == 0 and (ties[2] > 0) == relaxable, ties     # distinct values: no contest
    assert np.array_equal(host(K.watershed3_heap(dev(f), dev(mk), dev(mask))), want)


@pytest.mark.parametrize("shape", SHAPES)
def test_watershed3_quantised(K, ws_refs, shape):
    f, mk, mask, want = ws_refs(shape, True)
    ties = []
    got = host(K.watershed3(dev(f), dev(mk), dev(mask), False, ties=ties))
    assert np.array_equal(got, want)
    assert ties[1] == int(ties[0] > 0), ties
    if np.prod(shape) > 10000:
        assert ties[0] > 0, ties                                                 # plateaus with competing labels
    assert np.array_equal(host(K.watershed3_heap(dev(f), dev(mk), dev(mask))), want)


def test_watershed3_constant_volume_two_markers(K):
    f = np.zeros(BIG)
    mk = np.zeros(BIG, np.int32)
    mk[3, 2, 5] = 1
    mk[29, 14, 61] = 2
    want = VR.flood(f, mk)
    ties = []
    assert np.array_equal(host(K.watershed3(dev(f), dev(mk), None, False, ties=ties)), want)
    assert ties[1] == int(ties[0] > 0)
    assert np.array_equal(host(K.watershed3_heap(dev(f), dev(mk))), want)


@pytest.mark.parametrize("quantised", [False, True])
@pytest.mark.parametrize("shape", FLAT)
def test_watershed3_flat_volumes_equal_2d(K, orc, ws_refs, shape, quantised):
    f, mk, mask, want = ws_refs(shape, quantised)
    s2 = tuple(d for d in shape if d > 1)
    f2, mk2, mask2 = f.reshape(s2), mk.reshape(s2), mask.reshape(s2)
    assert np.array_equal(want.reshape(s2), orc.watershed(f2, mk2, mask2))
    got = host(K.watershed3(dev(f), dev(mk), dev(mask))).reshape(s2)
    assert np.array_equal(got, host(K.watershed(dev(f2), dev(mk2), dev(mask2))))
    assert np.array_equal(host(K.watershed3_heap(dev(f), dev(mk), dev(mask))).reshape(s2),
                          host(K.watershed_heap(dev(f2), dev(mk2), dev(mask2))))


def test_watershed3_every_voxel_a_marker(K):
    rng = np.random.default_rng(9)
    mask = rng.random(BIG) < 0.6
    mk = (VR.label(mask, 3)[0] * mask).astype(np.int32)
    mk[~mask] = rng.integers(1, 5, BIG)[~mask]                 # markers outside the mask are ignored
    f = rng.random(BIG)
    ties = []
    got = host(K.watershed3(dev(f), dev(mk), dev(mask), True, ties=ties))
    assert ties == [0, 0, 0]
    assert np.array_equal(got, mk * mask)


def test_watershed3_markers_outside_mask_and_none(K, ws_refs):
    f, mk, mask, _ = ws_refs((5, 70, 3), False)
    mk = mk.copy()
    out_of_mask = np.argwhere(~mask)[0]
    mk[tuple(out_of_mask)] = 99
    want = VR.flood(f, mk, mask)
    got = host(K.watershed3(dev(f), dev(mk), dev(mask)))
    assert np.array_equal(got, want) and not (got == 99).any()
    none = np.zeros_like(mk)
    assert not host(K.watershed3(dev(f), dev(none), dev(mask))).any()
    assert not host(K.watershed3_heap(dev(f), dev(none), dev(mask))).any()


@pytest.mark.parametrize("quantised", [False, True])
def test_watershed3_negate(K, ws_refs, quantised):
    f, mk, mask, _ = ws_refs(BIG, quantised)
    want = VR.flood(-f, mk, mask)
    assert np.array_equal(host(K.watershed3(dev(f), dev(mk), dev(mask), True)), want)
    assert np.array_equal(host(K.watershed3_heap(dev(f), dev(mk), dev(mask), negate=True)), want)


# ---- the chain -------------------------------------------------------------------------------
NAMES = ("rough_mask", "rsf", "opened", "small", "bfh", "rough_bfh", "watershed_mask", "seeds", "bkg_mask",
         "seeds_bkg", "watershed_mask_bkg", "watershed", "adjacency_watershed", "adjacency_seg")


def test_segment_volume_equals_fixture(P, g):
    keep = {}
    final, reg = dev(g["c_final"].astype(np.float64)), dev(g["c_reg_sum"].astype(np.float64))
    seg, n, final_bkg, adj, n_adj = P.segment_volume(final, reg, keep=keep, adjacency=True)
    before = live()                                            # after the first call: lazy tables exist
    for name in NAMES:
        assert np.array_equal(host(keep[name]).astype(np.int64), g["c_" + name].astype(np.int64)), name
    assert keep["nseeds"] == int(g["c_nseeds"])
    assert np.array_equal(host(seg), g["c_seg"]) and n == int(g["c_n"])
    assert np.array_equal(host(adj), g["c_adjacency_seg"]) and n_adj == int(g["c_n_adj"])
    assert np.array_equal(host(final_bkg), g["c_final"].astype(np.float64) * g["c_bkg_mask"])
    for k in ("centers2", "centers3", "centers_bkg"):
        assert np.allclose(keep[k], g["c_" + k], rtol=1e-12, atol=0), k
    assert keep["ties"] == [0, 0, 0]                           # :858 floods nothing
    assert keep["ties_adjacency"][2] > 0                       # :497 does
    seg2, n2, _ = P.segment_volume(final, reg)
    assert n2 == n and np.array_equal(host(seg2), g["c_seg"])
    del keep, seg, adj, final_bkg, seg2
    assert live() == before


def test_segment_volume_stack_equals_helper_chain(P, K, orc):
    rng = np.random.default_rng(21)
    X, Y, Z, C = 24, 24, 16, 6
    _, s = VR.synthetic_volume((X, Y, Z), seed=5, nblobs=9)
    spec = 0.2 + rng.random(C)
    vol = (s[..., None] * spec * (0.9 + 0.2 * rng.random((X, Y, Z, C)))).astype(np.float32)
    keep = {}
    seg, n, final_bkg, adj, n_adj = P.segment_volume_stack(dev(vol), keep=keep, adjacency=True)
    sm = np.sum(vol.astype(np.float64), axis=3)
    sm = sm / np.max(sm)
    assert np.array_equal(host(keep["reg_sum"]), sm)
    final = orc.enhance_3d(np.pad(sm, 5, mode="edge"))
    assert np.array_equal(host(keep["final"]), final)

    def km(x, k):
        lab, cen, _ = orc.kmeans_sk(x, k)
        return lab, cen

    c = VR.chain(final, sm, km, log10=orc.cr_log10)
    for name in NAMES:
        assert np.array_equal(host(keep[name]).astype(np.int64), np.asarray(c[name]).astype(np.int64)), name
    assert np.array_equal(host(seg), c["seg"]) and n == c["n"] and n >= 2
    assert np.array_equal(host(adj), c["adjacency_seg"]) and n_adj == c["n_adj"]
    assert np.array_equal(host(final_bkg), c["final_bkg"])
    # per-label mean spectra through the flat reductions
    m = P.measure_volume(dev(vol), seg, n)
    lab = host(seg)
    want = np.stack([vol[lab == l].astype(np.float64).mean(axis=0) for l in range(1, n + 1)])
    assert np.array_equal(host(m.labels), np.arange(1, n + 1))
    assert np.allclose(host(m.avgint), want, rtol=1e-12, atol=0)


# ---- ownership and limits --------------------------------------------------------------------
def test_volume_calls_leave_no_allocation(K, ws_refs):
    f, mk, mask, _ = ws_refs((5, 70, 3), True)
    K.watershed3(dev(f), dev(mk), dev(mask))
    torch.cuda.synchronize()
    before = live()
    K.watershed3(dev(f), dev(mk), dev(mask))
    K.watershed3_heap(dev(f), dev(mk), dev(mask))
    K.label3(dev(mask))
    K.fill_holes3(dev(mask))
    K.remove_small_objects3(dev(mask), 10)
    torch.cuda.synchronize()
    assert live() == before


def test_volume_over_the_size_limit_raises(K):
    from hiprfish_image_analysis_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    one = torch.zeros(8, dtype=torch.int32, device="cuda")
    p = one.data_ptr()
    for shape in ((2048, 2048, 512), (1 << 31, 1, 1), (1, (1 << 31) - 2, 1), (1 << 21, 1 << 21, 1 << 21)):
        X, Y, Z = shape
        with pytest.raises(ValueError):
            _lib.call("hrf_cc_roots3", p, 0, X, Y, Z, 3, p, st)
        with pytest.raises(ValueError):
            _lib.call("hrf_binary_erosion3", p, X, Y, Z, 0, p + 4, st)
        with pytest.raises(ValueError):
            _lib.call("hrf_watershed3", p, 0, p, None, X, Y, Z, p, p, p, 10, None, None, st)
        with pytest.raises(ValueError):
            _lib.call("hrf_watershed3_heap", p, 0, p, None, X, Y, Z, p + 4, st)
        assert _lib.lib().hrf_watershed3_workspace_bytes(X, Y, Z) == -1
    assert _lib.lib().hrf_watershed3_workspace_bytes(1, 1, (1 << 31) - 3) > 0
    with pytest.raises(ValueError):                             # the wrapper checks before it allocates
        K.label3(torch.zeros(1, dtype=torch.uint8, device="cuda").expand(2048, 2048, 512))
    with pytest.raises(ValueError):
        K.label3(torch.zeros((4, 4), dtype=torch.uint8, device="cuda"))
