"""The inputs of tests/test_reductions_gpu.py discriminate (numpy alone, no device).

A bit-for-bit comparison with np.sum pins numpy's pairwise order only when a kernel summing in
another order would give another answer on the very array the device test uses.  Asserted here,
per channel count:
  (a) the left-to-right sum differs from np.sum on at least one row, for every C >= 8;
  (b) one 8-accumulator block over the whole row (no split at 128) differs, for every C > 128.
Also: reduction_inputs.numpy_pairwise, the restatement the device tests are written against, equals
np.sum for every n in 1..512, and uniform data -- what the suite summed before -- separates nothing.
"""
import numpy as np
import pytest

import reduction_inputs as RI


def np_sum(x):
    return np.sum(x.astype(np.float64), axis=-1)


def differs(a, b):
    return int(np.count_nonzero(RI.bits(a) != RI.bits(b)))


def test_numpy_pairwise_restated_for_every_n():
    x = RI.order_sensitive((64, 512), seed=1)
    for n in range(1, 513):
        a = np.ascontiguousarray(x[:, :n])
        assert differs(RI.numpy_pairwise(a), np_sum(a)) == 0, n


def test_uniform_data_cannot_tell_orders_apart():
    """the reason for order_sensitive(): on rng.random f32 rows every order gives np.sum"""
    rng = np.random.default_rng(0)
    for C in (8, 23, 95, 128, 250, 512):
        x = rng.random((2000, C)).astype(np.float32)
        assert differs(RI.left_to_right(x), np_sum(x)) == 0, C
        assert differs(RI.one_block(x), np_sum(x)) == 0, C


def test_sweep_stacks_separate_the_wrong_orders():
    few = []
    for C in RI.SWEEP_CS:
        x = RI.sweep_stack(C)
        assert x.shape == (RI.sweep_rows(C), 65, C) and (x.shape[0] * 65) % 64 != 0
        ref = np_sum(x)
        if C >= 8:
            n = differs(RI.left_to_right(x), ref)
            assert n > 0, "left-to-right equals np.sum on every row at C = %d" % C
            few.append((n, C))
        if C > 128:
            assert differs(RI.one_block(x), ref) > 0, "one unsplit block equals np.sum on every row at C = %d" % C
    print("fewest rows telling left-to-right from np.sum: %s" % sorted(few)[:5])


def two_level(x):
    """the split the device code made before it followed numpy to the third level: at most two
    halvings, so a piece above 128 (n = 250: 120 + 130) went to one block"""
    x = np.asarray(x, np.float64)

    def l1(a):
        n = a.shape[-1]
        if n <= 128:
            return RI._block(a)
        n2 = n // 2
        n2 -= n2 % 8
        return RI._block(a[..., :n2]) + RI._block(a[..., n2:])

    n = x.shape[-1]
    if n <= 256:
        return 0.0 + l1(x)
    n2 = n // 2
    n2 -= n2 % 8
    return 0.0 + (l1(x[..., :n2]) + l1(x[..., n2:]))


def test_sweep_stacks_separate_the_two_level_split():
    wrong = [C for C in RI.SWEEP_CS if differs(two_level(RI.sweep_stack(C)), np_sum(RI.sweep_stack(C)))]
    assert set(range(249, 256)) <= set(wrong) and 500 in wrong and 505 in wrong
    assert not set(wrong) & {7, 8, 9, 23, 95, 128, 129, 136, 200, 248, 256, 257, 300, 400, 512}
    print("widths at which a two-level split is not numpy's: %d, first %s" % (len(wrong), wrong[:8]))


@pytest.mark.parametrize("C", RI.EDGE_CS)
def test_edge_stacks_log_inputs_separate(C):
    """modes 1 and 2 take logs of the sums of |x|: the same condition on the absolute values"""
    x = np.abs(RI.sweep_stack(C))
    if C >= 8:
        assert differs(RI.left_to_right(x), np_sum(x)) > 0
    if C > 128:
        assert differs(RI.one_block(x), np_sum(x)) > 0


@pytest.mark.parametrize("C", [c for c in RI.CAL_CS if c >= 8])
def test_cal_stacks_separate(C):
    """the calibrated sums divide first; the undivided stacks at the larger pixel counts already
    separate the orders (npix 1 rides along: one row cannot be required to)"""
    n = sum(differs(RI.left_to_right(x), np_sum(x)) for x in (RI.cal_stack(p, C) for p in RI.CAL_NPIX))
    assert n > 0


@pytest.mark.parametrize("name", sorted(RI.LAYOUTS))
@pytest.mark.parametrize("apply_mask", [False, True])
def test_laser_layouts_separate(name, apply_mask):
    widths, H, W = RI.LAYOUTS[name]
    for lasers in (RI.lasers_for(name), [np.abs(l) for l in RI.lasers_for(name)]):
        st = RI.register_restate(lasers, RI.SHIFTS[:len(widths)], apply_mask)
        assert st.shape == (H, W, sum(widths)) and st.dtype == np.float32
        assert differs(RI.left_to_right(st), np_sum(st)) > 0
        if sum(widths) > 128:
            assert differs(RI.one_block(st), np_sum(st)) > 0
