"""Inputs and host restatements shared by tests/test_reductions_gpu.py (device) and
tests/test_reduction_inputs.py (numpy alone: the inputs tell summation orders apart).

Why not rng.random: f32 values of similar magnitude have an f64 sum that is exact in any order
(24-bit mantissas, a few hundred terms, 53 bits to hold them), so a kernel summing left to right
equals np.sum on every row and a test on such data pins no order.  order_sensitive() spreads the
magnitudes over ~e^{+-18}: partial sums round, and the rounding depends on the order.
"""
import numpy as np

# ---- channel counts and shapes the device tests run ---------------------------------------------
SWEEP_CS = tuple(range(1, 513))                       # every C the channel_sum ABI accepts
EDGE_CS = (1, 3, 7, 8, 9, 63, 95, 127, 128, 129, 250, 300, 511, 512)
CAL_CS = (1, 7, 8, 9, 23, 63, 95, 120, 128)
CAL_NPIX = (1, 63, 64, 65, 130)

# per-laser channel layouts for the fused image_cn, by the kernel register_assemble dispatches to
# (stack.hip register_assemble): (widths, H, W)
LAYOUTS = {
    "ecoli": ((32, 23, 20, 14, 6), 70, 80),           # assemble_ecoli_kernel (W % 16 == 0: pixtable too)
    "ecoli_lds": ((32, 23, 20, 14, 6), 70, 66),       # the same widths, W % 4 != 0: assemble_lds_kernel
    "narrow": ((5, 3, 4), 70, 66),                    # C = 12, a laser below 8: assemble_lds_kernel
    "ragged": ((40, 30, 9), 70, 66),                  # C = 79: assemble_lds_kernel
    "wide": ((100, 60, 7), 70, 66),                   # C = 167 > 128: assemble_kernel + channel_sum_kernel
}
SHIFTS = ((0, 0), (3, -2), (-5, 4), (0, 7), (-1, -1))


def order_sensitive(shape, seed):
    """(standard_normal * exp(normal(0, 6))).astype(float32), fixed seed"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) * np.exp(rng.normal(0.0, 6.0, shape))).astype(np.float32)


def sweep_rows(C):
    """leading dimension of the sweep stack: (2, 65, C) = 130 pixels, two full 64-pixel chunks and
    a ragged one.  Below C = 32 few rows have an order-dependent sum (about 2 % at C = 8), so
    those widths get 32 x 65 = 2080 pixels (still ragged) to hold some with certainty."""
    return 2 if C >= 32 else 32


def sweep_stack(C):
    """the exact stack test_channel_sum_every_width sums at width C"""
    return order_sensitive((sweep_rows(C), 65, C), seed=1000 + C)


def cal_stack(npix, C):
    return order_sensitive((1, npix, C), seed=5000 + 7 * C + npix)


def lasers_for(name):
    widths, H, W = LAYOUTS[name]
    seed = 9000 + sorted(LAYOUTS).index(name)
    return [order_sensitive((H, W, c), seed=seed * 10 + i) for i, c in enumerate(widths)]


def register_restate(lasers, shifts, apply_mask):
    """ecoli measurement.py:51-70 in numpy: each laser shifted by (dr, dc), zero outside its
    coverage; apply_mask zeroes every pixel some laser does not cover (np.where, so a negative
    value under the mask becomes +0.0 as the device writes it)"""
    H, W = lasers[0].shape[:2]
    reg, masks = [], []
    for img, (sr, sc) in zip(lasers, shifts):
        r = np.zeros_like(img)
        m = np.zeros((H, W), bool)
        r[max(0, sr):H + min(0, sr), max(0, sc):W + min(0, sc)] = \
            img[-min(0, sr):H - max(0, sr), -min(0, sc):W - max(0, sc)]
        m[max(0, sr):H + min(0, sr), max(0, sc):W + min(0, sc)] = True
        reg.append(r)
        masks.append(m)
    st = np.dstack(reg)
    if apply_mask:
        st = np.where(np.logical_and.reduce(masks)[:, :, None], st, np.float32(0.0))
    return st


# ---- summation schemes, each over the last axis of an f64 array --------------------------------
def _block(x):
    """numpy's unrolled block: eight accumulators over the multiple-of-8 head, combined as
    ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail in order (n < 8: in order from -0.0)"""
    n = x.shape[-1]
    if n < 8:
        res = np.full(x.shape[:-1], -0.0)
        for i in range(n):
            res = res + x[..., i]
        return res
    n8 = n - n % 8
    r = x[..., :8].copy()
    for i in range(8, n8, 8):
        r = r + x[..., i:i + 8]
    res = ((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])) + ((r[..., 4] + r[..., 5]) + (r[..., 6] + r[..., 7]))
    for i in range(n8, n):
        res = res + x[..., i]
    return res


def _pairwise(x):
    n = x.shape[-1]
    if n <= 128:
        return _block(x)
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(x[..., :n2]) + _pairwise(x[..., n2:])


def numpy_pairwise(x):
    """np.add.reduce's order over the last (contiguous) axis, restated: the identity 0.0 plus
    pairwise_sum, which halves a run (first half rounded down to a multiple of 8) until a piece
    holds at most 128 values and sums a piece with _block"""
    return 0.0 + _pairwise(np.asarray(x, np.float64))


def left_to_right(x):
    """wrong scheme (a): one accumulator, channel 0 first"""
    return np.cumsum(np.asarray(x, np.float64), axis=-1)[..., -1]


def one_block(x):
    """wrong scheme (b): the 8-accumulator block over the whole row, without the split at 128"""
    return 0.0 + _block(np.asarray(x, np.float64))


def bits(a):
    """the bit patterns of an f64 array (signed zeros and NaN payloads compare as written)"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- exact-valued stacks for the per-label sums ------------------------------------------------
def integer_stack(shape, seed):
    """small integers stored as f32: every partial sum is an integer below 2^53, so the f64 sum
    is exact in whatever order the atomics land"""
    return np.random.default_rng(seed).integers(-50, 200, size=shape).astype(np.float32)


def pow2_cal(shape, seed):
    """calibration values 2^-3 .. 2^3: a quotient of a small integer by one is exact"""
    return np.exp2(np.random.default_rng(seed).integers(-3, 4, size=shape)).astype(np.float32)
