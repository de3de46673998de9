"""io.load_tstack: the time points of a biofilm acquisition as (H, W, Z, C) f32 z-stacks, from a CZI
file with a T axis (czi.get_t_range, czi.load_image_zstack_fixed_t) or from the array beside it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from czi_writer import write_czi  # noqa: E402

from hiprfish_image_analysis_amd import czi, io  # noqa: E402


def test_load_tstack_reads_every_time_point(tmp_path):
    rng = np.random.default_rng(9)
    T, H, W, Z, C = 3, 10, 12, 4, 5
    vol = rng.integers(0, 65536, (T, H, W, Z, C), dtype=np.uint16)
    p = str(tmp_path / "s_488.czi")
    write_czi(p, [(vol[t, :, :, z, c], {"T": t, "Z": z, "C": c}) for t in range(T) for z in range(Z) for c in range(C)])
    assert czi.get_t_range(p) == T
    ts = io.load_tstack(p)
    assert len(ts) == T and all(a.shape == (H, W, Z, C) and a.dtype == np.float32 and a.flags.c_contiguous for a in ts)
    for t in range(T):
        assert np.array_equal(ts[t], czi.load_image_zstack_fixed_t(p, t).astype(np.float32))
        # bioformats' rescale: the reader divides by the pixel type's range
        assert np.array_equal(czi.load_image_zstack_fixed_t(p, t, rescale=False), vol[t])
    assert not np.array_equal(ts[0], ts[1])


def test_load_tstack_from_the_array_beside_it(tmp_path):
    a = np.arange(2 * 3 * 4 * 2 * 3, dtype=np.float64).reshape(2, 3, 4, 2, 3)
    np.save(str(tmp_path / "s_514.npy"), a)
    ts = io.load_tstack(str(tmp_path / "s_514.czi"))
    assert len(ts) == 2 and ts[1].dtype == np.float32 and np.array_equal(ts[1], a[1])
    np.save(str(tmp_path / "bad.npy"), a[0])
    with pytest.raises(ValueError):
        io.load_tstack(str(tmp_path / "bad.npy"))
    with pytest.raises(FileNotFoundError):
        io.load_tstack(str(tmp_path / "none.czi"))
