"""bench.py's plain run and --dump-outputs, once on hardware at the smallest schedule (one tile in
flight, two timed steps over two resident tiles): the result line carries the headline fields and
nothing that belongs to --full; the dumped arrays are f32 / f64, within the size limit, and equal
to what the native tile path returns in this process for the tile of the last timed step (the f64
per-cell spectra and distances within 1e-12, everything else bit for bit)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_run_dumps_last_step(tmp_path):
    out = tmp_path / "dump"
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "0",
           "--concurrent", "1", "--tiles", "2", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0
    # value = pixels of the timed steps / their time
    assert rec["value"] == pytest.approx(2048 * 2048 / rec["ms_per_step"] / 1e3, rel=1e-3)
    for k in ("roofline", "extras", "cpu_baseline"):
        assert k not in rec

    sys.path.insert(0, REPO)
    import bench
    files = sorted(os.listdir(out))
    assert all(f.endswith(".npy") for f in files)
    got = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_MAX_BYTES
    assert rec["config"]["cells_counted"] == int(got["counts"].sum())

    # the last timed step's tile (step 1, slot 0 -> resident tile 1), through the same call here
    from hiprfish_image_analysis_amd import pipeline as P
    from hiprfish_image_analysis_amd import synthetic as S
    dev = torch.device("cuda", 0)
    ref = S.reference_library(bench.NBIT, S.ECOLI_BOUNDS)
    lib = P.Library(torch.from_numpy(ref.astype(np.float64)).to(dev), S.ECOLI_BOUNDS, bench.NBIT)
    cal = S.flat_field(bench.H, bench.W, device=dev)
    seed = 20190101 + 1
    lay = S.cell_layout(bench.H, bench.W, S.default_ncells(bench.H, bench.W), lib.R, seed)
    truth, prof = S.render_truth(bench.H, bench.W, lay, with_profile=True)
    stack = S.render_stack(truth, lay, ref, seed=seed, device=dev, profile=prof)
    res = P.process_tile_native(S.laser_split(stack), lib, calibration=cal, per_pixel=True, variant=1)
    torch.cuda.synchronize()
    sel = got["sample_px"].astype(np.int64)
    assert sel.size == bench.DUMP_SAMPLE_PX and np.all(np.diff(sel) > 0) and sel[-1] < bench.H * bench.W
    want = {"counts": res.counts, "labels": res.meas.labels, "avgint": res.meas.avgint,
            "avgint_norm": res.meas.avgint_norm, "cell_idx": res.cell_idx, "cell_dist": res.cell_dist}
    for name, t in (("segmentation", res.meas.segmentation), ("identification", res.identification),
                    ("pixel_idx", res.pixel_idx), ("pixel_dist", res.pixel_dist)):
        want[name] = t.reshape(-1).cpu()[torch.from_numpy(sel)]
    assert res.cell_idx.numel() > 100
    for name, t in want.items():
        a = got["tile0_" + name]
        assert a.shape == tuple(t.shape), name
        w = t.cpu().numpy().astype(a.dtype)
        if name in ("avgint", "avgint_norm", "cell_dist"):
            # the f64 per-cell sums accumulate in the order the device schedules them: a cell of n
            # pixels (a few thousand at most) differs by up to n * 2^-53 relative from run to run,
            # well inside 1e-12, the suite's bound for spectra against the restatement
            np.testing.assert_allclose(a, w, rtol=1e-12, atol=1e-12, err_msg=name)
        else:
            assert np.array_equal(a, w), name
    assert set(got) == {"counts", "sample_px"} | {"tile0_" + n for n in want}
