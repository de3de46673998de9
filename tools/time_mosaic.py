"""Time the tiled 3-D mosaic (pipeline.segment_volume_mosaic, csrc/mosaic.hip, the `+ 1e-8` mode of
csrc/enhance.hip) stage by stage.

python tools/time_mosaic.py [--n N] [--tile X Y Z] [--channels C] [--T T] [--overlap OV] [--reps R]
                            [--no-segment]

On crops of one synthetic scene (default: the reference's acquisition, 4 x 4 tiles of 500 x 500 x
150, C = 14, T = 2, overlap 50), one tile's time points resident at a time, milliseconds from device
events, each stage printed as it finishes:
* per tile, summed over the tiles: the time points' channel sums, the t shift estimate, the time
  sum with its coverage mask;
* the neighbour shifts on the overlap strips, the placement (its one device-to-host copy), the
  accumulation, the normalisation, the edge pad, the enhancement in chunks of 100, the segmentation;
* for the two new kernels the achieved bytes/s against their algorithmic bytes, written beside it,
  and the share of the 8 TB/s HBM peak.  Time sum: T V C 4 read, 9 V written (f64 sum, u8 mask).
  Accumulation: 9 bytes read per tile voxel (its f64 sum and u8 mask, each once) and 12 written per
  canvas voxel (f64 full, int32 count); the canvas voxels under no tile only cost their 12.
The kernels' first calls (one small tile) run before anything is timed, except the segmentation's,
which is run once.  One JSON line at the end.
No device: fails."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
from hiprfish_image_analysis_amd import kernels as K  # noqa: E402
from hiprfish_image_analysis_amd import pipeline as P  # noqa: E402

HBM_PEAK = 8.0e12      # bytes/s, MI355X
PAD = 8                # the scene is this much larger than the mosaic on every side


def scene_of(n, tile, ov, seed=7):
    """a sparse positive texture, lightly smoothed: strips of it correlate with a sharp peak"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    shape = [n * tile[0] - (n - 1) * ov + 2 * PAD, n * tile[1] - (n - 1) * ov + 2 * PAD, tile[2] + 2 * PAD]
    s = torch.rand(shape, generator=g, device="cuda") ** 12 * 190
    for ax in range(3):
        s = (2 * s + torch.roll(s, 1, ax) + torch.roll(s, -1, ax)) / 4
    return s, g


def tile_tstack(scene, w, tile, base, t_off, T):
    out = []
    for t in range(T):
        o = [PAD + b + v for b, v in zip(base, t_off[t % len(t_off)])]
        crop = scene[o[0]:o[0] + tile[0], o[1]:o[1] + tile[1], o[2]:o[2] + tile[2]]
        out.append(torch.floor(1 + crop[..., None] * w).contiguous())
    return out


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--tile", type=int, nargs=3, default=[500, 500, 150])
    ap.add_argument("--channels", type=int, default=14)
    ap.add_argument("--T", type=int, default=2)
    ap.add_argument("--overlap", type=int, default=50)
    ap.add_argument("--chunk", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-segment", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mosaic: no device")
    n, tile, C, T, ov, reps = a.n, tuple(a.tile), a.channels, a.T, a.overlap, a.reps
    Vt = tile[0] * tile[1] * tile[2]
    res = dict(n=n, tile=tile, C=C, T=T, overlap=ov, chunk=a.chunk, stages_ms={})
    st = res["stages_ms"]

    def put(name, ms, add=False):
        st[name] = (st.get(name, 0.0) if add else 0.0) + min(ms)
        if not add:
            print("  %-56s %10.2f ms" % (name, st[name]), flush=True)

    # warm-up: every kernel's first call, on one small tile
    g0 = torch.Generator(device="cuda").manual_seed(1)
    small = [torch.floor(torch.rand((32, 32, 16, C), generator=g0, device="cuda") * 50) for _ in range(T)]
    P.enhance_mosaic(P.stitch_volume_tiles([small], 1, overlap=8)[0], 16)
    P.estimate_tile_shifts([torch.rand((16, 16, 8), generator=g0, device="cuda", dtype=torch.float64)] * 4, 2, 4)
    del small

    scene, g = scene_of(n, tile, ov)
    w = 0.3 + 0.7 * torch.rand(C, generator=g, device="cuda")
    off = torch.randint(-3, 4, (n * n, 3), generator=g, device="cuda").cpu().tolist()
    off[0] = [0, 0, 0]
    t_off = [(0, 0, 0), (2, -1, 1), (-1, 2, 0), (1, 1, -1)]
    print("mosaic %d x %d tiles of %d x %d x %d, C = %d, T = %d, overlap %d" % (n, n, *tile, C, T, ov), flush=True)
    sums, masks = [], []
    tsum_ms = []
    for k in range(n * n):
        i, j = divmod(k, n)
        ts = tile_tstack(scene, w, tile, (i * (tile[0] - ov) + off[k][0], j * (tile[1] - ov) + off[k][1], off[k][2]),
                         t_off, T)
        cs = torch.empty((T,) + tile, dtype=torch.float64, device="cuda")
        _, ms = timed(lambda: [K.channel_sum(v.reshape(tile[0] * tile[1], tile[2], C),
                                             out=cs[q].view(tile[0] * tile[1], tile[2])) for q, v in enumerate(ts)], reps)
        put("channel sums of the time points (:206, :212)", ms, add=True)
        shifts, ms = timed(lambda: P.estimate_shifts3(cs), reps)
        put("t shift estimates (:213)", ms, add=True)
        (s, m), ms = timed(lambda: K.volume_tsum_masked(ts, shifts), reps)
        put("time sums with coverage masks (:214-236, :1073-1076)", ms, add=True)
        tsum_ms.append(min(ms))
        if k == 0:
            res["t_shifts_tile0"] = shifts.cpu().tolist()
        sums.append(s)
        masks.append(m)
        del ts, cs
    for name in list(st):
        print("  %-56s %10.2f ms  (%d tiles)" % (name, st[name], n * n), flush=True)
    nbytes = T * Vt * C * 4 + 9 * Vt
    best = min(tsum_ms)
    res["tsum"] = dict(bytes_per_tile=nbytes, ms_per_tile=tsum_ms, TBps=nbytes / best / 1e9,
                       hbm_share=nbytes / best * 1e3 / HBM_PEAK)
    print("  time sum, per tile: %.3f ms best, %.3f ms mean, %.2f GB, %.2f TB/s, %.1f %% of the HBM peak"
          % (best, sum(tsum_ms) / len(tsum_ms), nbytes / 1e9, res["tsum"]["TBps"], 100 * res["tsum"]["hbm_share"]),
          flush=True)
    del scene

    shifts, ms = timed(lambda: P.estimate_tile_shifts(sums, n, ov), reps)
    put("neighbour shifts on the strips (:1077-1087)", ms)
    want = [[0, 0, 0]] + [[p - q for p, q in zip(off[k], off[k - 1 if k % n else k - n])] for k in range(1, n * n)]
    res["tile_shifts"] = shifts.cpu().reshape(-1, 3).tolist()
    res["tile_shifts_equal_planted"] = res["tile_shifts"] == want
    (org, canvas), ms = timed(lambda: P.mosaic_origins(shifts.cpu().numpy(), tile, ov, 10), reps)
    put("placement: D2H copy of the shifts, origins (:1088-1097)", ms)
    (full, count), ms = timed(lambda: K.mosaic_accumulate3(sums, masks, org, canvas, want_count=True), reps)
    put("accumulation (:1098-1101)", ms)
    Vc = canvas[0] * canvas[1] * canvas[2]
    nbytes = 9 * Vt * n * n + 12 * Vc
    res["accumulate"] = dict(canvas=canvas, bytes=nbytes, ms=min(ms), TBps=nbytes / min(ms) / 1e9,
                             hbm_share=nbytes / min(ms) * 1e3 / HBM_PEAK)
    print("  accumulation: %.2f GB, %.2f TB/s, %.1f %% of the HBM peak; shifts equal the planted ones: %s"
          % (nbytes / 1e9, res["accumulate"]["TBps"], 100 * res["accumulate"]["hbm_share"],
             res["tile_shifts_equal_planted"]), flush=True)
    del sums, masks, count
    norm, ms = timed(lambda: K.div_scalar(full, K.max_f64(full)), reps)
    put("normalisation (:1102)", ms)
    del full
    pad, ms = timed(lambda: K.pad_edge_3d(norm, 5), reps)
    put("edge pad (:1103)", ms)
    final, ms = timed(lambda: K.enhance_3d_eps(pad, a.chunk), reps)
    put("enhancement, + 1e-8 form, chunks of %d (:1104-1126)" % a.chunk, ms)
    del pad
    if not a.no_segment:
        out, ms = timed(lambda: P.segment_volume(final, norm, background="log10eps_positive"), 1)
        put("segmentation (:1127-1170), one run", ms)
        res["cells"] = int(out[1])
    res["total_ms"] = sum(st.values())
    print("  %-56s %10.2f ms" % ("total", res["total_ms"]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
