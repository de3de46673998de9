"""Time the z-stack registration (pipeline.register_volume_tstacks, csrc/volreg.hip, the 3-D
correlations of csrc/xcorr.hip and csrc/register.hip) stage by stage.

python tools/time_register_volume.py [--size X Y Z] [--channels C ...] [--T T] [--reps N]
python tools/time_register_volume.py --corr-sizes X Y Z [X Y Z ...]

On rolled copies of one synthetic scene (default cfg4: 1024 x 1024 x 64, C = 23 20 14 6, T = 2),
after one warm-up of the whole chain, milliseconds from device events:
* per stage: the time points' channel sums, the t shift estimate, the t-average kernel (with its
  fused log sum), the laser shift estimate, the laser assembly (with its fused sum);
* for the two assembly kernels the achieved bytes/s against their algorithmic bytes (t-average:
  T V C 4 read, V C 4 written, 8 V for the sum; assembly: V C 4 read and written, 8 V) and the
  share of the 8 TB/s HBM peak;
* the hand-written correlation against the hipFFT path on the same volumes (the two t sums of
  laser 0; the four lasers' log sums), alternating, three pairs each, where the size is supported.
One JSON line at the end.  No device: fails."""
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


def acquisitions(shape, channels, T, seed=7):
    """tstacks[l][t] (X, Y, Z, C_l) f32, integer valued: one sparse scene rolled by the laser's and
    the time point's offset, seen through the laser's channel weights"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    scene = torch.rand(shape, generator=g, device="cuda") ** 12 * 190
    for ax in range(3):
        scene = (2 * scene + torch.roll(scene, 1, ax) + torch.roll(scene, -1, ax)) / 4
    l_off = [(0, 0, 0), (3, -2, 1), (-2, 4, 0), (1, 1, -1)]
    t_off = [(0, 0, 0), (2, -1, 1), (-1, 2, 0), (1, 1, -1)]
    out = []
    for l, c in enumerate(channels):
        w = 0.3 + 0.7 * torch.rand(c, generator=g, device="cuda")
        ts = []
        for t in range(T):
            o = [a + b for a, b in zip(l_off[l % 4], t_off[t % 4])]
            s = torch.roll(scene, [-v for v in o], (0, 1, 2))
            ts.append(torch.floor(1 + s[..., None] * w).contiguous())
        out.append(ts)
    return out, l_off, t_off


def timed(fn, reps):
    """(result, [ms] * reps) from device events"""
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return out, ms


def correlations(vols, pairs=3, inner=1):
    """hand-written and hipFFT shifts of the same (n, X, Y, Z) volumes, alternating; a sample is the
    mean of `inner` back-to-back calls (small volumes: a single call is a few launch gaps long)"""
    if not K.xcorr3_supported(*vols.shape):
        return None
    K.xcorr3_shifts_dev(vols), K.register3_translations_dev(vols)          # warm-up: plans, twiddles
    hand, fft = [], []
    for _ in range(pairs):
        a, ms = timed(lambda: [K.xcorr3_shifts_dev(vols) for _ in range(inner)][-1], 1)
        hand.append(ms[0] / inner)
        b, ms = timed(lambda: [K.register3_translations_dev(vols) for _ in range(inner)][-1], 1)
        fft.append(ms[0] / inner)
        assert torch.equal(a, b)
    return dict(n=int(vols.shape[0]), xcorr_ms=hand, hipfft_ms=fft, shifts=a.cpu().tolist(),
                xcorr_not_slower_in_every_pair=all(h <= f for h, f in zip(hand, fft)))


def correlation_sweep(sizes):
    """both paths on rolled copies of a random volume, n = 2 and n = 4, per size"""
    res = []
    g = torch.Generator(device="cuda").manual_seed(11)
    for X, Y, Z in sizes:
        v = torch.rand((X, Y, Z), generator=g, device="cuda", dtype=torch.float64) ** 8
        vols = torch.stack([torch.roll(v, (-i, 2 * i, -(i % 2)), (0, 1, 2)) for i in range(4)])
        inner = max(1, (1 << 25) // (X * Y * Z))
        for n in (2, 4):
            r = correlations(vols[:n].contiguous(), inner=inner)
            r.update(shape=(X, Y, Z), inner=inner)
            res.append(r)
            print("  %4d x %4d x %4d n = %d (%3d calls per sample): hand-written %s ms, hipFFT %s ms%s" % (
                X, Y, Z, n, inner, ["%.3f" % q for q in r["xcorr_ms"]], ["%.3f" % q for q in r["hipfft_ms"]],
                "" if r["xcorr_not_slower_in_every_pair"] else "   <- hipFFT wins a pair"))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[1024, 1024, 64])
    ap.add_argument("--channels", type=int, nargs="+", default=[23, 20, 14, 6])
    ap.add_argument("--T", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--corr-sizes", type=int, nargs="+", default=None, metavar="N",
                    help="X Y Z [X Y Z ...]: only compare the two correlation paths at these sizes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_register_volume: no device")
    if a.corr_sizes:
        sizes = [tuple(a.corr_sizes[i:i + 3]) for i in range(0, len(a.corr_sizes), 3)]
        print("3-D correlation, hand-written (xcorr.hip) against hipFFT (register.hip), alternating")
        print(json.dumps(dict(correlation_sweep=correlation_sweep(sizes))))
        return
    X, Y, Z = a.size
    V, T, reps = X * Y * Z, a.T, a.reps
    tstacks, l_off, t_off = acquisitions((X, Y, Z), a.channels, T)
    stack, ssum = P.register_volume_tstacks(tstacks, "keep", want_sum=True)   # warm-up of the whole chain
    del stack, ssum
    res = dict(shape=(X, Y, Z), channels=a.channels, T=T, route="xcorr" if P.XCORR3 != "0" and V >= P.XCORR3_MIN_VOXELS and K.xcorr3_supported(2, X, Y, Z) else "hipfft", stages_ms={})
    st = res["stages_ms"]

    def put(name, ms):
        st[name] = st.get(name, 0.0) + min(ms)

    avg, logs, tavg_bw = [], [], []
    for l, ts in enumerate(tstacks):
        C = a.channels[l]
        sums = torch.empty((T, X, Y, Z), dtype=torch.float64, device="cuda")
        _, ms = timed(lambda: [K.channel_sum(v.reshape(X * Y, Z, C), out=sums[i].view(X * Y, Z))
                               for i, v in enumerate(ts)], reps)
        put("channel sums of the time points (:137, :142)", ms)
        shifts, ms = timed(lambda: P.estimate_shifts3(sums), reps)
        put("t shift estimate (:143)", ms)
        (out, s), ms = timed(lambda: K.volume_taverage(ts, shifts, "log"), reps)
        put("t-average + log sum (:144-165, :536-537)", ms)
        nbytes = T * V * C * 4 + V * C * 4 + 8 * V
        tavg_bw.append(dict(C=C, ms=min(ms), bytes=nbytes, TBps=nbytes / min(ms) / 1e9,
                            hbm_share=nbytes / min(ms) * 1e3 / HBM_PEAK, shifts=shifts.cpu().tolist()))
        if l == 0:
            res["correlation_t_sums"] = correlations(sums)
        avg.append(out)
        logs.append(s)
        del sums
    del tstacks, ts
    logs = torch.stack(logs)
    shifts, ms = timed(lambda: P.estimate_shifts3(logs), reps)
    put("laser shift estimate (:537-538)", ms)
    res["correlation_laser_log_sums"] = correlations(logs)
    (stack, ssum), ms = timed(lambda: K.volume_assemble(avg, shifts, "keep", "sum"), reps)
    put("laser assembly + sum (:539-558, :808)", ms)
    Ct = sum(a.channels)
    nbytes = 2 * V * Ct * 4 + 8 * V
    res["assemble"] = dict(C=Ct, ms=min(ms), bytes=nbytes, TBps=nbytes / min(ms) / 1e9,
                           hbm_share=nbytes / min(ms) * 1e3 / HBM_PEAK, shifts=shifts.cpu().tolist())
    res["taverage"] = tavg_bw
    res["total_ms"] = sum(st.values())
    res["planted"] = dict(lasers=l_off[:len(a.channels)], t=t_off[:T])
    print("register_volume_tstacks %d x %d x %d, C = %s, T = %d (shift estimates through %s)"
          % (X, Y, Z, a.channels, T, res["route"]))
    for k, v in st.items():
        print("  %-48s %10.2f ms" % (k, v))
    print("  %-48s %10.2f ms" % ("total", res["total_ms"]))
    for b in tavg_bw + [res["assemble"]]:
        print("  C = %2d: %8.2f ms, %6.2f GB, %5.2f TB/s, %4.1f %% of the HBM peak"
              % (b["C"], b["ms"], b["bytes"] / 1e9, b["TBps"], 100 * b["hbm_share"]))
    for k in ("correlation_t_sums", "correlation_laser_log_sums"):
        if res[k]:
            print("  %s (n = %d): hand-written %s ms, hipFFT %s ms" % (
                k, res[k]["n"], ["%.2f" % v for v in res[k]["xcorr_ms"]], ["%.2f" % v for v in res[k]["hipfft_ms"]]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
