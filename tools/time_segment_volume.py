"""Time the 3-D segmentation chain (pipeline.segment_volume, csrc/volume.hip) stage by stage.

python tools/time_segment_volume.py [--size X Y Z] [--host-size X Y Z | --no-host] [--heap-size X Y Z]

* the device chain on a synthetic blob volume of --size (default cfg4, 1024 x 1024 x 64): per-stage
  milliseconds (host clock around work that ends in a device synchronise; one warm-up run of the
  whole chain first), relaxation passes and contested voxels of both floods, the total, and the
  adjacency flood (:489, :497-499) on its own;
* the heap flood (hrf_watershed3_heap, one workgroup, serial) on a volume built to contest -- a
  constant volume with two markers, every voxel a plateau voxel -- of --heap-size;
* the scipy / sklearn / helper-flood chain (tests/golden/make_volume_golden.py) on the host at
  --host-size, once, with the device chain at the same size beside it.
One JSON line at the end.  No device: fails."""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "golden")]
from hiprfish_image_analysis_amd import kernels as K  # noqa: E402
from hiprfish_image_analysis_amd import pipeline as P  # noqa: E402


def blob_volume(shape, seed=3):
    """(final, reg_sum) f64 on the device: a 128 x 128 x Z block of Gaussian blobs, tiled with
    per-tile gains, plus noise, over its maximum; final a noisy multiple with 2 % exact zeros"""
    X, Y, Z = shape
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    bx, by = min(X, 128), min(Y, 128)
    ax = [torch.arange(n, dtype=torch.float64, device="cuda") for n in (bx, by, Z)]
    gx, gy, gz = torch.meshgrid(*ax, indexing="ij")
    blk = torch.zeros((bx, by, Z), dtype=torch.float64, device="cuda")
    nblobs = max(4, bx * by * Z // 4000)
    c = torch.rand((nblobs, 3), generator=g, device="cuda", dtype=torch.float64) * torch.tensor(
        [bx, by, Z], dtype=torch.float64, device="cuda")
    r = 2.5 + 2.5 * torch.rand(nblobs, generator=g, device="cuda", dtype=torch.float64)
    a = 0.5 + torch.rand(nblobs, generator=g, device="cuda", dtype=torch.float64)
    for i in range(nblobs):
        blk += a[i] * torch.exp(-((gx - c[i, 0]) ** 2 + (gy - c[i, 1]) ** 2 + (gz - c[i, 2]) ** 2) / (2 * r[i] ** 2))
    tx, ty = -(-X // bx), -(-Y // by)
    gain = 0.6 + 0.4 * torch.rand((tx, 1, ty, 1, 1), generator=g, device="cuda", dtype=torch.float64)
    s = (blk.reshape(1, bx, 1, by, Z) * gain).reshape(tx * bx, ty * by, Z)[:X, :Y].contiguous()
    s += 0.03 * torch.rand(s.shape, generator=g, device="cuda", dtype=torch.float64)
    s /= s.max()
    final = s * (0.8 + 0.4 * torch.rand(s.shape, generator=g, device="cuda", dtype=torch.float64))
    final[torch.rand(s.shape, generator=g, device="cuda") < 0.02] = 0.0
    return final, s


class Clock:
    def __init__(self):
        self.ms = {}

    def __call__(self, name, fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        self.ms[name] = self.ms.get(name, 0.0) + (time.perf_counter() - t) * 1e3
        return out


def staged(final, reg):
    """pipeline.segment_volume's calls, one by one under the clock -> (per-stage ms, stats)"""
    ck = Clock()
    pos = final > 0
    share = {}
    rough = ck("kmeans k=2 (:818-828)", lambda: K.kmeans_1d(final, 2, valid=pos, want_labels=False, share=share,
                                                            rule=2)[1])
    rsf = ck("kmeans k=3, shared sort (:829-838)", lambda: K.kmeans_1d(final, 3, valid=pos, want_labels=False,
                                                                       share=share, rule=0)[1])
    opened = ck("opening (:839)", lambda: K.binary_opening3(rsf))
    small = ck("remove_small_objects (:840)", lambda: K.remove_small_objects3(opened, 10))
    bfh = ck("fill_holes x2 (:841-842)", lambda: K.fill_holes3(small))
    rbfh = ck("fill_holes x2 (:841-842)", lambda: K.fill_holes3(rough))
    wmask = ck("and + label 26 (:843-844)", lambda: K.and_mask(bfh, rbfh))
    seeds, nseeds = ck("and + label 26 (:843-844)", lambda: K.label3(wmask, conn=3))
    logsum = ck("log10 + kmeans bkg (:845-854)", lambda: K.log10p1(reg))
    bkg = ck("log10 + kmeans bkg (:845-854)", lambda: K.kmeans_1d(logsum, 2, want_labels=False, rule=1)[1])
    fb, sb, wb = ck("masked products (:855-857)",
                    lambda: (K.mask_mul(final, bkg), K.mask_labels(seeds, bkg), K.and_mask(wmask, bkg)))
    ties = []
    ws = ck("watershed (:858)", lambda: K.watershed3(fb, sb, wb, True, ties=ties))
    seg, n = ck("relabel_sequential (:859)", lambda: K.relabel_sequential(ws, nseeds))
    total = sum(ck.ms.values())
    ties_adj = []
    sum_bkg = ck("adjacency: reg_sum * bkg (:489)", lambda: K.mask_mul(reg, bkg))
    aws = ck("adjacency: watershed (:497)", lambda: K.watershed3(sum_bkg, sb, bkg, True, ties=ties_adj))
    ck("adjacency: relabel_sequential (:499)", lambda: K.relabel_sequential(aws, nseeds))
    stats = dict(seeds=nseeds, labels=n, total_ms=total, adjacency_ms=sum(ck.ms.values()) - total,
                 watershed_contested=ties[0], watershed_heap=ties[1], watershed_passes=ties[2],
                 adjacency_contested=ties_adj[0], adjacency_heap=ties_adj[1], adjacency_passes=ties_adj[2],
                 bkg_voxels=K.count_nonzero(bkg), flooded_voxels=K.count_nonzero(aws) - K.count_nonzero(sb))
    return ck.ms, stats


def report(title, ms, stats):
    print(title)
    for k, v in ms.items():
        print("  %-40s %10.2f ms" % (k, v))
    print("  " + "  ".join("%s=%s" % (k, ("%.2f" % v) if isinstance(v, float) else v) for k, v in stats.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[1024, 1024, 64])
    ap.add_argument("--host-size", type=int, nargs=3, default=[256, 256, 64])
    ap.add_argument("--heap-size", type=int, nargs=3, default=[128, 128, 64])
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_segment_volume: no device")
    res = {}
    # the small sizes first, so a run cut short still reports them
    for key, shape in ((("device_host_size", tuple(a.host_size)),) if not a.no_host else ()) + \
            (("heap", tuple(a.heap_size)), ("device", tuple(a.size))):
        if key == "heap":
            res["heap"] = heap_section(shape)
            continue
        final, reg = blob_volume(shape)
        P.segment_volume(final, reg, adjacency=True)              # warm-up: code objects, pools
        ms, stats = staged(final, reg)
        n = final.numel()
        stats["Mvoxel_per_s"] = n / stats["total_ms"] / 1e3
        report("device chain %d x %d x %d" % shape, ms, stats)
        res[key] = dict(shape=shape, stages_ms=ms, **stats)
        if key == "device_host_size":
            import numpy as np
            import make_volume_golden as G
            f, s = final.cpu().numpy(), reg.cpu().numpy()
            t = time.perf_counter()
            c = G.scipy_chain(f, s)
            host_ms = (time.perf_counter() - t) * 1e3
            seg, nl, _, adj, nadj = P.segment_volume(final, reg, adjacency=True)
            same = bool(np.array_equal(seg.cpu().numpy(), c["seg"]) and np.array_equal(adj.cpu().numpy(),
                                                                                      c["adjacency_seg"]))
            print("host scipy/sklearn/helper chain %d x %d x %d, with the adjacency flood, once: %.0f ms; device %.1f ms;"
                  " label maps equal: %s" % (shape + (host_ms, stats["total_ms"] + stats["adjacency_ms"], same)))
            res["host"] = dict(shape=shape, ms=host_ms, equal=same)
        del final, reg
    print(json.dumps(res))


def heap_section(shape):
    X, Y, Z = shape
    f = torch.zeros((X, Y, Z), dtype=torch.float64, device="cuda")
    mk = torch.zeros((X, Y, Z), dtype=torch.int32, device="cuda")
    mk[X // 4, Y // 4, Z // 4] = 1
    mk[3 * X // 4, 3 * Y // 4, 3 * Z // 4] = 2
    K.watershed3_heap(f[:8, :8, :8].contiguous(), mk[:8, :8, :8].contiguous())   # warm-up
    ck = Clock()
    ties = []
    ck("relaxation + heap (hrf_watershed3)", lambda: K.watershed3(f, mk, None, False, ties=ties))
    ck("heap flood alone (hrf_watershed3_heap)", lambda: K.watershed3_heap(f, mk))
    heap_ms = ck.ms["heap flood alone (hrf_watershed3_heap)"]
    report("contested volume %d x %d x %d (constant, two markers)" % (X, Y, Z), ck.ms,
           dict(contested=ties[0], heap=ties[1], passes=ties[2], ns_per_voxel=heap_ms * 1e6 / (X * Y * Z)))
    return dict(shape=(X, Y, Z), ms=ck.ms, contested=ties[0], passes=ties[2],
                ns_per_voxel=heap_ms * 1e6 / (X * Y * Z))


if __name__ == "__main__":
    main()
