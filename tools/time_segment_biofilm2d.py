"""Time the 2-D biofilm segmentation (pipeline.segment_biofilm_2d, csrc/biofilm2d.hip) stage by stage.

python tools/time_segment_biofilm2d.py [--size N] [--small N] [--radius R] [--no-host | --host-only]

* the device chain on a synthetic field of --size (default 2048) squared and of --small (512) squared,
  63 channels, disk radius --radius (100): per-stage milliseconds (host clock around work that ends
  in a device synchronise; one warm-up run of the whole chain first), the three disk passes' share;
* each disk kernel alone on the chain's own masks: dilation, erosion, and their two passes apart
  (hrf_binary_dilation_disk on a mask whose every pixel is hit at once: pass A plus a pass B that
  leaves its loop on the first ballot);
* once, at --small squared on the host, the chain of tests/biofilm2d_ref.py with scipy.ndimage's
  binary_dilation / binary_erosion by skimage's disk as the reference runs them, and whether the
  device's label maps and epithelial area equal it (sha1 of each array is printed, so a host-only
  run on another machine can be compared with a device run).
One JSON line at the end.  Without --host-only and no device: fails."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")]

CHANNELS = 63


def field(N, seed=3):
    """(N, N, 63) f32 on the host: a dark background on the left and below, a glowing field of Gaussian
    cells on the upper right (open to the top and right borders), one dim tissue blob on the lower
    border; 2 % multiplicative noise, six unit-sum spectra by nearest cell"""
    rng = np.random.default_rng(seed)
    ax = np.arange(N, dtype=np.float64)
    yy, xx = np.meshgrid(ax, ax, indexing="ij")

    def step(v, at, width=1.5):
        return 1.0 / (1.0 + np.exp(-np.clip((v - at) / width, -60, 60)))

    img = 0.05 + 0.02 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 0.25 * step(xx, 0.38 * N) * step(-yy, -0.62 * N)
    B = 128                                                             # a block of cells, tiled with gains
    by, bx = np.meshgrid(np.arange(B, dtype=np.float64), np.arange(B, dtype=np.float64), indexing="ij")
    cy, cx = np.meshgrid(np.arange(8, B, 16.0), np.arange(7, B, 14.0), indexing="ij")
    cy = cy.ravel() + rng.uniform(-2, 2, cy.size)
    cx = cx.ravel() + rng.uniform(-2, 2, cx.size)
    amp = rng.uniform(0.6, 1.0, cy.size)
    sig = rng.uniform(2.6, 3.4, cy.size)
    d2 = (by[..., None] - cy) ** 2 + (bx[..., None] - cx) ** 2
    blk = (amp * np.exp(-d2 / (2 * sig ** 2))).sum(axis=2)
    kind_blk = np.argmin(d2, axis=2) % 6
    t = -(-N // B)
    gain = rng.uniform(0.7, 1.0, (t, 1, t, 1))
    cells = (blk.reshape(1, B, 1, B) * gain).reshape(t * B, t * B)[:N, :N]
    kind = np.tile(kind_blk, (t, t))[:N, :N]
    img += cells * (xx > 0.38 * N + 8) * (yy < 0.62 * N - 8)
    img += 0.14 * np.exp(-(((yy - 0.95 * N) / (0.14 * N)) ** 4 + ((xx - 0.7 * N) / (0.2 * N)) ** 4))
    img *= 1.0 + 0.02 * rng.standard_normal((N, N))
    sp = np.random.default_rng(5).random((6, CHANNELS)) ** 2 + 0.05
    sp /= sp.sum(axis=1, keepdims=True)
    out = np.empty((N, N, CHANNELS), np.float32)
    for r0 in range(0, N, 256):                                         # by row bands: the f64 product is large
        out[r0:r0 + 256] = img[r0:r0 + 256, :, None] * sp[kind[r0:r0 + 256]]
    return out


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


class Clock:
    def __init__(self, sync):
        self.ms = {}
        self.sync = sync

    def __call__(self, name, fn):
        self.sync()
        t = time.perf_counter()
        out = fn()
        self.sync()
        self.ms[name] = self.ms.get(name, 0.0) + (time.perf_counter() - t) * 1e3
        return out


DISK_STAGES = ("closing: dilation by the disk (:408)", "closing: erosion by the disk (:408)",
               "dilation by the disk (:413)")


def staged(stack, radius, bkg_min_size):
    """pipeline.segment_biofilm_2d's calls, one by one under the clock -> (per-stage ms, stats, results)"""
    import torch
    from hiprfish_image_analysis_amd import kernels as K
    ck = Clock(torch.cuda.synchronize)
    s = ck("channel sum, / max (:347-348)", lambda: K.channel_sum(stack))
    norm = ck("channel sum, / max (:347-348)", lambda: K.div_scalar(s, K.max_f64(s)))
    nl = ck("NL-means (:350)", lambda: K.nl_means_2d(norm, 7, 11, 0.02, 0.0))
    ck("count of nl <= 0", lambda: K.count_nonzero(~(nl > 0)))
    final = ck("pad, line profiles, image_final (:351-366)", lambda: K.enhance_2d(K.pad_edge(nl, 5)))
    rough = ck("kmeans image_final (:367-377)", lambda: K.kmeans_1d(final, 2, want_labels=False, rule=1)[1])
    opened = ck("opening, rso 10 (:378-379)", lambda: K.remove_small_objects(K.binary_opening(rough), 10, conn=1))
    wm0 = ck("fill_holes x2, product (:380-382)", lambda: K.and_mask(K.fill_holes(opened), K.fill_holes(rough)))
    nl_log = ck("log10 (:383)", lambda: K.log10(nl))
    blabels = ck("kmeans log10 (:384)", lambda: K.kmeans_1d(nl_log, 2, want_labels=True)[0])

    def rule():
        sums, counts = K.cluster_positive_means(blabels, s, 2)
        i0, i1 = (sums / counts.double()).tolist()
        return (blabels == (1 if i0 < i1 else 0)).to(torch.uint8)
    bkg = ck("cluster means, mask (:385-392)", rule)
    fb, sb = ck("products, rso 10 (:393-396)", lambda: (K.mask_mul(nl, bkg), K.mask_mul(s, bkg)))
    wmask = ck("products, rso 10 (:393-396)", lambda: K.remove_small_objects(K.and_mask(wm0, bkg), 10, conn=1))
    seeds, nseeds = ck("label (:397)", lambda: K.label(wmask, conn=2))
    fmask = ck("products, rso 10 (:393-396)", lambda: K.and_mask(rough, bkg))
    t1, t2, t3 = [], [], []
    ws = ck("watershed (:399)", lambda: K.watershed(fb, seeds, fmask, negate=True, ties=t1))
    aws = ck("adjacency watershed (:400)", lambda: K.watershed(sb, seeds, bkg, negate=True, ties=t2))
    seg, n = ck("relabel_sequential x2 (:401-402)", lambda: K.relabel_sequential(ws, nseeds))
    adj, n_adj = ck("relabel_sequential x2 (:401-402)", lambda: K.relabel_sequential(aws, nseeds))
    ib = ck("bkg == 0, rso, fill_holes (:404-406)",
            lambda: K.fill_holes(K.remove_small_objects(bkg == 0, bkg_min_size, conn=1)))
    H, W = ib.shape
    from hiprfish_image_analysis_amd import _lib
    work = torch.empty(int(_lib.lib().hrf_disk_workspace_bytes(H, W, radius)), dtype=torch.uint8, device="cuda")
    dil = ck(DISK_STAGES[0], lambda: K.binary_dilation_disk(ib, radius, work=work))
    closed = ck(DISK_STAGES[1], lambda: K.binary_erosion_disk(dil, radius, 1, work=work))
    objects, nobj = ck("label, largest (:409-412)", lambda: K.label(closed, conn=2))
    big = ck("label, largest (:409-412)", lambda: K.largest_label(objects, nobj)[0])
    bfin = (objects == big).to(torch.uint8)
    bd = ck(DISK_STAGES[2], lambda: K.binary_dilation_disk(bfin, radius, work=work))
    overall, nover = ck("label 1 - bd (:414)", lambda: K.label(1 - bd, conn=2))
    oseg = ck("unmasked watershed (:415)", lambda: K.watershed(s, overall, None, negate=True, ties=t3))
    epi = ck("largest, compare (:416-418)", lambda: (oseg != K.largest_label(oseg, nover)[0]).to(torch.uint8))
    total = sum(ck.ms.values())
    disk = sum(ck.ms[k] for k in DISK_STAGES)
    stats = dict(cells=n, adjacency_cells=n_adj, objects_overall=nover, total_ms=total, disk_ms=disk,
                 disk_share=disk / total, nl_means_ms=ck.ms["NL-means (:350)"], ties=t1, ties_adjacency=t2,
                 ties_epithelial=t3, bkg_fraction=float(ib.float().mean()), epithelial_fraction=float(epi.float().mean()))
    # the disk kernels alone, on the chain's own masks (a second, warm call each)
    alone = Clock(torch.cuda.synchronize)
    alone("dilation of the filled background", lambda: K.binary_dilation_disk(ib, radius, work=work))
    alone("erosion (border 1) of its dilation", lambda: K.binary_erosion_disk(dil, radius, 1, work=work))
    alone("erosion (border 0) of its dilation", lambda: K.binary_erosion_disk(dil, radius, 0, work=work))
    alone("dilation of the largest component", lambda: K.binary_dilation_disk(bfin, radius, work=work))
    ones, zeros = torch.ones_like(ib), torch.zeros_like(ib)
    alone("dilation of an all-set mask (pass A + first-ballot pass B)",
          lambda: K.binary_dilation_disk(ones, radius, work=work))
    alone("dilation of an empty mask (pass B runs all 2 r + 1 offsets)",
          lambda: K.binary_dilation_disk(zeros, radius, work=work))
    return ck.ms, stats, alone.ms, dict(seg=seg, adj=adj, epi=epi)


def report(title, ms, stats=None):
    print(title)
    for k, v in ms.items():
        print("  %-62s %10.3f ms" % (k, v))
    if stats:
        print("  " + "  ".join("%s=%s" % (k, ("%.3f" % v) if isinstance(v, float) else v) for k, v in stats.items()))


def host_chain(stack, radius, bkg_min_size):
    import scipy.ndimage as ndi
    import biofilm2d_ref as R

    def dilate(m, r):
        return ndi.binary_dilation(m, structure=R.disk(r))
    t = time.perf_counter()
    d = ndi.binary_dilation(np.zeros(stack.shape[:2], bool), structure=R.disk(radius))
    empty_ms = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    out = R.segment_biofilm_2d_ref(stack, disk_radius=radius, bkg_min_size=bkg_min_size, dilate=dilate)
    ms = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    R.segment_biofilm_2d_ref(stack, epithelial=False)
    ms_noepi = (time.perf_counter() - t) * 1e3
    assert not d.any()
    return dict(ms=ms, ms_without_epithelial=ms_noepi, scipy_dilation_of_empty_mask_ms=empty_ms, cells=out[1],
                sha1=dict(seg=digest(out[0]), adj=digest(out[2]), epi=digest(out[6].astype(np.uint8))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--small", type=int, default=512)
    ap.add_argument("--radius", type=int, default=100)
    ap.add_argument("--bkg-min-size", type=int, default=10000)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    res = {}
    if not a.host_only:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("time_segment_biofilm2d: no device")
        from hiprfish_image_analysis_amd import pipeline as P
        for key, N in (("device_small", a.small), ("device", a.size)):     # the small size first
            stack = torch.from_numpy(field(N)).cuda()
            P.segment_biofilm_2d(stack, disk_radius=a.radius, bkg_min_size=a.bkg_min_size)   # warm-up
            ms, stats, alone, arrays = staged(stack, a.radius, a.bkg_min_size)
            stats["Mpixel_per_s"] = N * N / stats["total_ms"] / 1e3
            report("device chain %d x %d x %d, disk radius %d" % (N, N, CHANNELS, a.radius), ms, stats)
            report("disk kernels alone, %d x %d, radius %d" % (N, N, a.radius), alone)
            sha = {k: digest(v.cpu().numpy()) for k, v in arrays.items()}
            print("  sha1 " + "  ".join("%s=%s" % kv for kv in sha.items()))
            res[key] = dict(size=N, stages_ms=ms, disk_alone_ms=alone, sha1=sha, **stats)
            del stack, arrays
    if not a.no_host:
        h = host_chain(field(a.small), a.radius, a.bkg_min_size)
        print("host chain %d x %d (oracle restatement, scipy.ndimage disk morphology), once: %.0f ms; without the "
              "epithelial stages %.0f ms; scipy's dilation of an empty mask by disk(%d) %.0f ms"
              % (a.small, a.small, h["ms"], h["ms_without_epithelial"], a.radius, h["scipy_dilation_of_empty_mask_ms"]))
        print("  sha1 " + "  ".join("%s=%s" % kv for kv in h["sha1"].items()))
        if "device_small" in res:
            h["equal"] = h["sha1"] == res["device_small"]["sha1"]
            print("  label maps and epithelial area equal the device's: %s" % h["equal"])
        res["host"] = h
    print(json.dumps(res))


if __name__ == "__main__":
    main()
