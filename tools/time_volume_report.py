"""Time the 3-D per-cell report (biofilm.volume_report, csrc/report3.hip) kernel by kernel and whole.

python tools/time_volume_report.py [--size X Y Z] [--host-size X Y Z | --no-host] [--reps N]

* the label volumes are pipeline.segment_volume's (segmentation and adjacency_seg) on the synthetic
  blob volume of tools/time_segment_volume.py, --size (default cfg4, 1024 x 1024 x 64);
* per kernel (hrf_region_moments3, hrf_rag_edges3 at conn 2 and the default capacity,
  hrf_paint_planes3, hrf_barcode_adjacency_edges): device events around the library call on
  preallocated buffers, median and minimum of --reps after one warm-up, the algorithmic bytes
  (moments 4 V read, edges 4 V read, planes 4 V read + 12 V written) and their share of the 8 TB/s
  peak; the distinct edges and the final table load;
* volume_report's stages and the whole call (write=False, so no file is written; host clock around
  work that ends in a device synchronise, after one warm-up run of the whole report) on a random
  63-channel volume with a classifier bundle fitted here (synthetic_bundle);
* the host side at --host-size, once: the scipy restatement of the edge set plus numpy moments
  (tests/report3_ref.py), with the device kernels at the same size beside it.
One JSON line at the end.  No device: fails."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
from hiprfish_image_analysis_amd import _lib  # noqa: E402
from hiprfish_image_analysis_amd import kernels as K  # noqa: E402
from hiprfish_image_analysis_amd import pipeline as P  # noqa: E402

PEAK = 8e12   # HBM bytes per second


def synthetic_bundle(path, seed=31):
    """fit and export a community classifier bundle (four check SVCs on the scaled segments, a
    stand-in UMAP, an rbf SVC with probability=True over six 7-bit barcodes) -> (model, the sklearn
    SVC, the six (63,) class spectra); tests/test_report3_gpu.py uses it too"""
    from types import SimpleNamespace

    from sklearn.preprocessing import StandardScaler
    from sklearn.svm import SVC
    from tools.export_classifier import export_bundle
    from hiprfish_image_analysis_amd import backend as B
    rng = np.random.default_rng(seed)
    spectra = rng.random((6, 63)) ** 2 + 0.05
    y = np.repeat(np.arange(6), 30)
    xt = spectra[y] * rng.uniform(0.8, 1.2, (len(y), 1)) + rng.normal(0, 0.02, (len(y), 63))
    xt /= xt.max(axis=1, keepdims=True)
    sc = StandardScaler().fit(xt)
    xs = sc.transform(xt)
    feats = np.zeros((len(y), 67))
    feats[:, :63] = xt
    checks = []
    for k, (lo, hi) in enumerate(B.MULTI_SEGMENTS):
        seg_max = xt[:, lo:hi].max(axis=1)
        lab = np.zeros(len(y))
        lab[np.argsort(seg_max, kind="stable")[len(y) // 2:]] = 1.0      # two classes always
        checks.append(SVC(kernel="linear", C=1.0).fit(xs[:, lo:hi], lab))
        feats[:, 63 + k] = checks[-1].predict(xs[:, lo:hi])
    emb = (rng.normal(0, 5, (6, 2))[y] + rng.normal(0, 0.4, (len(y), 2))).astype(np.float32)
    codes = np.array([format(v + 1, "07b") for v in y])
    clf = SVC(kernel="rbf", gamma=0.5, C=10.0, probability=True, random_state=0).fit(emb.astype(float), codes)
    um = SimpleNamespace(_raw_data=feats, embedding_=emb, n_neighbors=15, local_connectivity=1.0,
                         metric=SimpleNamespace(__name__="channel_cosine_intensity_7b_v2"), _a=1.577, _b=0.8951,
                         repulsion_strength=1.0, negative_sample_rate=5, n_epochs=None, _initial_alpha=1.0)
    export_bundle(path, um, clf, checks, sc)
    return B.ClassifierModel.load(path), clf, spectra


def event_ms(fn, reps):
    """device milliseconds of fn() per repetition: events on the current stream, after one warm-up"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def kernels_section(seg, adj, n, reps):
    X, Y, Z = seg.shape
    V = seg.numel()
    st = torch.cuda.current_stream().cuda_stream
    dev = seg.device
    mom = torch.empty((n + 1, 4), dtype=torch.int64, device=dev)
    cap = 1 << (32 * (n + 1) - 1).bit_length()
    table = torch.empty(cap, dtype=torch.int64, device=dev)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    colour = torch.rand((n + 1, 3), device=dev)
    planes = torch.empty((3, Z, Y, X), dtype=torch.float32, device=dev)
    rows = {}

    def row(name, fn, nbytes):
        ms = event_ms(fn, reps)
        med, lo = float(np.median(ms)), float(min(ms))
        rows[name] = dict(ms_median=med, ms_min=lo, bytes=nbytes, peak_share=nbytes / (med * 1e-3) / PEAK)
        print("  %-34s %9.3f ms median %9.3f min  %8.1f MB  %5.1f %% of 8 TB/s" % (
            name, med, lo, nbytes / 1e6, 100 * rows[name]["peak_share"]))

    print("kernels %d x %d x %d, %d labels" % (X, Y, Z, n))
    row("hrf_region_moments3", lambda: _lib.call("hrf_region_moments3", seg.data_ptr(), X, Y, Z, n, mom.data_ptr(),
                                                 st), 4 * V)
    row("hrf_rag_edges3 (conn 2)", lambda: _lib.call("hrf_rag_edges3", adj.data_ptr(), X, Y, Z, 2, table.data_ptr(),
                                                     cap, info.data_ptr(), st), 4 * V)
    count, overflow = (int(v) for v in info.cpu())
    row("hrf_paint_planes3", lambda: _lib.call("hrf_paint_planes3", seg.data_ptr(), X, Y, Z, colour.data_ptr(), n,
                                               planes.data_ptr(), st), 16 * V)
    keys = torch.sort(table[table != -1]).values
    bc = torch.randint(0, 5, (n + 1,), dtype=torch.int32, device=dev)
    keep = torch.randint(0, 2, (n + 1,), dtype=torch.uint8, device=dev)
    a1 = torch.empty((5, 5), dtype=torch.int64, device=dev)
    a2 = torch.empty((5, 5), dtype=torch.int64, device=dev)
    row("hrf_barcode_adjacency_edges", lambda: _lib.call("hrf_barcode_adjacency_edges", keys.data_ptr(), keys.numel(),
                                                         bc.data_ptr(), keep.data_ptr(), n, 5, a1.data_ptr(),
                                                         a2.data_ptr(), st), 8 * keys.numel())
    ms = event_ms(lambda: K.rag_edges3(adj), reps)
    rows["kernels.rag_edges3 (build, read back, compact, sort)"] = dict(ms_median=float(np.median(ms)))
    print("  kernels.rag_edges3 with its read-back, compaction and sort: %.3f ms median" % float(np.median(ms)))
    print("  distinct edges %d (%d with the background), capacity %d, load %.4f, overflow %d" % (
        int((keys >> 32 >= 1).sum()), count, cap, count / cap, overflow))
    return dict(shape=(X, Y, Z), labels=n, voxels=V, rows=rows, edges=count, capacity=cap, load=count / cap,
                overflow=overflow)


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


def report_section(seg, adj, n, model, taxon_codes):
    from hiprfish_image_analysis_amd import biofilm
    X, Y, Z = seg.shape
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    stack = torch.rand((X, Y, Z, 63), generator=g, device="cuda", dtype=torch.float32)
    biofilm.volume_report("timing", stack, seg, adj, model, taxon_codes, write=False)     # warm-up
    ck = Clock()
    sums, counts = ck("label_sums (:1363-1367)", lambda: K.label_sums(stack.reshape(X * Y, Z, 63),
                                                                      seg.reshape(X * Y, Z), n))
    _, labels, _, avgn = ck("cell_table (:1368)", lambda: K.cell_table(sums, counts, n))

    def chain():
        feats = model.features(avgn)
        emb = model.umap.transform(feats).double()
        return model.svc.predict(emb), model.svc.predict_proba(emb)

    cls, prob = ck("classifier chain (:1369-1377)", chain)
    maxp = prob.max(dim=1).values
    ck("region_props3 (:1381-1386)", lambda: K.region_props3(seg, n))
    bc = torch.randint(0, len(taxon_codes), (labels.numel(),), dtype=torch.int32, device="cuda")
    ck("typing + edge set + adjacency (:1411)", lambda: P.biofilm_typing_and_adjacency3(
        seg, adj, bc, len(taxon_codes), maxp, prob_min=0.5))
    code = torch.randint(1, 64, (n,), dtype=torch.int32, device="cuda")
    ck("paint_ids x 2 (:1392-1396)", lambda: (K.paint_ids(seg, code), K.paint_ids(seg, code)))
    colour = torch.rand((n + 1, 3), device="cuda")
    ck("paint_planes3 x 2 (:280-289)", lambda: (K.paint_planes3(seg, colour), K.paint_planes3(seg, colour)))
    whole = Clock()
    whole("volume_report(write=False)", lambda: biofilm.volume_report("timing", stack, seg, adj, model, taxon_codes,
                                                                      write=False))
    print("volume_report %d x %d x %d x 63, %d cells" % (X, Y, Z, labels.numel()))
    for k, v in list(ck.ms.items()) + list(whole.ms.items()):
        print("  %-40s %10.2f ms" % (k, v))
    del stack
    return dict(stages_ms=ck.ms, stages_total_ms=sum(ck.ms.values()), whole_ms=whole.ms["volume_report(write=False)"],
                cells=int(labels.numel()))


def host_section(seg, adj, n):
    import report3_ref as R3
    hs, ha = seg.cpu().numpy(), adj.cpu().numpy()
    t = time.perf_counter()
    keys = R3.rag_edges3(ha, 2)
    t_edges = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    mom = R3.moments3(hs, n)
    t_mom = (time.perf_counter() - t) * 1e3
    same = bool(np.array_equal(K.rag_edges3(adj).cpu().numpy(), keys) and
                np.array_equal(K.region_moments3(seg, n).cpu().numpy(), mom))
    print("host %d x %d x %d, once: scipy edge set %.0f ms, numpy moments %.0f ms; equal to the device: %s" % (
        tuple(seg.shape) + (t_edges, t_mom, same)))
    return dict(edges_ms=t_edges, moments_ms=t_mom, equal=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[1024, 1024, 64])
    ap.add_argument("--host-size", type=int, nargs=3, default=[256, 256, 64])
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_volume_report: no device")
    from tools.time_segment_volume import blob_volume
    with tempfile.TemporaryDirectory() as d:
        model, _, _ = synthetic_bundle(os.path.join(d, "bundle.npz"))
    taxon_codes = [format(v + 1, "07b") for v in range(5)]
    res = {}
    # the small size first, so a run cut short still reports it
    for key, shape in ((("host_size", tuple(a.host_size)),) if not a.no_host else ()) + (("size", tuple(a.size)),):
        final, reg = blob_volume(shape)
        seg, n, _, adj, _ = P.segment_volume(final, reg, adjacency=True)
        del final, reg
        r = kernels_section(seg, adj, n, a.reps)
        r["report"] = report_section(seg, adj, n, model, taxon_codes)
        if key == "host_size":
            r["host"] = host_section(seg, adj, n)
        res[key] = r
        del seg, adj
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
