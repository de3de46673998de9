"""Generate tests/golden/mosaic.npz from the reference's own lines (run by hand, where the reference
checkout is available and oracle/build_ref.sh has built oracle/_ref):

    python tests/golden/make_mosaic_golden.py <reference root>

hiprfish-image-analysis-biofilm/hiprfish_imaging_biofilm_analysis.py is read at generation time
and two fragments are executed as they stand, taken by text slice (the file as a whole does not
parse): get_registered_image_from_tstack_tile (:203-236) and the body of
generate_3d_segmentation_tile_memory_efficient from :1066 to :1126 (dedented) -- tile sums and
masks, neighbour shifts, placement, accumulation, normalisation, padding and the chunked `+ 1e-8`
enhancement.  A third run executes :1112-1125 alone on a free-standing chunk.

Stubs: load_image_zstack_fixed_t_tile and get_t_range serve the generated time points (as f64),
get_tile_size the mosaic's side, skimage.feature.register_translation is
oracle.register_translation (the numpy restatement of skimage's integer path), skimage.util.pad
is numpy.pad and line_profile_v2 is the reference's own Cython from oracle/_ref.

The second fragment hard-codes the acquisition's sizes.  Exactly these NUMBER tokens are rewritten
(by tokenize, never by substring) before it is executed, and each must occur:

    500  -> T          the tile's side (tiles are square)
    450  -> T - ov
    50   -> ov         the overlap
    150  -> Tz
    2020 -> n T + 20   the canvas side
    170  -> Tz + 20
    100  -> chunk
    20   -> the chunk count per side

The margin 10, the chunk halo 10, the pad 5 and the line-profile parameters stay as written.

Only arrays are written: the inputs (uint8: integer valued, below 256), the shifts the stub
returned and the fragments' results.  No reference text enters the fixture.  The origins recorded
are the restatement's; the fragment keeps none, and `full` and `count` equal to the fragment's pin
them.  Two conditions are asserted here: every strip correlation's peak is at least 1.05 times its
runner-up, so that FFT rounding cannot move an argmax, and some neighbour shift is non-zero on
each axis."""
import io
import os
import sys
import tokenize
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), os.path.join(REPO, "oracle"), os.path.join(REPO, "oracle", "_ref")):
    sys.path.insert(0, p)

import oracle as O  # noqa: E402
import mosaic_ref as MR  # noqa: E402

BIOF = "hiprfish-image-analysis-biofilm/hiprfish_imaging_biofilm_analysis.py"


def fragment(lines, first, last, dedent=0):
    return "".join(l[dedent:] if l.strip() else l for l in lines[first - 1:last])


def rewrite_numbers(src, table):
    """replace NUMBER tokens by `table`; every key must occur"""
    seen = set()
    toks = []
    for tok in tokenize.generate_tokens(io.StringIO(src).readline):
        if tok.type == tokenize.NUMBER and tok.string in table:
            seen.add(tok.string)
            tok = tok._replace(string=str(table[tok.string]))
        toks.append((tok.type, tok.string))
    missing = sorted(set(table) - seen)
    assert not missing, "tokens not found: %s" % missing
    return tokenize.untokenize(toks)


def main(ref_root):
    import neighbor  # the reference's Cython (oracle/build_ref.sh)

    lines = open(os.path.join(ref_root, BIOF)).readlines()
    g = MR.GOLDEN
    n, (T, Ty, Tz), ov, m = g["n"], g["tile"], g["ov"], g["margin"]
    assert T == Ty and m == 10
    assert g["nchunk"] == (n * T + 20) // g["chunk"]      # the reference's 2020 // 100 = 20
    tiles = MR.golden_case()
    calls = []

    def register_translation(a, b):
        s = O.register_translation(a, b)
        calls.append(np.array(s, np.int32))
        return s, 0.0, 0.0

    skimage = types.SimpleNamespace(feature=types.SimpleNamespace(register_translation=register_translation),
                                    util=types.SimpleNamespace(pad=np.pad))
    ns = dict(np=np, skimage=skimage, print=lambda *a, **k: None, image_name="s_561.czi",      # :1065
              line_profile_v2=neighbor.line_profile_v2, get_tile_size=lambda f: n,
              get_t_range=lambda f: len(tiles[0]),
              load_image_zstack_fixed_t_tile=lambda f, t, tile: tiles[tile][t].astype(np.float64))
    exec(fragment(lines, 203, 236), ns)
    table = {"500": T, "450": T - ov, "50": ov, "150": Tz, "2020": n * T + 20, "170": Tz + 20, "100": g["chunk"],
             "20": g["nchunk"]}
    exec(rewrite_numbers(fragment(lines, 1066, 1126, dedent=4), table), ns)

    out = {}
    nt = len(tiles[0])
    for k, ts in enumerate(tiles):
        for t, a in enumerate(ts):
            assert a.min() >= 0 and a.max() < 256 and np.array_equal(a, np.floor(a))
            out["in_k%d_t%d" % (k, t)] = a.astype(np.uint8)
    per_tile = (nt - 1)
    for k in range(n * n):
        out["t_shifts_k%d" % k] = np.stack([np.zeros(3, np.int32)] + calls[k * per_tile:(k + 1) * per_tile])
        out["sum_filtered_k%d" % k] = ns["image_sum_filtered_list"][k]
        out["mask_k%d" % k] = ns["shift_filter_mask_list"][k].astype(np.uint8)
    assert len(calls) == n * n * per_tile + n * n - 1
    shifts = ns["shift_vector_full"]
    assert np.array_equal(shifts, np.round(shifts))
    out["shifts"] = shifts.astype(np.int32)
    out["full"] = ns["image_full"]
    out["count"] = ns["image_overlap_full"].astype(np.int32)
    out["norm"] = ns["image_norm"]
    out["final"] = ns["image_final"]

    # the conditions on the case, and the restatement's origins pinned by the fragment's canvas
    sums = [out["sum_filtered_k%d" % k] for k in range(n * n)]
    ratios = [MR.peak_ratio(a, b) for _, a, b in MR.strip_pairs(sums, n, ov)]
    print("strip peak / runner-up:", " ".join("%.3f" % r for r in ratios))
    assert min(ratios) >= 1.05
    assert all(np.abs(out["shifts"][..., a]).max() > 0 for a in range(3)), out["shifts"]
    org, canvas = MR.origins(out["shifts"], (T, Ty, Tz), ov, m)
    full, count = MR.accumulate(sums, [out["mask_k%d" % k] for k in range(n * n)], org, canvas)
    assert np.array_equal(full, out["full"]) and np.array_equal(count, out["count"])
    out["origins"] = org
    print("shifts", out["shifts"].reshape(-1, 3).tolist(), "origins", org.tolist(), "canvas", canvas)
    print("count values", np.unique(out["count"]).tolist(), " final non-zero %d of %d" % (
        int((out["final"] != 0).sum()), out["final"].size))

    # :1112-1125 alone
    chunk = MR.enhance_chunk_case()
    es = dict(np=np, line_profile_v2=neighbor.line_profile_v2, image_chunk=chunk)
    exec(fragment(lines, 1112, 1125, dedent=12), es)
    out["e_chunk"] = chunk
    out["e_final"] = es["image_final_chunk"]

    path = os.path.join(HERE, "mosaic.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main(sys.argv[1])
