"""Generate tests/golden/volreg.npz from the reference's own lines (run by hand, where the
reference checkout is available):

    python tests/golden/make_volreg_golden.py <reference root>

hiprfish-image-analysis-biofilm/hiprfish_imaging_biofilm_analysis.py is read at generation time
and three fragments are executed as they stand: get_registered_average_image_from_tstack
(:134-165), get_t_average_image (:532-559) and the zero-fill loop of generate_3d_segmentation
(:428-449, dedented).  They are taken by text slice -- the file as a whole does not parse
(SyntaxError at :1254).  Their three outside calls are stubbed: load_image_zstack_fixed_t and
get_t_range serve the generated time points (as f64, what the reference's loader hands out) and
skimage.feature.register_translation is oracle.register_translation, the numpy restatement of
skimage's integer path.  Only arrays are written: inputs, the shifts the stub returned and the
fragments' results.  No reference text enters the fixture.

The inputs (tests/volreg_ref.py golden_case: 16 x 12 x 8, C = (3, 2, 2, 1), T = 4) are integer
valued with sums far below 2^24 and T a power of two, so the reference's f64 results are exactly
representable in the f32 this project stores."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), os.path.join(REPO, "oracle")):
    sys.path.insert(0, p)

import oracle as O  # noqa: E402
import volreg_ref as R  # noqa: E402

BIOF = "hiprfish-image-analysis-biofilm/hiprfish_imaging_biofilm_analysis.py"
EXCITATIONS = ["488", "514", "561", "633"]


def fragment(lines, first, last, dedent=0):
    return "".join(l[dedent:] if l.strip() else l for l in lines[first - 1:last])


def main(ref_root):
    lines = open(os.path.join(ref_root, BIOF)).readlines()
    tstacks = R.golden_case()
    files = {"s_%s.czi" % x: ts for x, ts in zip(EXCITATIONS, tstacks)}
    calls = []

    def register_translation(a, b):
        s = O.register_translation(a, b)
        calls.append(np.array(s, np.int32))
        return s, 0.0, 0.0

    skimage = types.SimpleNamespace(feature=types.SimpleNamespace(register_translation=register_translation))
    ns = dict(np=np, skimage=skimage, os=os, print=lambda *a, **k: None,
              load_image_zstack_fixed_t=lambda f, t: files[os.path.basename(f)][t].astype(np.float64),
              get_t_range=lambda f: len(files[os.path.basename(f)]))
    exec(fragment(lines, 134, 165), ns)
    exec(fragment(lines, 532, 559), ns)
    assert "get_registered_average_image_from_tstack" in ns and "get_t_average_image" in ns

    out = {}
    for l, ts in enumerate(tstacks):
        for t, a in enumerate(ts):
            out["in_l%d_t%d" % (l, t)] = a
    T = len(tstacks[0])
    avg = []
    for l, x in enumerate(EXCITATIONS):
        del calls[:]
        avg.append(ns["get_registered_average_image_from_tstack"]("s_%s.czi" % x))
        out["avg_l%d" % l] = avg[-1]
        out["tshifts_l%d" % l] = np.stack([np.zeros(3, np.int32)] + calls)
        assert len(calls) == T - 1
    del calls[:]
    out["keep"] = ns["get_t_average_image"]("s")
    out["lshifts"] = np.stack([np.zeros(3, np.int32)] + calls[-(len(EXCITATIONS) - 1):])

    # :428-449 on the same averaged lasers and shift vectors (:425-427 restated: there the sums
    # come from t-stacked 5-D arrays, out of scope here)
    zs = dict(np=np, print=lambda *a, **k: None, image_stack=[a.copy() for a in avg],
              shift_vectors=[np.zeros(3)] + [s.astype(np.float64) for s in out["lshifts"][1:]])
    exec(fragment(lines, 428, 449, dedent=4), zs)
    out["zero"] = np.concatenate(zs["image_registered"], axis=3)

    for k in ("keep", "zero") + tuple("avg_l%d" % l for l in range(len(avg))):
        assert out[k].dtype == np.float64 and np.array_equal(out[k].astype(np.float32).astype(np.float64), out[k]), k
    path = os.path.join(HERE, "volreg.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
