"""Generate tests/golden/report3.npz from the reference's own lines (run by hand, where the
reference checkout is available):

    python tests/golden/make_report3_golden.py <reference root>

hiprfish-image-analysis-biofilm/hiprfish_imaging_biofilm_analysis.py is read at generation time
and save_identification_bvox (:280-289) is executed as it stands, taken by text slice -- the file
as a whole does not parse (SyntaxError at :1254).  It is called on a 3 x 4 x 5 x 3 colour volume
painted from a random label volume and colour table, in a scratch directory; the fixture holds
the labels, the colour table, the volume and the bytes of the three files it wrote.  Only arrays
are written.  No reference text enters the fixture."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
BIOF = "hiprfish-image-analysis-biofilm/hiprfish_imaging_biofilm_analysis.py"


def main(ref_root):
    lines = open(os.path.join(ref_root, BIOF)).readlines()
    ns = dict(np=np)
    exec("".join(lines[280 - 1:289]), ns)
    assert "save_identification_bvox" in ns
    rng = np.random.default_rng(7)
    labels = rng.integers(0, 6, (3, 4, 5)).astype(np.int32)
    colour = np.zeros((6, 3))
    colour[1:] = rng.integers(0, 9, (5, 3)) / 8.0            # exact in f32
    image = colour[labels]                                     # (3, 4, 5, 3) f64, as :1391 holds it
    out = dict(labels=labels, colour=colour, image=image)
    with tempfile.TemporaryDirectory() as d:
        ns["save_identification_bvox"](image, os.path.join(d, "s"))
        for c in "rgb":
            out["bvox_" + c] = np.fromfile(os.path.join(d, "s_identification_%s.bvox" % c), np.uint8)
    path = os.path.join(HERE, "report3.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
