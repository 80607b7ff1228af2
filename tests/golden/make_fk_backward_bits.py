"""Maker of tests/golden/fk_backward_bits.npz: the inputs of tests/fk_bits_ref.py and what mgr_fk_backward, mgr_fk_backward_terms and
mgr_fk_backward_terms2d of the library in the tree give for them on the GPU, bit for bit.

    python -m manus_amd.build && python tests/golden/make_fk_backward_bits.py [--out FILE]

Run it on the commit whose bits are to be held (LAB.md names the one that wrote the committed file), never to make a failing
tests/test_gpu_fk_backward_golden.py pass.  Arrays only: `values` in float64, everything else in the dtype the entry takes.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    import fk_bits_ref as B
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else B.GOLDEN
    d = B.build()
    for name in B.case_names(d):
        for _ in range(2):                                                     # twice: the bits must not depend on the run
            res = {k: v.cpu().numpy() for k, v in B.call(d, name).items()}
            for k, v in res.items():
                key = "case/%s/%s" % (name, k)
                assert key not in d or np.array_equal(d[key], v, equal_nan=True), key
                d[key] = v
        print("%-34s d_theta |max| %.3e  values %s" % (name, float(np.nanmax(np.abs(res["d_theta"]))),
                                                         " ".join("%.6e" % x for x in res.get("values", []))))
    np.savez_compressed(path, **B.pack(d))
    print("%s: %d cases, %d arrays, %d bytes" % (path, len(B.case_names(d)), len(B.pack(d)), os.path.getsize(path)))


if __name__ == "__main__":
    main()
