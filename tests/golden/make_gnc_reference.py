"""Writes tests/golden/gnc_reference.npz on the CPU: the restated runs of graduated non-convexity (tests/gnc_restatement.run) on
the inputs of tests/gnc_inputs.py, TLS and GM, from the start and from the perturbed start.  tests/test_gnc_host.py checks
the file against the restatement; the GPU tests read it, so that none of them waits for a restated run.

    python tests/golden/make_gnc_reference.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import gnc_inputs as gi  # noqa: E402

if __name__ == "__main__":
    out = {}
    for name in gi.CASES:
        for kind in (0, 1):
            out.update(gi.pack(name, kind, gi.compute(name, kind)))
            print(name, kind, "done", flush=True)
    np.savez_compressed(os.path.join(HERE, "gnc_reference.npz"), **out)
