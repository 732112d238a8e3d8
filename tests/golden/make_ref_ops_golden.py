"""Generates tests/golden/ref_cpu_ops.npz: the reference's own CPU nms / roi_align (oracle/_ref/libmmcv_ref.so, built by
`python oracle/build_ref.py <reference checkout>`) on the cases of tests/test_oracle_vs_ref.py.
Run from the repository root: `python tests/golden/make_ref_ops_golden.py`."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import cref  # noqa: E402
from tests import test_oracle_vs_ref as T  # noqa: E402

if __name__ == "__main__":
    if not cref.ref_available():
        raise SystemExit("oracle/_ref/libmmcv_ref.so is not built (python oracle/build_ref.py <reference checkout>)")
    out = T.reference_outputs()
    assert all(v is not None for v in out.values())
    np.savez_compressed(T.GOLDEN, **out)
    print("wrote", T.GOLDEN, {k: v.shape for k, v in out.items()})
