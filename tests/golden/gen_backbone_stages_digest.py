"""sha256 of what `opp_forward_coarse` + the fine level (dense fine map inside the call, no overlap) and `opp_backbone` give on the cases
of tests/golden/backbone_stages_cases.py, taken from the build that PRECEDES the named backbone stages of csrc/api.hip (one backbone_impl
behind a phase number): tests/test_backbone_stages_gpu.py holds the present host driver to these digests bit for bit.  Needs a GPU and that build:

    OPP_HIP_LIB=<libopp_hip.so of the preceding commit> OPP_ALLOW_STALE_LIB=1 python tests/golden/gen_backbone_stages_digest.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.golden import backbone_stages_cases as BC  # noqa: E402

if __name__ == "__main__":
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), BC.PARENT_DIGEST + ".npz")
    out = {}
    for precision, hw in BC.LEGS:
        for k, v in BC.digests(precision, hw).items():
            out[k] = np.array(v)
            print(k, v)
    np.savez_compressed(out_path, **out)
