"""sha256 of what `opp_coarse_match` gives on the cases x legs of tests/golden/score_gemm_cases.py, taken from the build that PRECEDES
the shared tile setup, K stage and epilogues of csrc/gemm_ss.hip (three kernels that each restated them): tests/test_score_gemm_gpu.py
holds the present kernels to these digests bit for bit.  Needs a GPU and that build:

    OPP_HIP_LIB=<libopp_hip.so of the preceding commit> OPP_ALLOW_STALE_LIB=1 python tests/golden/gen_score_gemm_digest.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.golden import score_gemm_cases as SC  # noqa: E402

if __name__ == "__main__":
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), SC.PARENT_DIGEST + ".npz")
    out = {}
    for k, v in SC.all_digests().items():
        assert not k.endswith(".skip"), (k, v)
        out[k] = np.array(v)
        print(k, v)
    np.savez_compressed(out_path, **out)
