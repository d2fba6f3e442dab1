"""sha256 of the keypoint encoder's output (`opp_encode_points`, default config = no norm affine) on the inputs of
tests/golden/encopt_cases.py `kpt_kernel_inputs`, taken from the build that PRECEDES the optional LayerNorm affine of kpt_encode_kernel:
the test holds the present kernel, called with null affine pointers, to these digests bit for bit.  Needs a GPU and that build:

    OPP_HIP_LIB=<libopp_hip.so of the preceding commit> OPP_ALLOW_STALE_LIB=1 python tests/golden/gen_encoder_options_kpt_digest.py [out.npz]
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from onepose_plus_plus_amd.config import default_config  # noqa: E402
from onepose_plus_plus_amd.synthetic import make_state_dict  # noqa: E402
from tests import hip_ops as ops  # noqa: E402
from tests import mask_cases as MC  # noqa: E402
from tests.golden import encopt_cases as EC  # noqa: E402

if __name__ == "__main__":
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), EC.KPT_PARENT_DIGEST + ".npz")
    cfg = default_config()
    model = ops.make_model(cfg, make_state_dict(cfg, 5))
    out = {}
    for n in EC.KPT_KERNEL_SIZES:
        kpts, bank = EC.kpt_kernel_inputs(n)
        tok = ops.encode_points(model, kpts, bank, extent_ref=MC.kpt_extent_cloud() if n == 1 else None)
        assert np.isfinite(tok.numpy()).all()
        out["n%d" % n] = np.array(hashlib.sha256(tok.contiguous().numpy().tobytes()).hexdigest())
        print(n, out["n%d" % n])
    np.savez_compressed(out_path, **out)
