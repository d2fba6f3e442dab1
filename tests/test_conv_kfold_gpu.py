"""The K slices of a long-K bf16x3 convolution summed inside one 128 x 128 workgroup per tile (gemm_mfma.hip, opp_gemm_kfold_kernel): taken
under the throughput tile policy where K / 32 is a multiple of 8, instead of four K-slice workgroups + splitk_epilogue_kernel.  Same bits:
the digests of the build that preceded the named backbone stages (tests/golden/backbone_stages_parent_digest.npz) and the latency-policy
run.  At these image sizes every 3 x 3 convolution of the backbone is split by shape; the ones of 56 and 72 chunks (layer3 among them, over
one row tile at 64 x 96 and two at 136 x 104) fold, the ones of 36 chunks (layer1, layer2.0.conv1: slices of 9) keep the slices."""
import ctypes
import os

import pytest
import torch

from tests import helpers as H
from tests import hip_ops as ops
from tests.golden import backbone_stages_cases as BC

pytestmark = pytest.mark.gpu

PROF_CONV_SPLITK, PROF_SPLITK_EPILOGUE = 1014, 1015     # csrc/opp_internal.h
# K chunks (opp_conv_packed_k / 32) of the backbone's 3 x 3 convolutions in launch order: layer1 (4), layer2 (4), layer3 (4),
# layer2_outconv2 (2), layer1_outconv2 (2); 196 input channels pack to 6 x 9 + 2 = 56 chunks
CHUNKS = (36, 36, 36, 36, 36, 56, 56, 56, 56, 72, 72, 72, 72, 72, 56, 56)
N_SPLIT = len(CHUNKS)
N_FOLD = sum(1 for c in CHUNKS if c % 8 == 0)
LEGS = [leg for leg in BC.LEGS if leg[0] == "bf16x3"]


def _launches(m, data, symbol):
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    _lib.check(lib.opp_profile_start(symbol, 0, 256), "profile_start")
    try:
        BC.run_pattern(m, data, "dense")
        torch.cuda.synchronize()
    finally:
        n = ctypes.c_int(0)
        _lib.check(lib.opp_profile_stop(None, None, ctypes.byref(n)), "profile_stop")
    return n.value


@pytest.fixture(scope="module", params=LEGS, ids=BC.leg_id)
def runs(request):
    precision, hw = request.param
    cfg, sd, data = BC.setup(hw)
    out = {}
    for policy in ("throughput", "latency"):
        for overlap in (True, False):
            m = BC.make_pattern_model(cfg, sd, precision, "dense", overlap).set_tile_policy(policy)
            outs = [BC.run_pattern(m, data, "dense") for _ in range(2)]      # twice on one module
            fc, ff = ops.backbone(m, data["query_image"])
            counts = (_launches(m, data, PROF_CONV_SPLITK), _launches(m, data, PROF_SPLITK_EPILOGUE))
            os.environ["OPP_CONV_KFOLD"] = "0"
            try:
                off = BC.run_pattern(m, data, "dense")
                counts_off = (_launches(m, data, PROF_CONV_SPLITK), _launches(m, data, PROF_SPLITK_EPILOGUE))
            finally:
                del os.environ["OPP_CONV_KFOLD"]
            out[policy, overlap] = (outs + [off], fc, ff, counts, counts_off)
    return precision, hw, out


def test_outputs_equal_the_preceding_build_and_the_latency_policy(runs):
    precision, hw, out = runs
    gold = H.load_golden(BC.PARENT_DIGEST)
    pre = BC.leg_id((precision, hw))
    for case, (outs, fc, ff, _, _) in out.items():
        assert BC.sha(fc) == str(gold[pre + ".feat_c"]), case
        assert BC.sha(ff) == str(gold[pre + ".feat_f"]), case
        for i, got in enumerate(outs):
            for k in BC.MATCH_KEYS + BC.FINE_KEYS:
                assert BC.sha(got[k]) == str(gold["%s.%s" % (pre, k)]), (case, i, k)
                assert torch.equal(got[k], out["latency", False][0][0][k]), (case, i, k)


def test_which_convolutions_fold(runs):
    """one OPP_PROF_CONV_SPLITK record per split convolution either way; a reduction launch only for the ones that keep their slices"""
    _, _, out = runs
    for overlap in (True, False):
        print(overlap, out["throughput", overlap][3:], out["latency", overlap][3:])
        assert out["latency", overlap][3] == (N_SPLIT, N_SPLIT)
        assert out["latency", overlap][4] == (N_SPLIT, N_SPLIT)
        assert out["throughput", overlap][3] == (N_SPLIT, N_SPLIT - N_FOLD)       # layer3's four among the folded, layer1's four not
        assert out["throughput", overlap][4] == (N_SPLIT, N_SPLIT)                # OPP_CONV_KFOLD=0 restores the slices
