"""GPU: the eval-mode backbone as named stages (csrc/api.hip: trunk, fine branch at 1/4 and at 1/2 resolution) behind every call pattern of
`opp_forward_coarse`, with the fine branch beside the coarse level (`fpn_overlap`) and on one stream.  Small images: the dense convolutions
run as K slices there, the case in which the two split-K scratch buffers of the overlapping branches matter.  Host code only decides
what is launched where, so the bar is equality: between the patterns, and with the build that preceded the stages (sha256 digests)."""
import os

import pytest
import torch

from tests import helpers as H
from tests.golden import backbone_stages_cases as BC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=BC.LEGS, ids=BC.leg_id)
def runs(request):
    """every pattern x overlap setting, each run twice on one module (the side stream and its events are created by the first call
    and reused by the second)"""
    from tests import hip_ops as ops
    precision, hw = request.param
    cfg, sd, data = BC.setup(hw)
    fine = {}
    for pattern in BC.FINE_PATTERNS:
        for overlap in (True, False):
            m = BC.make_pattern_model(cfg, sd, precision, pattern, overlap)
            fine[pattern, overlap] = [BC.run_pattern(m, data, pattern) for _ in range(2)]
    trunk = {}
    for overlap in (True, False):
        for skip in (False, True):
            m = ops.make_model(BC.coarse_only(cfg), sd, precision).set_fpn_overlap(overlap).set_skip_unused_fine_map(skip).cuda()
            trunk[overlap, skip] = [ops.run_model(m, data) for _ in range(2)]
    return precision, hw, fine, trunk


def test_fine_patterns_agree_bit_for_bit(runs):
    """Dense fine map inside the call (trunk + both fine stages), per-match patches (trunk + the 1/4-resolution stage, x1 / x2_out in
    the caller's buffers) and the dense map completed afterwards (the same + `opp_backbone_fine_branch`: the 1/2-resolution stage alone):
    one set of bits, on the side stream or not, first call or second."""
    _, _, fine, _ = runs
    ref = fine["dense", False][0]
    assert len(ref["mconf"]) > 1 and ref["expec_f"].shape[0] == len(ref["mconf"])
    for case, outs in fine.items():
        for i, got in enumerate(outs):
            for k in BC.MATCH_KEYS + BC.FINE_KEYS:
                assert torch.equal(got[k], ref[k]), (case, i, k)


def test_trunk_only_equals_its_dead_map_run(runs):
    """Fine matching disabled + `set_skip_unused_fine_map(True)`: feat_f = NULL without patch buffers launches the trunk only, and every
    output equals the run that computes the dead fine map -- and the coarse level of the runs with fine matching enabled."""
    _, _, fine, trunk = runs
    for overlap in (True, False):
        ref = trunk[overlap, False][0]
        assert "expec_f" not in ref
        for got in trunk[overlap, True] + trunk[overlap, False]:
            assert set(got) == set(ref)
            for k in BC.MATCH_KEYS + ("mkpts_query_f", "mkpts_3d_db"):
                assert torch.equal(got[k], ref[k]), (overlap, k)
        for k in BC.MATCH_KEYS:
            assert torch.equal(ref[k], fine["dense", False][0][k]), (overlap, k)


def test_outputs_equal_the_preceding_build(runs):
    """tests/golden/backbone_stages_parent_digest.npz (gen_backbone_stages_digest.py, run on the build with one backbone_impl behind a phase
    number): the one-stream dense pattern and both maps of `opp_backbone` (trunk + both fine stages on one stream), bit for bit."""
    precision, hw, fine, _ = runs
    gold = H.load_golden(BC.PARENT_DIGEST)
    got = BC.digests(precision, hw)
    assert got == {k: str(gold[k]) for k in got}
    assert all(BC.sha(fine["dense", False][0][k]) == got["%s.%s" % (BC.leg_id((precision, hw)), k)] for k in BC.MATCH_KEYS + BC.FINE_KEYS)


def test_presplit_chain_beside_the_coarse_level_is_bit_identical():
    """OPP_ASP=1 (the opt-in pre-split activation chain, tests/test_stages_gpu.py): the twins the trunk decides on (x1, x2) are read by
    the fine stages on the side stream.  Same bits as the default chain."""
    precision, hw = BC.LEGS[0]
    cfg, sd, data = BC.setup(hw)
    ref = BC.run_pattern(BC.make_pattern_model(cfg, sd, precision, "dense", True), data, "dense")
    os.environ["OPP_ASP"] = "1"
    try:
        m = BC.make_pattern_model(cfg, sd, precision, "dense", True)
        outs = [BC.run_pattern(m, data, "dense") for _ in range(2)]
    finally:
        del os.environ["OPP_ASP"]
    for got in outs:
        for k in BC.MATCH_KEYS + BC.FINE_KEYS:
            assert torch.equal(got[k], ref[k]), k
