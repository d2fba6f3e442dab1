"""Case table of the full-attention fixtures (`attention: "full"` in loftr_coarse and loftr_fine; transformer.py:32-40).
Shared by tests/golden/gen_full_attention_golden.py (the only reader of the reference) and the tests."""
import torch

from onepose_plus_plus_amd.config import default_config
from onepose_plus_plus_amd.synthetic import make_state_dict, make_inputs

# name -> (L image tokens, N points, input seed, q_proj / k_proj weight factor of every loftr_coarse layer)
FULLATTN_TRANSFORMER_CASES = {
    "fullattn_transformer_l4096_n5000": (4096, 5000, 8, 1.0),
    # peaked softmax (most row maxima > 0.5): exercises the online-max rescaling; the generator prints the share.  Factor 2, not more:
    # at 3 the reference's own fp32 result is 9e-5 (relative) away from an fp64 evaluation, above the 5e-5 bar of the GPU test
    "fullattn_sharp_transformer_l1024_n3000": (1024, 3000, 9, 2.0),
}
# name -> (hw, n points, thr, weight seed, input seed, fine matching)   (as tests/golden/cases.py E2E_CASES)
FULLATTN_E2E_CASES = {
    "fullattn_e2e_128x128_n300_thr0": ((128, 128), 300, 0.0, 0, 1, True),
    "fullattn_e2e_512x512_n2000_thr0": ((512, 512), 2000, 0.0, 0, 1, True),
    "fullattn_e2e_512x512_n5000_coarse": ((512, 512), 5000, 0.0, 0, 1, False),
}
# name -> (hw, n points, thr, weight seed, per-sample input seeds)   B > 1, no mask
FULLATTN_BATCH_CASES = {
    "fullattn_e2e_b2_128x128_n300": ((128, 128), 300, 0.0, 0, [1, 5]),
}


def full_config(cfg, coarse=True, fine=True):
    """cfg with FullAttention selected at the given levels (any value but "linear" selects it upstream)"""
    if coarse:
        cfg["loftr_coarse"]["attention"] = "full"
    if fine:
        cfg["loftr_fine"]["attention"] = "full"
    return cfg


def scale_qk(sd, factor, prefix="loftr_coarse."):
    """state dict with every q_proj / k_proj weight of the given transformer scaled by `factor`"""
    sd = dict(sd)
    if factor != 1.0:
        for k in list(sd):
            if k.startswith(prefix) and (".q_proj." in k or ".k_proj." in k):
                sd[k] = sd[k] * factor
    return sd


def fullattn_transformer_setup(name):
    """-> cfg, state dict, tokens2d [1, L, 256], bank [1, 256, N] of a loftr_coarse-alone case"""
    from tests.helpers import transformer_inputs
    L, n, seed, factor = FULLATTN_TRANSFORMER_CASES[name]
    cfg = full_config(default_config())
    sd = scale_qk(make_state_dict(cfg, 0), factor)
    tokens2d, bank = transformer_inputs(L, n, seed)
    return cfg, sd, tokens2d, bank


def fullattn_e2e_setup(name):
    hw, n, thr, wseed, iseed, fine = FULLATTN_E2E_CASES[name]
    cfg = full_config(default_config(thr=thr, fine=fine))
    return cfg, make_state_dict(cfg, wseed), make_inputs(n, hw, iseed)


def fullattn_batch_setup(name):
    """B > 1 without a mask, distinct image scales and keypoint extents (as tests/helpers.py batch_setup)"""
    hw, n, thr, wseed, seeds = FULLATTN_BATCH_CASES[name]
    cfg = full_config(default_config(thr=thr))
    sd = make_state_dict(cfg, wseed)
    parts = [make_inputs(n, hw, s) for s in seeds]
    data = {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}
    B = len(seeds)
    data["query_image_scale"] = torch.tensor([[1.0 + 0.25 * b, 1.0 - 0.125 * b] for b in range(B)])
    data["keypoints3d"] = data["keypoints3d"] * torch.tensor([1.0 + 0.5 * b for b in range(B)]).view(B, 1, 1)
    return cfg, sd, data
