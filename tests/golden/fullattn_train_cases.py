"""Case table of the full-attention TRAINING fixtures (`attention: "full"`, the reference module in train() mode with gradients).
Shared by tests/golden/gen_full_attention_train_golden.py (the only reader of the reference) and the tests."""
import torch

from onepose_plus_plus_amd.config import default_config
from onepose_plus_plus_amd.synthetic import make_state_dict, make_inputs
from tests.golden.fullattn_cases import full_config

# name -> ((hw, n, thr, weight seed, input seeds, n_gt per sample, train_coarse_percent, pad min), (coarse full, fine full))
# the sizes of tests/golden/encopt_cases.py ENCOPT_TRAIN_CASES with the threshold of train_b4_64x96_n150 (0.0: the default feature
# normalisation).  L = 8 x 12 = 96 image tokens and N = 150 points are the smallest sizes
# that give the 64-row tiles of csrc/full_attention_train.hip a full tile, a half tile (96 = 64 + 32) and a 22-row tail (150 = 128 + 22)
FULLATTN_TRAIN_CASES = {
    "fullattn_train_b2_64x96_n150": (((64, 96), 150, 0.0, 7, [2, 3], 30, 0.3, 10), (True, True)),
    "fullattn_coarse_train_b2_64x96_n150": (((64, 96), 150, 0.0, 7, [2, 3], 30, 0.3, 10), (True, False)),
}


def train_setup(name):
    """as tests/helpers.py train_setup, with FullAttention at the case's levels"""
    (hw, n, thr, wseed, seeds, n_gt, pct, pad_min), (coarse, fine) = FULLATTN_TRAIN_CASES[name]
    cfg = full_config(default_config(thr=thr), coarse=coarse, fine=fine)
    cfg["coarse_matching"]["train"] = {"train_padding": True, "train_coarse_percent": pct, "train_pad_num_gt_min": pad_min}
    sd = make_state_dict(cfg, wseed)
    parts = [make_inputs(n, hw, s) for s in seeds]
    data = {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}
    B, L = len(seeds), (hw[0] // 8) * (hw[1] // 8)
    data["query_image_scale"] = torch.tensor([[1.0 + 0.25 * (b % 2), 1.0 - 0.125 * (b % 3)] for b in range(B)])
    g = torch.Generator().manual_seed(1000 + wseed)
    gt = torch.zeros(B, n, L, dtype=torch.int16)
    for b in range(B):
        gt[b, torch.randperm(n, generator=g)[:n_gt], torch.randperm(L, generator=g)[:n_gt]] = 1
    data["conf_matrix_gt"] = gt
    return cfg, sd, data
