"""Case table of the encoder-option fixtures: `loftr_*.rezero` (transformer.py:61-63, :94), `loftr_*.norm_method: "instancenorm"`
(transformer.py:52-54), `coarse_matching.feat_norm_method: "none"` (coarse_matching.py:49-50) and `keypoints_encoding.norm_method:
"layernorm"` (position_encoding.py:71-72), alone and together.  Shared by tests/golden/gen_encoder_options_golden.py (the only reader
of the reference) and the tests."""
import hashlib

import torch

from onepose_plus_plus_amd.config import default_config
from onepose_plus_plus_amd.synthetic import make_state_dict, make_inputs

# setting name -> keyword of `encopt_config`
SETTINGS = ("rezero", "instancenorm", "featnone", "kptln")
VARIANTS = {s: (s,) for s in SETTINGS}
VARIANTS["all4"] = SETTINGS
REZERO_INIT = {"loftr_coarse": 0.5, "loftr_fine": 0.25}     # constructor values (a state dict overrides them)


def encopt_config(cfg, settings):
    """cfg with the named settings switched on at both transformer levels"""
    for s in settings:
        if s == "rezero":
            for lv, v in REZERO_INIT.items():
                cfg[lv]["rezero"] = v
        elif s == "instancenorm":
            cfg["loftr_coarse"]["norm_method"] = cfg["loftr_fine"]["norm_method"] = "instancenorm"
        elif s == "featnone":
            cfg["coarse_matching"]["feat_norm_method"] = "none"
        elif s == "kptln":
            cfg["keypoints_encoding"]["norm_method"] = "layernorm"
        else:
            raise ValueError(s)
    return cfg


def has_featnone(settings):
    return "featnone" in settings


# name -> (hw, n points, thr, weight seed, input seed, variant).  64 x 96 / 100 points = the smallest end-to-end size of the suite;
# 128 x 128 / 300 points: the fused layer kernels see full and partial 64-row tiles (L = 256 image tokens, 300 points)
# thr: 0 where the scores keep their 1 / C scaling.  With feat_norm_method none the softmaxes saturate and most confidences underflow to
# exactly 0 in fp32 while they stay positive in float64, so `conf > 0` is not a property two correct evaluations share: those cases take
# thr 0.1 (as e2e_64x96_n100_thr01)
THR_FEATNONE = 0.1
ENCOPT_E2E_CASES = {}
for _v in VARIANTS:
    _thr = THR_FEATNONE if has_featnone(VARIANTS[_v]) else 0.0
    ENCOPT_E2E_CASES["encopt_%s_64x96_n100" % _v] = ((64, 96), 100, _thr, 0, 1, _v)
    ENCOPT_E2E_CASES["encopt_%s_128x128_n300" % _v] = ((128, 128), 300, _thr, 0, 1, _v)
# full attention at both levels together with rezero and instancenorm at both levels
ENCOPT_FULLATTN_CASES = {"encopt_fullattn_rezero_instancenorm_128x128_n300": ((128, 128), 300, 0.0, 0, 1, ("rezero", "instancenorm"))}
# B = 2 with query_image_mask, all four settings, in the layout of e2e_b2_mask_64x96_n200 (tests/helpers.py batch_setup)
ENCOPT_BATCH_CASES = {"encopt_all4_b2_mask_64x96_n200": ((64, 96), 200, THR_FEATNONE, 0, [3, 4])}
# train()-mode forward + gradients, all four settings: (hw, n, thr, weight seed, input seeds, n_gt per sample, train_coarse_percent, pad min)
ENCOPT_TRAIN_CASES = {"encopt_all4_train_b2_64x96_n150": ((64, 96), 150, THR_FEATNONE, 7, [2, 3], 30, 0.3, 10)}

MODULE_CONTRACT = "encopt_module_contract"        # keys / shapes of the reference's state dict per variant
KPT_PARENT_DIGEST = "encopt_kpt_parent_digest"    # sha256 of the keypoint encoder's output before it took an affine
KPT_KERNEL_SIZES = (1, 63, 300)

# `param_spec` / `make_state_dict` of the DEFAULT config as they were before these settings existed: sha256 over the keys and the raw
# bytes of make_state_dict(default_config(), 0), in order
DEFAULT_STATE_DICT_SHA256 = "eff6621bdd5369deee328c3c559344f57becfdb975748cd25982a129a87c9804"


def state_dict_sha256(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.contiguous().numpy().tobytes())
    return h.hexdigest()


def e2e_setup(name, table=None):
    hw, n, thr, wseed, iseed, variant = (table or ENCOPT_E2E_CASES)[name]
    settings = VARIANTS[variant] if isinstance(variant, str) else variant
    cfg = encopt_config(default_config(thr=thr), settings)
    return cfg, make_state_dict(cfg, wseed), make_inputs(n, hw, iseed)


def fullattn_setup(name):
    from tests.golden.fullattn_cases import full_config
    cfg, _, data = e2e_setup(name, ENCOPT_FULLATTN_CASES)
    cfg = full_config(cfg)
    return cfg, make_state_dict(cfg, ENCOPT_FULLATTN_CASES[name][3]), data


def batch_setup(name):
    """B = 2, per-sample clouds / images, distinct image scales and extents, padding masks (as tests/helpers.py batch_setup)"""
    hw, n, thr, wseed, seeds = ENCOPT_BATCH_CASES[name]
    cfg = encopt_config(default_config(thr=thr), SETTINGS)
    sd = make_state_dict(cfg, wseed)
    parts = [make_inputs(n, hw, s) for s in seeds]
    data = {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}
    B = len(seeds)
    data["query_image_scale"] = torch.tensor([[1.0 + 0.25 * b, 1.0 - 0.125 * b] for b in range(B)])
    data["keypoints3d"] = data["keypoints3d"] * torch.tensor([1.0 + 0.5 * b for b in range(B)]).view(B, 1, 1)
    hc, wc = hw[0] // 8, hw[1] // 8
    m = torch.ones(B, hc, wc)
    m[0, :, wc - 3:] = 0            # right padding of sample 0
    m[1, hc - 2:, :] = 0            # bottom padding of sample 1
    data["query_image_mask"] = m
    return cfg, sd, data


def train_setup(name):
    """as tests/helpers.py train_setup, with the four settings"""
    hw, n, thr, wseed, seeds, n_gt, pct, pad_min = ENCOPT_TRAIN_CASES[name]
    cfg = encopt_config(default_config(thr=thr), SETTINGS)
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


def train_grad_tensors(cfg):
    """whole gradient tensors the training fixture stores: tests/helpers.py GRAD_TENSORS without its norm2 entry (an "instancenorm" level
    has none) + every res_weight + the keypoint encoder's LayerNorm affine"""
    from tests.helpers import GRAD_TENSORS
    names = [n for n in GRAD_TENSORS if ".norm1." not in n and ".norm2." not in n]
    for lv in ("loftr_coarse", "loftr_fine"):
        n_layers = len(list(cfg[lv]["layer_names"])) * cfg[lv]["layer_iter_n"]
        names += ["%s.layers.%d.res_weight" % (lv, i) for i in range(n_layers)]
    names += ["kpt_3d_pos_encoding.encoder.%d.%s" % (i, w) for i in (1, 4, 7) for w in ("weight", "bias")]
    return tuple(names)


def kpt_kernel_inputs(n):
    """-> keypoints [1, n, 3], coarse bank [1, 256, n] of the keypoint-encoder kernel cases"""
    g = torch.Generator().manual_seed(4200 + n)
    return torch.rand(1, n, 3, generator=g) - 0.5, torch.randn(1, 256, n, generator=g)
