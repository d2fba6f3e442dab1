"""Case table of the 2D-2D matcher fixtures (onepose_plus_plus_amd/loftr.py).  Shared by tests/golden/gen_loftr_golden.py and the
tests.  The fixtures hold RESULTS only (float64 restatement, tests/loftr_reference.py); the inputs are regenerated from the seeds
here: shifted crops of one smooth random texture, so that real correspondences exist, and `synthetic.make_state_dict` weights on
the LoFTR-shaped config."""
import copy

import torch
import torch.nn.functional as F

from onepose_plus_plus_amd.loftr import default_cfg, model_config
from onepose_plus_plus_amd.synthetic import make_state_dict

WEIGHT_SEED = 7
TEXTURE_SEED = 3
TEXTURE_HW = (224, 256)
THR = 0.02                         # the threshold the generator's assertions are made at (the shipped 0.2 is one of the variants)
# name -> ((H0, W0), (H1, W1), shift (dy, dx) of image 1's crop against image 0's in pixels, top-left of image 0's crop inside the
# texture).  The origins were searched (steps of 2 - 3 pixels around (45, 45)) for crops on which the float64 result decides every
# selection, at every threshold of VARIANTS, with a margin above 10 x TOL_CONF: what gen_loftr_golden.py asserts.
LOFTR_PAIRS = {
    "loftr_96x128_128x96": ((96, 128), (128, 96), (8, 16), (49, 40)),       # w0c = 16, w1c = 12: catches i / j and width mix-ups
    "loftr_128x128": ((128, 128), (128, 128), (16, 8), (45, 53)),
    "loftr_120x160": ((120, 160), (120, 160), (8, 24), (49, 40)),          # 300 tokens: every 16 / 32 / 64-row tile has a tail
}
# what a fixture holds beside conf_matrix: name -> (thr, (scale0, scale1) or None); every variant at windows 9 and 5
VARIANTS = {
    "thr002": (0.02, None),
    "thr02": (0.2, None),
    "thr09": (0.9, None),                                           # no match: the M = 0 branch
    "thr0005s": (0.005, ((1.5, 0.75), (1.25, 2.0))),                # scale0 != scale1, (h_scale, w_scale)
}
WINDOWS = (9, 5)


def texture(seed=TEXTURE_SEED, hw=TEXTURE_HW):
    """smooth random texture in [0, 1]: white noise through Gaussian blurs of three widths, summed"""
    g = torch.Generator().manual_seed(seed)
    h, w = hw
    out = torch.zeros(1, 1, h, w, dtype=torch.float64)
    for sigma, weight in ((2.0, 1.0), (5.0, 1.5), (11.0, 2.0)):
        r = int(3 * sigma)
        x = torch.arange(-r, r + 1, dtype=torch.float64)
        k = torch.exp(-0.5 * (x / sigma) ** 2)
        k = k / k.sum()
        n = torch.randn(1, 1, h + 2 * r, w + 2 * r, generator=g, dtype=torch.float64)
        n = F.conv2d(F.conv2d(n, k.view(1, 1, 1, -1)), k.view(1, 1, -1, 1))
        out = out + weight * n / n.std()
    out = (out - out.min()) / (out.max() - out.min())
    return out[0, 0].float()


def loftr_cfg(thr=THR, window=9):
    cfg = copy.deepcopy(default_cfg)
    cfg["match_coarse"]["thr"] = thr
    cfg["fine_window_size"] = window
    return cfg


def loftr_state_dict():
    return make_state_dict(model_config(default_cfg), WEIGHT_SEED)


def loftr_pair(name, variant="thr002"):
    """-> data dict (CPU float32): image0, image1 [1,1,H,W] and, for a scaled variant, scale0 / scale1 [1,2]"""
    hw0, hw1, (dy, dx), (y0, x0) = LOFTR_PAIRS[name]
    tex = texture()
    data = {"image0": tex[y0:y0 + hw0[0], x0:x0 + hw0[1]][None, None].contiguous(),
            "image1": tex[y0 + dy:y0 + dy + hw1[0], x0 + dx:x0 + dx + hw1[1]][None, None].contiguous()}
    scales = VARIANTS[variant][1]
    if scales is not None:
        data["scale0"] = torch.tensor([scales[0]], dtype=torch.float32)
        data["scale1"] = torch.tensor([scales[1]], dtype=torch.float32)
    return data


def content_state_dict(scale=16.0, gain=500.0):
    """Weights under which coarse matching follows the image content (random weights follow the sine table: same position in both
    images): the 1/8-resolution features are `scale` times larger than the position encoding; the coarse layers but the last are the
    identity (mlp.2 = 0, norm2.bias = 0); the last one ignores its attention message (the message columns of mlp.0 are 0) and adds
    `gain` x LayerNorm(mlp(x)) to x -- tokens of equal norm that depend on their own cell only, so that the dual softmax picks equal
    cells.  The fine level keeps its random weights (its features are not shift-equivariant anyway: the FPN upsamples with
    align_corners=True), so the detector case runs the matcher without it."""
    sd = dict(loftr_state_dict())
    sd["backbone.layer3_outconv.weight"] = sd["backbone.layer3_outconv.weight"] * scale
    n, C = len(default_cfg["coarse"]["layer_names"]), default_cfg["coarse"]["d_model"]
    for i in range(n):
        p = "loftr_coarse.layers.%d." % i
        sd[p + "norm2.bias"] = torch.zeros(C)
        if i < n - 1:
            sd[p + "mlp.2.weight"] = torch.zeros(C, 2 * C)
        else:
            w = sd[p + "mlp.0.weight"].clone()
            w[:, C:] = 0
            sd[p + "mlp.0.weight"] = w
            sd[p + "norm2.weight"] = torch.full((C,), gain)
    return sd


def detector_case():
    """-> view [128, 160] uint8, frame [224, 256] uint8 (the whole texture), (dy, dx) = where the view lies inside the frame"""
    u8 = (texture() * 255).round().clamp(0, 255).to(torch.uint8)
    dy, dx = 48, 48
    return u8[dy:dy + 128, dx:dx + 160].contiguous(), u8, (dy, dx)
