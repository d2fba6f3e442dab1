"""float64 / float32 torch restatement of `onepose_plus_plus_amd.loftr.LoFTRMatcher.forward` (TEST INFRASTRUCTURE).

The pinned blocks come from oracle/onepose_oracle.py (`backbone_forward`, `sine_position_table`, `encoder_layer` with its
`linear_attention`); the four pieces of glue that live in the LoFTR submodule -- absent from the reference checkout, so "parity
unpinned": our reading of the published LoFTR -- are restated here:

  schedule        self: f0 = layer(f0, f0), f1 = layer(f1, f1); cross: f0 = layer(f0, f1), THEN f1 = layer(f1, f0) with the updated
                  f0 (`sequential=False` gives quirk q6 of the 2D-3D model instead: both from the pre-update tokens)
  coarse match    both streams / sqrt(C), sim / T with T exactly as configured, dual softmax, conf > thr, border cleared at both
                  ends of both grids, mutual maximum, first j per row, ascending i
  fine windows    F.unfold(kernel W, stride 4, padding W // 2) of both 1/2-resolution maps at the matched cells
  fine head       the centre token of window 0 against the W^2 tokens of window 1, then oracle.fine_matching's expectation
"""
import torch
import torch.nn.functional as F

from oracle import onepose_oracle as O

POS_EMB_SHAPE = (256, 256)


def cast_sd(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def transformer(sd, name, nhead, layer_names, f0, f1, sequential=True):
    """f0 [B, L0, C], f1 [B, L1, C] -> the two streams after every layer"""
    for i, kind in enumerate(layer_names):
        p = "%s.layers.%d" % (name, i)
        if kind == "self":
            f0 = O.encoder_layer(sd, p, nhead, f0, f0)
            f1 = O.encoder_layer(sd, p, nhead, f1, f1)
        elif sequential:
            f0 = O.encoder_layer(sd, p, nhead, f0, f1)
            f1 = O.encoder_layer(sd, p, nhead, f1, f0)
        else:
            f0, f1 = O.encoder_layer(sd, p, nhead, f0, f1), O.encoder_layer(sd, p, nhead, f1, f0)
    return f0, f1


def coarse_tokens(sd, cfg, image, dtype):
    feat_c, feat_f = O.backbone_forward(sd, image.to(dtype))
    pe = O.sine_position_table(cfg["coarse"]["d_model"], POS_EMB_SHAPE).to(dtype)     # the module's float32 buffer, widened
    tok = (feat_c + pe[:, :, :feat_c.size(2), :feat_c.size(3)]).flatten(2).transpose(1, 2)
    return tok, feat_f, tuple(feat_c.shape[2:])


def conf_matrix(f0, f1, temperature):
    C = f0.shape[-1]
    sim = torch.einsum("nlc,nsc->nls", f0 / C ** 0.5, f1 / C ** 0.5) / temperature
    return F.softmax(sim, 1) * F.softmax(sim, 2)


def border_mask(hw0, hw1, b):
    """[L0, L1] bool: False where either cell lies within b cells of any edge of its own grid"""
    def inside(hw):
        h, w = hw
        m = torch.ones(h, w, dtype=torch.bool)
        if b > 0:
            m[:b] = False
            m[:, :b] = False
            m[h - b:] = False
            m[:, w - b:] = False
        return m.flatten()
    return inside(hw0)[:, None] & inside(hw1)[None, :]


def select(conf, hw0, hw1, thr, border_rm):
    """conf [1, L0, L1] -> i_ids, j_ids, mconf"""
    c = conf[0]
    mask = (c > thr) & border_mask(hw0, hw1, border_rm)
    mask = mask & (c == c.max(dim=1, keepdim=True)[0]) & (c == c.max(dim=0, keepdim=True)[0])
    has, j_all = mask.max(dim=1)
    i_ids = torch.where(has)[0]
    j_ids = j_all[i_ids]
    return i_ids, j_ids, c[i_ids, j_ids]


def windows(feat_f, W, ids, stride=4):
    """feat_f [1, C, Hf, Wf] -> [M, W*W, C] around the coarse cells `ids`"""
    C = feat_f.shape[1]
    u = F.unfold(feat_f, kernel_size=(W, W), stride=stride, padding=W // 2)         # [1, C*WW, L]
    return u.view(1, C, W * W, -1).permute(0, 3, 2, 1)[0, ids]


def fine_head(w0, w1, W):
    """-> expec_f [M, 3] (oracle.fine_matching's arithmetic with the centre token of window 0 as the query)"""
    C = w0.shape[-1]
    sim = torch.einsum("mc,mrc->mr", w0[:, W * W // 2, :], w1)
    heat = torch.softmax((1.0 / C ** 0.5) * sim, dim=1)
    lin = ((torch.linspace(0, W - 1, W) / (W - 1) - 0.5) * 2).to(heat.dtype)
    gx = lin.view(1, W).expand(W, W).reshape(-1)
    gy = lin.view(W, 1).expand(W, W).reshape(-1)
    grid = torch.stack([gx, gy], dim=-1)
    coords = torch.stack([(gx * heat).sum(-1), (gy * heat).sum(-1)], dim=-1)
    var = torch.sum(grid[None] ** 2 * heat[:, :, None], dim=1) - coords ** 2
    std = torch.sum(torch.sqrt(torch.clamp(var, min=1e-10)), -1)
    return torch.cat([coords, std[:, None]], -1)


def forward(sd, data, cfg, enable_fine=True, dtype=torch.float64, sequential=True, ids=None):
    """-> dict of the matcher's outputs (CPU tensors of `dtype`).  `ids` = (i_ids, j_ids): run the fine level on GIVEN matches (what a
    device test uses to compare the fine level on the device's own index set)."""
    sd = cast_sd(sd, dtype)
    out = {}
    with torch.no_grad():
        t0, ff0, hw0 = coarse_tokens(sd, cfg, data["image0"], dtype)
        t1, ff1, hw1 = coarse_tokens(sd, cfg, data["image1"], dtype)
        f0, f1 = transformer(sd, "loftr_coarse", cfg["coarse"]["nhead"], cfg["coarse"]["layer_names"], t0, t1, sequential)
        mc = cfg["match_coarse"]
        conf = conf_matrix(f0, f1, mc["dsmax_temperature"])
        i_ids, j_ids, mconf = select(conf, hw0, hw1, mc["thr"], mc["border_rm"])
        if ids is not None:
            i_ids, j_ids = ids
            mconf = conf[0, i_ids, j_ids]
        scale = data["image0"].shape[2] / hw0[0]
        s0 = scale * data["scale0"][0, [1, 0]].to(dtype) if "scale0" in data else scale
        s1 = scale * data["scale1"][0, [1, 0]].to(dtype) if "scale1" in data else scale
        mk0 = torch.stack([i_ids % hw0[1], i_ids // hw0[1]], dim=1).to(dtype) * s0
        mk1 = torch.stack([j_ids % hw1[1], j_ids // hw1[1]], dim=1).to(dtype) * s1
        out.update(hw0_c=hw0, hw1_c=hw1, tokens0=t0, tokens1=t1, feat_c0=f0, feat_c1=f1, conf_matrix=conf, i_ids=i_ids, j_ids=j_ids,
                   mconf=mconf, mkpts0_c=mk0, mkpts1_c=mk1, mkpts0_f=mk0, mkpts1_f=mk1)
        if not enable_fine:
            return out
        W = cfg["fine_window_size"]
        if len(i_ids) == 0:
            out["expec_f"] = torch.empty(0, 3, dtype=dtype)
            return out
        w0, w1 = windows(ff0, W, i_ids), windows(ff1, W, j_ids)
        w0, w1 = transformer(sd, "loftr_fine", cfg["fine"]["nhead"], cfg["fine"]["layer_names"], w0, w1, sequential)
        expec = fine_head(w0, w1, W)
        fs = data["image0"].shape[2] / ff0.shape[2]
        fs1 = fs * data["scale1"][0, [1, 0]].to(dtype) if "scale1" in data else fs
        out.update(expec_f=expec, mkpts1_f=mk1 + expec[:, :2] * (W // 2) * fs1)
    return out
