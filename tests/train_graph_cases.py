"""Seeded cases of the training graph BEHIND the backbone (onepose_plus_plus_amd/train_autograd.py): the matcher node, single encoder
layers, a two-layer transformer, the keypoint encoder and the fine level, each with a float64 torch.autograd reference on the CPU, the
float32 evaluation of the same reference (the yardstick the bars are made of) and a probe of the ReLU kinks.  Shared by
tests/test_train_graph_cases_cpu.py (which establishes from the references alone that the cases can carry their bars) and
tests/test_train_graph_nodes_gpu.py (which holds the HIP nodes to them).  Nothing here touches a GPU on import; `forward` with `hp` set
builds the device graph out of the product's own nodes.

References
  transformer / keypoint encoder  the product's own torch formula: `_encoder_layer` / `_transformer` / `_kpt_encoding` with hp = None on
                                  float64 CPU tensors (pinned against the reference project's gradients by tests/test_train_autograd_cpu.py)
  matcher                         sim = einsum(f3, f2) * scale (+ where(mask, 0, -1e9)); conf = softmax(sim, 1) * softmax(sim, 2), plain
                                  autograd; `scale` is derived HERE from the config (coarse_matching.py:46-50, :99-107), not read from the node
  fine level                      tests/torch_graph_ref.fine_level_ref, the fine half of `differentiable_forward`

Error measure, for a tensor t of a case:  err(t) = max|got - ref64| / max(max|ref64(t)|, FLOOR * S), S = the largest max|ref64| among the
case's gradient tensors (among its outputs when t is an output).  The floor exists because some gradients cancel analytically: with one
source token linear attention returns v whatever q and k are, so the q_proj / k_proj gradients of the fine cross layer are rounding noise
around 0 (torch's own float32 result is 300 % of those tensors' largest entry away from float64).
Bar of t: min(BAR_FACTOR * d32(t), BAR_CAP), d32 = the same measure of torch's float32 CPU evaluation of the reference -- computed from the
two reference chains, never from the kernel (the scheme of tests/test_train_sample_gpu.py; 16 instead of its 4 because a case is a chain
of four to eight kernels, each with its own association: split-K partials in fixed order, chunked attention sums, wave-shuffle LayerNorm).

ReLU kinks: `mlp.0` of every layer and the keypoint encoder's ReLUs.  `record_relus` replaces `train_autograd.F` by a shim that forwards
everything and records the argument of `relu`.  Every case's seed was chosen on the CPU so that over all of the case's ReLUs
min|z64| >= KINK_MARGIN * max|z32 - z64|  and no pre-activation changes sign between the float64 and the float32 run: two correct
evaluations then differentiate the same function.  The seed is the first of 0, 1, 2, ... with THREE times that margin (24 x), because
max|z32 - z64| moves by some 20 % from host to host; the two-layer transformer (83 968 pre-activations) has none among 0 .. 39 and keeps
seed 0 at 16 x (22 x on the MI355X host).
One more rule, for `layer_coarse_self_masked_rezero_instancenorm` only: its `res_weight` gradient is ONE number, so d32 of that tensor is one
sample of float32 rounding and can land anywhere -- over seeds 0 .. 59 it is 4e-8 .. 2.7e-6 on the build host, and at one and the same seed
5.9e-7 on one host and 4.3e-8 on the other.  A float32 result closer to float64 than one float32 ulp (2^-23 = 1.2e-7) is luck, and 16 x luck
is no bar (at seed 5 the MI355X host's bar for that number came out 6.9e-7, i.e. six ulps of a sum of 20 480 products that cancel; the device
graph -- torch's own reduction of res_weight's product there -- was 1.2e-6 (bf16x3) and 1.9e-6 (fp32) from float64).  So this case takes the
first seed with the 24 x margin at which d32(res_weight) >= 2^-23 on both hosts: 17 (5 is passed over; 1.9e-7 and 3.3e-7 at 17).
`fine_transformer_on` cannot meet that margin at any seed: 37 matches x 26 tokens x 256 channels x 2 layers are 492 544 pre-activations
of rms ~0.5, so about 25 of them lie within 8 x 4e-6 of zero whatever the seed (seeds 0 .. 7: min|z64| 3e-7 .. 6e-6 against
max|z32 - z64| 4.0e-6 .. 4.9e-6).  It is marked `kinks="device_sides"`: its seed (1, the largest margin of seeds 0 .. 7) still has no sign
change between the float64 and the float32 run, and the GPU test gives the float64 reference's ReLU DERIVATIVES the sides the device took
(`record_relus(sides=...)`, the scheme of test_backbone_node_vs_autograd) after asserting that the sides differ only where
|z64| <= BAR_FACTOR * max|z32 - z64| -- where rounding alone can move a pre-activation across zero.  No tensor is left out.
"""
import contextlib
import copy
import functools
import types

import torch
import torch.nn.functional as F

from onepose_plus_plus_amd import train_autograd as TA
from onepose_plus_plus_amd.config import default_config
from onepose_plus_plus_amd.synthetic import make_state_dict
from tests.golden.encopt_cases import encopt_config
from tests.torch_graph_ref import fine_level_ref

WEIGHT_SEED = 3
BAR_FACTOR = 16.0
BAR_CAP = 5e-5
FLOOR = 1e-3
KINK_MARGIN = 8.0
VAR_MIN = 1e-6                      # test_fine_head_backward_vs_fp64: rows whose heatmap variance is below it sit on the clamp of the std column
N_FOCAL = 20                        # entries of the matcher's grad_conf multiplied by -100: the shape of a focal-loss gradient

# name -> kind, seed of the inputs, and what the kind needs.  `settings`: names of tests/golden/encopt_cases.py::encopt_config
CASES = {
    # A. HipCoarseMatch as a node: (B, N, hc, wc, masked)
    "match_b2_n77_5x13_masked": dict(kind="matcher", seed=0, shape=(2, 77, 5, 13), masked=True, settings=()),            # L = 65: L % 32 and L % 4 != 0
    "match_b1_n33_4x8": dict(kind="matcher", seed=0, shape=(1, 33, 4, 8), masked=False, settings=()),                    # L = 32: no padding path
    "match_b3_n130_6x6_masked_featnone": dict(kind="matcher", seed=0, shape=(3, 130, 6, 6), masked=True, settings=("featnone",)),
    # B. one encoder layer: x <- source; masks: which of x_mask / source_mask are given
    "layer_coarse_self": dict(kind="layer", seed=0, level="loftr_coarse", layer=0, x="image", source="image", masks=(), settings=()),
    "layer_coarse_self_masked": dict(kind="layer", seed=11, level="loftr_coarse", layer=0, x="image", source="image", masks=("x", "source"), settings=()),
    "layer_coarse_cross_image_points": dict(kind="layer", seed=9, level="loftr_coarse", layer=0, x="image", source="points", masks=("x",), settings=()),
    "layer_coarse_cross_points_image": dict(kind="layer", seed=4, level="loftr_coarse", layer=0, x="points", source="image", masks=("source",), settings=()),
    "layer_coarse_self_masked_rezero_instancenorm": dict(kind="layer", seed=17, level="loftr_coarse", layer=0, x="image", source="image",
                                                         masks=("x", "source"), settings=("rezero", "instancenorm")),
    "layer_fine_self": dict(kind="layer", seed=9, level="loftr_fine", layer=1, x="image", source="image", masks=(), settings=()),
    "layer_fine_cross_windows_point": dict(kind="layer", seed=0, level="loftr_fine", layer=1, x="image", source="points", masks=(), settings=()),   # S = 1
    "layer_fine_cross_point_windows": dict(kind="layer", seed=0, level="loftr_fine", layer=1, x="points", source="image", masks=(), settings=()),   # L = 1
    # C. self + cross through _transformer, masked: quirk q6 and the mask routing of all four layer calls
    "transformer_self_cross_masked": dict(kind="transformer", seed=0, settings=()),
    # D. _kpt_encoding
    "kpt_default": dict(kind="kpt", seed=1, settings=()),
    "kpt_layernorm": dict(kind="kpt", seed=0, settings=("kptln",)),
    # E. fine_level_graph: gather -> loftr_fine -> head
    "fine_transformer_on": dict(kind="fine", seed=1, enable=True, settings=(), kinks="device_sides"),
    "fine_transformer_off": dict(kind="fine", seed=0, enable=False, settings=()),
}
# token counts: (B, image tokens, point tokens)
LAYER_SHAPES = {"loftr_coarse": (2, 40, 33), "loftr_fine": (5, 25, 1)}
TRANSFORMER_SHAPE = (2, 3, 8, 17)                   # B, hc, wc, N: L = 24
KPT_SHAPE = (2, 50)
FINE_SHAPE = dict(B=2, Hf=16, Wf=24, hc=4, wc=6, M=37, N=20)      # the geometry of test_fine_window_gather_node_vs_unfold, W = 5
FINE_DUPLICATE_ROWS = (5, 6)

# d32 of every case: the largest one among the outputs and among the gradients, as (smallest, largest) over the two hosts it was measured
# on (the build host and the MI355X host: same torch, same thread count, different CPUs -- torch's CPU kernels vectorise differently from
# machine to machine; the matcher's gradients swing most, 2.0e-7 .. 2.1e-6, because a few of the twenty -100 entries of grad_conf carry
# them).  tests/test_train_graph_cases_cpu.py asserts that both stay within D32_RANGE times beyond these, each way.
D32_RANGE = 3.0
D32 = {                                                       # outputs, gradients
    "match_b2_n77_5x13_masked": ((7.30e-7, 1.24e-6), (3.70e-7, 2.14e-6)),
    "match_b1_n33_4x8": ((9.79e-7, 1.80e-6), (6.53e-7, 7.61e-7)),
    "match_b3_n130_6x6_masked_featnone": ((1.11e-6, 2.08e-6), (2.04e-7, 9.62e-7)),
    "layer_coarse_self": ((3.18e-7, 3.96e-7), (6.68e-7, 7.78e-7)),
    "layer_coarse_self_masked": ((3.51e-7, 4.30e-7), (6.41e-7, 7.56e-7)),
    "layer_coarse_cross_image_points": ((3.98e-7, 4.04e-7), (7.07e-7, 9.12e-7)),
    "layer_coarse_cross_points_image": ((3.08e-7, 4.15e-7), (6.59e-7, 7.28e-7)),
    "layer_coarse_self_masked_rezero_instancenorm": ((1.62e-7, 2.19e-7), (5.79e-7, 7.50e-7)),
    "layer_fine_self": ((3.10e-7, 3.83e-7), (6.87e-7, 7.10e-7)),
    "layer_fine_cross_windows_point": ((2.68e-7, 3.32e-7), (3.56e-5, 3.60e-5)),     # gradients: q_proj / k_proj, rounding noise over the floor
    "layer_fine_cross_point_windows": ((1.88e-7, 2.76e-7), (6.02e-7, 6.22e-7)),
    "transformer_self_cross_masked": ((3.59e-7, 5.06e-7), (1.59e-6, 2.25e-6)),
    "kpt_default": ((9.92e-8, 9.92e-8), (4.68e-7, 5.53e-7)),
    "kpt_layernorm": ((1.13e-7, 1.13e-7), (5.06e-7, 8.84e-7)),
    "fine_transformer_on": ((1.73e-6, 2.20e-6), (2.67e-6, 3.32e-6)),
    "fine_transformer_off": ((2.67e-7, 3.98e-7), (2.96e-7, 3.37e-7)),
}


def names(kind=None):
    return [n for n, c in CASES.items() if kind is None or c["kind"] == kind]


def config(name):
    """the model configuration of a case"""
    case = CASES[name]
    cfg = encopt_config(default_config(), case["settings"])
    if case["kind"] == "fine":
        cfg["loftr_fine"]["enable"] = case["enable"]
    return cfg


@functools.lru_cache(maxsize=None)
def _state_dict(settings):
    return make_state_dict(encopt_config(default_config(), settings), WEIGHT_SEED)


def state_dict(name):
    """float32 weights of the case's configuration.  Read-only: shared between the cases"""
    return _state_dict(tuple(CASES[name]["settings"]))


def transformer_config(name):
    """`tcfg` of a transformer case: loftr_coarse with one self and one cross layer"""
    tcfg = copy.deepcopy(config(name)["loftr_coarse"])
    tcfg["layer_names"], tcfg["layer_iter_n"] = ["self", "cross"], 1
    return tcfg


def matcher_scale(cfg):
    """what CoarseMatching multiplies <f3, f2> by (coarse_matching.py:46-50: both token sets over sqrt(C), or left alone under
    feat_norm_method "none"; :107: over temperature + 1e-4)"""
    cm = cfg["coarse_matching"]
    C = cfg["loftr_coarse"]["d_model"]
    norm = 1.0 / C if cm["feat_norm_method"] == "sqrt_feat_dim" else 1.0
    return norm / (cm["dual_softmax"]["temperature"] + 1e-4)


def _param_names(name):
    case, sd = CASES[name], state_dict(name)
    kind = case["kind"]
    if kind == "layer":
        pre = ("%s.layers.%d." % (case["level"], case["layer"]),)
    elif kind == "transformer":
        pre = ("loftr_coarse.layers.0.", "loftr_coarse.layers.1.")
    elif kind == "kpt":
        pre = ("kpt_3d_pos_encoding.",)
    elif kind == "fine":
        pre = ("loftr_fine.",) if case["enable"] else ()
    else:
        pre = ()
    return [k for k in sd if pre and k.startswith(pre)]


def _matcher_mask(B, L):
    """sample 0 loses its last three cells, the last sample cells 2..6, the samples between them nothing"""
    m = torch.ones(B, L)
    m[0, -3:] = 0
    m[-1, 2:7] = 0
    return m


def _token_mask(B, L):
    m = torch.ones(B, L)
    m[0, -3:] = 0
    m[1, 5:9] = 0
    return m


def inputs(name, seed=None):
    """-> namespace of float32 CPU tensors: `leaves` (inputs that take a gradient), `consts` (masks, keypoints, ids, the fine bank),
    `params` (the weights that take a gradient), `grad_out` (what arrives on every output)."""
    case = CASES[name]
    kind = case["kind"]
    g = torch.Generator().manual_seed(case["seed"] if seed is None else seed)
    sd = state_dict(name)
    leaves, consts, grad_out = {}, {}, {}
    if kind == "matcher":
        B, N, hc, wc = case["shape"]
        L, C = hc * wc, 256
        amp = 1.0 / 8 if "featnone" in case["settings"] else 2.0
        leaves["f3"] = torch.randn(B, N, C, generator=g) * amp
        leaves["f2"] = torch.randn(B, L, C, generator=g) * amp
        consts["kpts"] = torch.rand(B, N, 3, generator=g) - 0.5
        consts["mask"] = _matcher_mask(B, L) if case["masked"] else None
        gc = torch.rand(B, N, L, generator=g)
        gc.view(-1)[torch.randperm(B * N * L, generator=g)[:N_FOCAL]] *= -100.0
        grad_out["conf"] = gc
    elif kind == "layer":
        B, n_img, n_pts = LAYER_SHAPES[case["level"]]
        C = config(name)[case["level"]]["d_model"]
        rows = {"image": n_img, "points": n_pts}
        leaves["x"] = torch.randn(B, rows[case["x"]], C, generator=g)
        if case["source"] != case["x"]:
            leaves["source"] = torch.randn(B, rows[case["source"]], C, generator=g)
        consts["mask"] = _token_mask(B, n_img) if case["masks"] else None
        grad_out["out"] = torch.randn(B, rows[case["x"]], C, generator=g)
    elif kind == "transformer":
        B, hc, wc, N = TRANSFORMER_SHAPE
        leaves["f3"] = torch.randn(B, N, 256, generator=g)
        leaves["f2"] = torch.randn(B, hc * wc, 256, generator=g)
        consts["mask"] = _token_mask(B, hc * wc)
        grad_out["f3"] = torch.randn(B, N, 256, generator=g)
        grad_out["f2"] = torch.randn(B, hc * wc, 256, generator=g)
    elif kind == "kpt":
        B, N = KPT_SHAPE
        kpts = torch.rand(B, N, 3, generator=g) - 0.5
        kpts[1] = kpts[1] * torch.tensor([1.7, 0.6, 1.2]) + torch.tensor([0.3, -0.2, 0.1])      # another extent and centre than sample 0 (quirk q4)
        consts["kpts"] = kpts
        leaves["desc"] = torch.randn(B, 256, N, generator=g)
        grad_out["tokens"] = torch.randn(B, 256, N, generator=g)
    elif kind == "fine":
        s = FINE_SHAPE
        leaves["feat_f"] = torch.randn(s["B"], s["Hf"] * s["Wf"], 128, generator=g)                # NHWC tokens, as HipBackbone hands them on
        consts["bank_f"] = torch.randn(s["B"], 128, s["N"], generator=g)
        b_ids = torch.randint(0, s["B"], (s["M"],), generator=g)
        i_ids = torch.randint(0, s["N"], (s["M"],), generator=g)
        j_ids = torch.randint(0, s["hc"] * s["wc"], (s["M"],), generator=g)
        j_ids[:4] = torch.tensor([0, s["wc"] - 1, s["hc"] * s["wc"] - 1, (s["hc"] - 1) * s["wc"]])      # image corners: windows reach outside
        a, b = FINE_DUPLICATE_ROWS
        j_ids[a], b_ids[a] = j_ids[b], b_ids[b]                                                    # a duplicated (b, j) pair
        consts.update(b_ids=b_ids, i_ids=i_ids, j_ids=j_ids)
        grad_out["expec_f"] = torch.randn(s["M"], 3, generator=g)
    else:
        raise ValueError(kind)
    params = {k: sd[k] for k in _param_names(name)}
    return types.SimpleNamespace(leaves=leaves, consts=consts, params=params, grad_out=grad_out)


def tensors(name, dtype, device="cpu", seed=None):
    """the case's inputs in `dtype` on `device`; leaves and parameters require a gradient"""
    inp = inputs(name, seed)

    def cast(v, grad):
        if not torch.is_tensor(v):
            return v
        v = v.detach().clone()                      # never the shared state dict's own tensor
        v = v.to(device=device, dtype=dtype) if v.is_floating_point() else v.to(device)
        return v.contiguous().requires_grad_(True) if grad else v.contiguous()
    return types.SimpleNamespace(leaves={k: cast(v, True) for k, v in inp.leaves.items()}, consts={k: cast(v, False) for k, v in inp.consts.items()},
                                 params={k: cast(v, True) for k, v in inp.params.items()}, grad_out={k: cast(v, False) for k, v in inp.grad_out.items()})


def matcher_aux(model, t, name):
    """`aux` of HipCoarseMatch as `coarse_level_graph` builds it"""
    _, _, hc, wc = CASES[name]["shape"]
    lib, c = model._ensure_ready(t.leaves["f3"].device)
    return {"model": model, "lib": lib, "ctx": c, "hc": hc, "wc": wc, "kpts": t.consts["kpts"], "mask": t.consts["mask"], "qscale": None,
            "scale_c": 8.0, "hp": TA.graph_precision(model)}


def forward(name, t, hp=None, model=None):
    """-> dict of the case's outputs.  hp = None: the float reference in the dtype of `t`; hp set: the graph of HIP nodes on the device
    tensors of `t` (`model`: a module of the case's configuration, for the matcher node and the fine level)"""
    case = CASES[name]
    kind = case["kind"]
    cfg = config(name)
    if kind == "matcher":
        f3, f2, mask = t.leaves["f3"], t.leaves["f2"], t.consts["mask"]
        if hp is not None:
            return {"conf": TA.HipCoarseMatch.apply(f3, f2, matcher_aux(model, t, name))}
        sim = torch.einsum("nlc,nsc->nls", f3, f2) * matcher_scale(cfg)
        if mask is not None:
            sim = sim + torch.where(mask[:, None].bool(), 0.0, -1e9).to(sim.dtype)
        return {"conf": torch.softmax(sim, 1) * torch.softmax(sim, 2)}
    if kind == "layer":
        x = t.leaves["x"]
        source = t.leaves.get("source", x)
        mask = t.consts["mask"]
        lname = "%s.layers.%d" % (case["level"], case["layer"])
        return {"out": TA._encoder_layer(t.params, lname, cfg[case["level"]]["nhead"], x, source, mask if "x" in case["masks"] else None,
                                         mask if "source" in case["masks"] else None, hp)}
    if kind == "transformer":
        f3, f2 = TA._transformer(t.params, "loftr_coarse", transformer_config(name), t.leaves["f3"], t.leaves["f2"], t.consts["mask"], hp)
        return {"f3": f3, "f2": f2}
    if kind == "kpt":
        return {"tokens": TA._kpt_encoding(t.params, t.consts["kpts"], t.leaves["desc"], hp)}
    s = FINE_SHAPE
    ids = (t.consts["b_ids"], t.consts["i_ids"], t.consts["j_ids"])
    if hp is not None:
        return {"expec_f": TA.fine_level_graph(model, t.params, t.leaves["feat_f"], t.consts["bank_f"], *ids, s["B"], s["Hf"], s["Wf"], s["hc"], s["wc"])}
    feat = t.leaves["feat_f"].view(s["B"], s["Hf"], s["Wf"], -1).permute(0, 3, 1, 2)
    expec, var = fine_level_ref(t.params, cfg, feat, t.consts["bank_f"], *ids, s["Hf"] // s["hc"], with_var=True)
    return {"expec_f": expec, "var": var}


class _ReluWithSides(torch.autograd.Function):
    """ReLU whose DERIVATIVE takes the side of the kink another evaluation took (`side` = that evaluation's z > 0), the scheme of
    tests/test_train_bwd_gpu.py::_ActWithMask: the value is relu(z) as ever"""

    @staticmethod
    def forward(ctx, z, side):
        ctx.save_for_backward(side)
        return torch.clamp(z, min=0)

    @staticmethod
    def backward(ctx, g):
        (side,) = ctx.saved_tensors
        return g * side.to(g.dtype), None


class _RecordingF:
    """stands in for `torch.nn.functional` inside train_autograd: forwards everything, records what `relu` is applied to"""

    def __init__(self, rec, sides):
        self._rec, self._sides = rec, sides

    def __getattr__(self, attr):
        return getattr(F, attr)

    def relu(self, z, *args, **kw):
        self._rec.append(z.detach())
        if self._sides is not None:
            return _ReluWithSides.apply(z, self._sides[len(self._rec) - 1].to(z.device))
        return F.relu(z, *args, **kw)


@contextlib.contextmanager
def record_relus(sides=None):
    """-> the list every ReLU pre-activation of train_autograd's helpers is appended to while the block runs (product code untouched).
    sides: optional list of bool tensors, one per ReLU in order: the derivative of the i-th ReLU is sides[i] instead of z > 0"""
    rec = []
    saved = TA.F
    TA.F = _RecordingF(rec, sides)
    try:
        yield rec
    finally:
        TA.F = saved


def evaluate(name, dtype, device="cpu", hp=None, model=None, seed=None, sides=None):
    """one forward + backward of the case -> namespace: outs (detached, as the comparison takes them), grads (of every leaf and parameter),
    relus (the pre-activations, in order), var (fine cases of the reference: the heatmap variances)"""
    t = tensors(name, dtype, device, seed)
    with record_relus(sides) as rec:
        outs = forward(name, t, hp, model)
    var = outs.pop("var", None)
    nodes = graph_node_names(outs.values())
    loss = sum((outs[k] * t.grad_out[k]).sum() for k in outs)
    loss.backward()
    wanted = dict(t.leaves)
    wanted.update(t.params)
    grads = {k: (v.grad.detach() if v.grad is not None else None) for k, v in wanted.items()}
    outs = {k: v.detach() for k, v in outs.items()}
    if CASES[name]["kind"] == "fine":         # the std column is not compared (test_fine_head_backward_vs_fp64); its gradient still flows
        outs = {"expec_f[:, :2]": outs["expec_f"][:, :2]}
    return types.SimpleNamespace(outs=outs, grads=grads, relus=rec, var=var, nodes=nodes)


# what a graph on the device must be made of, and what must not appear in it: a GEMM, normalisation, attention or softmax of torch's own
# would mean that a helper of train_autograd fell back to a vendor kernel without saying so
HIP_NODES = {
    "matcher": {"HipCoarseMatchBackward"},
    "layer": {"HipLinearBackward", "HipLinearAttentionBackward", "HipLayerNormBackward"},
    "transformer": {"HipLinearBackward", "HipLinearAttentionBackward", "HipLayerNormBackward"},
    "kpt": {"HipLinearBackward"},
    "fine": {"HipFineGatherBackward", "HipFineHeadBackward"},
}
TORCH_NODES = ("MmBackward", "AddmmBackward", "BmmBackward", "NativeLayerNormBackward", "EluBackward", "SoftmaxBackward", "Im2ColBackward",
               "EinsumBackward", "LinearBackward")


def graph_node_names(outputs):
    """names of all autograd nodes the outputs hang on"""
    seen, todo, found = set(), [o.grad_fn for o in outputs if o.grad_fn is not None], set()
    while todo:
        fn = todo.pop()
        if fn in seen:
            continue
        seen.add(fn)
        found.add(type(fn).__name__)
        todo += [nf for nf, _ in fn.next_functions if nf is not None]
    return found


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (float64 evaluation, float32 evaluation) of the reference on the CPU.  Read-only: shared between tests"""
    return evaluate(name, torch.float64), evaluate(name, torch.float32)


def errors(got, ref64):
    """err(t) of every output ("out:<name>") and every gradient ("grad:<name>") of a case, as the module docstring defines it"""
    res = {}
    for tag, g, r in (("out", got.outs, ref64.outs), ("grad", got.grads, ref64.grads)):
        assert set(g) == set(r), (sorted(g), sorted(r))
        S = max(float(v.abs().max()) for v in r.values())
        for k, want in r.items():
            assert g[k] is not None, "%s:%s is missing" % (tag, k)
            assert tuple(g[k].shape) == tuple(want.shape), (k, tuple(g[k].shape), tuple(want.shape))
            den = max(float(want.abs().max()), FLOOR * S)
            res["%s:%s" % (tag, k)] = float((g[k].detach().cpu().double() - want).abs().max()) / den
    return res


@functools.lru_cache(maxsize=None)
def d32(name):
    r64, r32 = reference(name)
    return errors(r32, r64)


def bars(name):
    return {k: min(BAR_FACTOR * v, BAR_CAP) for k, v in d32(name).items()}


def d32_summary(d):
    """-> (largest d32 among the outputs, largest among the gradients)"""
    return max(v for k, v in d.items() if k.startswith("out:")), max(v for k, v in d.items() if k.startswith("grad:"))


def kink_margin(z_a, z_ref):
    """two recordings of a case's ReLU pre-activations -> (number of pre-activations, min|z_ref|, max|z_a - z_ref|, sign changes)"""
    assert len(z_a) == len(z_ref)
    if not z_ref:
        return 0, float("inf"), 0.0, 0
    a = torch.cat([z.detach().cpu().double().flatten() for z in z_a])
    r = torch.cat([z.detach().cpu().double().flatten() for z in z_ref])
    return r.numel(), float(r.abs().min()), float((a - r).abs().max()), int(((a > 0) != (r > 0)).sum())


def kinks_are_clear(name):
    """the condition the seed of a case was chosen for"""
    r64, r32 = reference(name)
    n, zmin, dz, flips = kink_margin(r32.relus, r64.relus)
    return (flips == 0 and zmin >= KINK_MARGIN * dz), (n, zmin, dz, flips)
