"""GPU: the training graph BEHIND the backbone, node composition by node composition, against float64 torch.autograd on the CPU -- the
cases of tests/train_graph_cases.py (which see for the references, the error measure and the ReLU-kink conditions):
  A  `HipCoarseMatch` as a node: conf, grad f3, grad f2; masked cells exact zeros; second backward bit-identical; mask reset afterwards
  B  one `_encoder_layer` on the device: coarse self / cross with every mask routing, rezero + instancenorm, the fine level's one-token segments
  C  self + cross through `_transformer` under a mask (quirk q6, the masks of all four layer calls)
  D  `_kpt_encoding` (K = 3 padded to 32, per-point norm, optional LayerNorm affine, batch-0 extent)
  E  `fine_level_graph`: gather -> loftr_fine -> head
in both arithmetics (`hp` from `train_autograd.graph_precision`).  Every output, every input gradient and every parameter gradient is held
to   err(t) <= min(16 * d32(t), 5e-5),   err(t) = max|kernel - f64| / max(max|f64(t)|, 1e-3 * S), d32 = the same measure of torch's float32
CPU evaluation of the reference; each test prints both distances.

Measured on one MI355X and its host (largest err among a case's outputs and among its gradients; largest d32 beside them; the bar of each
tensor is 16 x its own d32, so the tensor nearest its bar is not always the one with the largest err -- the tests print it):
  case                                           outputs: bf16x3  fp32      d32      | gradients: bf16x3  fp32      d32
  match_b2_n77_5x13_masked                                1.84e-06  1.74e-06  7.30e-07 |            4.26e-07  2.85e-06  3.70e-07
  match_b1_n33_4x8                                        9.96e-07  1.61e-06  9.79e-07 |            1.11e-06  1.83e-06  7.61e-07
  match_b3_n130_6x6_masked_featnone                       9.47e-07  1.58e-06  1.11e-06 |            4.11e-07  1.10e-06  2.04e-07
  layer_coarse_self                                       6.53e-07  6.68e-07  3.18e-07 |            6.72e-07  6.88e-07  6.68e-07
  layer_coarse_self_masked                                7.23e-07  5.10e-07  3.51e-07 |            6.56e-07  7.42e-07  6.41e-07
  layer_coarse_cross_image_points                         6.85e-07  6.16e-07  3.98e-07 |            9.43e-07  7.90e-07  7.07e-07
  layer_coarse_cross_points_image                         5.49e-07  5.74e-07  3.08e-07 |            6.52e-07  8.71e-07  6.59e-07
  layer_coarse_self_masked_rezero_instancenorm            2.68e-07  2.73e-07  1.62e-07 |            1.11e-06  7.24e-07  5.79e-07
  layer_fine_self                                         3.61e-07  3.23e-07  3.10e-07 |            5.57e-07  6.72e-07  6.87e-07
  layer_fine_cross_windows_point                          3.39e-07  3.37e-07  2.68e-07 |            3.19e-05  3.19e-05  3.60e-05   (q_proj / k_proj: noise over the floor)
  layer_fine_cross_point_windows                          4.53e-07  3.94e-07  2.76e-07 |            6.48e-07  8.29e-07  6.02e-07
  transformer_self_cross_masked                           5.76e-07  6.02e-07  3.59e-07 |            1.52e-06  1.52e-06  2.25e-06
  kpt_default                                             1.27e-07  1.07e-07  9.92e-08 |            4.61e-07  4.42e-07  4.68e-07
  kpt_layernorm                                           1.50e-07  1.09e-07  1.13e-07 |            6.14e-07  1.08e-06  5.06e-07
  fine_transformer_on                                     1.49e-06  1.49e-06  1.73e-06 |            2.96e-06  2.52e-06  3.32e-06
  fine_transformer_off                                    1.92e-07  1.92e-07  2.67e-07 |            2.70e-07  2.70e-07  2.96e-07
The tightest tensor is grad f3 of match_b3_n130_6x6_masked_featnone in fp32: 1.10e-6 of a bar of 1.70e-6.  No ReLU pre-activation took
another side on the device than in float64 in any case (largest |z - z64| 5.7e-6 in the two-layer transformer, 2.3e-6 for torch's float32),
so the float64 reference of fine_transformer_on was used as it is.
"""
import functools

import pytest
import torch

from tests import train_graph_cases as TC

pytestmark = pytest.mark.gpu

PRECISIONS = ("bf16x3", "fp32")


@functools.lru_cache(maxsize=None)
def _model_of(settings, fine_enable, precision):
    from onepose_plus_plus_amd.config import default_config
    from onepose_plus_plus_amd.synthetic import make_state_dict
    from tests import hip_ops as ops
    from tests.golden.encopt_cases import encopt_config
    cfg = encopt_config(default_config(), settings)
    cfg["loftr_fine"]["enable"] = fine_enable
    return ops.make_model(cfg, make_state_dict(cfg, TC.WEIGHT_SEED), precision)


def _model(name, precision):
    """a module of the case's configuration in the given arithmetic (weights of the cases: WEIGHT_SEED)"""
    case = TC.CASES[name]
    return _model_of(tuple(case["settings"]), case.get("enable", True), precision)


def _check(name, precision):
    """the case on the device against its float64 reference -> (device evaluation, float64 reference, model)"""
    from onepose_plus_plus_amd import train_autograd as TA
    model = _model(name, precision)
    hp = TA.graph_precision(model)
    assert hp == {"bf16x3": 2, "fp32": 0}[precision]
    r64, _ = TC.reference(name)
    clear, (n_relu, zmin, dz32, flips32) = TC.kinks_are_clear(name)
    got = TC.evaluate(name, torch.float32, "cuda", hp, model)
    torch.cuda.synchronize()
    kind = TC.CASES[name]["kind"]
    need = set(TC.HIP_NODES[kind])
    if kind == "fine" and TC.CASES[name]["enable"]:
        need |= TC.HIP_NODES["transformer"]
    assert need <= got.nodes, (name, sorted(need - got.nodes))
    assert not [n for n in got.nodes if n.startswith(TC.TORCH_NODES)], sorted(got.nodes)
    # ReLU kinks: the conditions of the case, then the sides the device took
    _, _, dz_dev, flips_dev = TC.kink_margin(got.relus, r64.relus)
    ref = r64
    if TC.CASES[name].get("kinks") == "device_sides":
        assert flips32 == 0
        near = TC.BAR_FACTOR * dz32
        for zd, zr in zip(got.relus, r64.relus):
            differ = (zd.cpu() > 0) != (zr > 0)
            assert float(zr[differ].abs().max() if differ.any() else 0.0) <= near, "a pre-activation beyond rounding of zero changed sides"
        if flips_dev:
            ref = TC.evaluate(name, torch.float64, sides=[z.cpu() > 0 for z in got.relus])
            assert all(torch.equal(a, b) for a, b in zip(ref.outs.values(), r64.outs.values()))
    else:
        assert n_relu == 0 or clear, (name, zmin, dz32)
        assert flips_dev == 0, "%d pre-activations changed sides on the device (largest |z - z64| %.2e, min|z64| %.2e)" % (flips_dev, dz_dev, zmin)
    err, d32, bars = TC.errors(got, ref), TC.d32(name), TC.bars(name)
    for tag in ("out", "grad"):
        keys = [k for k in err if k.startswith(tag)]
        worst = max(keys, key=lambda k: err[k] - bars[k])
        print("%s %s %s: max |kernel - f64| = %.2e, max d32 = %.2e; nearest its bar: %s %.2e of %.2e" % (
            name, precision, tag, max(err[k] for k in keys), max(d32[k] for k in keys), worst, err[worst], bars[worst]))
    if n_relu:
        print("%s %s relu: %d pre-activations, max |z - z64| = %.2e (float32: %.2e), min|z64| = %.2e, %d took the other side" % (
            name, precision, n_relu, dz_dev, dz32, zmin, flips_dev))
    bad = {k: (err[k], bars[k], d32[k]) for k in err if not err[k] <= bars[k]}
    assert not bad, "(err, bar, d32) " + str(sorted(bad.items(), key=lambda kv: -kv[1][0] / max(kv[1][1], 1e-30))[:8])
    return got, r64, model


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", TC.names("matcher"))
def test_coarse_match_node_vs_fp64(name, precision):
    """A. `HipCoarseMatch.apply(f3, f2, aux)` with `aux` as `coarse_level_graph` builds it: the recomputed scores, `ctx.scale` (restated in
    the reference from the config, incl. feat_norm_method none), the -1e9 mask term and the zero padding of L to a multiple of 32"""
    from onepose_plus_plus_amd import _lib
    from onepose_plus_plus_amd import train_autograd as TA
    got, r64, model = _check(name, precision)
    inp = TC.inputs(name)
    mask = inp.consts["mask"]
    if mask is not None:
        dead = mask == 0
        assert (got.outs["conf"].cpu().transpose(1, 2)[dead] == 0).all(), "conf columns of masked cells must be exact zeros"
        assert (got.grads["f2"].cpu()[dead] == 0).all(), "grad f2 rows of masked cells must be exact zeros"
        assert (got.grads["f2"].cpu()[~dead].abs().amax(-1) > 0).all()
    # a second backward of the same graph gives the same bits (fixed-order reductions, nothing consumed by the first)
    t = TC.tensors(name, torch.float32, "cuda")
    conf = TC.forward(name, t, TA.graph_precision(model), model)["conf"]
    leaves = [t.leaves["f3"], t.leaves["f2"]]
    first = torch.autograd.grad(conf, leaves, t.grad_out["conf"], retain_graph=True)
    second = torch.autograd.grad(conf, leaves, t.grad_out["conf"])
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert torch.equal(first[0], got.grads["f3"]) and torch.equal(first[1], got.grads["f2"])
    # the node reset the context's query mask: a plain opp_coarse_match on the same context, mask state untouched here, sees every cell
    lib, c = model._ensure_ready(conf.device)
    B, N, hc, wc = TC.CASES[name]["shape"]
    L = hc * wc
    f3, f2, kpts = t.leaves["f3"].detach(), t.leaves["f2"].detach(), t.consts["kpts"]
    plain = torch.full((N, L), float("nan"), device="cuda")
    i_ids, j_ids = torch.empty(N, dtype=torch.int64, device="cuda"), torch.empty(N, dtype=torch.int64, device="cuda")
    mconf, mkc, mk3 = torch.empty(N, device="cuda"), torch.empty(N, 2, device="cuda"), torch.empty(N, 3, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(lib.opp_coarse_match_workspace_bytes(c, N, L), 4096), dtype=torch.uint8, device="cuda")
    _lib.check(lib.opp_coarse_match(c, f3[0].data_ptr(), f2[0].data_ptr(), N, hc, wc, kpts[0].data_ptr(), 8.0, None, plain.data_ptr(),
                                    i_ids.data_ptr(), j_ids.data_ptr(), mconf.data_ptr(), mkc.data_ptr(), mk3.data_ptr(), cnt.data_ptr(),
                                    ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "opp_coarse_match")
    torch.cuda.synchronize()
    sim = torch.einsum("lc,sc->ls", inp.leaves["f3"][0].double(), inp.leaves["f2"][0].double()) * TC.matcher_scale(TC.config(name))
    want = torch.softmax(sim, 0) * torch.softmax(sim, 1)
    e = float((plain.cpu().double() - want).abs().max()) / float(want.abs().max())
    assert e <= TC.bars(name)["out:conf"], e
    if mask is not None:
        assert (plain.cpu()[:, mask[0] == 0].amax(0) > 0).all()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", TC.names("layer"))
def test_encoder_layer_vs_fp64(name, precision):
    """B. `_encoder_layer(p_cuda, name, nhead, ...)` with `hp` set: the stacked [3C | 2C] x C projection node and its split, the masks
    handed to `HipLinearAttention`, `res_weight`, the constant affine of instancenorm through `HipLayerNorm`, segments of one token"""
    got, r64, _ = _check(name, precision)
    if "rezero" in TC.CASES[name]["settings"]:
        assert not [k for k in got.grads if ".norm" in k]                   # instancenorm: constants, nothing to take a gradient
        rw = [k for k in got.grads if k.endswith(".res_weight")]
        assert len(rw) == 1 and float(got.grads[rw[0]].abs().max()) > 0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", TC.names("transformer") + TC.names("kpt") + TC.names("fine"))
def test_graph_composition_vs_fp64(name, precision):
    """C. two layers through `_transformer` under a mask; D. `_kpt_encoding`; E. `fine_level_graph` with loftr_fine on and off"""
    got, r64, _ = _check(name, precision)
    if TC.CASES[name]["kind"] == "fine":
        assert set(got.grads) == set(r64.grads) and ("feat_f" in got.grads)
