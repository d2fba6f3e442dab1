"""Training with `attention: "full"` on the GPU (csrc/full_attention_train.hip): the forward-with-statistics and backward kernels through
the C ABI against float64 autograd, the `HipFullAttention` node against the plain-torch formula, and the whole training graph against
the reference's train()-mode fixtures (tests/golden/fullattn*_train_*.npz)."""
import math

import numpy as np
import pytest
import torch

from onepose_plus_plus_amd import _lib
from onepose_plus_plus_amd import train_autograd as TA
from tests import helpers as H
from tests.golden.fullattn_cases import fullattn_e2e_setup
from tests.golden.fullattn_train_cases import train_setup

pytestmark = pytest.mark.gpu

PRECISIONS = {"bf16x3": 3, "fp32": 0}
HP = {"bf16x3": 2, "fp32": 0}
NHEAD = 8

# (B, L, S, D, q / k factor)
MFMA_SHAPES = [(1, 96, 77, 32, 1.0), (2, 65, 129, 32, 1.0), (3, 64, 64, 32, 1.0), (1, 1, 64, 32, 1.0), (1, 200, 1, 32, 1.0),
               (1, 700, 1300, 32, 1.0),
               # peaked softmax: Q and K x 2 (logits x 4).  Not more: tests/golden/fullattn_cases.py -- at 3 an fp32 evaluation of the
               # reference's formula is itself 9e-5 away from float64
               (2, 65, 129, 32, 2.0)]
SMALL_SHAPES = [(1, 31, 1, 32, 1.0), (2, 32, 32, 32, 1.0), (37, 25, 1, 16, 1.0), (37, 1, 25, 16, 1.0), (1, 49, 1, 16, 1.0), (5, 9, 1, 16, 1.0),
                (3, 1, 1, 16, 1.0)]


def _inputs(B, L, S, D, factor, seed=0):
    g = torch.Generator().manual_seed(1000 * L + 10 * S + B + seed)
    q, k, v = (torch.randn(B, n, NHEAD, D, generator=g) for n in (L, S, S))
    go = torch.randn(B, L, NHEAD, D, generator=g)
    return (q * factor).cuda(), (k * factor).cuda(), v.cuda(), go.cuda()


def _attention(q, k, v):
    """the reference's formula (linear_attention.py:83-93) on plain torch operators, in the dtype of its inputs"""
    QK = torch.einsum("nlhd,nshd->nlsh", q, k)
    A = torch.softmax((1.0 / q.size(3) ** 0.5) * QK, dim=2)
    return torch.einsum("nlsh,nshd->nlhd", A, v)


def _autograd(q, k, v, go, dtype):
    qq, kk, vv = (t.detach().to(dtype).requires_grad_(True) for t in (q, k, v))
    out = _attention(qq, kk, vv)
    return (out.detach(),) + torch.autograd.grad((out * go.to(dtype)).sum(), (qq, kk, vv))


def _kernels(q, k, v, go, precision):
    """forward with lse + backward through the C ABI, every output pre-filled with NaN"""
    lib = _lib.load()
    B, L, Hh, D = q.shape
    S = k.shape[1]
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    out, lse = nan(B, L, Hh, D), nan(B, Hh, L)
    gq, gk, gv = nan(B, L, Hh, D), nan(B, S, Hh, D), nan(B, S, Hh, D)
    nb = lib.opp_full_attention_train_workspace_bytes(B, L, S, Hh, D)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.opp_full_attention_train_forward(q.data_ptr(), k.data_ptr(), v.data_ptr(), B, L, S, Hh, D, precision, out.data_ptr(),
                                                    lse.data_ptr(), ws.data_ptr(), nb, stream), "opp_full_attention_train_forward")
    _lib.check(lib.opp_full_attention_train_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), go.data_ptr(),
                                                     B, L, S, Hh, D, precision, gq.data_ptr(), gk.data_ptr(), gv.data_ptr(), ws.data_ptr(), nb,
                                                     stream), "opp_full_attention_train_backward")
    torch.cuda.synchronize()
    return out, lse, gq, gk, gv


def _rel(a, ref, scale=None):
    return float((a.double() - ref).abs().max()) / (float(ref.abs().max()) if scale is None else scale)


def _check_grads(got, ref64, ref32, where):
    """per tensor: distance from the float64 gradient relative to its largest entry <= max(1e-5, 3 d_ref), d_ref = the same distance of
    an fp32 evaluation of the reference's formula with torch operators (a tile-wise recomputation sums in another order than a
    whole-row softmax; both are correct fp32 evaluations).  A gradient that is identically zero (dq, dk with one key): absolute bar
    1e-5 max|dv|."""
    dv_max = float(ref64[2].abs().max())
    for name, g, r64, r32 in zip(("dq", "dk", "dv"), got, ref64, ref32):
        assert torch.isfinite(g).all(), (where, name)
        if float(r64.abs().max()) == 0.0:
            err = float(g.abs().max())
            print("%s %s: true gradient 0, |kernel| = %.3e (bar %.3e)" % (where, name, err, 1e-5 * dv_max))
            assert err <= 1e-5 * dv_max, (where, name, err)
            continue
        d_ref, d = _rel(r32, r64), _rel(g, r64)
        print("%s %s: d_ref = %.3e, kernel = %.3e" % (where, name, d_ref, d))
        assert d <= max(1e-5, 3.0 * d_ref), (where, name, d, d_ref)


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("shape", MFMA_SHAPES + SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_full_attention_train_kernels_vs_fp64(shape, precision):
    """out within 2e-5 max|ref| (the bar of test_full_attention_kernel_vs_fp64), lse within 2e-5 max|lse| of the float64 logsumexp,
    gradients within `_check_grads`; every output finite (pre-filled with NaN) and bit-identical on a second call"""
    B, L, S, D, factor = shape
    q, k, v, go = _inputs(B, L, S, D, factor)
    ref64 = _autograd(q, k, v, go, torch.float64)
    ref32 = _autograd(q, k, v, go, torch.float32)
    a = _kernels(q, k, v, go, PRECISIONS[precision])
    b = _kernels(q, k, v, go, PRECISIONS[precision])
    where = "%s %s" % ("x".join(map(str, shape)), precision)
    for x, y, name in zip(a, b, ("out", "lse", "dq", "dk", "dv")):
        assert torch.isfinite(x).all(), (where, name)
        assert torch.equal(x, y), (where, name)
    e_out = _rel(a[0], ref64[0])
    lse64 = torch.logsumexp(torch.einsum("nlhd,nshd->nhls", q.double(), k.double()) / D ** 0.5, dim=-1)          # [B, H, L]
    e_lse = float((a[1].double() * math.log(2.0) - lse64).abs().max()) / max(float(lse64.abs().max()), 1e-30)
    print("%s: out %.3e, lse %.3e" % (where, e_out, e_lse))
    assert e_out <= 2e-5, (where, e_out)
    assert e_lse <= 2e-5, (where, e_lse)
    _check_grads(a[2:], ref64[1:], ref32[1:], where)
    if L == 1 and S == 1:       # one token attending to itself: dv = dO exactly, dq = dk = 0 exactly
        assert torch.equal(a[4], go) and float(a[2].abs().max()) == 0.0 and float(a[3].abs().max()) == 0.0


def test_full_attention_train_refusals():
    lib = _lib.load()
    q, k, v, go = _inputs(1, 70, 5, 16, 1.0)
    out, lse = torch.zeros_like(q), torch.zeros(1, NHEAD, 70, device="cuda")
    args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), 1, 70, 5, NHEAD, 16)
    assert lib.opp_full_attention_train_forward(*args, 0, out.data_ptr(), lse.data_ptr(), None, 0, None) == -2      # D = 16, 70 rows
    q, k, v, go = _inputs(1, 40, 40, 32, 1.0)
    out, lse = torch.zeros_like(q), torch.zeros(1, NHEAD, 40, device="cuda")
    args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), 1, 40, 40, NHEAD, 32)
    assert lib.opp_full_attention_train_forward(*args, 1, out.data_ptr(), lse.data_ptr(), None, 0, None) == -2      # precision 1
    assert lib.opp_full_attention_train_forward(*args, 3, out.data_ptr(), lse.data_ptr(), None, 0, None) == 0
    g = torch.zeros_like(q)
    assert lib.opp_full_attention_train_backward(*args[:3], out.data_ptr(), lse.data_ptr(), go.data_ptr(), *args[3:], 3, g.data_ptr(),
                                                 g.data_ptr(), g.data_ptr(), None, 0, None) == -4                      # no workspace
    torch.cuda.synchronize()


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("shape", [(2, 65, 129, 32), (37, 25, 1, 16)], ids=lambda s: "x".join(map(str, s)))
def test_node_vs_plain_torch(shape, precision):
    """`HipFullAttention` under torch.autograd.grad against the plain-torch `_full_attention` (both measured from float64, the torch
    one setting the bar of `_check_grads`), with only q and with only k and v requiring a gradient"""
    B, L, S, D = shape
    q, k, v, go = _inputs(B, L, S, D, 1.0, seed=5)
    ref64 = _autograd(q, k, v, go, torch.float64)
    where = "node %s %s" % ("x".join(map(str, shape)), precision)
    for need in ((True, False, False), (False, True, True)):
        outs = []
        for hp in (HP[precision], None):
            t = [x.detach().clone().requires_grad_(n) for x, n in zip((q, k, v), need)]
            out = TA._full_attention(*t, hp=hp)
            assert (type(out.grad_fn).__name__ == "HipFullAttentionBackward") == (hp is not None)
            grads = torch.autograd.grad((out * go).sum(), [x for x, n in zip(t, need) if n])
            it = iter(grads)
            outs.append((out.detach(), [next(it) if n else None for n in need]))
        torch.cuda.synchronize()
        (o_hip, g_hip), (o_t, g_t) = outs
        assert _rel(o_hip, ref64[0]) <= 2e-5
        idx = [i for i, n in enumerate(need) if n]
        full = lambda gs: [gs[i] if gs[i] is not None else ref64[1 + i].float() for i in range(3)]
        _check_grads(full(g_hip), ref64[1:], full(g_t), "%s need=%s" % (where, idx))


# ---- the whole training graph ---------------------------------------------------------------------------------------------------
# whole backbone tensors of H.GRAD_TENSORS whose fixture gradient is compared at 1e-2 instead of 2e-3: a pre-activation within fp32
# rounding of zero takes different sides of a ReLU kink in two fp32 evaluations (tests/test_e2e_gpu.py::test_training_step_gradients,
# tests/test_encoder_options_gpu.py::test_training_step_gradients).  Measured on the full / full fixture: 2.9e-3 .. 4.2e-3 for these four
# (their digests, and every digest of the backbone, stay within 2e-3: worst 7.9e-4); the transformer and keypoint-encoder tensors are at
# 1.3e-5 .. 3.5e-5 and keep 2e-3
BACKBONE_KINK_TENSORS = ("backbone.conv1.weight", "backbone.bn1.weight", "backbone.layer3.1.bn2.bias", "backbone.layer1_outconv.weight")


def _assert_grads(grads, gold, where, monkeypatch):
    """H.assert_train_grads at its default rel = 2e-3: the digest of EVERY parameter and the whole non-backbone tensors; the whole
    backbone tensors above at 1e-2"""
    assert all(n.startswith("backbone.") for n in BACKBONE_KINK_TENSORS) and set(BACKBONE_KINK_TENSORS) <= set(H.GRAD_TENSORS)
    strict = tuple(n for n in H.GRAD_TENSORS if n not in BACKBONE_KINK_TENSORS)
    assert any(n.startswith("loftr_coarse.") for n in strict) and any(n.startswith("loftr_fine.") for n in strict)
    monkeypatch.setattr(H, "GRAD_TENSORS", strict)
    H.assert_train_grads(grads, gold, where=where)
    monkeypatch.setattr(H, "GRAD_TENSORS", BACKBONE_KINK_TENSORS)
    H.assert_train_grads(grads, gold, rel=1e-2, where=where)


def _train_model(name, precision, graph=True):
    from tests import hip_ops as ops
    cfg, sd, data = train_setup(name)
    gold = H.load_golden(name)
    model = ops.make_model(cfg, sd, precision)
    model.full_attention_training = True
    model.train()
    model.train_randint = H.RecordedRandint([gold["randint_%d" % i] for i in range(int(gold["n_randint"]))])
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in data.items()}
    if graph:
        model(d)
    else:
        with torch.no_grad():
            model(d)
    torch.cuda.synchronize()
    return cfg, model, d, gold


def _grad_report(grads, gold, where):
    """largest error of every digest / tensor in the units of H.assert_train_grads, by group"""
    worst = {}
    for n, (gs, gn) in zip([str(x) for x in gold["grad_names"]], gold["grad_digest"]):
        g = grads[n].double().cpu()
        e = max(abs(float(g.norm()) - gn) / max(gn, 1e-12), abs(float(g.sum()) - gs) / max(gn * g.numel() ** 0.5, 1e-12))
        grp = n.split(".")[0]
        if e > worst.get(grp, ("", 0.0))[1]:
            worst[grp] = (n, e)
    for n in H.GRAD_TENSORS:
        v = gold["grad/" + n]
        e = float(np.abs(H.to_np(grads[n]) - v).max() / np.abs(v).max())
        print("%s whole tensor %s: %.3e" % (where, n, e))
    for grp, (n, e) in sorted(worst.items()):
        print("%s worst digest of %s: %s %.3e" % (where, grp, n, e))


def _step(name, precision):
    cfg, model, d, gold = _train_model(name, precision)
    assert d["conf_matrix"].requires_grad and d["expec_f"].requires_grad
    H.assert_train_outputs(d, model.state_dict(), gold, tol_bn=1e-4, where=name)
    wc, we = H.train_loss_weights(d["conf_matrix"].shape, d["expec_f"].shape)
    ((d["conf_matrix"] * wc.cuda()).sum() + (d["expec_f"] * we.cuda()).sum()).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert set(str(n) for n in gold["grad_names"]) <= set(grads)
    for n, g in grads.items():
        assert torch.isfinite(g).all(), n
        if n.startswith(("loftr_coarse.", "loftr_fine.")):
            assert float(g.abs().max()) > 0, n
    _grad_report(grads, gold, "%s %s" % (name, precision))
    return cfg, model, grads, gold


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_training_step_gradients_vs_reference(precision, monkeypatch):
    """`full_attention_training = True`, the fixture's draws replayed: outputs with the helpers of the linear-attention train tests,
    every parameter gradient against the reference's own autograd (`_assert_grads`)"""
    name = "fullattn_train_b2_64x96_n150"
    cfg, model, grads, gold = _step(name, precision)
    _assert_grads(grads, gold, name, monkeypatch)


def test_training_step_mixed_levels(monkeypatch):
    """coarse full, fine linear: one forward + backward; gradients finite, non-zero in both transformers, and equal to the reference's"""
    name = "fullattn_coarse_train_b2_64x96_n150"
    cfg, model, grads, gold = _step(name, "bf16x3")
    assert cfg["loftr_coarse"]["attention"] == "full" and cfg["loftr_fine"]["attention"] == "linear"
    _assert_grads(grads, gold, name, monkeypatch)


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_training_graph_matches_the_fused_train_forward(precision):
    """with the opt-in, the graph of HIP nodes and the no-grad fused train()-mode forward select the same matches, and their
    confidences / offsets agree within the bars of tests/test_train_bwd_gpu.py's linear-attention version of this test"""
    name = "fullattn_train_b2_64x96_n150"
    _, _, g, _ = _train_model(name, precision, graph=True)
    _, _, f, _ = _train_model(name, precision, graph=False)
    assert g["conf_matrix"].requires_grad and not f["conf_matrix"].requires_grad
    assert torch.equal(g["b_ids"], f["b_ids"]) and torch.equal(g["i_ids"], f["i_ids"]) and torch.equal(g["j_ids"], f["j_ids"])
    assert float((g["conf_matrix"].detach() - f["conf_matrix"]).abs().max()) <= H.TOL_CONF
    assert float((g["mconf"].detach() - f["mconf"]).abs().max()) <= H.TOL_CONF
    assert float((g["expec_f"].detach()[:, :2] - f["expec_f"][:, :2]).abs().max()) <= H.TOL_OFFSET
    assert float((g["mkpts_query_f"] - f["mkpts_query_f"]).abs().max()) <= H.TOL_PIXEL


def test_eval_outputs_do_not_depend_on_the_opt_in():
    from tests import hip_ops as ops
    cfg, sd, data = fullattn_e2e_setup("fullattn_e2e_128x128_n300_thr0")
    off, on = ops.make_model(cfg, sd), ops.make_model(cfg, sd)
    on.full_attention_training = True
    a, b = ops.run_model(off, data), ops.run_model(on, data)
    assert len(a["mconf"]) > 0
    for k in ("conf_matrix", "i_ids", "j_ids", "mconf", "expec_f", "mkpts_query_f"):
        assert torch.equal(a[k], b[k]), k
