"""Full attention on the GPU (csrc/full_attention.hip through include/opp_hip.h `opp_full_attention` and the model): the kernels against
an fp64 softmax attention, loftr_coarse and the whole model against the reference's full-attention fixtures, and the refusals."""
import numpy as np
import pytest
import torch

from onepose_plus_plus_amd import _lib
from onepose_plus_plus_amd.synthetic import make_state_dict
from tests import helpers as H
from tests.golden.fullattn_cases import (FULLATTN_TRANSFORMER_CASES, FULLATTN_E2E_CASES, FULLATTN_BATCH_CASES, fullattn_transformer_setup,
                                         fullattn_e2e_setup, fullattn_batch_setup, full_config)

pytestmark = pytest.mark.gpu

PRECISIONS = {"bf16x3": 3, "fp32": 0}


def _full_attention(qkv, n_seg, len0, len1, C, nhead, cross, precision):
    lib = _lib.load()
    msg = torch.full((qkv.shape[0], C), float("nan"), device="cuda")
    nb = lib.opp_full_attention_workspace_bytes(n_seg, len0, len1, C, nhead)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")
    _lib.check(lib.opp_full_attention(qkv.data_ptr(), n_seg, len0, len1, C, nhead, cross, precision, msg.data_ptr(), ws.data_ptr(), nb,
                                      torch.cuda.current_stream().cuda_stream), "opp_full_attention")
    torch.cuda.synchronize()
    return msg


def _reference(qkv, n_seg, len0, len1, C, nhead, cross):
    """fp64 softmax attention of both streams (stream 0 = [n_seg][len0] rows first), on the device in query chunks"""
    x = qkv.double()
    D = C // nhead
    T0 = n_seg * len0
    s0 = x[:T0].view(n_seg, len0, 3, nhead, D)
    s1 = x[T0:].view(n_seg, len1, 3, nhead, D)

    def att(qs, ks):
        out = []
        for i in range(0, qs.shape[1], 1024):
            logits = torch.einsum("nlhd,nshd->nlsh", qs[:, i:i + 1024, 0], ks[:, :, 1]) / D ** 0.5
            out.append(torch.einsum("nlsh,nshd->nlhd", torch.softmax(logits, 2), ks[:, :, 2]))
        return torch.cat(out, 1)
    o0 = att(s0, s1 if cross else s0).reshape(T0, C)
    o1 = att(s1, s0 if cross else s1).reshape(-1, C)
    return torch.cat([o0, o1], 0)


SHAPES = [(1, 4096, 5000, 256, 8), (1, 4096, 15000, 256, 8), (1, 96, 77, 256, 8), (1, 31, 1, 256, 8), (1, 65, 129, 256, 8),
          (1, 1, 64, 256, 8), (500, 25, 1, 128, 8), (37, 25, 1, 128, 8), (1, 25, 1, 128, 8), (37, 9, 1, 128, 8),
          (37, 49, 1, 128, 8)]


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_full_attention_kernel_vs_fp64(shape, precision, cross, sharp):
    """error <= 2e-5 max|ref|, finite everywhere (msg prefilled with NaN), bit-identical on a second call.  sharp: Q and K scaled so
    that |logit| / sqrt(D) reaches ~60 (a missing max subtraction overflows exp, a wrong rescale shows)"""
    n_seg, len0, len1, C, nhead = shape
    g = torch.Generator().manual_seed(7 * len0 + 3 * len1 + cross)
    qkv = torch.randn(n_seg * (len0 + len1), 3 * C, generator=g)
    if sharp:       # Q and K x 3.5: logits x 12.25, max |logit| / sqrt(D) ~ 60 at the large shapes
        qkv[:, :2 * C] *= 3.5
    x = qkv.cuda()
    ref = _reference(x, n_seg, len0, len1, C, nhead, cross)
    a = _full_attention(x, n_seg, len0, len1, C, nhead, cross, PRECISIONS[precision])
    b = _full_attention(x, n_seg, len0, len1, C, nhead, cross, PRECISIONS[precision])
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)
    err = float((a.double() - ref).abs().max())
    assert err <= 2e-5 * float(ref.abs().max()), (err, float(ref.abs().max()))


def test_full_attention_refuses_other_precisions():
    lib = _lib.load()
    qkv = torch.zeros(10, 768, device="cuda")
    msg = torch.zeros(10, 256, device="cuda")
    assert lib.opp_full_attention(qkv.data_ptr(), 1, 5, 5, 256, 8, 0, 1, msg.data_ptr(), None, 0, None) == -2


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("name", list(FULLATTN_TRANSFORMER_CASES))
def test_full_attention_transformer_stage_vs_golden(name, precision):
    from tests import hip_ops as ops
    cfg, sd, tokens2d, bank = fullattn_transformer_setup(name)
    L, n = tokens2d.shape[1], bank.shape[2]
    model = ops.make_model(cfg, sd, precision)
    x = torch.cat([tokens2d[0], bank[0].t().contiguous()], 0)
    y = ops.transformer(model, 0, x, 1, L, n)
    H.assert_transformer_digest(H.transformer_digest(y[L:], y[:L]), H.load_golden(name), rel=5e-5, where=name)


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("name", list(FULLATTN_E2E_CASES))
def test_full_attention_e2e_vs_golden(name, precision):
    from tests import hip_ops as ops
    cfg, sd, data = fullattn_e2e_setup(name)
    out = ops.run_model(ops.make_model(cfg, sd, precision), data)
    gold = H.load_golden(name)
    assert len(gold["mconf"]) > 0
    H.assert_match_outputs(out, gold, where=name)


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("name", list(FULLATTN_BATCH_CASES))
def test_full_attention_batch_vs_golden(name, precision):
    from tests import hip_ops as ops
    cfg, sd, data = fullattn_batch_setup(name)
    out = ops.run_model(ops.make_model(cfg, sd, precision), data)
    gold = H.load_golden(name)
    assert len(np.unique(gold["b_ids"])) == len(FULLATTN_BATCH_CASES[name][4])
    H.assert_batched_outputs(out, gold, where=name)


def _launch_counter(monkeypatch):
    calls = []
    lib = _lib.load()
    for sym in ("opp_forward_coarse", "opp_backbone", "opp_transformer", "opp_create", "opp_pack_weights"):
        orig = getattr(lib, sym)
        monkeypatch.setattr(lib, sym, lambda *a, _o=orig, _s=sym: calls.append(_s) or _o(*a))
    return calls


def test_full_attention_mask_and_training_refusals(monkeypatch):
    from tests import hip_ops as ops
    cfg, sd, data = fullattn_e2e_setup("fullattn_e2e_128x128_n300_thr0")
    model = ops.make_model(cfg, sd)
    calls = _launch_counter(monkeypatch)
    d = {k: v.cuda() for k, v in data.items()}
    d["query_image_mask"] = torch.ones(1, 16, 16, device="cuda")
    with pytest.raises(TypeError, match="q_mask"):
        model(d)
    selfonly = full_config(H.default_config(thr=0.0))
    selfonly["loftr_coarse"]["layer_names"] = ["self"]
    m2 = ops.make_model(selfonly, {k: v for k, v in sd.items() if k in dict(ops.OnePosePlus_model(selfonly).state_dict())})
    with pytest.raises(NotImplementedError):
        m2(d)
    model.train()
    d.pop("query_image_mask")
    with pytest.raises(NotImplementedError, match="training"):
        model(d)
    assert calls == []


def test_full_attention_object_cache_changes_nothing():
    from tests import hip_ops as ops
    cfg, sd, data = fullattn_e2e_setup("fullattn_e2e_128x128_n300_thr0")
    cached, plain = ops.make_model(cfg, sd), ops.make_model(cfg, sd)
    plain.cache_object_tokens = False
    outs = [ops.run_model(m, data) for m in (cached, plain, cached)]
    for o in outs[1:]:
        for k in ("conf_matrix", "i_ids", "j_ids", "mconf", "expec_f", "mkpts_query_f"):
            assert torch.equal(outs[0][k], o[k]), k
    lib, ctx = ops.ctx_of(cached)
    assert lib.opp_object_prefix_bytes(ctx, 300) == 0


# (which, n_seg, len0, len1): coarse tiles that end inside a 32-row block and a one-token stream; fine windows, many segments and one
FUSION_SHAPES = [(0, 1, 96, 77), (0, 1, 65, 129), (0, 1, 31, 1), (1, 37, 25, 1), (1, 1, 25, 1)]


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("shape", FUSION_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_full_attention_encoder_fusion_levels_are_bit_identical(shape, precision):
    """A full-attention layer behind its softmax attention is the dense merge / norm1 / MLP / norm2 GEMMs (encoder_fusion 0) or one
    fused launch on the given message (1 and 2; bf16x3 only -- fp32 ignores the level): both walk K in the same k16-steps with the
    same bf16 products, so the whole transformer must agree bit for bit between the three levels, at both levels of the model."""
    from tests import hip_ops as ops
    which, n_seg, len0, len1 = shape
    cfg = full_config(H.default_config())
    sd = make_state_dict(cfg, 3)
    g = torch.Generator().manual_seed(11 + len0 + n_seg)
    tokens = torch.randn(n_seg * (len0 + len1), 256 if which == 0 else 128, generator=g)
    outs = [ops.transformer(ops.make_model(cfg, sd, precision).set_encoder_fusion(level).cuda(), which, tokens, n_seg, len0, len1)
            for level in (0, 1, 2)]
    for level, a in enumerate(outs):
        assert torch.isfinite(a).all(), level
        assert not torch.equal(a, tokens), level
        assert torch.equal(a, outs[0]), "level %d: max |fused - plain| = %.3e" % (level, (a - outs[0]).abs().max().item())
