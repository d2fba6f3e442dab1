"""The encoder options on the GPU: `loftr_*.rezero`, `loftr_*.norm_method: "instancenorm"`, `coarse_matching.feat_norm_method: "none"`
and `keypoints_encoding.norm_method: "layernorm"`, alone and together, against the reference's fixtures
(tests/golden/gen_encoder_options_golden.py) through every entry point of the module.

Bars are those of the default configuration (tests/helpers.py).  Fixtures with feat_norm_method none hold the reference's float64
outputs and `ref_fp32_err`, the reference's own fp32-to-fp64 distance in conf_matrix: their bar on conf_matrix / mconf is
max(1e-4, 2 * ref_fp32_err) (the generator's docstring gives the reason)."""
import hashlib

import numpy as np
import pytest
import torch

from onepose_plus_plus_amd import _lib
from onepose_plus_plus_amd.config import default_config
from onepose_plus_plus_amd.synthetic import make_state_dict
from tests import helpers as H
from tests import mask_cases as MC
from tests.golden import encopt_cases as EC

pytestmark = pytest.mark.gpu

PRECISIONS = ("bf16x3", "fp32")


def _tol_conf(gold):
    return max(H.TOL_CONF, 2.0 * float(gold["ref_fp32_err"])) if "ref_fp32_err" in gold else H.TOL_CONF


def _outputs(gold):
    return {k: v for k, v in gold.items() if k != "ref_fp32_err"}


# ---- 1. eval against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(EC.ENCOPT_E2E_CASES))
def test_eval_vs_reference(name, precision):
    from tests import hip_ops as ops
    cfg, sd, data = EC.e2e_setup(name)
    out = ops.run_model(ops.make_model(cfg, sd, precision), data)
    gold = H.load_golden(name)
    assert len(gold["mconf"]) > 0
    if EC.has_featnone(EC.VARIANTS[EC.ENCOPT_E2E_CASES[name][5]]):
        assert "ref_fp32_err" in gold and float(gold["mconf"].max()) > 0.99          # saturated softmaxes
    err = float(np.abs(out["conf_matrix"][0].cpu().numpy() - gold["conf_matrix"]).max())
    print("%s %s: max |conf - golden| = %.3e (bar %.3e), M = %d" % (name, precision, err, _tol_conf(gold), len(gold["mconf"])))
    H.assert_match_outputs(out, _outputs(gold), tol_conf=_tol_conf(gold), where=name)


# ---- 2. B = 2 with query_image_mask --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(EC.ENCOPT_BATCH_CASES))
def test_masked_batch_vs_reference(name, precision):
    from tests import hip_ops as ops
    cfg, sd, data = EC.batch_setup(name)
    out = ops.run_model(ops.make_model(cfg, sd, precision), data)
    gold = H.load_golden(name)
    assert len(gold["mconf"]) > 0
    H.assert_batched_outputs(out, _outputs(gold), tol_conf=_tol_conf(gold), where=name)
    m = data["query_image_mask"].flatten(-2).bool()
    conf = out["conf_matrix"].cpu()
    assert (~m).any() and (conf.transpose(1, 2)[~m] == 0).all()           # masked cells: exactly zero, never matched
    assert m[out["b_ids"].cpu(), out["j_ids"].cpu()].all()


# ---- 3. full attention with rezero and instancenorm ----------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(EC.ENCOPT_FULLATTN_CASES))
def test_full_attention_with_rezero_and_instancenorm(name, precision):
    from tests import hip_ops as ops
    cfg, sd, data = EC.fullattn_setup(name)
    assert cfg["loftr_coarse"]["attention"] == cfg["loftr_fine"]["attention"] == "full"
    out = ops.run_model(ops.make_model(cfg, sd, precision), data)
    gold = H.load_golden(name)
    assert len(gold["mconf"]) > 0
    H.assert_match_outputs(out, gold, where=name)


# ---- 4. fusion levels ----------------------------------------------------------------------------------------------------------
FUSION_SHAPES = [(0, 1, 96, 77), (0, 1, 65, 129), (0, 1, 31, 1), (1, 37, 25, 1)]


def _fusion_tokens(shape):
    which, n_seg, len0, len1 = shape
    g = torch.Generator().manual_seed(11 + len0 + n_seg)
    return torch.randn(n_seg * (len0 + len1), 256 if which == 0 else 128, generator=g)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", FUSION_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fusion_levels_are_bit_identical_with_rezero_and_instancenorm(shape, precision):
    """res_weight is folded into the packed norm2 affine and instancenorm is a constant affine, so the dense tail, enc_chain and
    enc_layer64 read the same operands: the transformer alone agrees bit for bit between the three levels (linear attention)."""
    from tests import hip_ops as ops
    which, n_seg, len0, len1 = shape
    cfg = EC.encopt_config(default_config(), ("rezero", "instancenorm"))
    sd = make_state_dict(cfg, 3)
    tokens = _fusion_tokens(shape)
    outs = [ops.transformer(ops.make_model(cfg, sd, precision).set_encoder_fusion(level).cuda(), which, tokens, n_seg, len0, len1)
            for level in (0, 1, 2)]
    for level, a in enumerate(outs):
        assert torch.isfinite(a).all(), level
        assert not torch.equal(a, tokens), level
        assert torch.equal(a, outs[0]), "level %d: max |fused - plain| = %.3e" % (level, (a - outs[0]).abs().max().item())


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("shape", FUSION_SHAPES[1:], ids=lambda s: "x".join(map(str, s)))
def test_zero_res_weight_returns_the_input_tokens(shape, level, precision):
    """x + 0 * message = x exactly, in every layer implementation"""
    from tests import hip_ops as ops
    which, n_seg, len0, len1 = shape
    cfg = EC.encopt_config(default_config(), ("rezero", "instancenorm"))
    sd = make_state_dict(cfg, 3)
    for k in sd:
        if k.endswith(".res_weight"):
            sd[k] = torch.zeros(1)
    tokens = _fusion_tokens(shape)
    out = ops.transformer(ops.make_model(cfg, sd, precision).set_encoder_fusion(level).cuda(), which, tokens, n_seg, len0, len1)
    assert torch.equal(out, tokens)


# ---- 5. object cache -----------------------------------------------------------------------------------------------------------
CACHE_KEYS = ("conf_matrix", "i_ids", "j_ids", "mconf", "expec_f", "mkpts_query_f")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_object_cache_changes_nothing(precision):
    from tests import hip_ops as ops
    cfg, sd, data = EC.e2e_setup("encopt_all4_128x128_n300")
    cached, plain = ops.make_model(cfg, sd, precision), ops.make_model(cfg, sd, precision)
    plain.cache_object_tokens = False
    resident = {k: v.cuda() for k, v in data.items()}
    outs = []
    for m in (cached, plain, cached):
        d = dict(resident)                    # the same keypoint / bank tensors: the third run hits the cache
        with torch.no_grad():
            m(d)
        outs.append(d)
    torch.cuda.synchronize()
    assert cached._rt["obj"] is not None and plain._rt.get("obj") is None
    for o in outs[1:]:
        for k in CACHE_KEYS:
            assert torch.equal(outs[0][k], o[k]), k


@pytest.mark.parametrize("precision", PRECISIONS)
def test_repack_carries_res_weight_and_keypoint_affine_into_the_next_eval(precision):
    """res_weight and the keypoint LayerNorm affine changed in place + repack(): the next eval on the SAME resident tensors equals a
    freshly built module that loaded the new state dict (the fold and the token cache follow the parameters)"""
    from tests import hip_ops as ops
    cfg, sd, data = EC.e2e_setup("encopt_all4_128x128_n300")
    model = ops.make_model(cfg, sd, precision)
    resident = {k: v.cuda() for k, v in data.items()}
    with torch.no_grad():
        d0 = dict(resident)
        model(d0)
        touched = 0
        for n, p in model.named_parameters():
            if n.endswith(".res_weight"):
                p.mul_(0.5).add_(0.1)
                touched += 1
            elif n.startswith("kpt_3d_pos_encoding.encoder.") and n.split(".")[2] in "147":
                p.mul_(1.25).add_(0.05)
                touched += 1
        assert touched == 8 + 6
        model.repack()
        d1 = dict(resident)
        model(d1)
        fresh = ops.make_model(cfg, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, precision)
        d2 = {k: v.clone() for k, v in resident.items()}
        fresh(d2)
    torch.cuda.synchronize()
    assert not torch.equal(d0["conf_matrix"], d1["conf_matrix"])
    for k in CACHE_KEYS:
        assert torch.equal(d1[k], d2[k]), k


# ---- 6. keypoint encoder kernel ------------------------------------------------------------------------------------------------
def _kpt_extent_ref(n):
    """one point has no extent (NaN tokens upstream): it is scaled by another cloud's bounding box, as a B > 1 sample is (quirk q4)"""
    return MC.kpt_extent_cloud() if n == 1 else None


def _kpt_ref_fp64(sd, kpts, bank, extent_ref):
    """float64 normalize_3d_keypoints + KeypointEncoding_linear with norm_method "layernorm" -> [n, 256]"""
    F = torch.nn.functional
    k = kpts[0].double()
    e = extent_ref.double() if extent_ref is not None else k
    x = (k - k.mean(0, keepdim=True)) / ((e.max(0).values - e.min(0).values).max() * 0.6)
    pre = "kpt_3d_pos_encoding.encoder."
    for i in (0, 3, 6, 9):
        x = F.linear(x, sd[pre + "%d.weight" % i].double(), sd[pre + "%d.bias" % i].double())
        if i < 9:
            x = F.relu(F.layer_norm(x, (x.shape[-1],), sd[pre + "%d.weight" % (i + 1)].double(), sd[pre + "%d.bias" % (i + 1)].double(), 1e-5))
    return bank[0].double().t() + x


@pytest.mark.parametrize("n", EC.KPT_KERNEL_SIZES)
def test_keypoint_encoder_layernorm_vs_fp64(n):
    """bar: MC.BAR_KPT of max(1, |ref|max), the bar of the existing keypoint-token tests (test_query_mask_gpu.py)"""
    from tests import hip_ops as ops
    cfg = EC.encopt_config(default_config(), ("kptln",))
    sd = make_state_dict(cfg, 5)
    kpts, bank = EC.kpt_kernel_inputs(n)
    ext = _kpt_extent_ref(n)
    tok = ops.encode_points(ops.make_model(cfg, sd), kpts, bank, extent_ref=ext)
    ref = _kpt_ref_fp64(sd, kpts, bank, ext)
    no_affine = dict(sd)
    for i in (1, 4, 7):
        no_affine["kpt_3d_pos_encoding.encoder.%d.weight" % i] = torch.ones_like(sd["kpt_3d_pos_encoding.encoder.%d.weight" % i])
        no_affine["kpt_3d_pos_encoding.encoder.%d.bias" % i] = torch.zeros_like(sd["kpt_3d_pos_encoding.encoder.%d.bias" % i])
    assert MC.rel_err(_kpt_ref_fp64(no_affine, kpts, bank, ext), ref) > 1e-2            # the affine matters on this input
    e = MC.rel_err(tok, ref)
    print("keypoint encoder with LayerNorm affine, N = %d: %.3e" % (n, e))
    assert tok.shape == (n, 256) and torch.isfinite(tok).all() and e < MC.BAR_KPT, (n, e)


@pytest.mark.parametrize("n", EC.KPT_KERNEL_SIZES)
def test_keypoint_encoder_without_affine_is_bit_identical_to_its_predecessor(n):
    """null affine pointers (the default "instancenorm"): the kernel's output has the sha256 that the kernel had before it took an
    affine (tests/golden/encopt_kpt_parent_digest.npz, written by tests/golden/gen_encoder_options_kpt_digest.py on that build)"""
    from tests import hip_ops as ops
    cfg = default_config()
    kpts, bank = EC.kpt_kernel_inputs(n)
    tok = ops.encode_points(ops.make_model(cfg, make_state_dict(cfg, 5)), kpts, bank, extent_ref=_kpt_extent_ref(n))
    assert torch.isfinite(tok).all()
    gold = H.load_golden(EC.KPT_PARENT_DIGEST)
    assert hashlib.sha256(tok.contiguous().numpy().tobytes()).hexdigest() == str(gold["n%d" % n])


# ---- 7. training ---------------------------------------------------------------------------------------------------------------
def _train_model(name, precision=None):
    from tests import hip_ops as ops
    cfg, sd, data = EC.train_setup(name)
    gold = H.load_golden(name)
    model = ops.make_model(cfg, sd, precision)
    model.train()
    model.train_randint = H.RecordedRandint([gold["randint_%d" % i] for i in range(int(gold["n_randint"]))])
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in data.items()}
    return cfg, model, d, gold


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(EC.ENCOPT_TRAIN_CASES))
def test_train_mode_forward_vs_reference(name, precision):
    cfg, model, d, gold = _train_model(name, precision)
    with torch.no_grad():
        model(d)
    torch.cuda.synchronize()
    H.assert_train_outputs(d, model.state_dict(), _outputs(gold), tol_conf=_tol_conf(gold), tol_bn=1e-4, where=name)
    assert d["gt_mask"].sum().item() == len(gold["b_ids"]) - len(gold["mconf"])


@pytest.mark.parametrize("name", list(EC.ENCOPT_TRAIN_CASES))
def test_training_step_gradients(name, monkeypatch):
    """The whole-graph bar of tests/test_e2e_gpu.py::test_training_step_gradients (rel 1e-2; the reason is given there).  The helper's
    list of whole tensors names a norm2 weight, which an instancenorm level does not have: it is replaced by the fixture's own list
    (the helper's other entries + every res_weight + the keypoint LayerNorm affine)."""
    cfg, model, d, gold = _train_model(name)
    model(d)                                                        # gradients enabled
    assert d["conf_matrix"].requires_grad and d["expec_f"].requires_grad
    H.assert_train_outputs(d, model.state_dict(), _outputs(gold), tol_conf=_tol_conf(gold), tol_bn=1e-4, where=name)
    wc, we = H.train_loss_weights(d["conf_matrix"].shape, d["expec_f"].shape)
    ((d["conf_matrix"] * wc.cuda()).sum() + (d["expec_f"] * we.cuda()).sum()).backward()
    grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    names = [str(n) for n in gold["grad_names"]]
    new = [n for n in names if n.endswith(".res_weight") or (n.startswith("kpt_3d_pos_encoding.encoder.") and n.split(".")[2] in "147")]
    assert len(new) == 8 + 6 and not any(".norm1." in n or ".norm2." in n for n in names)
    assert set(names) <= set(grads) and not any(".norm1." in n or ".norm2." in n for n in grads)
    tensors = EC.train_grad_tensors(cfg)
    for n in new:
        assert n in tensors and float(np.abs(gold["grad/" + n]).max()) > 0 and float(grads[n].abs().max()) > 0, n
    monkeypatch.setattr(H, "GRAD_TENSORS", tensors)
    H.assert_train_grads(grads, gold, rel=1e-2, where=name)


# ---- 8. temparature ------------------------------------------------------------------------------------------------------------
def test_temparature_raises_keyerror_before_any_launch(monkeypatch):
    from tests import hip_ops as ops
    cfg = default_config(thr=0.0)
    cfg["coarse_matching"]["feat_norm_method"] = "temparature"
    model = ops.make_model(cfg, make_state_dict(cfg, 0))
    calls = []
    lib = _lib.load()
    for sym in ("opp_forward_coarse", "opp_backbone", "opp_transformer", "opp_create", "opp_pack_weights", "opp_encode_points"):
        orig = getattr(lib, sym)
        monkeypatch.setattr(lib, sym, lambda *a, _o=orig, _s=sym: calls.append(_s) or _o(*a))
    _, _, data = EC.e2e_setup("encopt_rezero_64x96_n100")
    d = {k: v.cuda() for k, v in data.items()}
    with pytest.raises(KeyError, match="temparature"):
        model(d)
    model.train()
    with pytest.raises(KeyError, match="temparature"):
        model(d)
    assert calls == []
