"""Training with `attention: "full"` without a GPU: the functional restatement against the gradients of the reference's own autograd
(tests/golden/fullattn*_train_*.npz), the plain-torch formula of `train_autograd._full_attention`, the opt-in and its refusals, the
C ABI declarations and the static code-generation checks of csrc/full_attention_train.hip."""
import os
import re
import shutil
import tempfile

import numpy as np
import pytest
import torch

from onepose_plus_plus_amd import OnePosePlus_model, _lib
from onepose_plus_plus_amd import train_autograd as TA
from onepose_plus_plus_amd.config import default_config
from onepose_plus_plus_amd.model import _sine_table
from tests import helpers as H
from tests.golden.fullattn_cases import full_config
from tests.golden.fullattn_train_cases import FULLATTN_TRAIN_CASES, train_setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAS_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")


@pytest.mark.parametrize("name", list(FULLATTN_TRAIN_CASES))
def test_differentiable_forward_matches_reference_gradients(name):
    """`tests.torch_graph_ref.differentiable_forward` with FullAttention at the case's levels, on the fixture's inputs and matches,
    against the reference's train()-mode run: conf_matrix, expec_f and every parameter gradient.  The bars are those of
    tests/test_train_autograd_cpu.py for the linear-attention train fixtures (2e-5 / 5e-5 / rel 5e-4); they are met as they stand."""
    cfg, sd, data = train_setup(name)
    gold = H.load_golden(name)
    p = {k: v.clone().requires_grad_(not k.endswith(("running_mean", "running_var"))) for k, v in sd.items() if v.is_floating_point()}
    inputs = {k: data[k] for k in ("query_image", "keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
    inputs["query_image_mask"] = None
    matches = tuple(torch.from_numpy(gold[k]) for k in ("b_ids", "i_ids", "j_ids"))
    pe = _sine_table(256, cfg["positional_encoding"]["pos_emb_shape"])
    from tests.torch_graph_ref import differentiable_forward
    conf, expec = differentiable_forward(p, cfg, inputs, matches, pe)
    e_conf = np.abs(conf.detach().numpy() - gold["conf_matrix"]).max()
    e_off = np.abs(expec.detach().numpy() - gold["expec_f"])[:, :2].max()
    print("%s: |conf - ref| = %.3e, |offsets - ref| = %.3e" % (name, e_conf, e_off))
    assert e_conf < 2e-5
    assert e_off < 5e-5
    wc, we = H.train_loss_weights(conf.shape, expec.shape)
    names = [str(n) for n in gold["grad_names"]]
    grads = torch.autograd.grad((conf * wc).sum() + (expec * we).sum(), [p[n] for n in names])
    H.assert_train_grads(dict(zip(names, grads)), gold, rel=5e-4, where=name)


def _attention_fp64(q, k, v):
    logits = torch.einsum("nlhd,nshd->nhls", q, k) / q.shape[-1] ** 0.5
    return torch.einsum("nhls,nshd->nlhd", torch.softmax(logits, dim=-1), v)


def test_full_attention_fallback_formula_vs_fp64():
    """`_full_attention(hp=None)` against a float64 softmax attention at (B, L, S, H, D) = (2, 7, 5, 8, 16): forward and the three
    gradients within 1e-6 relative (of each tensor's largest entry)"""
    B, L, S, Hh, D = 2, 7, 5, 8, 16
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(B, n, Hh, D, generator=g, requires_grad=True) for n in (L, S, S))
    go = torch.randn(B, L, Hh, D, generator=g)
    out = TA._full_attention(q, k, v)
    grads = torch.autograd.grad((out * go).sum(), (q, k, v))
    q64, k64, v64 = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    ref = _attention_fp64(q64, k64, v64)
    refs = torch.autograd.grad((ref * go.double()).sum(), (q64, k64, v64))
    assert out.shape == (B, L, Hh, D) and out.dtype == torch.float32
    for what, a, b in [("out", out.detach(), ref.detach())] + list(zip(("dq", "dk", "dv"), grads, refs)):
        err = float((a.double() - b).abs().max())
        assert err <= 1e-6 * float(b.abs().max()), (what, err)


def test_transformer_dispatches_on_the_attention_setting():
    """any value but "linear" selects the softmax attention (transformer.py:29-38); "linear" keeps the linear one"""
    cfg = default_config()
    g = torch.Generator().manual_seed(0)
    from onepose_plus_plus_amd.synthetic import make_state_dict
    sd = make_state_dict(cfg, 1)
    f3, f2 = torch.randn(1, 9, 256, generator=g), torch.randn(1, 6, 256, generator=g)
    outs = {}
    for att in ("linear", "full", "anything"):
        t = dict(cfg["loftr_coarse"], attention=att)
        outs[att] = TA._transformer(sd, "loftr_coarse", t, f3, f2)
    assert torch.equal(outs["full"][0], outs["anything"][0]) and torch.equal(outs["full"][1], outs["anything"][1])
    assert not torch.equal(outs["full"][0], outs["linear"][0])
    with pytest.raises(NotImplementedError, match="mask"):
        TA._transformer(sd, "loftr_coarse", dict(cfg["loftr_coarse"], attention="full"), f3, f2, mask=torch.ones(1, 6))


class _FakeCuda(torch.Tensor):
    """a CPU tensor that reports is_cuda: takes a forward up to the first point the device is needed"""
    is_cuda = True


def _fake_device_data(masked):
    img = torch.zeros(1, 1, 64, 64).as_subclass(_FakeCuda)
    d = {"query_image": img}
    if masked:
        d["query_image_mask"] = torch.ones(1, 8, 8)
    return d


def test_training_refusal_is_the_default_and_the_opt_in_lifts_only_that():
    """default: `model.train()` with a full config raises NotImplementedError("... training ...") before anything else; with
    `full_attention_training = True` that refusal is gone, and the two mask refusals are still raised (checked up to the point the
    device is needed: the checks run before the first launch)"""
    cfg = full_config(default_config())
    m = OnePosePlus_model(cfg).train()
    assert OnePosePlus_model.full_attention_training is False and m.full_attention_training is False
    with pytest.raises(NotImplementedError, match="training"):
        m(_fake_device_data(False))
    with pytest.raises(NotImplementedError, match="training"):
        m._check_full_attention(False)
    m.full_attention_training = True
    m._check_full_attention(False)                                   # no refusal
    with pytest.raises(TypeError, match="q_mask"):
        m(_fake_device_data(True))
    selfonly = full_config(default_config())
    selfonly["loftr_coarse"]["layer_names"] = ["self"]
    m2 = OnePosePlus_model(selfonly).train()
    m2.full_attention_training = True
    with pytest.raises(NotImplementedError, match="query_image_mask"):
        m2(_fake_device_data(True))
    # a linear configuration is not concerned
    m3 = OnePosePlus_model(default_config()).train()
    m3._check_full_attention(True)
    assert hasattr(TA.HipFullAttention, "apply")


def test_abi_declares_the_training_trio():
    names = ("opp_full_attention_train_workspace_bytes", "opp_full_attention_train_forward", "opp_full_attention_train_backward")
    hdr = open(os.path.join(ROOT, "include", "opp_hip.h")).read()
    for n in names:
        assert n in _lib.SIGNATURES, n
        assert re.search(r"\b%s\s*\(" % n, hdr), n
    assert len(_lib.SIGNATURES["opp_full_attention_train_forward"][1]) == 14
    assert len(_lib.SIGNATURES["opp_full_attention_train_backward"][1]) == 18


def test_workspace_is_linear_in_the_token_counts():
    lib = _lib.load()
    nb = lib.opp_full_attention_train_workspace_bytes(1, 4096, 15000, 8, 32)
    assert 0 < nb <= 4 << 20
    assert lib.opp_full_attention_train_workspace_bytes(1, 15000, 4096, 8, 32) <= 4 << 20
    assert lib.opp_full_attention_train_workspace_bytes(1, 4096, 15000, 8, 8) == 0          # D = 8: no kernel
    assert lib.opp_full_attention_train_workspace_bytes(1, 65, 25, 8, 16) == 0              # D = 16 with a stream longer than 64 rows
    assert lib.opp_full_attention_train_workspace_bytes(65536, 25, 1, 8, 16) == 0           # B > 65535
    assert lib.opp_full_attention_train_workspace_bytes(500, 25, 1, 8, 16) > 0


@pytest.mark.skipif(not HAS_HIPCC, reason="needs hipcc")
def test_full_attention_train_kernels_have_no_scratch_and_fit_two_workgroups():
    """every kernel without scratch and without waterfall loops; the MFMA kernels (forward, dQ, dK/dV in both arithmetics) at
    vgpr + agpr <= 256 = two workgroups of 256 threads per CU, with MFMAs of the right kind in each arithmetic"""
    from tools import isa_audit
    with tempfile.TemporaryDirectory() as tmp:
        src, rows, err = isa_audit.audit_source("full_attention_train.hip", False, tmp)
        assert rows is not None, err
        text = open(os.path.join(tmp, "full_attention_train.hip.s")).read()
    names = [r[0] for r in rows]
    tile = [k for k in names if "fat_tile_kernel" in k]
    assert len(tile) == 6 and any("fat_small_bwd_kernel" in k for k in names) and any("fat_delta_kernel" in k for k in names)
    for k, vg, ag, sc, water, mfma, pk in rows:
        assert sc == 0 and water == 0, (k, sc, water)
        if "fat_tile_kernel" in k:
            assert mfma > 0, k
            assert vg + ag <= 256, (k, vg, ag)
        else:
            assert mfma == 0, k
    for k in tile:      # fat_tile_kernel<PREC, MODE>: PREC 2 = OPP_PREC_BF16X3, 0 = OPP_PREC_FP32
        body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(k), text, re.S | re.M).group(0)
        b3 = "fat_tile_kernelILi2E" in k
        assert ("v_mfma_f32_16x16x32_bf16" in body) == b3 and ("v_mfma_f32_16x16x4_f32" in body) == (not b3), k
