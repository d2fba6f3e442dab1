"""GPU: the per-sample state of the coarse level -- `query_image_mask` (opp_set_query_mask) and the keypoint extent of batch element 0
(opp_set_keypoint_extent_ref) -- through every kernel that reads it, against oracle/onepose_oracle.py evaluated in float64 on the cases
of tests/mask_cases.py.  The mask is read with its own tile offset in the QKV epilogue of the MFMA GEMM, in the fused 64-token encoder
layer kernel, in the dense score GEMM and in the three split-operand score kernels (gemm_mfma.hip, enc_layer64.hip, gemm_ss.hip); the
shapes put masked cells into a second and third tile of each.  tests/test_mask_cases_cpu.py shows that these references move by 200
times the bars below when the mask is dropped or shifted.

Measured on an MI355X (maxima over the cases of each test; bars in brackets):
  transformer, masks a / b / d, all rows        bf16x3 9.2e-7, fp32 9.1e-7 of max(1, |ref|max)  [5e-5]; bit-identical at encoder_fusion 0, 1, 2
  conf_matrix, masks a / b, four score paths    bf16x3 5.4e-6, fp32 7.4e-6 absolute             [1e-4]; mconf the same figures
  match lists                                   equal to the reference's in all 48 cases (41 .. 461 matches, at most one non-decisive)
  keypoint tokens, N = 2 .. 2100, extent case   1.5e-7 of max(1, |ref|max)                       [3e-5]
  keypoint tokens, cloud centred on (5, -3, 2)  1.0e-6; the float32 oracle itself is 1.6e-6 from float64 on that input  [3e-5]
No combination of arithmetic, encoder_fusion and score path is refused by the library: nothing skips.
"""
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import mask_cases as MC

pytestmark = pytest.mark.gpu

PRECISIONS = ("bf16x3", "fp32")
# (set_score_two_sweep, OPP_SS_RES3): the dense score GEMM, two sweeps, one sweep on the three-resident kernel (default) and on the
# two-resident one
SCORE_PATHS = {"dense": (0, None), "two_sweep": (1, None), "single_res3": (2, None), "single_res2": (2, "0")}
_models = {}


def _model(precision, fusion=2, score=2, kpt_enc=True):
    """one module per configuration for the whole file (weights of MC.state_dict)"""
    from tests import hip_ops as ops
    key = (precision, fusion, score, kpt_enc)
    if key not in _models:
        m = ops.make_model(MC.config(kpt_enc), MC.state_dict(torch.float32, kpt_enc), precision)
        _models[key] = m.set_encoder_fusion(fusion).set_score_two_sweep(score).cuda()
    return _models[key]


def _refused(call):
    """runs `call`; a configuration the library refuses as unsupported skips with the library's own words, any other error is a failure"""
    from onepose_plus_plus_amd._lib import OppError
    try:
        return call()
    except OppError as e:
        if "unsupported" in str(e):
            pytest.skip(str(e))
        raise


def _transformer(shape, kind, precision, fusion):
    from tests import hip_ops as ops
    L, n = shape[0] * shape[1], shape[2]
    return _refused(lambda: ops.transformer(_model(precision, fusion=fusion), 0, MC.transformer_tokens(shape), 1, L, n, mask=MC.mask(shape, kind)))


def _match(shape, kind, precision, path):
    from tests import hip_ops as ops
    score, res3 = SCORE_PATHS[path]
    f3d, f2d, kpts = MC.matcher_inputs(shape)
    before = os.environ.get("OPP_SS_RES3")
    if res3 is not None:
        os.environ["OPP_SS_RES3"] = res3
    try:
        return _refused(lambda: ops.coarse_match(_model(precision, score=score), f3d, f2d, shape[:2], kpts, 8.0, None, mask=MC.mask(shape, kind)))
    finally:
        if res3 is not None:
            if before is None:
                del os.environ["OPP_SS_RES3"]
            else:
                os.environ["OPP_SS_RES3"] = before


@pytest.mark.parametrize("fusion", [0, 1, 2])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["a", "b", "d"])
@pytest.mark.parametrize("shape", MC.SHAPES)
def test_masked_transformer_vs_fp64(shape, kind, precision, fusion):
    """opp_transformer(which = 0, n_seg = 1) under a query mask: every row within 5e-5 of max(1, |ref|max).  The masked image rows count:
    the stage returns them, and with a zero message the reference defines them as x + norm2(mlp([x, norm1.bias])) per layer."""
    L = shape[0] * shape[1]
    ref = MC.transformer_ref(shape, kind)
    out = _transformer(shape, kind, precision, fusion)
    assert torch.isfinite(out).all()
    m = MC.mask(shape, kind).bool()
    scale = max(1.0, ref.abs().max().item())
    d = (out.double() - ref).abs()
    errs = {"unmasked image rows": d[:L][m].max().item() / scale, "masked image rows": d[:L][~m].max().item() / scale,
            "point rows": d[L:].max().item() / scale}
    print("transformer %s mask %s %s fusion %d: %s" % (shape, kind, precision, fusion, errs))
    assert max(errs.values()) < MC.BAR_TRANSFORMER, (shape, kind, precision, fusion, errs)


@pytest.mark.parametrize("fusion", [0, 1, 2])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", MC.SHAPES)
def test_all_ones_mask_is_no_mask_in_the_transformer(shape, precision, fusion):
    """multiplying by 1.0f may not change a bit, and no kernel choice may depend on the mask pointer"""
    a, b = _transformer(shape, "c", precision, fusion), _transformer(shape, None, precision, fusion)
    assert torch.equal(a, b), "max |all ones - no mask| = %.3e" % (a - b).abs().max().item()
    assert not torch.equal(a, _transformer(shape, "a", precision, fusion))


@pytest.mark.parametrize("path", list(SCORE_PATHS))
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", MC.SHAPES)
def test_all_ones_mask_is_no_mask_in_the_matcher(shape, precision, path):
    """adding 0.0f to the scores may not change a bit of conf_matrix, the match list or mconf"""
    a, b = _match(shape, "c", precision, path), _match(shape, None, precision, path)
    assert len(b["i_ids"]) > 20
    for k in ("conf_matrix", "i_ids", "j_ids", "mconf", "mkpts_query_c", "mkpts_3d_db"):
        assert torch.equal(a[k], b[k]), (k, (a[k].double() - b[k].double()).abs().max().item() if a[k].shape == b[k].shape else (a[k].shape, b[k].shape))


@pytest.mark.parametrize("path", list(SCORE_PATHS))
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["a", "b"])
@pytest.mark.parametrize("shape", MC.SHAPES)
def test_masked_matcher_vs_fp64(shape, kind, precision, path):
    """opp_coarse_match under a query mask on every score path: conf_matrix and mconf within 1e-4, masked columns exactly 0.0 and never
    matched, every decisive reference match reported as (i, j), and nothing reported that the reference could not report (a reference
    match, or a pair within 1e-3 of thr and of its row and column maxima)."""
    ref = MC.matcher_ref(shape, kind)
    got = _match(shape, kind, precision, path)
    m = MC.mask(shape, kind).bool()
    conf = got["conf_matrix"][0]
    assert torch.isfinite(conf).all()
    err = (conf.double() - ref["conf"]).abs().max().item()
    i_ids, j_ids = got["i_ids"].tolist(), got["j_ids"].tolist()
    pairs = list(zip(i_ids, j_ids))
    merr = (got["mconf"].double() - ref["conf"][got["i_ids"], got["j_ids"]]).abs().max().item() if pairs else 0.0
    print("matcher %s mask %s %s %s: conf %.3e mconf %.3e, %d matches (reference %d, %d decisive)"
          % (shape, kind, precision, path, err, merr, len(pairs), len(ref["matches"]), len(ref["decisive"])))
    assert err < MC.BAR_CONF, (shape, kind, precision, path, err)
    assert (conf[:, ~m] == 0.0).all(), "masked columns carry confidence, max %.3e" % conf[:, ~m].abs().max().item()
    assert all(m[j] for j in j_ids), [j for j in j_ids if not m[j]][:10]
    assert i_ids == sorted(set(i_ids))                                   # one match per 3D point, ascending (quirk q9)
    missing = ref["decisive"] - set(pairs)
    assert not missing, ("decisive reference matches not reported", sorted(missing)[:10], len(missing))
    extra = [ij for ij in pairs if not ref["candidates"][ij[0], ij[1]]]
    assert not extra, ("reported pairs that are neither reference matches nor within 1e-3 of one", extra[:10], len(extra))
    assert merr < MC.BAR_CONF, (shape, kind, precision, path, merr)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_mask_of_one_sample_reaches_no_other_sample_and_no_later_call(precision):
    """B = 2 through the module at 160 x 208 (L = 520, N = 333): sample 0 has a padding mask, sample 1 an all-ones one.  The batch meets
    the float32 oracle at the bars of test_batched_masked_vs_golden; sample 1 does not see sample 0's mask (its outputs are bit-identical
    when sample 0's mask is all ones too); and the next, unmasked B = 1 call of the same module is bit-identical to a fresh module's."""
    from oracle import onepose_oracle as O
    from tests import hip_ops as ops
    cfg, sd, data = MC.batch_case()
    ref = dict(data)
    O.forward(sd, ref, cfg)
    gold = {k: H.to_np(ref[k]) for k in ("b_ids", "i_ids", "j_ids", "m_bids", "gt_mask", "mconf", "mkpts_query_c", "mkpts_3d_db", "expec_f",
                                         "mkpts_query_f", "conf_matrix")}
    gold["mkpts_query_c"] = gold["mkpts_query_c"].astype(np.float32)
    hw, hc, wc = MC.BATCH_HW, MC.BATCH_HW[0] // 8, MC.BATCH_HW[1] // 8
    gold["meta"] = np.array([2, hw[0], hw[1], hc, wc])
    assert len(gold["mconf"]) > 0 and set(gold["b_ids"].tolist()) == {0, 1}
    model = ops.make_model(cfg, sd, precision)
    out = ops.run_model(model, data)
    H.assert_batched_outputs(out, gold, where="b2 %s" % precision)
    m = data["query_image_mask"].flatten(-2).bool()
    conf = out["conf_matrix"].cpu()
    assert (~m[0]).sum() > 0 and (conf.transpose(1, 2)[~m] == 0).all()
    assert m[out["b_ids"].cpu(), out["j_ids"].cpu()].all()
    # sample 1 inside the batch: the same bits whether or not sample 0 is masked
    ones = dict(data, query_image_mask=torch.ones_like(data["query_image_mask"]))
    out1 = ops.run_model(ops.make_model(cfg, sd, precision), ones)
    c1 = out1["conf_matrix"].cpu()
    assert torch.equal(conf[1], c1[1]) and not torch.equal(conf[0], c1[0])
    s, s1 = (out["b_ids"] == 1).cpu(), (out1["b_ids"] == 1).cpu()
    for k in ("i_ids", "j_ids", "mconf", "expec_f", "mkpts_query_f"):
        assert torch.equal(out[k].cpu()[s], out1[k].cpu()[s1]), k
    # the next call: sample 1 alone, no mask key, on the used module and on a fresh one
    alone = {k: v[1:2].clone() for k, v in data.items() if k != "query_image_mask"}
    used = ops.run_model(model, alone)
    fresh = ops.run_model(ops.make_model(cfg, sd, precision), alone)
    assert len(fresh["mconf"]) > 0
    for k in ("conf_matrix", "i_ids", "j_ids", "mconf", "mkpts_query_c", "expec_f", "mkpts_query_f"):
        assert torch.equal(used[k], fresh[k]), k


# ---- keypoint tokens ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", MC.KPT_SIZES)
def test_keypoint_tokens_vs_fp64(n):
    """opp_encode_points against float64 KeypointEncoding_linear on normalize_3d_keypoints: one point short of, at and past the 32 points
    of a kpt_encode_kernel block and the 1024 threads of kpt_stats_kernel"""
    from tests import hip_ops as ops
    kpts, bank = MC.kpt_inputs(n)
    tok = ops.encode_points(_model("bf16x3"), kpts, bank)
    e = MC.rel_err(tok, MC.kpt_ref(kpts, bank))
    print("keypoint tokens N = %d: %.3e" % (n, e))
    assert tok.shape == (n, MC.C) and e < MC.BAR_KPT, (n, e)


def test_keypoint_tokens_with_the_extent_of_batch_element_0():
    """opp_set_keypoint_extent_ref: the cloud is centred on its own mean and scaled by the bounding box of ANOTHER cloud (quirk q4, B > 1);
    opp_coarse_tokens and opp_encode_points write the same point rows"""
    from tests import hip_ops as ops
    model = _model("bf16x3")
    kpts, bank = MC.kpt_inputs(MC.KPT_EXTENT_N)
    e0 = MC.kpt_extent_cloud()
    own, other = ops.encode_points(model, kpts, bank), ops.encode_points(model, kpts, bank, extent_ref=e0)
    e = MC.rel_err(other, MC.kpt_ref(kpts, bank, e0))
    print("keypoint tokens, extent of batch element 0: %.3e (own extent %.3e)" % (e, MC.rel_err(own, MC.kpt_ref(kpts, bank))))
    assert e < MC.BAR_KPT, e
    assert (own - other).abs().max().item() > 1e-2
    assert torch.equal(ops.encode_points(model, kpts, bank), own)                # the reference cloud does not outlive its call
    feat = torch.randn(1, MC.C, 3, 5, generator=torch.Generator().manual_seed(1))
    for ref_cloud, want in ((None, own), (e0, other)):
        tok = ops.coarse_tokens(model, feat, None, kpts, bank, extent_ref=ref_cloud)
        assert torch.equal(tok[15:], want)
        assert torch.equal(tok[:15], feat[0].permute(1, 2, 0).reshape(15, MC.C))


@pytest.mark.parametrize("n", MC.KPT_DISABLED_SIZES)
def test_point_tokens_without_keypoint_encoding_are_the_bank(n):
    """keypoints_encoding.enable = False (OnePosePlusModel.py:145-156 skips the encoder): bank_transpose_kernel, point rows = bank^T exactly"""
    from tests import hip_ops as ops
    model = _model("bf16x3", kpt_enc=False)
    kpts, bank = MC.kpt_inputs(n)
    assert torch.equal(ops.encode_points(model, kpts, bank), bank[0].t())
    feat = torch.randn(1, MC.C, 3, 5, generator=torch.Generator().manual_seed(2))
    assert torch.equal(ops.coarse_tokens(model, feat, None, kpts, bank)[15:], bank[0].t())


def test_keypoint_tokens_of_an_off_centre_cloud():
    """A cloud of extent 0.3 centred on (5, -3, 2): subtracting the mean in float32 loses digits, in the float32 reference as well.  Bar: 4
    times the float32 oracle's own distance from float64 on this input, but not below the 3e-5 of the centred clouds.  Measured on an
    MI355X: 1.0e-6 for the kernel, 1.6e-6 for the float32 oracle, so the bar is 3e-5."""
    from tests import hip_ops as ops
    n, centre, extent = MC.KPT_OFFCENTRE
    kpts, bank = MC.kpt_inputs(n, centre, extent)
    ref = MC.kpt_ref(kpts, bank)
    floor = MC.rel_err(MC.kpt_ref(kpts, bank, dtype=torch.float32), ref)
    e = MC.rel_err(ops.encode_points(_model("bf16x3"), kpts, bank), ref)
    bar = max(MC.BAR_KPT, 4.0 * floor)
    print("off-centre cloud: kernel %.3e, float32 oracle %.3e, bar %.3e" % (e, floor, bar))
    assert e < bar, "kernel %.3e from float64, float32 oracle %.3e, bar %.3e" % (e, floor, bar)
