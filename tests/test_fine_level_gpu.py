"""GPU: the fine level -- opp_fine's window gather, loftr_fine on M x (W^2 + 1) tokens and the expectation head -- at window sizes 3, 5
and 7 against oracle/onepose_oracle.py evaluated in float64 on the cases of tests/fine_cases.py.  The window size changes the kernels:
10 and 26 tokens per match run linattn_small_pair_kernel, 50 run the generic opp_linattn_kv / opp_linattn_apply pair with one segment per
match; the 32-token tiles of enc_chain.hip straddle matches differently; fine_head_kernel uses 9, 25 or 49 lanes and redoes the last
match in its spare waves when M % 4 != 0; fine_gather_kernel pads 1, 2 or 3 pixels.  tests/test_fine_cases_cpu.py shows that these
references are exact to a tenth of the bars below and move by 100 bars when the window is shifted by a pixel, flattened column-major,
paired with other points or converted to pixels with the scales swapped.

Bars (tests/fine_cases.py): transformer 5e-5 of max(1, |ref|max); offsets 1e-4; std column 5e-4 on the rows whose float64 variances
both exceed VAR_MIN (every row of the soft cases), finite and non-negative on the others; pixels 1e-3.

Measured on an MI355X (maxima over the cases of each test, bf16x3 / fp32; bars in brackets):
  gather + head                 offsets 3.9e-7 / 3.9e-7 [1e-4], std 2.6e-6 / 2.6e-6 [5e-4], pixels 3.6e-6 / 3.6e-6 [1e-3]
  whole stage                   offsets 2.9e-6 / 2.7e-6,        std 2.5e-6 / 2.5e-6,        pixels 1.2e-5 / 1.7e-5
  loftr_fine tokens             4.9e-7 / 5.3e-7 of max(1, |ref|max) [5e-5]; the same figures at encoder_fusion 0, 1, 2
  module forward, W = 3 / 7     expec_f 5.5e-6 / 6.2e-6 [1e-4], pixels 1.1e-5 / 3.8e-5 [1e-3], conf_matrix 4.5e-6 [1e-4]
A window origin off by one pixel in fine_gather_kernel, or Wwin for Wwin - 1 in the head's grid, turns these tests red.
"""
import pytest
import torch

from tests import fine_cases as FC

pytestmark = pytest.mark.gpu

PRECISIONS = ("bf16x3", "fp32")          # tests/hip_ops.py PRECISIONS
_models = {}


def _model(precision, W=5, fusion=2):
    """one module per configuration for the whole file (weights of FC.state_dict)"""
    from tests import hip_ops as ops
    key = (precision, W, fusion)
    if key not in _models:
        _models[key] = ops.make_model(FC.config(W), FC.state_dict(torch.float32), precision).set_encoder_fusion(fusion).cuda()
    return _models[key]


def _fine(precision, W, M, amp, scaled, run_transformer):
    """-> expec_f [M, 3], mkpts_query_f [M, 2]; one spare output row behind them must come back untouched"""
    from tests import hip_ops as ops
    feat, bank = FC.features(amp, M)
    i_ids, j_ids = FC.match_ids(M)
    q = FC.query_scale(scaled)
    ex, mf = ops.fine(_model(precision, W), feat, bank, i_ids, j_ids, FC.HW_C, FC.coarse_points(M, scaled), FC.BASE_SCALE,
                      q[0] if q is not None else None, run_transformer=int(run_transformer), spare_rows=1)
    assert ex.shape == (M + 1, 3) and mf.shape == (M + 1, 2)
    assert torch.isnan(ex[M:]).all() and torch.isnan(mf[M:]).all(), "rows past the last match were written"
    return ex[:M], mf[:M]


def _hold_to_reference(precision, W, M, run_transformer):
    """both amplitudes, with and without the query scale, against fine_ref"""
    for amp in FC.AMPS:
        rows = FC.std_rows(W, M, amp, run_transformer)
        for scaled in (True, False):
            ref_e, ref_m, _ = FC.fine_ref(W, M, amp, scaled, run_transformer, torch.float64)
            ex, mf = _fine(precision, W, M, amp, scaled, run_transformer)
            assert torch.isfinite(ex).all() and torch.isfinite(mf).all(), (W, M, amp, scaled)
            d = (ex.double() - ref_e).abs()
            off, px = d[:, :2].max().item(), (mf.double() - ref_m).abs().max().item()
            std = d[:, 2][rows].max().item() if rows.any() else 0.0
            print("fine %s W %d M %d amp %.1f scale %d transformer %d: offsets %.3e std %.3e (%d of %d rows) pixels %.3e"
                  % (precision, W, M, amp, scaled, run_transformer, off, std, int(rows.sum()), M, px))
            assert off < FC.BAR_OFFSET, (precision, W, M, amp, scaled, off)
            assert std < FC.BAR_STD, (precision, W, M, amp, scaled, std)
            assert (ex[:, 2] >= 0).all()
            assert px < FC.BAR_PIXEL, (precision, W, M, amp, scaled, px)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("M", FC.M_HEAD)
@pytest.mark.parametrize("W", FC.WINDOWS)
def test_gather_and_head_vs_fp64(W, M, precision):
    """opp_fine(run_transformer = 0): fine_gather_kernel and fine_head_kernel alone, the only outside view of the gather.  The float32
    oracle is 1.6e-6 from float64 here, so a window off by one pixel or one cell cannot hide."""
    _hold_to_reference(precision, W, M, False)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("M", FC.M_HEAD)
@pytest.mark.parametrize("W", FC.WINDOWS)
def test_fine_stage_vs_fp64(W, M, precision):
    """opp_fine(run_transformer = 1): gather, loftr_fine, head"""
    _hold_to_reference(precision, W, M, True)


@pytest.mark.parametrize("fusion", [0, 1, 2])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("W,M", [(W, M) for W in FC.WINDOWS for M in FC.M_TRANSFORMER] + [(FC.W_LARGE, FC.M_LARGE)])
def test_fine_transformer_vs_fp64(W, M, precision, fusion):
    """opp_transformer(which = 1, n_seg = M, len0 = W^2, len1 = 1) on the gathered tokens (border windows with all-zero rows included):
    every row within 5e-5 of max(1, |ref|max)"""
    from tests import hip_ops as ops
    ref = FC.transformer_ref(W, M, FC.AMP_SOFT, torch.float64)
    tokens = FC.transformer_tokens(W, M)
    out = ops.transformer(_model(precision, 5, fusion), 1, tokens, M, W * W, 1)
    assert out.shape == ref.shape and torch.isfinite(out).all()
    scale = max(1.0, ref.abs().max().item())
    d = (out.double() - ref).abs()
    errs = {"window rows": d[:M * W * W].max().item() / scale, "point rows": d[M * W * W:].max().item() / scale}
    print("fine transformer W %d M %d %s fusion %d: %s" % (W, M, precision, fusion, errs))
    assert max(errs.values()) < FC.BAR_TRANSFORMER, (W, M, precision, fusion, errs)


@pytest.mark.parametrize("run_transformer", [0, 1])
@pytest.mark.parametrize("W", FC.WINDOWS)
def test_empty_match_list_writes_nothing(W, run_transformer):
    """M = 0: the call returns 0 (ops.fine raises otherwise) and leaves a one-row output buffer as it found it"""
    from tests import hip_ops as ops
    feat, bank = FC.features(FC.AMP_SOFT, 0)
    none = torch.empty(0, dtype=torch.long)
    ex, mf = ops.fine(_model("bf16x3", W), feat, bank, none, none, FC.HW_C, torch.empty(0, 2), FC.BASE_SCALE, FC.query_scale(True)[0],
                      run_transformer=run_transformer, spare_rows=1)
    assert ex.shape == (1, 3) and mf.shape == (1, 2) and torch.isnan(ex).all() and torch.isnan(mf).all()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("W", FC.WINDOWS)
def test_equal_matches_give_equal_rows(W, precision):
    """rows of the match list with equal (i, j) give the same bits wherever they stand in the list, with and without the transformer"""
    for amp in FC.AMPS:
        for run_transformer in (False, True):
            ex, mf = _fine(precision, W, 41, amp, True, run_transformer)
            for a, b in FC.DUPLICATE_ROWS:
                assert torch.equal(ex[a], ex[b]) and torch.equal(mf[a], mf[b]), (W, precision, amp, run_transformer, a, b, ex[a], ex[b])
            a, b = FC.SAME_J_ROWS
            assert not torch.equal(ex[a], ex[b])
            a, b = FC.SAME_I_ROWS
            assert not torch.equal(ex[a], ex[b])


@pytest.mark.parametrize("window", FC.MODULE_WINDOWS)
def test_module_forward_vs_oracle_at_windows_3_and_7(window):
    """One forward through the module at 64 x 96 with 136 points, thr = 0 and border_rm = 0, against the float32 oracle at the bars of
    test_tiny_shapes_vs_oracle: the path users run (loftr_fine.window_size from the configuration, the choice between the dense fine map
    and the per-match patch pyramid), with matches on the border of the coarse grid."""
    from tests import hip_ops as ops
    cfg, sd, data = FC.module_case(window)
    ref = FC.module_ref(window, torch.float32)
    assert FC.border_matches(ref["j_ids"]) > 0, "no border match: the case tests nothing"
    out = ops.run_model(ops.make_model(cfg, sd), data)
    assert out["i_ids"].tolist() == ref["i_ids"].tolist() and out["j_ids"].tolist() == ref["j_ids"].tolist()
    assert out["expec_f"].shape == (len(ref["mconf"]), 3) and torch.isfinite(out["expec_f"]).all() and torch.isfinite(out["mkpts_query_f"]).all()
    errs = {k: (out[k].cpu() - ref[k]).abs().max().item() for k in FC.MODULE_BARS}
    print("module W %d: %d matches, %s" % (window, len(ref["mconf"]), errs))
    for k, bar in FC.MODULE_BARS.items():
        assert errs[k] < bar, (window, errs)
