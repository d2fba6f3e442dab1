"""The 2D-2D matcher on the device against its float64 fixtures (tests/golden/loftr_*.npz, tests/loftr_reference.py): whole forward
at four thresholds, two windows and both arithmetics; the sequential encoder schedule alone at both levels; the workspace contract
of the new entry points; no state shared with a 2D-3D model of the same process; the detector on top of the matcher."""
import numpy as np
import pytest
import torch

from onepose_plus_plus_amd import AffineBoxDetector, _lib
from onepose_plus_plus_amd.loftr import LoFTRMatcher, default_cfg
from tests import helpers as H
from tests import hip_ops as ops
from tests import loftr_reference as R
from tests import memory_contract as MC
from tests.golden.loftr_cases import VARIANTS, WINDOWS, content_state_dict, detector_case, loftr_cfg, loftr_pair, loftr_state_dict

pytestmark = pytest.mark.gpu

PRECISIONS = ("bf16x3", "fp32")
GPU_PAIRS = ("loftr_96x128_128x96", "loftr_120x160")
_matchers, _sd = {}, []


def state_dict():
    if not _sd:
        _sd.append(loftr_state_dict())
    return _sd[0]


def matcher(precision, thr=default_cfg["match_coarse"]["thr"], window=9, fine=True, sd=None):
    key = (precision, thr, window, fine, id(sd))
    if key not in _matchers:
        m = LoFTRMatcher(loftr_cfg(thr, window), enable_fine_matching=fine).eval()
        m.load_state_dict(sd or state_dict(), strict=True)
        m.set_gemm_precision(precision)
        _matchers[key] = m.cuda()
    return _matchers[key]


def run(m, data_cpu):
    d = {k: v.cuda() for k, v in data_cpu.items()}
    with torch.no_grad():
        out = m(d)
    torch.cuda.synchronize()
    assert out is d
    return d


def _err(got, want):
    got, want = got.detach().double().cpu().numpy(), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max()) if want.size else 0.0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", GPU_PAIRS)
def test_forward_with_fine_level(name, variant, window, precision):
    gold = H.load_golden(name)
    thr = VARIANTS[variant][0]
    d = run(matcher(precision, thr, window), loftr_pair(name, variant))
    p = "%s/w%d/" % (variant, window)
    M = len(gold[p + "i_ids"])
    hw = [tuple(d["image%d" % k].shape[2:]) for k in (0, 1)]
    assert d["bs"] == 1 and tuple(d["hw0_i"]) == hw[0] and tuple(d["hw1_i"]) == hw[1]
    assert tuple(d["hw0_c"]) == (hw[0][0] // 8, hw[0][1] // 8) and tuple(d["hw1_f"]) == (hw[1][0] // 2, hw[1][1] // 2) and d["W"] == window
    e_conf = _err(d["conf_matrix"][0], gold["conf_matrix"])
    print("%s %s w%d %s: M %d, |conf - conf64| %.3e" % (name, variant, window, precision, M, e_conf))
    assert e_conf <= H.TOL_CONF
    for k in ("i_ids", "j_ids"):
        assert d[k].dtype == torch.int64 and np.array_equal(d[k].cpu().numpy(), gold[p + k]), (k, d[k].cpu().numpy(), gold[p + k])
    assert d["b_ids"].shape == (M,) and d["m_bids"].shape == (M,) and d["gt_mask"].dtype == torch.bool and not d["gt_mask"].any()
    errs = {k: _err(d[k], gold[p + k]) for k in ("mconf", "mkpts0_c", "mkpts1_c", "mkpts1_f")}
    errs["mkpts0_f"] = _err(d["mkpts0_f"], gold[p + "mkpts0_c"])
    assert tuple(d["expec_f"].shape) == (M, 3)
    errs["offset"] = _err(d["expec_f"][:, :2], gold[p + "expec_f"][:, :2])
    errs["std"] = _err(d["expec_f"][:, 2], gold[p + "expec_f"][:, 2])
    print("    " + ", ".join("%s %.3e" % kv for kv in errs.items()))
    assert errs["mconf"] <= H.TOL_CONF
    assert errs["offset"] <= H.TOL_OFFSET and errs["std"] <= H.TOL_OFFSET * H.STD_TOL_FACTOR
    for k in ("mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f"):
        assert errs[k] <= H.TOL_PIXEL, k
    if variant == "thr09":
        assert M == 0                                  # the empty branch: coarse points, empty expec_f
    if variant == "thr0005s":
        assert M >= 6


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", GPU_PAIRS)
def test_forward_coarse_only(name, variant, precision):
    """enable_fine_matching=False (SfM's coarse matching): mkpts*_f are the coarse points, no fine outputs"""
    gold = H.load_golden(name)
    d = run(matcher(precision, VARIANTS[variant][0], 9, fine=False), loftr_pair(name, variant))
    p = "%s/w9/" % variant
    assert _err(d["conf_matrix"][0], gold["conf_matrix"]) <= H.TOL_CONF
    for k in ("i_ids", "j_ids"):
        assert np.array_equal(d[k].cpu().numpy(), gold[p + k]), k
    assert _err(d["mconf"], gold[p + "mconf"]) <= H.TOL_CONF
    for k in ("0", "1"):
        assert _err(d["mkpts%s_c" % k], gold[p + "mkpts%s_c" % k]) <= H.TOL_PIXEL
        assert torch.equal(d["mkpts%s_f" % k], d["mkpts%s_c" % k])
    assert "expec_f" not in d and "W" not in d


def test_match_returns_the_fine_points():
    m = matcher("bf16x3", 0.005, 9)
    data = loftr_pair(GPU_PAIRS[0], "thr0005s")
    d = run(m, data)
    mk0, mk1, mconf = m.match(data["image0"].cuda(), data["image1"].cuda(), scale0=data["scale0"].cuda(), scale1=data["scale1"].cuda())
    assert torch.equal(mk0, d["mkpts0_f"]) and torch.equal(mk1, d["mkpts1_f"]) and torch.equal(mconf, d["mconf"]) and mk0.is_cuda


# ---- the encoder alone under the sequential schedule --------------------------------------------------------------------------
def _transformer(m, which, x, n_seg, len0, len1, bufs=None):
    lib, ctx = m._ensure_ready(torch.device("cuda", torch.cuda.current_device()))
    bufs = bufs or ops.DEFAULT_BUFFERS
    t = bufs.inout(x, "tokens")
    ws = bufs.workspace(lib.opp_transformer_workspace_bytes(ctx, which, n_seg, len0, len1))
    bufs.call(lib.opp_transformer(ctx, which, t.data_ptr(), n_seg, len0, len1, ws.data_ptr(), bufs.ws_bytes(ws),
                                  torch.cuda.current_stream().cuda_stream), "transformer")
    torch.cuda.synchronize()
    return t.cpu()


def _encoder_case(level, n_seg, len0, len1, seed):
    C = 256 if level == "coarse" else 128
    x = torch.randn(n_seg * (len0 + len1), C, generator=torch.Generator().manual_seed(seed))
    return x, x[:n_seg * len0].view(n_seg, len0, C), x[n_seg * len0:].view(n_seg, len1, C)


ENCODER_CASES = {"coarse-192+300": ("coarse", 1, 192, 300), "fine-m37-81+81": ("fine", 37, 81, 81), "fine-m37-25+25": ("fine", 37, 25, 25)}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", list(ENCODER_CASES))
def test_sequential_encoder_vs_fp64(case, precision):
    """distance from the float64 restatement relative to its largest entry <= max(1e-5, 3 d_ref), d_ref = the same distance of the
    float32 CPU restatement (the rule of tests/test_full_attention_train_gpu.py); and the parallel schedule is far away"""
    level, n_seg, len0, len1 = ENCODER_CASES[case]
    x, f0, f1 = _encoder_case(level, n_seg, len0, len1, 11)
    sd = state_dict()
    name, names, nhead = "loftr_" + level, default_cfg[level]["layer_names"], default_cfg[level]["nhead"]
    ref = {}
    for dt in (torch.float64, torch.float32):
        with torch.no_grad():
            a, b = R.transformer(R.cast_sd(sd, dt), name, nhead, names, f0.to(dt), f1.to(dt))
        ref[dt] = torch.cat([a.reshape(-1, x.shape[1]), b.reshape(-1, x.shape[1])]).double()
    with torch.no_grad():
        a, b = R.transformer(R.cast_sd(sd, torch.float64), name, nhead, names, f0.double(), f1.double(), sequential=False)
    par = torch.cat([a.reshape(-1, x.shape[1]), b.reshape(-1, x.shape[1])])
    got = _transformer(matcher(precision), 0 if level == "coarse" else 1, x, n_seg, len0, len1).double()
    scale = float(ref[torch.float64].abs().max())
    d_ref = float((ref[torch.float32] - ref[torch.float64]).abs().max()) / scale
    d = float((got - ref[torch.float64]).abs().max()) / scale
    d_par = float((par - ref[torch.float64]).abs().max()) / scale
    print("%s %s: d_ref %.3e, device %.3e, parallel schedule %.3e" % (case, precision, d_ref, d, d_par))
    assert torch.isfinite(got).all()
    assert d_par > 1e-2
    assert d <= max(1e-5, 3.0 * d_ref)


# ---- workspace contract of the new entry points (and of opp_transformer on its new path) ----------------------------------------
def _match2d(m, f0, f1, hw0, hw1, scales, bufs):
    lib, ctx = m._ensure_ready(torch.device("cuda", torch.cuda.current_device()))
    L0, L1 = hw0[0] * hw0[1], hw1[0] * hw1[1]
    a, b = bufs.input(f0, "f0"), bufs.input(f1, "f1")
    s0, s1 = bufs.input(scales[0], "scale0"), bufs.input(scales[1], "scale1")
    conf = bufs.output((L0, L1), name="conf")
    i_ids, j_ids = bufs.output(L0, torch.int64, -1, "i_ids"), bufs.output(L0, torch.int64, -1, "j_ids")
    mconf, mk0, mk1 = bufs.output(L0, name="mconf"), bufs.output((L0, 2), name="mkpts0_c"), bufs.output((L0, 2), name="mkpts1_c")
    cnt = bufs.output(1, torch.int32, 0, "count")
    ws = bufs.workspace(lib.opp_match2d_workspace_bytes(ctx, L0, L1))
    bufs.call(lib.opp_match2d(ctx, a.data_ptr(), b.data_ptr(), hw0[0], hw0[1], hw1[0], hw1[1], 8.0, s0.data_ptr(), s1.data_ptr(), conf.data_ptr(),
                              i_ids.data_ptr(), j_ids.data_ptr(), mconf.data_ptr(), mk0.data_ptr(), mk1.data_ptr(), cnt.data_ptr(), ws.data_ptr(),
                              bufs.ws_bytes(ws), torch.cuda.current_stream().cuda_stream), "match2d")
    torch.cuda.synchronize()
    M = int(cnt.item())
    assert (i_ids[M:] == -1).all() and torch.isnan(mk0[M:]).all(), "rows past the last match were written"
    return {"conf": conf.cpu(), "i_ids": i_ids[:M].cpu(), "j_ids": j_ids[:M].cpu(), "mconf": mconf[:M].cpu(), "mkpts0_c": mk0[:M].cpu(),
            "mkpts1_c": mk1[:M].cpu()}


def _planted2d(hw0, hw1, seed):
    """tokens of two grids with planted pairs (image 0's cells copied from image 1's with noise), some of them in the border bands"""
    g = torch.Generator().manual_seed(seed)
    L0, L1 = hw0[0] * hw0[1], hw1[0] * hw1[1]
    f0, f1 = torch.randn(L0, 256, generator=g) * 4, torch.randn(L1, 256, generator=g) * 4
    n = min(L0, L1) // 2
    rows, cols = torch.randperm(L0, generator=g)[:n], torch.randperm(L1, generator=g)[:n]
    f0[rows] = f1[cols] + 0.4 * torch.randn(n, 256, generator=g)
    return f0, f1, rows, cols


def _fine2d(m, ff0, ff1, hw0, hw1, i_ids, j_ids, mk1, scale1, bufs):
    lib, ctx = m._ensure_ready(torch.device("cuda", torch.cuda.current_device()))
    M = len(i_ids)
    a, b = bufs.input(ff0, "feat_f0"), bufs.input(ff1, "feat_f1")
    ii, jj = bufs.input(i_ids, "i_ids"), bufs.input(j_ids, "j_ids")
    k1, s1 = bufs.input(mk1, "mkpts1_c"), bufs.input(scale1, "scale1")
    ex, mf = bufs.output((M + 1, 3), name="expec_f"), bufs.output((M + 1, 2), name="mkpts1_f")
    ws = bufs.workspace(lib.opp_fine2d_workspace_bytes(ctx, M))
    bufs.call(lib.opp_fine2d(ctx, a.data_ptr(), hw0[0] * 4, hw0[1] * 4, b.data_ptr(), hw1[0] * 4, hw1[1] * 4, ii.data_ptr(), jj.data_ptr(), M, hw0[1],
                             hw1[1], 4, k1.data_ptr(), 2.0, s1.data_ptr(), ex.data_ptr(), mf.data_ptr(), ws.data_ptr(), bufs.ws_bytes(ws),
                             torch.cuda.current_stream().cuda_stream), "fine2d")
    torch.cuda.synchronize()
    assert torch.isnan(ex[M:]).all() and torch.isnan(mf[M:]).all(), "rows past the last match were written"
    return {"expec_f": ex.cpu(), "mkpts1_f": mf.cpu()}


def _contract_cases():
    out = []
    for precision in PRECISIONS:
        def match(b, s, precision=precision):
            hw0, hw1 = s
            f0, f1, rows, cols = _planted2d(hw0, hw1, hw0[0] * 100 + hw1[1])
            got = _match2d(matcher(precision, 0.2), f0, f1, hw0, hw1, (torch.tensor([1.5, 0.75]), torch.tensor([1.25, 2.0])), b)
            assert len(got["i_ids"]) > 5, len(got["i_ids"])
            return got
        shapes = [(((8, 12), (9, 11)), ((15, 20), (12, 16))), (((15, 20), (12, 16)), ((16, 24), (18, 20)))]
        out += [pytest.param(lambda b, s=s, f=match: f(b, s), lambda b, s=big, f=match: f(b, s), id="match2d-%dx%d-%dx%d-%s" % (s[0] + s[1] + (precision,)))
                for s, big in shapes]
        for window in WINDOWS:
            def fine(b, M, precision=precision, window=window):
                g = torch.Generator().manual_seed(M + window)
                hw0, hw1 = (6, 8), (7, 5)
                ff0, ff1 = (torch.randn(h * 4, w * 4, 128, generator=g) for h, w in (hw0, hw1))
                i_ids, j_ids = torch.randint(0, 48, (M,), generator=g), torch.randint(0, 35, (M,), generator=g)
                i_ids[0], j_ids[0] = 0, 34                                   # windows that hang over two corners of their maps
                return _fine2d(matcher(precision, 0.2, window), ff0, ff1, hw0, hw1, i_ids, j_ids, torch.rand(M, 2, generator=g) * 40, torch.tensor([1.25, 2.0]), b)
            out += [pytest.param(lambda b, M=M, f=fine: f(b, M), lambda b, M=big, f=fine: f(b, M), id="fine2d-w%d-m%d-%s" % (window, M, precision))
                    for M, big in ((1, 37), (37, 64))]
        for case, (level, n_seg, len0, len1) in ENCODER_CASES.items():
            def enc(b, n, level=level, len0=len0, len1=len1, precision=precision):
                x, _, _ = _encoder_case(level, n, len0, len1, 5)
                return {"tokens": _transformer(matcher(precision), 0 if level == "coarse" else 1, x, n, len0, len1, bufs=b)}
            big = (n_seg + 11) if level == "fine" else None
            larger = (lambda b, f=enc, n=big: f(b, n)) if level == "fine" else (lambda b, f=enc: f(b, 1, len0=256, len1=333))
            out.append(pytest.param(lambda b, f=enc, n=n_seg: f(b, n), larger, id="transformer-%s-%s" % (case, precision)))
    return out


@pytest.mark.parametrize("run_stage,larger", _contract_cases())
def test_new_entry_points_keep_the_memory_contract(run_stage, larger):
    problems = MC.fill_problems(run_stage, larger) + MC.refusal_problems(run_stage)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_match2d_selection_against_the_restatement(precision):
    """the selection on planted pairs, many of them in the border bands: the index set of the float64 restatement on the DEVICE's
    confidences (exact by construction), the keypoints of both images with scale0 != scale1"""
    hw0, hw1 = (15, 20), (12, 16)
    f0, f1, rows, cols = _planted2d(hw0, hw1, 77)
    s0, s1 = torch.tensor([1.5, 0.75]), torch.tensor([1.25, 2.0])
    got = _match2d(matcher(precision, 0.2), f0, f1, hw0, hw1, (s0, s1), ops.DEFAULT_BUFFERS)
    ref = R.conf_matrix(f0[None].double(), f1[None].double(), default_cfg["match_coarse"]["dsmax_temperature"])
    assert float((got["conf"].double() - ref[0]).abs().max()) <= H.TOL_CONF
    i, j, mconf = R.select(got["conf"][None], hw0, hw1, 0.2, 2)
    i_all, _, _ = R.select(got["conf"][None], hw0, hw1, 0.2, 0)
    assert len(i) > 10 and len(i_all) > len(i) + 10                    # the border removes pairs that pass every other test
    assert torch.equal(got["i_ids"], i) and torch.equal(got["j_ids"], j) and torch.equal(got["mconf"], mconf)
    mk0 = torch.stack([i % hw0[1], i // hw0[1]], 1).float() * (8.0 * s0[[1, 0]])
    mk1 = torch.stack([j % hw1[1], j // hw1[1]], 1).float() * (8.0 * s1[[1, 0]])
    assert torch.equal(got["mkpts0_c"], mk0) and torch.equal(got["mkpts1_c"], mk1)


def test_no_state_is_shared_with_a_2d3d_model():
    """a 2D-3D forward before and after a LoFTRMatcher forward of the same process: bit-identical outputs"""
    cfg, sd, data = H.e2e_setup("e2e_64x96_n100_thr01")
    model = ops.make_model(cfg, sd)
    keys = ("conf_matrix", "i_ids", "j_ids", "mconf", "mkpts_query_c", "mkpts_3d_db", "expec_f", "mkpts_query_f")
    before = {k: v.clone() for k, v in ops.run_model(model, data).items() if k in keys}
    run(matcher("bf16x3", 0.005, 9), loftr_pair(GPU_PAIRS[0], "thr0005s"))
    after = ops.run_model(model, data)
    assert len(before["i_ids"]) > 0
    for k in keys:
        assert torch.equal(MC.bits(before[k]), MC.bits(after[k])), k


@pytest.mark.parametrize("kind", ["uint8", "float"])
def test_detector_on_a_shifted_crop(kind):
    """AffineBoxDetector(m.as_detector_matcher(), [view]) on the frame the view was cut from: the box holds the view's corners moved by
    the known shift, each side within 8 px (one coarse cell).  Weights under which matching follows the content
    (tests/golden/loftr_cases.py: content_state_dict); uint8 views go through the device ingest, float views are uploaded as they are."""
    view, frame, (dy, dx) = detector_case()
    m = LoFTRMatcher(loftr_cfg(default_cfg["match_coarse"]["thr"], 9), enable_fine_matching=False).eval()
    m.load_state_dict(content_state_dict(), strict=True)
    m.cuda()
    if kind == "float":
        view, frame = view.float() / 255, frame.float().cuda() / 255
    det = AffineBoxDetector(m.as_detector_matcher(), [view])
    box = np.asarray(det(frame))
    want = np.array([dx, dy, dx + view.shape[1], dy + view.shape[0]])
    print("detector %s: box %s, the view lies at %s, view / inliers %s" % (kind, box, want, det.last))
    assert det.last[0] == 0 and det.last[1] >= 30
    assert np.abs(box - want).max() <= 8, (box, want)
