"""GPU: the workspace contract ("The workspace contract") of the C-ABI calls that take `(ws, ws_bytes)`, stage by stage.

For every entry of the table below, at every shape and in both arithmetics (bf16x3, fp32), the stage runs on `GuardedBuffers`
(tests/hip_ops.py) with a zero-filled, a NaN-filled (0x7FC00000 in every word) and a left-over workspace -- the prefix of the
allocation the same stage just used at a strictly larger shape, which is what `OnePosePlus_model._workspace` hands a small forward after a
large one -- and must
  1. return outputs that are bit-identical (integer views: NaN payloads and signed zeros count) to the zero-filled run, which is the run
     the reference tests of the other stage files pin: no new numeric bar here;
  2. leave the 4 KiB canary bands around its workspace, every output and every input intact, and its read-only inputs unchanged;
  3. refuse a workspace declared half as large as its size query says, and an empty one, with OPP_ERR_WORKSPACE (-4) and without
     changing a byte of an output, of the workspace or of a guard band.
tests/test_memory_contract_cpu.py shows on three fake stages in torch -- run here on the device as well -- that the harness tells a
clean stage from one that reads a workspace word before writing it and from one that stores one element past an output.

One stage is order-dependent by design: the window scatter of
opp_fine_window_gather_backward sums overlapping windows with fp32 atomicAdd (csrc/train_misc.hip, fine_scatter_batch_kernel) -- the only
floating-point atomic add in csrc/ (the matcher's atomicMax on LDS bit patterns is order-independent); it is held to 1e-5 by
test_train_bwd_gpu.py::test_fine_window_gather_node_vs_unfold, and the comparisons that include it (the fine_window_gather entry, the
backbone gradients of the graph step with the fine level) use that bar or the graph test's, not bit identity.

Workspace regions that hold indices, counters or flags, from a reading of every plan (csrc/api.hip plan_* and Arena uses; linear_bwd.hip
make_plan, loss.hip dsm_plan, linattn_train.hip make_plan, full_attention_train.hip, coarse_match.hip, gemm_ss.hip, conv_bwd.hip) -- a
NaN word read as an index is a large integer, so each was shown to be written before its first read BEFORE this file first ran; every
other region is floats (fp64 partials in loss.hip / conv_bwd.hip included) and left to the poison:
  - matcher scratch, row_arg / row_ties [Np] int (coarse_match.hip opp_dual_softmax_select layout): written for every row < N by
    conf_reg_kernel / conf_kernel (lane 0 of the row's wave), or by point_best_merge_kernel (thread per point) on the two-sweep path;
    first read by select_kernel, launched behind them, for rows < N only, and row_arg only where row_ties == 1.
  - matcher statistics, part_arg / part_ties [tl][N] int (two-sweep path): written by the OPP_SS_CONF sweep of gemm_ss.hip
    (ss_conf_tile, every cell tile x every column < N); first read by point_best_merge_kernel behind it, over t < tl, i < N.
  - convolution backward, geo [opp_conv_geo_entries(P)] int2 (pixel origin, valid-tap bits): conv_geo_kernel writes all P_pad entries
    (zeros behind P) before conv_wgrad_kernel reads the first ceil(P / 32) * 32 of them through a buffer descriptor of exactly that length.
  - there are no counters, tickets or flags in any workspace: `count` and the fp16x2 status flag are caller-owned outputs, the chunk
    partials of every reduction are indexed by block id.
What the refusal part holds the library to, beyond the error code: an entry that runs several stages (opp_forward_coarse, opp_fine,
opp_fine_patches, opp_coarse_tokens, opp_object_prefix) tries every stage's plan before its first launch, and a size query reports what
the plan of the same arguments takes, so that half of it is never enough.  Two-call rows (linear_attention_train, the taped backbone) have a
"forward" and a "backward" entry: in the second the forward gets its full size, so that the refusal seen is the backward's.

Entries that take no workspace -- opp_full_attention (its size query is 0 and `ws` is ignored), opp_fine_head_train_*,
opp_fine_window_gather and its backward -- are in the table for the bounds part: guard bands around every output (msg, expec_f, scratch_xy,
grad_f3, grad_win, windows, grad_feat_f) and unchanged inputs; there is nothing to refuse.  Where a call cannot fall short -- an empty
match list, the point encoder switched off -- the refusal part is left out as well.

Choices the issue's table leaves open: `fpn_overlap` is read by opp_forward_coarse alone (opp_backbone runs one stream), so the backbone
entry varies the stem and the forward_coarse entry the overlap.  opp_linear_backward refuses N = 196 as an argument (feature counts are
multiples of 32: the encoder's Linears are 128 / 256 wide), so the GEMM-backed shapes with 196 columns run as 1 x 1 convolutions over
M = 33 and 300 pixels through opp_conv2d_backward_nhwc.  Entries without an arithmetic option (attention, loss, normalisation kernels,
fine head, window gather) run once, opp_object_prefix only in bf16x3 (the fp32 configuration has no prefix).  Nothing skips.

The pose, pose-metrics, point-cloud, optimiser and tracking entry points allocate inside their Python front ends and are out of scope.

Measured on an MI355X: 315 cases, 9.2 s for the whole file (the largest case 0.6 s).
"""
import contextlib
import os

import pytest
import torch

from tests import fine_cases as FC
from tests import hip_ops as ops
from tests import mask_cases as MCASE
from tests import memory_contract as MC

pytestmark = pytest.mark.gpu

PRECISIONS = ops.PRECISIONS
PREC_ABI = {"bf16x3": 2, "fp32": 0}                 # `prec` of the building-block entries
SCORE_PATHS = {"dense": (0, None), "two_sweep": (1, None), "single_res3": (2, None), "single_res2": (2, "0")}    # test_query_mask_gpu.SCORE_PATHS
_models = {}


def _model(precision, fusion=2, score=2, kpt_enc=True, window=5, attention="linear", fpn_overlap=True):
    key = (precision, fusion, score, kpt_enc, window, attention, fpn_overlap)
    if key not in _models:
        from onepose_plus_plus_amd.synthetic import make_state_dict
        cfg = MCASE.config(kpt_enc)
        cfg["loftr_fine"]["window_size"] = window
        cfg["loftr_coarse"]["attention"] = attention
        m = ops.make_model(cfg, make_state_dict(cfg, MCASE.WEIGHT_SEED), precision)
        _models[key] = m.set_encoder_fusion(fusion).set_score_two_sweep(score).set_fpn_overlap(fpn_overlap).cuda()
    return _models[key]


@contextlib.contextmanager
def _env(name, value):
    before = os.environ.get(name)
    if value is not None:
        os.environ[name] = value
    try:
        yield
    finally:
        if value is not None:
            if before is None:
                del os.environ[name]
            else:
                os.environ[name] = before


def _g(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(s) for i, s in enumerate(seed)) % (2 ** 31))


def _chain(shapes, own):
    """[(shape, the next larger shape of the list, or `own` for the largest)]"""
    return [(s, shapes[i + 1] if i + 1 < len(shapes) else own) for i, s in enumerate(shapes)]


# ---- the table: name -> builder(precision) -> list of (case id, run, run_larger, options) ---------------------------------------
IMAGES = _chain([(40, 72), (64, 96)], (128, 192))
POINTS = _chain([77, 129, 257], 333)
TOKENS = _chain([(31, 1), (45, 77), (65, 129)], (96, 200))
MATCHER = _chain([(8, 12, 77), (16, 24, 300)], (16, 32, 333))          # (hc, wc, N): N x L = 77 x 96 and 300 x 384
GEMM = _chain([(33, 128, 128), (33, 196, 256), (300, 128, 256), (300, 196, 128)], (333, 256, 256))     # (M, N, K)
BATCH = (1, 3)
STAGES = {}


def stage(f):
    STAGES[f.__name__] = f
    return f


def _image(hw, B=1):
    return torch.rand(B, 1, hw[0], hw[1], generator=_g(hw[0], hw[1], B))


@stage
def backbone(precision):
    out = []
    for stem in ("direct", "im2col"):
        def run(b, hw, stem=stem):
            with _env("OPP_STEM_DIRECT", "0" if stem == "im2col" else None):
                fc, ff = ops.backbone(_model(precision), _image(hw), bufs=b)
            return {"feat_c": fc, "feat_f": ff}
        out += [("%s-%dx%d" % ((stem,) + hw), lambda b, hw=hw, run=run: run(b, hw), lambda b, big=big, run=run: run(b, big), {}) for hw, big in IMAGES]
    return out


@stage
def backbone_fine_branch(precision):
    def run(b, hw):
        g = _g(hw[0], hw[1], 5)
        x1 = torch.randn(hw[0] // 2, hw[1] // 2, 128, generator=g)
        x2o = torch.randn(hw[0] // 4, hw[1] // 4, 224, generator=g)
        x2o[..., 196:] = 0
        return {"feat_f": ops.backbone_fine_branch(_model(precision), x1, x2o, hw[0], hw[1], bufs=b)}
    return [("%dx%d" % hw, lambda b, hw=hw: run(b, hw), lambda b, big=big: run(b, big), {}) for hw, big in IMAGES]


def _points(n):
    g = _g(n, 3)
    return torch.rand(1, n, 3, generator=g) - 0.5, torch.randn(1, 256, n, generator=g)


@stage
def encode_points(precision):
    out = []
    for variant in ("encoder", "no-encoder", "extent-ref"):
        def run(b, n, variant=variant):
            k, bank = _points(n)
            ext = (torch.rand(50, 3, generator=_g(n, 9)) - 0.5) * 3 if variant == "extent-ref" else None
            return {"tokens3d": ops.encode_points(_model(precision, kpt_enc=variant != "no-encoder"), k, bank, extent_ref=ext, bufs=b)}
        # without the keypoint encoder the call takes nothing from its workspace: there is no size to fall short of
        opts = {"refusal": variant != "no-encoder"}
        out += [("%s-n%d" % (variant, n), lambda b, n=n, run=run: run(b, n), lambda b, big=big, run=run: run(b, big), opts) for n, big in POINTS]
    return out


@stage
def coarse_tokens(precision):
    out = []
    for variant in ("encoder", "no-encoder", "extent-ref"):
        def run(b, n, variant=variant):
            k, bank = _points(n)
            hc, wc = 5, 9
            g = _g(n, 11)
            fc, pe = torch.randn(1, 256, hc, wc, generator=g), torch.randn(hc * wc, 256, generator=g)
            ext = (torch.rand(50, 3, generator=_g(n, 9)) - 0.5) * 3 if variant == "extent-ref" else None
            return {"tokens": ops.coarse_tokens(_model(precision, kpt_enc=variant != "no-encoder"), fc, pe, k, bank, extent_ref=ext, bufs=b)}
        opts = {"refusal": variant != "no-encoder"}
        out += [("%s-n%d" % (variant, n), lambda b, n=n, run=run: run(b, n), lambda b, big=big, run=run: run(b, big), opts) for n, big in POINTS]
    return out


@stage
def object_prefix(precision):
    def run(b, n):
        blob = ops.object_prefix(_model(precision), torch.randn(n, 256, generator=_g(n, 13)), bufs=b)
        assert blob is not None, "the default configuration has an object prefix"
        return {"prefix": blob}
    # only the default arithmetic has a prefix (opp_object_prefix_bytes is 0 in fp32: every layer is evaluated per image)
    return [("n%d" % n, lambda b, n=n: run(b, n), lambda b, big=big: run(b, big), {}) for n, big in POINTS] if precision == "bf16x3" else []


@stage
def transformer(precision):
    out = []
    variants = [("coarse-fusion%d" % f, dict(fusion=f), False) for f in (0, 1, 2)]
    variants += [("coarse-full", dict(attention="full"), False), ("coarse-masked", {}, True)]
    for name, kw, masked in variants:
        def run(b, s, kw=kw, masked=masked):
            l0, l1 = s
            x = torch.randn(l0 + l1, 256, generator=_g(l0, l1))
            mask = None
            if masked:
                mask = torch.ones(l0)
                mask[::7] = 0
                mask[-1] = 0
            return {"tokens": ops.transformer(_model(precision, **kw), 0, x, 1, l0, l1, mask=mask, bufs=b)}
        out += [("%s-%dx%d" % ((name,) + s), lambda b, s=s, run=run: run(b, s), lambda b, big=big, run=run: run(b, big), {}) for s, big in TOKENS]
    for window, (M, bigM) in [(5, (1, 37)), (5, (37, 64)), (7, (37, 64))]:
        def run(b, M, window=window):
            ww = window * window
            x = torch.randn(M * (ww + 1), 128, generator=_g(M, ww))
            return {"tokens": ops.transformer(_model(precision, window=window), 1, x, M, ww, 1, bufs=b)}
        out.append(("fine-w%d-m%d" % (window, M), lambda b, M=M, run=run: run(b, M), lambda b, bigM=bigM, run=run: run(b, bigM), {}))
    return out


@stage
def linear_attention(precision):
    out = []
    for n_seg, C, shapes in ((1, 256, TOKENS), (3, 128, _chain([(25, 1), (49, 1)], (64, 3)))):
        for cross in (0, 1):
            def run(b, s, n_seg=n_seg, C=C, cross=cross):
                l0, l1 = s
                g = _g(l0, l1, n_seg)
                qkv = torch.randn(n_seg * (l0 + l1), 3 * C, generator=g)
                qkv[:, :2 * C] = qkv[:, :2 * C].abs() + 0.1            # phi(Q), phi(K) > 0
                return {"msg": ops.linear_attention(qkv, n_seg, l0, l1, C, 8, cross, bufs=b)}
            out += [("seg%d-%s-%dx%d" % ((n_seg, "cross" if cross else "self") + s), lambda b, s=s, run=run: run(b, s),
                     lambda b, big=big, run=run: run(b, big), {}) for s, big in shapes]
    return out if precision == "bf16x3" else []          # no arithmetic option: one set of cases


def _cell_mask(L):
    m = torch.ones(L)
    m[::5] = 0
    return m


def _planted(shape):
    """Inputs as test_two_sweep_matcher_equals_the_materialised_path plants them (tests/mask_cases.matcher_inputs: features of magnitude 4,
    points copied from cells with 0.4 noise), with the planted cells drawn from those a match can come from under border_rm = 2 and the
    mask of the masked variant, so that more than 20 matches exist at 77 x 96 as well.  -> f3d [N, 256], f2d [L, 256], kpts [N, 3]"""
    hc, wc, n = shape
    L = hc * wc
    g = _g(hc, wc, n)
    f2d = torch.randn(L, 256, generator=g) * 4
    f3d = torch.randn(n, 256, generator=g) * 4
    ok = _cell_mask(L).view(hc, wc).clone()
    ok[:2, :] = 0
    ok[:, :2] = 0
    cells = ok.flatten().nonzero().flatten()
    m = min(n // 2, len(cells))
    cells = cells[torch.randperm(len(cells), generator=g)[:m]]
    f3d[:m] = f2d[cells] + 0.4 * torch.randn(m, 256, generator=g)
    return f3d, f2d, torch.rand(n, 3, generator=g) - 0.5


@stage
def coarse_match(precision):
    out = []
    for path, (score, res3) in SCORE_PATHS.items():
        for masked in (False, True):
            def run(b, shape, score=score, res3=res3, masked=masked):
                f3d, f2d, kpts = _planted(shape)
                mask = _cell_mask(shape[0] * shape[1]) if masked else None
                with _env("OPP_SS_RES3", res3):
                    got = ops.coarse_match(_model(precision, score=score), f3d, f2d, shape[:2], kpts, 8.0, None, mask=mask, bufs=b)
                assert len(got["i_ids"]) > 20, len(got["i_ids"])
                return {k: got[k] for k in ("conf_matrix", "i_ids", "j_ids", "mconf", "mkpts_query_c", "mkpts_3d_db")}
            out += [("%s-%s-%dx%dx%d" % ((path, "masked" if masked else "plain") + s), lambda b, s=s, run=run: run(b, s),
                     lambda b, big=big, run=run: run(b, big), {}) for s, big in MATCHER]
    return out


@stage
def forward_coarse(precision):
    out = []
    for overlap in (True, False):
        def run(b, hw, n, overlap=overlap):
            k, bank = _points(n)
            L = (hw[0] // 8) * (hw[1] // 8)
            pe = torch.randn(L, 256, generator=_g(L, 17))
            return ops.forward_coarse(_model(precision, fpn_overlap=overlap), _image(hw), pe, k, bank, bufs=b)
        shapes = [(((40, 72), 77), ((64, 96), 129)), (((64, 96), 129), ((128, 192), 333))]
        out += [("%s-%dx%d-n%d" % (("overlap" if overlap else "one-stream",) + hw + (n,)), lambda b, hw=hw, n=n, run=run: run(b, hw, n),
                 lambda b, big=big, run=run: run(b, *big), {}) for (hw, n), big in shapes]
    return out


@stage
def fine(precision):
    out = []
    for window in (5, 7):
        for rt in (1, 0):
            def run(b, M, window=window, rt=rt):
                feat, bank = FC.features(FC.AMP_SOFT, M)
                i_ids, j_ids = FC.match_ids(M)
                ex, mf = ops.fine(_model(precision, window=window), feat, bank, i_ids, j_ids, FC.HW_C, FC.coarse_points(M, False), FC.BASE_SCALE, None,
                                  run_transformer=rt, spare_rows=1, bufs=b)
                assert torch.isnan(ex[M:]).all() and torch.isnan(mf[M:]).all(), "rows past the last match were written"
                return {"expec_f": ex, "mkpts_f": mf}
            # an empty match list needs no workspace and launches nothing: there is no size to fall short of
            out += [("w%d-%s-m%d" % (window, "transformer" if rt else "head", M), lambda b, M=M, run=run: run(b, M),
                     lambda b, big=big, run=run: run(b, big), {"refusal": M > 0}) for M, big in _chain([0, 1, 37], 64)]
    return out


@stage
def backbone_train(precision):
    def run(b, hw, B):
        fc, ff, st = ops.backbone_train(_model(precision), _image(hw, B), bufs=b)
        return {"feat_c": fc, "feat_f": ff, "bn_stats": st}
    return [("b%d-%dx%d" % ((B,) + hw), lambda b, hw=hw, B=B: run(b, hw, B), lambda b, big=big, B=B: run(b, big, B), {})
            for B in BATCH for hw, big in IMAGES]


@stage
def backbone_train_tape_and_backward(precision):
    """the taped forward and the backward on its tape: the tape is a guarded, NaN-prefilled output of the forward, so a gradient that is not
    finite shows a read of something the forward did not tape"""
    def run(b, hw, B, short_forward=True):
        g = _g(hw[0], hw[1], B, 21)
        gc, gf = torch.randn(B, hw[0] // 8, hw[1] // 8, 256, generator=g), torch.randn(B, hw[0] // 2, hw[1] // 2, 128, generator=g)
        out = ops.backbone_tape_backward(_model(precision), _image(hw, B), gc, gf, short_forward=short_forward, bufs=b)
        # (bn_stats: only the first 2 C of a layer's 512 floats are documented as written; the rest keeps the NaN prefill)
        bad = [k for k, v in out.items() if k != "bn_stats" and not bool(torch.isfinite(v).all())]
        assert not bad, bad
        return out
    out = []
    for B in BATCH:
        for hw, big in IMAGES:
            out.append(("forward-b%d-%dx%d" % ((B,) + hw), lambda b, hw=hw, B=B: run(b, hw, B), lambda b, big=big, B=B: run(b, big, B), {}))
            out.append(("backward-b%d-%dx%d" % ((B,) + hw), lambda b, hw=hw, B=B: run(b, hw, B, False), lambda b, big=big, B=B: run(b, big, B, False),
                        {"may_write": ("feat_c", "feat_f", "bn_stats", "tape", "ws_forward")}))
    return out


@stage
def fine_patches(precision):
    out = []
    H, W = 2 * FC.HW_F[0], 2 * FC.HW_F[1]
    for rt in (1, 0):
        def run(b, M, rt=rt):
            g = _g(M, 23)
            x1 = torch.randn(H // 2, W // 2, 128, generator=g)
            x2o = torch.randn(H // 4, W // 4, 224, generator=g)
            x2o[..., 196:] = 0
            _, bank = FC.features(FC.AMP_SOFT, M)
            i_ids, j_ids = FC.match_ids(M)
            ex, mf = ops.fine_patches(_model(precision), x1, x2o, H, W, bank, i_ids, j_ids, FC.HW_C, FC.coarse_points(M, False), FC.BASE_SCALE,
                                      run_transformer=rt, spare_rows=1, bufs=b)
            assert torch.isnan(ex[M:]).all() and torch.isnan(mf[M:]).all(), "rows past the last match were written"
            return {"expec_f": ex, "mkpts_f": mf}
        out += [("%s-m%d" % ("transformer" if rt else "head", M), lambda b, M=M, run=run: run(b, M), lambda b, big=big, run=run: run(b, big),
                 {"refusal": M > 0}) for M, big in _chain([0, 1, 37], 64)]
    return out


def _nhwc(B, H, W, c, g):
    cp = ops.pad32(c)
    t = torch.zeros(B, H, W, cp)
    t[..., :c] = torch.randn(B, H, W, c, generator=g)
    return t


@stage
def conv2d_backward(precision):
    # 196 channels (K tail packing, 224-column tiles), stride 1 and 2, a 1 x 1, and the long reduction of
    # test_conv_wgrad_long_reduction at the smallest size whose pixel range is cut into more than one split (B * H * W = 2 x 24 x 32)
    cases = [("s1-196", 196, 196, 3, 1, (5, 9), (10, 12)), ("s2-196", 128, 196, 3, 2, (10, 18), (16, 24)), ("1x1-s2", 196, 256, 1, 2, (10, 18), (16, 24)),
             ("ksplit", 64, 64, 3, 1, (24, 32), (32, 48)),
             # the GEMM-backed shapes with 196 columns (opp_linear_backward takes multiples of 32 only): 1 x 1 over M = 33 and 300 pixels at B = 1
             ("1x1-m33-k256", 256, 196, 1, 1, (3, 11), (15, 20)), ("1x1-m300-k128", 128, 196, 1, 1, (15, 20), (20, 24))]
    out = []
    for name, cin, cout, ks, stride, hw, big in cases:
        for B in BATCH:
            def run(b, hw, B=B, cin=cin, cout=cout, ks=ks, stride=stride):
                g = _g(hw[0], hw[1], B, cin, cout)
                x = _nhwc(B, hw[0], hw[1], cin, g)
                gy = _nhwc(B, (hw[0] + 2 * (ks // 2) - ks) // stride + 1, (hw[1] + 2 * (ks // 2) - ks) // stride + 1, cout, g)
                w = torch.randn(cout, cin, ks, ks, generator=g) / (cin * ks * ks) ** 0.5
                gx, gw = ops.conv2d_backward(x, w, gy, cin, cout, ks, stride, PREC_ABI[precision], bufs=b)
                return {"grad_x": gx.cpu(), "grad_w": gw.cpu()}
            out.append(("%s-b%d" % (name, B), lambda b, hw=hw, run=run: run(b, hw), lambda b, big=big, run=run: run(b, big), {}))
    return out


@stage
def batchnorm_backward(precision):
    def run(b, rows, C, act):
        ld = ops.pad32(C)
        g = _g(rows, C, act)
        def padded(t):
            o = torch.zeros(rows, ld)
            o[:, :C] = t
            return o
        raw, gy = torch.randn(rows, C, generator=g) * 2 + 0.5, torch.randn(rows, C, generator=g)
        mean, var = raw.mean(0), raw.var(0, unbiased=False)
        gamma = torch.rand(C, generator=g) + 0.5
        y = torch.relu((raw - mean) / torch.sqrt(var + 1e-5) * gamma)
        pm, pi = torch.zeros(ld), torch.zeros(ld)
        pm[:C], pi[:C] = mean, 1.0 / torch.sqrt(var + 1e-5)
        names = ("grad_raw", "grad_res", "grad_gamma", "grad_beta")
        return {k: v.cpu() for k, v in zip(names, ops.batchnorm_backward(padded(gy), padded(y), padded(raw), C, act, gamma, pm, pi, bufs=b))}
    shapes = [((45, 196), (180, 196)), ((180, 128), (720, 128)), ((720, 256), (1000, 256))]      # the predecessor keeps the row width
    return [("rows%d-c%d-act%d" % (s + (act,)), lambda b, s=s, act=act: run(b, *s, act), lambda b, big=big, act=act: run(b, *big, act), {})
            for s, big in shapes for act in (0, 1)] if precision == "bf16x3" else []


def _gemm_ok(shape):
    return shape[1] % 32 == 0 and shape[2] % 32 == 0


@stage
def linear_backward(precision):
    def run(b, s):
        M, N, K = s
        g = _g(M, N, K)
        gy, x, w = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
        dx, dw = ops.linear_backward(gy, x, w, PREC_ABI[precision], bufs=b)
        return {"grad_x": dx.cpu(), "grad_w": dw.cpu()}
    # N = 196 is no multiple of 32: opp_linear_backward refuses it as an argument error (the encoder's Linears are 128 / 256 wide), so the
    # GEMM-backed shapes with N = 196 run through conv2d_backward (above) and layer widths 128 / 256 here
    shapes = _chain([s for s, _ in GEMM if _gemm_ok(s)], (333, 256, 256))
    return [("m%d-n%d-k%d" % s, lambda b, s=s: run(b, s), lambda b, big=big: run(b, big), {}) for s, big in shapes]


@stage
def layer_norm_train_backward(precision):
    def run(b, rows, C):
        g = _g(rows, C)
        x, gy = torch.randn(rows, C, generator=g) * 3 + 1, torch.randn(rows, C, generator=g)
        gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
        return {k: v.cpu() for k, v in zip(("y", "grad_x", "grad_gamma", "grad_beta"), ops.layer_norm_train(x, gamma, beta, gy, bufs=b))}
    shapes = _chain([(33, 128), (300, 256)], (333, 256))
    return [("rows%d-c%d" % s, lambda b, s=s: run(b, *s), lambda b, big=big: run(b, *big), {"may_write": ("y", "mean", "rstd")})
            for s, big in shapes] if precision == "bf16x3" else []


def _heads(B, L, S, g):
    return (torch.randn(B, L, 8, 32, generator=g), torch.randn(B, S, 8, 32, generator=g), torch.randn(B, S, 8, 32, generator=g),
            torch.randn(B, L, 8, 32, generator=g))


@stage
def linear_attention_train(precision):
    def run(b, s, B, masked, short_forward=True):
        L, S = s
        g = _g(L, S, B)
        q, k, v, go = _heads(B, L, S, g)
        qm = (torch.rand(B, L, generator=g) < 0.8).float() if masked else None
        km = (torch.rand(B, S, generator=g) < 0.8).float() if masked else None
        names = ("out", "kv", "ks", "grad_q", "grad_k", "grad_v")
        return {n: t.cpu() for n, t in zip(names, ops.linear_attention_train(q, k, v, qm, km, go, short_forward=short_forward, bufs=b))}
    out = []
    # "forward": a short workspace stops the forward; "backward": the forward gets its full size, so that the backward's refusal is the one seen
    for which, short, opts in (("forward", True, {}), ("backward", False, {"may_write": ("out", "kv", "ks", "ws_forward")})):
        out += [("%s-b%d-%dx%d-%s" % ((which, B) + s + ("masked" if m else "plain",)), lambda b, s=s, B=B, m=m, short=short: run(b, s, B, m, short),
                 lambda b, big=big, B=B, m=m, short=short: run(b, big, B, m, short), opts) for B in BATCH for s, big in TOKENS for m in (False, True)]
    return out if precision == "bf16x3" else []


@stage
def full_attention_train(precision):
    def run(b, s, B):
        L, S = s
        q, k, v, go = _heads(B, L, S, _g(L, S, B, 1))
        names = ("out", "lse", "grad_q", "grad_k", "grad_v")
        return {n: t.cpu() for n, t in zip(names, ops.full_attention_train(q, k, v, go, 3 if precision == "bf16x3" else 0, bufs=b))}
    return [("b%d-%dx%d" % ((B,) + s), lambda b, s=s, B=B: run(b, s, B), lambda b, big=big, B=B: run(b, big, B), {"may_write": ("out", "lse")})
            for B in BATCH for s, big in TOKENS]


@stage
def dual_softmax(precision):
    def run(b, s, B):
        hc, wc, N = s
        L = hc * wc
        g = _g(N, L, B)
        S = torch.randn(B, N, L, generator=g) * 4
        S[:, :, ::7] -= 1e9
        lr, lc, conf = ops.dual_softmax_forward(S, bufs=b)
        ds = ops.dual_softmax_backward(torch.randn(B, N, L, generator=g), S, lr.cpu(), lc.cpu(), bufs=b)
        return {"lse_row": lr.cpu(), "lse_col": lc.cpu(), "conf": conf.cpu(), "grad_sim": ds.cpu()}
    return [("b%d-%dx%d" % (B, s[2], s[0] * s[1]), lambda b, s=s, B=B: run(b, s, B), lambda b, big=big, B=B: run(b, big, B), {})
            for B in BATCH for s, big in MATCHER] if precision == "bf16x3" else []


@stage
def dual_softmax_backward(precision):
    """the backward on its own: in `dual_softmax` a refused forward never reaches it"""
    def run(b, s, B):
        hc, wc, N = s
        L = hc * wc
        g = _g(N, L, B, 2)
        S = torch.randn(B, N, L, generator=g) * 4
        go = torch.randn(B, N, L, generator=g)
        return {"grad_sim": ops.dual_softmax_backward(go, S, torch.logsumexp(S, 2), torch.logsumexp(S, 1), bufs=b).cpu()}
    return [("b%d-%dx%d" % (B, s[2], s[0] * s[1]), lambda b, s=s, B=B: run(b, s, B), lambda b, big=big, B=B: run(b, big, B), {})
            for B in BATCH for s, big in MATCHER] if precision == "bf16x3" else []


@stage
def focal_loss(precision):
    def run(b, s, B):
        hc, wc, N = s
        L = hc * wc
        g = _g(N, L, B, 3)
        conf = torch.rand(B, N, L, generator=g)
        gt = (torch.rand(B, N, L, generator=g) < 0.1).float()
        m0, m1 = (torch.rand(B, N, generator=g) < 0.8).float(), (torch.rand(B, L, generator=g) < 0.9).float()
        sums, grad = ops.focal_loss(conf, gt, m0, m1, 0.5, 2.0, torch.tensor([0.7, 1.3]), bufs=b)
        return {"sums": sums.cpu(), "grad_conf": grad.cpu()}
    return [("b%d-%dx%d" % (B, s[2], s[0] * s[1]), lambda b, s=s, B=B: run(b, s, B), lambda b, big=big, B=B: run(b, big, B), {})
            for B in BATCH for s, big in MATCHER] if precision == "bf16x3" else []


# ---- entries that take no workspace: the fills change nothing for them, the guard bands and the input checks still hold them to their
# documented extents (full attention inside opp_transformer writes its message into the workspace, where no guard band stands) ----------
@stage
def full_attention(precision):
    out = []
    for n_seg, C, shapes in ((1, 256, TOKENS), (3, 128, _chain([(25, 1), (49, 1)], (64, 3)))):
        for cross in (0, 1):
            def run(b, s, n_seg=n_seg, C=C, cross=cross):
                l0, l1 = s
                qkv = torch.randn(n_seg * (l0 + l1), 3 * C, generator=_g(l0, l1, n_seg, 31))
                return {"msg": ops.full_attention(qkv, n_seg, l0, l1, C, 8, cross, 3 if precision == "bf16x3" else 0, bufs=b)}
            out += [("seg%d-%s-%dx%d" % ((n_seg, "cross" if cross else "self") + s), lambda b, s=s, run=run: run(b, s),
                     lambda b, big=big, run=run: run(b, big), {"refusal": False}) for s, big in shapes]
    return out


@stage
def fine_head_train(precision):
    def run(b, M, W):
        g = _g(M, W, 37)
        f3, win, ge = torch.randn(M, 128, generator=g), torch.randn(M, W * W, 128, generator=g), torch.randn(M, 3, generator=g)
        return dict(zip(("expec_f", "scratch_xy", "grad_f3", "grad_win"), ops.fine_head_train(f3, win, ge, bufs=b)))
    return [("w%d-m%d" % (W, M), lambda b, M=M, W=W: run(b, M, W), lambda b, big=big, W=W: run(b, big, W), {"refusal": False})
            for W, M, big in ((5, 1, 37), (5, 37, 64), (7, 37, 64))] if precision == "bf16x3" else []


@stage
def fine_window_gather(precision):
    """the gather, and the scatter of its backward: overlapping windows are summed with fp32 atomicAdd in whatever order the hardware takes
    them, so grad_feat_f is compared at the 1e-5 of test_fine_window_gather_node_vs_unfold, not bit for bit"""
    def run(b, geom):
        B, Hf, Wf, hc, wc, W, M = geom
        g = _g(*geom)
        feat = torch.randn(B, Hf, Wf, 128, generator=g)
        b_ids, j_ids = torch.randint(0, B, (M,), generator=g), torch.randint(0, hc * wc, (M,), generator=g)
        j_ids[:4] = torch.tensor([0, wc - 1, hc * wc - 1, (hc - 1) * wc])      # image corners: windows reach outside
        j_ids[5], b_ids[5] = j_ids[6], b_ids[6]                                  # a duplicate
        win, gf = ops.fine_window_gather(feat, b_ids, j_ids, hc, wc, W, torch.randn(M, W * W, 128, generator=g), bufs=b)
        return {"windows": win, "grad_feat_f": gf}
    shapes = _chain([(2, 16, 24, 4, 6, 5, 40), (3, 20, 28, 5, 7, 7, 37)], (3, 24, 36, 6, 9, 7, 64))
    return [("b%d-%dx%d-w%d-m%d" % (s[0], s[1], s[2], s[5], s[6]), lambda b, s=s: run(b, s), lambda b, big=big: run(b, big),
             {"refusal": False, "close": {"grad_feat_f": 1e-5}}) for s, big in shapes] if precision == "bf16x3" else []


def _cases():
    out = []
    for name, build in STAGES.items():
        for precision in PRECISIONS:
            for case_id, run, larger, opts in build(precision):
                out.append(pytest.param(run, larger, opts, id="%s-%s-%s" % (name, case_id, precision)))
    return out


@pytest.mark.parametrize("run,larger,opts", _cases())
def test_stage_keeps_the_memory_contract(run, larger, opts):
    from onepose_plus_plus_amd._lib import OppError
    try:
        problems = MC.fill_problems(run, larger, close=opts.get("close"))
    except OppError as e:
        if "unsupported" in str(e):
            pytest.skip(str(e))
        raise
    if opts.get("refusal", True):
        problems += MC.refusal_problems(run, may_write=opts.get("may_write", ()))
    assert not problems, "\n".join(problems)


def test_fake_stages_are_classified_on_the_device():
    from tests.test_memory_contract_cpu import check_fake_stages
    check_fake_stages("cuda")


# ---- module level: the grow-only cached workspace of OnePosePlus_model -------------------------------------------------------------
def _module(precision, patch_max=None, train=False):
    from onepose_plus_plus_amd.synthetic import make_state_dict
    cfg = MCASE.config()
    cfg["coarse_matching"]["thr"] = 0.0
    cfg["coarse_matching"]["train"] = {"train_padding": True, "train_coarse_percent": 0.3, "train_pad_num_gt_min": 5}
    m = ops.make_model(cfg, make_state_dict(cfg, MCASE.WEIGHT_SEED), precision)
    if patch_max is not None:
        m.set_fine_patch_max_matches(patch_max)
    if train:
        m.train()
        m.train_randint = lambda high, size, device=None, **kw: (torch.arange(size[0]) * 7 % high).to(device)
    return m


_OUT_KEYS = ("conf_matrix", "i_ids", "j_ids", "mconf", "mkpts_query_c", "mkpts_3d_db", "expec_f", "mkpts_query_f")


@pytest.mark.parametrize("path", ["patches", "whole-map", "train-no-grad"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_module_small_forward_after_a_large_one(precision, path):
    """128 x 192 / N = 333, then 64 x 96 / N = 77 on one module -- the small call runs on the large call's leftovers in the module's cached
    workspace -- and once more after the whole cached buffer is overwritten with the NaN pattern: every output of the small call equals a
    fresh module's, bit for bit.  The fused path with the match-driven fine branch, with the whole fine map, and train() under no_grad."""
    from onepose_plus_plus_amd.synthetic import make_inputs
    kw = {"patches": dict(patch_max=100000), "whole-map": dict(patch_max=0), "train-no-grad": dict(train=True)}[path]
    small, large = make_inputs(77, (64, 96), 5), make_inputs(333, (128, 192), 6)
    if path == "train-no-grad":
        for d, n, L in ((small, 77, 96), (large, 333, 384)):
            gt = torch.zeros(1, n, L, dtype=torch.int16)
            gt[0, torch.arange(20) * 3, torch.arange(20) * 4 + 2] = 1
            d["conf_matrix_gt"] = gt
    want = ops.run_model(_module(precision, **kw), small)
    assert len(want["mconf"]) > 0
    m = _module(precision, **kw)
    ops.run_model(m, large)
    cached = m._rt["ws"].numel()
    runs = {"leftover": ops.run_model(m, small)}
    assert m._rt["ws"].numel() == cached, "the cached workspace does not grow for the smaller call"
    m._rt["ws"].view(torch.int32).fill_(ops.NAN_WORD)
    runs["nan"] = ops.run_model(m, small)
    for fill, got in runs.items():
        for k in _OUT_KEYS:
            assert got[k].shape == want[k].shape and torch.equal(MC.bits(got[k]), MC.bits(want[k])), (fill, k)


def _graph_step_grads(fine, poison):
    """parameter gradients of the second training step of a fresh module at the train_b4_64x96_n150 size (the first step creates the cached
    workspace); poison: that buffer is overwritten with the NaN pattern before the step's forward and again before its backward"""
    from onepose_plus_plus_amd.config import default_config
    from tests import helpers as H
    cfg, sd, data = H.train_setup("train_b4_64x96_n150")
    cfg_v = default_config(thr=cfg["coarse_matching"]["thr"], fine=fine)
    cfg_v["coarse_matching"]["train"] = cfg["coarse_matching"]["train"]
    model = ops.make_model(cfg_v, sd, "bf16x3")
    model.train()
    model.train_randint = lambda high, size, device=None, **kw: (torch.arange(size[0]) % high).to(device)
    g = torch.Generator().manual_seed(5)
    wc = we = None
    for step in range(2):
        model.zero_grad(set_to_none=True)
        d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in data.items()}
        if poison and step == 1:
            assert model._rt["ws"] is not None
            model._rt["ws"].view(torch.int32).fill_(ops.NAN_WORD)
        model(d)
        if wc is None:
            wc = torch.rand(d["conf_matrix"].shape, generator=g).cuda()
            we = torch.randn(d["expec_f"].shape, generator=g).cuda() if fine else None
        loss = (d["conf_matrix"] * wc).sum()
        if fine:
            loss = loss + (d["expec_f"] * we).sum()
        if poison and step == 1:
            model._rt["ws"].view(torch.int32).fill_(ops.NAN_WORD)
        loss.backward()
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("fine", [False, True], ids=["coarse-only", "with-fine-level"])
def test_graph_training_step_on_a_poisoned_cached_workspace(fine):
    """One step of the gradient graph with the module's cached workspace overwritten by NaNs before the forward and before backward().  Fine
    level off: every parameter gradient equals the untouched run's bit for bit.  Fine level on: the same for every gradient that does not pass
    through the window scatter (opp_fine_window_gather_backward feeds the fine map's gradient, i.e. the backbone's parameters; fp32 atomicAdd,
    order-dependent by design); the backbone's are held to the bars of test_training_graph_vs_torch_autograd_at_an_odd_size (0.25 of the
    largest entry, cosine 0.98)."""
    want, got = _graph_step_grads(fine, False), _graph_step_grads(fine, True)
    assert want.keys() == got.keys() and len(want) > 100
    bad = []
    for k, w in want.items():
        if fine and k.startswith("backbone."):
            err = float((got[k] - w).abs().max()) / max(float(w.abs().max()), 1e-30)
            cos = float(torch.nn.functional.cosine_similarity(got[k].flatten().double(), w.flatten().double(), dim=0)) if float(w.abs().max()) > 0 else 1.0
            if not (err <= 0.25 and cos >= 0.98):
                bad.append((k, err, cos))
        elif not torch.equal(MC.bits(got[k]), MC.bits(w)):
            bad.append((k, float((got[k] - w).abs().max())))
    assert not bad, bad[:8]
