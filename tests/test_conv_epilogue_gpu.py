"""The store loop of the MFMA convolution (gemm_mfma.hip, opp_gemm_body): a thread loads the bias and the residual values of a batch of its
items ahead of the batch's stores.  Every bf16x3 tile must still give the same bits, within the bar of test_conv1x1_bilinear_residual of an
fp64 reference, with exact zeros in the padded channels -- for the bilinear x2 residual (batches of two), the direct residual (batches of
four), and ragged rows / columns; the residual may be the output map itself (the match-driven fine branch adds into its patch buffer), and a
residual that overlaps the output in any other way is refused."""
import pytest
import torch
import torch.nn.functional as F

from tests import hip_ops as ops

pytestmark = pytest.mark.gpu

RELU, LEAKY = 1, 2
DIRECT, BILINEAR = 1, 2
TILES = (2, 20, 22, 25, 26)

# cin, cout, ks, stride, H, W (input), residual mode, activation, is tile config 27 (128 x 224: <= 224 stored columns) legal
CASES = [
    pytest.param(196, 256, 1, 1, 12, 16, BILINEAR, 0, False, id="1x1-196to256-bilinear"),
    pytest.param(128, 196, 3, 2, 24, 40, DIRECT, LEAKY, True, id="3x3s2-128to196-direct-leaky"),
    pytest.param(64, 32, 3, 1, 9, 7, 0, 0, True, id="3x3-64to32-ragged"),
]


def _conv(x, w, bias, stride, residual, res_mode, act, cfg, in_place=False, res_offset=0):
    """For the aliasing cases only (ops.conv2d allocates its own output; these need the pointers): bf16x3 opp_conv2d_nhwc -> the whole stored
    NHWC output (cout padded to 32).  in_place: the (direct) residual buffer is the output buffer;
    res_offset != 0: the residual pointer is the output pointer moved by that many floats (a partial overlap)"""
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    cout, cin, ks, _ = w.shape
    cin_p, cout_p = ops.pad32(cin), ops.pad32(cout)
    xd = ops.to_nhwc_padded(x, cin_p)
    H, W = x.shape[2:]
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    wp = torch.empty(cout_p * lib.opp_conv_packed_k(cin, ks), device="cuda")
    wd = w.cuda().contiguous()
    _lib.check(lib.opp_pack_conv_weight(wd.data_ptr(), None, cout, cin, ks, cout_p, cin_p, wp.data_ptr(), ops._s()), "pack")
    wp = ops.pack_b3(wp)
    bd = torch.zeros(cout_p, device="cuda")
    bd[:cout] = bias.cuda()
    rd = ops.to_nhwc_padded(residual, cout_p) if residual is not None else None
    if in_place or res_offset:
        y = torch.zeros(Ho * Wo * cout_p + abs(res_offset), device="cuda")
        y[:Ho * Wo * cout_p] = rd.reshape(-1)
        r_ptr = y.data_ptr() + 4 * res_offset
    else:
        y = torch.full((Ho * Wo * cout_p,), float("nan"), device="cuda")
        r_ptr = rd.data_ptr() if rd is not None else None
    _lib.check(lib.opp_conv2d_nhwc(xd.data_ptr(), H, W, cin, wp.data_ptr(), bd.data_ptr(), cout_p, ks, stride, r_ptr, res_mode, act, y.data_ptr(), cfg, 2,
                                   None, ops._s()), "conv2d")
    torch.cuda.synchronize()
    return y[:Ho * Wo * cout_p].view(Ho, Wo, cout_p).cpu()


def _inputs(cin, cout, ks, stride, H, W, res_mode):
    g = torch.Generator().manual_seed(cin * 5 + cout + ks + stride + H * 3 + W)
    x = torch.randn(1, cin, H, W, generator=g)
    w = torch.randn(cout, cin, ks, ks, generator=g) * (1.0 / (cin * ks * ks)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    res = None
    if res_mode == DIRECT:
        res = torch.randn(1, cout, Ho, Wo, generator=g)
    elif res_mode == BILINEAR:
        res = torch.randn(1, cout, Ho // 2, Wo // 2, generator=g)
    return x, w, bias, res


def _reference(x, w, bias, stride, res, res_mode, act):
    ks = w.shape[2]
    ref = F.conv2d(x.double(), w.double(), bias.double(), stride, ks // 2)
    if res_mode == DIRECT:
        ref = ref + res.double()
    elif res_mode == BILINEAR:
        ref = ref + F.interpolate(res.double(), scale_factor=2.0, mode="bilinear", align_corners=True)
    if act == RELU:
        ref = F.relu(ref)
    elif act == LEAKY:
        ref = F.leaky_relu(ref, 0.01)
    return ref[0].permute(1, 2, 0)    # [Ho][Wo][cout]


@pytest.mark.parametrize("cin,cout,ks,stride,H,W,res_mode,act,ok27", CASES)
def test_every_tile_stores_the_same_bits_within_the_fp64_bar(cin, cout, ks, stride, H, W, res_mode, act, ok27):
    x, w, bias, res = _inputs(cin, cout, ks, stride, H, W, res_mode)
    ref = _reference(x, w, bias, stride, res, res_mode, act).permute(2, 0, 1).unsqueeze(0)
    bar = 2e-5 * max(1.0, ref.abs().max().item())
    first = None
    for cfg in TILES + ((27,) if ok27 else ()):
        got, pad_max = ops.conv2d(x, w, None, bias, stride, res, res_mode, act, cfg, h2=3)
        err = (got.double() - ref).abs().max().item()
        print("tile %d: max |err| %.3e (bar %.3e)" % (cfg, err, bar))
        assert torch.isfinite(got).all(), cfg
        assert err <= bar, (cfg, err, bar)
        assert pad_max == 0.0, cfg
        if first is None:
            first = got
        assert torch.equal(got, first), (cfg, (got - first).abs().max().item())


def test_residual_that_is_the_output_map():
    """R == C with the same row stride: each thread reads only what it writes later (api.hip: the lateral 1 x 1 of the match-driven fine patches)"""
    cin, cout, ks, stride, H, W = 128, 196, 3, 2, 24, 40
    x, w, bias, res = _inputs(cin, cout, ks, stride, H, W, DIRECT)
    for cfg in TILES + (27,):
        want = _conv(x, w, bias, stride, res, DIRECT, LEAKY, cfg)
        got = _conv(x, w, bias, stride, res, DIRECT, LEAKY, cfg, in_place=True)
        assert torch.equal(got, want), (cfg, (got - want).abs().max().item())


def test_partly_overlapping_residual_is_refused():
    from onepose_plus_plus_amd import _lib
    x, w, bias, res = _inputs(64, 32, 3, 1, 9, 7, DIRECT)
    with pytest.raises(_lib.OppError, match="overlaps"):
        _conv(x, w, bias, 1, res, DIRECT, 0, 25, res_offset=32)
