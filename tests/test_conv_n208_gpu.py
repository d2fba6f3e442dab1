"""The two-role 128 x 224 tile of the bf16x3 convolutions (gemm_mfma.hip, kRoles; reached through tile config 27): 13 computed column blocks
(208 columns) on 64 x 64 | 32 x 80 waves.  At every 196(->224)-channel layer shape of the backbone it must give the same bits as the 128 x 128
and 256 x 128 tiles and as the 128 x 256 tile config 22 runs when the real column count is unknown, stored pad columns 196 .. 223 included."""
import pytest
import torch

from tests import hip_ops as ops

pytestmark = pytest.mark.gpu

RELU, LEAKY = 1, 2
DIRECT, BILINEAR = 1, 2


def _conv_padded(x, w, scale, bias, stride, residual, res_mode, act, cfg):
    """ops.conv2d in bf16x3, but the whole stored NHWC output (cout padded to 32) comes back: the pad columns are part of the comparison"""
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    cout, cin, ks, _ = w.shape
    cin_p, cout_p = ops.pad32(cin), ops.pad32(cout)
    xd = ops.to_nhwc_padded(x, cin_p)
    H, W = x.shape[2:]
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    wp = torch.empty(cout_p * lib.opp_conv_packed_k(cin, ks), device="cuda")
    sd = torch.zeros(cout_p, device="cuda")
    sd[:cout] = scale.cuda()
    wd = w.cuda().contiguous()
    _lib.check(lib.opp_pack_conv_weight(wd.data_ptr(), sd.data_ptr(), cout, cin, ks, cout_p, cin_p, wp.data_ptr(), ops._s()), "pack")
    wp = ops.pack_b3(wp)
    bd = torch.zeros(cout_p, device="cuda")
    bd[:cout] = bias.cuda()
    rd = ops.to_nhwc_padded(residual, cout_p) if residual is not None else None
    y = torch.full((Ho, Wo, cout_p), float("nan"), device="cuda")
    _lib.check(lib.opp_conv2d_nhwc(xd.data_ptr(), H, W, cin, wp.data_ptr(), bd.data_ptr(), cout_p, ks, stride,
                                   rd.data_ptr() if rd is not None else None, res_mode, act, y.data_ptr(), cfg, 2, None, ops._s()), "conv2d")
    torch.cuda.synchronize()
    return y


# cin, cout, ks, stride, H, W (input), residual mode, activation
LAYERS = [
    pytest.param(128, 196, 3, 2, 256, 256, 0, RELU, id="layer2.0.conv1-3x3s2"),
    pytest.param(128, 196, 1, 2, 256, 256, 0, 0, id="layer2.0.downsample-1x1s2"),
    pytest.param(196, 196, 3, 1, 128, 128, DIRECT, RELU, id="layer2.x.conv2-3x3-residual"),
    pytest.param(196, 196, 3, 1, 128, 128, 0, RELU, id="layer2.1.conv1-3x3"),
    pytest.param(256, 196, 3, 1, 128, 128, 0, 0, id="layer2_outconv2.3-3x3"),
    pytest.param(128, 196, 1, 1, 256, 256, BILINEAR, 0, id="layer1_outconv-1x1-bilinear"),
    pytest.param(196, 196, 3, 1, 256, 256, 0, LEAKY, id="layer1_outconv2.0-3x3-leaky"),
    pytest.param(196, 196, 3, 1, 37, 53, DIRECT, LEAKY, id="ragged-M-3x3"),
    pytest.param(196, 196, 3, 2, 45, 61, 0, RELU, id="ragged-M-3x3s2"),
    pytest.param(128, 196, 1, 1, 29, 30, BILINEAR, LEAKY, id="ragged-M-1x1-bilinear"),
]


@pytest.mark.parametrize("cin,cout,ks,stride,H,W,res_mode,act", LAYERS)
def test_two_role_tile_matches_the_other_tiles(cin, cout, ks, stride, H, W, res_mode, act):
    g = torch.Generator().manual_seed(cin * 7 + cout + ks * 3 + stride + H + W + res_mode * 5 + act)
    x = torch.randn(1, cin, H, W, generator=g)
    w = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
    scale, bias = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    res = None
    if res_mode == DIRECT:
        res = torch.randn(1, cout, Ho, Wo, generator=g)
    elif res_mode == BILINEAR:
        res = torch.randn(1, cout, Ho // 2, Wo // 2, generator=g)
    got = _conv_padded(x, w, scale, bias, stride, res, res_mode, act, 27)
    assert torch.isfinite(got).all()
    assert (got[:, :, cout:] == 0).all()
    for cfg in (25, 20, 22):
        want = _conv_padded(x, w, scale, bias, stride, res, res_mode, act, cfg)
        assert torch.equal(got, want), (cfg, (got - want).abs().max().item())
