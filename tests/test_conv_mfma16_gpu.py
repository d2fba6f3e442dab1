"""bf16x3 convolutions on v_mfma_f32_16x16x32_bf16 (gemm_mfma.hip, kM16): precision through the convolution path at extreme operand
magnitudes, and tile independence at the real 196(->224)-channel layer shapes."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sa,sw", [(1e5, 1.0), (1e-6, 1.0), (1.0, 1e10), (1.0, 1.0)])
@pytest.mark.parametrize("cin,cout,ks", [(128, 128, 3), (196, 196, 3), (128, 196, 1)])
def test_conv_bf16x3_not_narrower_than_fp32(sa, sw, cin, cout, ks):
    """Error of the bf16x3 convolution vs fp64, relative to sum |a||w| per output, against the exact-fp32 MFMA convolution of the same
    inputs: no larger, at any operand magnitude (the 196-channel case covers the packed K tail)."""
    from tests import hip_ops as ops
    g = torch.Generator().manual_seed(cin + cout + ks)
    x = torch.randn(1, cin, 24, 20, generator=g) * sa
    w = torch.randn(cout, cin, ks, ks, generator=g) * sw
    ref = F.conv2d(x.double(), w.double(), None, 1, ks // 2)
    bound = F.conv2d(x.abs().double(), w.abs().double(), None, 1, ks // 2)
    y3, pad3 = ops.conv2d(x, w, None, None, 1, None, 0, 0, -1, h2=3)
    y0, _ = ops.conv2d(x, w, None, None, 1, None, 0, 0, -1, h2=0)
    assert pad3 == 0.0
    e_b3 = (y3.double() - ref).abs() / bound
    e_f32 = (y0.double() - ref).abs() / bound
    assert e_b3.max() <= 1.25 * e_f32.max() + 2.0 ** -26, (float(e_b3.max()), float(e_f32.max()))
    assert e_b3.mean() <= 1.25 * e_f32.mean() + 2.0 ** -28


@pytest.mark.parametrize("cin,cout,ks,stride,H,W", [
    (196, 196, 3, 1, 128, 128),     # layer2 3x3 196->196 @128^2
    (196, 196, 3, 1, 256, 256),     # layer1_outconv2.0 3x3 196->196 @256^2
    (256, 196, 3, 1, 128, 128),     # layer2_outconv2 3x3 256->196
    (128, 196, 1, 1, 256, 256),     # layer1_outconv 1x1 128->196
])
def test_conv_196_channel_outputs_do_not_depend_on_the_tile_shape(cin, cout, ks, stride, H, W):
    """Every bf16x3 convolution tile (22, 27, 25, 20, 26, 2) gives the same bits on the 196(->224)-channel layers, and the padded channels
    196 .. 223 of the stored output are exactly zero."""
    from tests import hip_ops as ops
    g = torch.Generator().manual_seed(cin * 3 + cout + H)
    x = torch.randn(1, cin, H, W, generator=g)
    w = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
    scale, bias = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    res = torch.randn(1, cout, Ho, Wo, generator=g)
    outs = []
    for cfg in (22, 27, 25, 20, 26, 2):
        y, pad_max = ops.conv2d(x, w, scale, bias, stride, res, 1, 1, cfg, h2=3)
        assert pad_max == 0.0, cfg
        outs.append(y)
    assert torch.isfinite(outs[0]).all()
    assert all(torch.equal(outs[0], o) for o in outs[1:])
