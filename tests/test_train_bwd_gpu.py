"""GPU: the hand-written backward kernels of the training step (csrc/conv_bwd.hip, csrc/train_misc.hip and the
graph nodes of onepose_plus_plus_amd/train_autograd.py), each through the C ABI against torch.autograd in fp64 on the CPU --
the checker, never the product (backbone/resnet.py:10-45, :101-164; loftr_module/transformer.py:87-94;
utils/coarse_matching.py:115; loftr_module/fine_preprocess.py:41-55)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _s():
    return torch.cuda.current_stream().cuda_stream


def _pad32(c):
    return (c + 31) // 32 * 32


def _nhwc(x, c_pad):
    """[B, C, H, W] -> device NHWC [B, H, W, c_pad] with zero padding channels"""
    b, c, h, w = x.shape
    out = torch.zeros(b, h, w, c_pad)
    out[..., :c] = x.permute(0, 2, 3, 1)
    return out.cuda().contiguous()


def _from_nhwc(y, c):
    return y[..., :c].permute(0, 3, 1, 2).cpu()


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / max(float(b.double().abs().max()), 1e-30))


@pytest.mark.parametrize("prec", [2, 0])
@pytest.mark.parametrize("B,cin,cout,ks,stride,H,W", [
    (2, 128, 128, 3, 1, 16, 24),      # layer1-style
    (1, 128, 196, 3, 2, 16, 16),      # layer2.0.conv1: stride 2, 196 (-> 224) output channels
    (2, 196, 196, 3, 1, 8, 12),       # K tail packing on the input-gradient convolution, two channel tiles
    (1, 128, 196, 1, 2, 16, 16),      # downsample 1x1 stride 2
    (2, 196, 256, 1, 1, 8, 8),        # lateral 1x1
    (1, 256, 256, 3, 1, 8, 8),
    (3, 64, 96, 3, 1, 5, 7),          # ragged sizes: pixel count not a multiple of 32
    (2, 196, 256, 3, 2, 16, 24),      # layer3.0.conv1 at a 128 x 192 image, B = 2
    (2, 196, 256, 1, 2, 16, 24),      # layer3.0.downsample
    (2, 196, 196, 3, 1, 16, 24),      # layer2.1 convolutions
    (2, 128, 196, 3, 2, 32, 48),      # layer2.0.conv1
])
def test_conv2d_backward_vs_autograd(B, cin, cout, ks, stride, H, W, prec):
    from tests import hip_ops as ops
    g = torch.Generator().manual_seed(B * 1000 + cin + cout + ks + stride)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, ks, ks, generator=g) / (cin * ks * ks) ** 0.5
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = F.conv2d(xd, wd, None, stride, ks // 2)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy.double())
    cin_p, cout_p = _pad32(cin), _pad32(cout)
    xn, gyn, wdev = _nhwc(x, cin_p), _nhwc(gy, cout_p), w.cuda().contiguous()
    gx, gw = ops.conv2d_backward(xn, wdev, gyn, cin, cout, ks, stride, prec)
    assert _rel(_from_nhwc(gx, cin), xd.grad) < 5e-6, "grad_x"
    # accumulation into a buffer that already holds another consumer's gradient (aliased, as the residual blocks use it)
    add = torch.randn(B, H, W, cin_p, generator=g)
    add[..., cin:] = 0
    acc, _ = ops.conv2d_backward(xn, wdev, gyn, cin, cout, ks, stride, prec, want_dw=False, add=add)
    assert _rel(_from_nhwc(acc, cin), xd.grad + add[..., :cin].permute(0, 3, 1, 2).double()) < 5e-6, "grad_x + add (aliased)"
    assert (gx[..., cin:] == 0).all(), "padded channels of grad_x must be exact zeros"
    assert _rel(gw.cpu(), wd.grad) < 5e-6, "grad_w"
    # deterministic: fixed-order split reduction
    _, gw2 = ops.conv2d_backward(xn, wdev, gyn, cin, cout, ks, stride, prec, want_dx=False)
    assert torch.equal(gw, gw2)


def test_conv_wgrad_long_reduction():
    """the reduction length of the real step (tens of thousands of pixels per split chain) keeps fp32-level accuracy"""
    from tests import hip_ops as ops
    B, cin, cout, H, W = 2, 64, 64, 96, 128
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, cin, H, W, generator=g)
    gy = torch.randn(B, cout, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g)
    xd, wd = x.double(), w.double().requires_grad_(True)
    F.conv2d(xd, wd, None, 1, 1).backward(gy.double())
    xn, gyn = _nhwc(x, cin), _nhwc(gy, cout)
    _, gw = ops.conv2d_backward(xn, w.cuda(), gyn, cin, cout, 3, 1, 2, want_dx=False)
    # error relative to sum |a||b| ~ sqrt(P) * 0.64: a few fp32 ulps of the largest partial sums
    err = float((gw.cpu().double() - wd.grad).abs().max())
    assert err < 5e-6 * (B * H * W) ** 0.5, err


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("rows,C,with_res", [(700, 128, True), (513, 196, False), (64, 256, True)])
def test_batchnorm_backward_vs_autograd(rows, C, act, with_res):
    from tests import hip_ops as ops
    ld = _pad32(C)
    g = torch.Generator().manual_seed(rows + C + act)
    raw = torch.randn(rows, C, generator=g) * 2 + 0.5
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    res = torch.randn(rows, C, generator=g) if with_res else None
    gy = torch.randn(rows, C, generator=g)
    rd, gd, bd = raw.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    resd = res.double().requires_grad_(True) if with_res else None
    mean = rd.mean(0)
    var = rd.var(0, unbiased=False)
    z = (rd - mean) / torch.sqrt(var + 1e-5) * gd + bd
    if with_res:
        z = z + resd
    y = F.relu(z) if act == 1 else F.leaky_relu(z, 0.01) if act == 2 else z
    y.backward(gy.double())

    def padded(t):
        o = torch.zeros(rows, ld)
        o[:, :C] = t
        return o.cuda()
    pm, pi = torch.zeros(ld), torch.zeros(ld)
    pm[:C] = mean.detach().float()
    pi[:C] = (1.0 / torch.sqrt(var.detach() + 1e-5)).float()
    gyn, yn, rawn = padded(gy), padded(y.detach().float()), padded(raw)
    gam_d, pm_d, pi_d = gamma.cuda(), pm.cuda(), pi.cuda()          # named: a temporary's pointer would dangle once the expression ends
    d_raw, d_res, dg, db = ops.batchnorm_backward(gyn, yn, rawn, C, act, gam_d, pm_d, pi_d)
    assert _rel(d_raw[:, :C].cpu(), rd.grad) < 1e-5
    assert (d_raw[:, C:] == 0).all()
    assert _rel(dg.cpu(), gd.grad) < 1e-5 and _rel(db.cpu(), bd.grad) < 1e-5
    if with_res:
        assert _rel(d_res[:, :C].cpu(), resd.grad) < 1e-6


@pytest.mark.parametrize("B,Hr,Wr,C", [(2, 4, 6, 32), (1, 1, 3, 64), (1, 16, 16, 224)])
def test_upsample2x_backward_vs_autograd(B, Hr, Wr, C):
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(Hr * 10 + Wr)
    r = torch.randn(B, C, Hr, Wr, generator=g).double().requires_grad_(True)
    up = F.interpolate(r, scale_factor=2.0, mode="bilinear", align_corners=True)
    go = torch.randn(up.shape, generator=g)
    up.backward(go.double())
    gon = _nhwc(go, C)
    base = torch.randn(B, Hr, Wr, C, generator=g).cuda()
    for acc in (0, 1):
        out = base.clone()
        _lib.check(lib.opp_upsample2x_backward_nhwc(gon.data_ptr(), B, Hr, Wr, C, out.data_ptr(), acc, _s()), "opp_upsample2x_backward_nhwc")
        torch.cuda.synchronize()
        want = r.grad.permute(0, 2, 3, 1) + (base.cpu().double() if acc else 0)
        assert float((out.cpu().double() - want).abs().max()) < 1e-5


@pytest.mark.parametrize("rows,C", [(1000, 256), (77, 128), (5, 64)])
def test_layer_norm_node_vs_autograd(rows, C):
    from onepose_plus_plus_amd.train_autograd import HipLayerNorm
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, C, generator=g) * 3 + 1
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    go = torch.randn(rows, C, generator=g)
    xd, gd, bd = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    F.layer_norm(xd, (C,), gd, bd, 1e-5).backward(go.double())
    xc, gc, bc = (t.cuda().requires_grad_(True) for t in (x, gamma, beta))
    y = HipLayerNorm.apply(xc.view(1, rows, C), gc, bc)
    assert _rel(y.detach().cpu().view(rows, C), F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5)) < 2e-6
    y.backward(go.cuda().view(1, rows, C))
    torch.cuda.synchronize()
    assert _rel(xc.grad.cpu(), xd.grad) < 1e-5 and _rel(gc.grad.cpu(), gd.grad) < 1e-5 and _rel(bc.grad.cpu(), bd.grad) < 1e-5


@pytest.mark.parametrize("B,N,L", [(2, 150, 96), (1, 333, 260), (3, 17, 8)])
def test_dual_softmax_forward_lse_and_conf(B, N, L):
    from tests import hip_ops as ops
    g = torch.Generator().manual_seed(N)
    S = torch.randn(B, N, L, generator=g) * 4
    S[0, :, :2] -= 1e9                                      # masked cells
    Sd = S.double()
    lr, lc, conf = ops.dual_softmax_forward(S, with_conf=L % 4 == 0)
    for got, want in ((lr, torch.logsumexp(Sd, 2)), (lc, torch.logsumexp(Sd, 1))):
        assert float(((got.cpu().double() - want).abs() / want.abs().clamp(min=1)).max()) < 2e-6
    if L % 4 == 0:
        want = F.softmax(Sd, 1) * F.softmax(Sd, 2)
        assert float((conf.cpu().double() - want).abs().max()) < 2e-6


def test_fine_window_gather_node_vs_unfold():
    from onepose_plus_plus_amd.train_autograd import HipFineGather
    B, C, Hf, Wf, hc, wc, W = 2, 128, 16, 24, 4, 6, 5
    g = torch.Generator().manual_seed(3)
    feat = torch.randn(B, C, Hf, Wf, generator=g)
    M = 40
    b_ids = torch.randint(0, B, (M,), generator=g)
    j_ids = torch.randint(0, hc * wc, (M,), generator=g)
    j_ids[:4] = torch.tensor([0, wc - 1, hc * wc - 1, (hc - 1) * wc])      # image corners: windows reach outside
    j_ids[5] = j_ids[6]                                                      # duplicates (ground-truth padding repeats cells)
    b_ids[5] = b_ids[6]
    fd = feat.double().requires_grad_(True)
    un = F.unfold(fd, kernel_size=(W, W), stride=Hf // hc, padding=W // 2).view(B, C, W * W, -1).permute(0, 3, 2, 1)[b_ids, j_ids]
    go = torch.randn(un.shape, generator=g)
    un.backward(go.double())
    fc = feat.permute(0, 2, 3, 1).reshape(B, Hf * Wf, C).contiguous().cuda().requires_grad_(True)
    win = HipFineGather.apply(fc, b_ids.cuda(), j_ids.cuda(), (B, Hf, Wf, hc, wc, W))
    assert torch.equal(win.detach().cpu().double(), un.detach())
    win.backward(go.cuda())
    torch.cuda.synchronize()
    want = fd.grad.permute(0, 2, 3, 1).reshape(B, Hf * Wf, C)
    assert float((fc.grad.cpu().double() - want).abs().max()) < 1e-5


class _ActWithMask(torch.autograd.Function):
    """ReLU / LeakyReLU whose DERIVATIVE takes the side of the kink the device took (mask = saved device output > 0).  A
    pre-activation within fp32 rounding of zero may land on the other side of the kink on the device than in the fp64 reference;
    the derivative of that ONE element then differs and moves the affected gradients by ~1e-2 of their size (tools/bwd_diag.py:
    the first inexact block is the one holding the smallest |pre-activation|, a different one per arithmetic).  With the device's
    own masks the reference differentiates exactly the function the device evaluated, and every kernel is held to 3e-5."""

    @staticmethod
    def forward(ctx, z, mask, slope):
        ctx.save_for_backward(mask)
        ctx.slope = slope
        return torch.where(z > 0, z, slope * z)

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return g * torch.where(mask, torch.ones_like(g), torch.full_like(g, ctx.slope)), None, None


def _tape_outputs(tape, B, H, W):
    """views of the activation outputs on HipBackbone's tape (layout = plan_tape in csrc/api.hip: every tensor NHWC with channels
    padded to 32, 256-byte aligned, in forward order) -> name -> [B, C, h, w] (real channels)"""
    flt = tape.view(torch.float32)
    p2, p4, p8 = B * (H // 2) * (W // 2), B * (H // 4) * (W // 4), B * (H // 8) * (W // 8)
    c1, c2, c3 = 128, 224, 256
    real = {128: 128, 224: 196, 256: 256}
    hw = {p2: (H // 2, W // 2), p4: (H // 4, W // 4), p8: (H // 8, W // 8)}
    off = [0]
    out = {}

    def take(name, px, ch):
        start = (off[0] + 63) // 64 * 64                  # 256-byte alignment in floats
        off[0] = start + px * ch
        if name:
            h, w = hw[px]
            out[name] = flt[start:start + px * ch].view(B, h, w, ch)[..., :real[ch]].permute(0, 3, 1, 2)
    take(None, p2, c1)
    take("x0", p2, c1)
    for i, (px, ch) in enumerate([(p2, c1), (p2, c1), (p4, c2), (p4, c2), (p8, c3), (p8, c3)]):
        take(None, px, ch)
        take("t%d" % i, px, ch)
        take(None, px, ch)
        if i in (2, 4):
            take(None, px, ch)
        take("y%d" % i, px, ch)
    take(None, p4, c3)
    take(None, p4, c3)
    take("u2", p4, c3)
    take(None, p4, c2)
    take(None, p2, c2)
    take(None, p2, c2)
    take("u1", p2, c2)
    return out


def _backbone_with_masks(p, img, masks):
    """ResNetFPN_8_2.forward (backbone/resnet.py:141-164) in torch ops with the activation derivatives of `_ActWithMask`"""
    def bn(n, x):
        return F.batch_norm(x, None, None, p[n + ".weight"], p[n + ".bias"], True, 0.0, 1e-5)

    def act(z, key, slope=0.0):
        return _ActWithMask.apply(z, masks[key], slope)

    def block(name, i, x, stride):
        y = act(bn(name + ".bn1", F.conv2d(x, p[name + ".conv1.weight"], None, stride, 1)), "t%d" % i)
        y = bn(name + ".bn2", F.conv2d(y, p[name + ".conv2.weight"], None, 1, 1))
        if stride != 1:
            x = bn(name + ".downsample.1", F.conv2d(x, p[name + ".downsample.0.weight"], None, stride, 0))
        return act(x + y, "y%d" % i)
    b = "backbone."
    x0 = act(bn(b + "bn1", F.conv2d(img, p[b + "conv1.weight"], None, 2, 3)), "x0")
    x1 = block(b + "layer1.1", 1, block(b + "layer1.0", 0, x0, 1), 1)
    x2 = block(b + "layer2.1", 3, block(b + "layer2.0", 2, x1, 2), 1)
    x3 = block(b + "layer3.1", 5, block(b + "layer3.0", 4, x2, 2), 1)
    x3o = F.conv2d(x3, p[b + "layer3_outconv.weight"])
    t = F.conv2d(x2, p[b + "layer2_outconv.weight"]) + F.interpolate(x3o, scale_factor=2.0, mode="bilinear", align_corners=True)
    t = act(bn(b + "layer2_outconv2.1", F.conv2d(t, p[b + "layer2_outconv2.0.weight"], None, 1, 1)), "u2", 0.01)
    x2o = F.conv2d(t, p[b + "layer2_outconv2.3.weight"], None, 1, 1)
    t = F.conv2d(x1, p[b + "layer1_outconv.weight"]) + F.interpolate(x2o, scale_factor=2.0, mode="bilinear", align_corners=True)
    t = act(bn(b + "layer1_outconv2.1", F.conv2d(t, p[b + "layer1_outconv2.0.weight"], None, 1, 1)), "u1", 0.01)
    return x3o, F.conv2d(t, p[b + "layer1_outconv2.3.weight"], None, 1, 1)


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_backbone_node_vs_autograd(precision):
    """`HipBackbone` (taped train-mode forward + opp_backbone_backward) against fp64 torch.autograd of the same network on the CPU:
    both outputs and the gradient of EVERY backbone parameter at 3e-5 of its largest entry, with the reference's activation
    derivatives taken on the side of each kink the device took (`_ActWithMask`); the number of elements where the two sides
    differ is reported and must be tiny."""
    from onepose_plus_plus_amd import train_autograd as TA
    from tests import torch_graph_ref as GR
    from onepose_plus_plus_amd.config import default_config
    from onepose_plus_plus_amd.synthetic import make_state_dict
    from tests import hip_ops as ops
    cfg = default_config()
    sd = make_state_dict(cfg, 4)
    B, H, W = 2, 64, 96
    g = torch.Generator().manual_seed(11)
    img = torch.rand(B, 1, H, W, generator=g)
    model = ops.make_model(cfg, sd, precision)
    model.train()
    lib, c = model._ensure_ready(torch.device("cuda:0"))
    fc, ff = TA.backbone_node(model, lib, c, img.cuda().contiguous())
    acts = {k: v.cpu() for k, v in _tape_outputs(fc.grad_fn.tape, B, H, W).items()}
    gfc, gff = torch.randn(fc.shape, generator=g), torch.randn(ff.shape, generator=g)
    (fc * gfc.cuda()).sum().add((ff * gff.cuda()).sum()).backward()
    torch.cuda.synchronize()
    p = {k: v.double().requires_grad_(k.startswith("backbone.") and not k.endswith(("running_mean", "running_var", "num_batches_tracked")))
         for k, v in sd.items() if v.is_floating_point()}
    masks = {k: v > 0 for k, v in acts.items()}
    rc, rf = _backbone_with_masks(p, img.double(), masks)
    rc_t = rc.flatten(2).transpose(1, 2)
    rf_t = rf.flatten(2).transpose(1, 2)
    assert _rel(fc.detach().cpu(), rc_t.detach()) < 1e-5 and _rel(ff.detach().cpu(), rf_t.detach()) < 1e-5
    # the tape holds what the reference computes (and the masks are the device's own): activations agree, kink sides almost everywhere
    with torch.no_grad():
        ref_plain = GR._backbone({k: v.detach() for k, v in p.items()}, img.double())
    assert _rel(fc.detach().cpu(), ref_plain[0].flatten(2).transpose(1, 2)) < 1e-5
    ((rc_t * gfc.double()).sum() + (rf_t * gff.double()).sum()).backward()
    bad = []
    n = 0
    n_expect = sum(1 for k in sd if k.startswith("backbone.") and not k.endswith(("running_mean", "running_var", "num_batches_tracked")))
    for name, prm in model.named_parameters():
        if not name.startswith("backbone."):
            assert prm.grad is None
            continue
        n += 1
        want = p[name].grad
        err = float((prm.grad.cpu().double() - want).abs().max())
        if err > 3e-5 * float(want.abs().max()) + 1e-9:
            bad.append((name, err / float(want.abs().max())))
    assert n == n_expect and n > 50 and not bad, sorted(bad, key=lambda t: -t[1])[:8]


@pytest.mark.parametrize("M,N,K", [(9096, 768, 256), (1000, 256, 512), (77, 128, 128)])
def test_linear_weight_gradient_on_the_pixel_major_kernel(M, N, K):
    """opp_linear_backward (bf16x3) now forms dW on conv_wgrad_kernel straight from the token-major operands"""
    from tests import hip_ops as ops
    g = torch.Generator().manual_seed(M)
    x, gy, w = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g), torch.randn(N, K, generator=g)
    want_w = gy.double().t() @ x.double()
    want_x = gy.double() @ w.double()
    xc, gc, wc = x.cuda(), gy.cuda(), w.cuda()
    dx, dw = ops.linear_backward(gc, xc, wc, 2)
    assert float((dw.cpu().double() - want_w).abs().max()) < 3e-6 * M ** 0.5
    assert float((dx.cpu().double() - want_x).abs().max()) < 1e-6 * N
    _, dw2 = ops.linear_backward(gc, xc, wc, 2, want_dx=False, dw_into=dw)
    assert float((dw2.cpu().double() - 2 * want_w).abs().max()) < 6e-6 * M ** 0.5      # accumulate_grad_w


def _train_variant(name, precision, fine, with_mask):
    """-> (results of the graph forward with gradients, results of the fused no-grad train()-mode forward, model of the graph run)"""
    from onepose_plus_plus_amd.config import default_config
    from tests import helpers as H
    from tests import hip_ops as ops
    cfg, sd, data = H.train_setup(name)
    gold = H.load_golden(name)
    cfg_v = default_config(thr=cfg["coarse_matching"]["thr"], fine=fine)
    cfg_v["coarse_matching"]["train"] = cfg["coarse_matching"]["train"]
    B, _, Himg, Wimg = data["query_image"].shape
    if with_mask:
        m = torch.ones(B, Himg // 8, Wimg // 8)
        m[0, :, -3:] = 0                                  # padded right border of sample 0
        m[-1, -2:, :] = 0                                 # padded bottom rows of the last sample
        data["query_image_mask"] = m
        gt = data["conf_matrix_gt"].view(B, -1, Himg // 8, Wimg // 8)
        gt[0, :, :, -3:] = 0                              # no ground truth on padding
        gt[-1, :, -2:, :] = 0
    outs = []
    for graph in (True, False):
        model = ops.make_model(cfg_v, sd, precision)
        model.train()
        model.train_randint = H.RecordedRandint([gold["randint_%d" % i] for i in range(int(gold["n_randint"]))]) if not with_mask else \
            (lambda high, size, device=None, **kw: (torch.arange(size[0]) % high).to(device))
        d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in data.items()}
        if graph:
            out = model(d)
            assert out is d
        else:
            with torch.no_grad():
                model(d)
        outs.append((d, model))
    torch.cuda.synchronize()
    return outs[0][0], outs[1][0], outs[0][1]


@pytest.mark.parametrize("precision,fine,with_mask", [("fp32", True, False), ("bf16x3", False, False), ("bf16x3", True, True), ("fp32", True, True)])
def test_training_graph_matches_the_fused_train_forward(precision, fine, with_mask):
    """The graph of HIP nodes (gradients enabled) and the fused train()-mode forward (no_grad; pinned to the reference by the train
    fixtures) are the same function: same matches, confidences and fine offsets within the forward tolerances -- in the fp32
    arithmetic, without the fine level, and with a `query_image_mask` (masked cells keep zero confidence and get no gradient); every
    parameter that takes part receives a finite gradient."""
    from tests import helpers as H
    g, f, model = _train_variant("train_b4_64x96_n150", precision, fine, with_mask)
    assert torch.equal(g["b_ids"], f["b_ids"]) and torch.equal(g["i_ids"], f["i_ids"]) and torch.equal(g["j_ids"], f["j_ids"])
    assert float((g["conf_matrix"].detach() - f["conf_matrix"]).abs().max()) <= H.TOL_CONF
    assert float((g["mconf"].detach() - f["mconf"]).abs().max()) <= H.TOL_CONF
    assert g["conf_matrix"].requires_grad
    loss = (g["conf_matrix"] * torch.rand_like(g["conf_matrix"])).sum()
    if fine:
        assert float((g["expec_f"].detach()[:, :2] - f["expec_f"][:, :2]).abs().max()) <= H.TOL_OFFSET
        assert float((g["mkpts_query_f"] - f["mkpts_query_f"]).abs().max()) <= H.TOL_PIXEL
        loss = loss + (g["expec_f"] ** 2).sum()
    else:
        assert "expec_f" not in g or not torch.is_tensor(g.get("expec_f")) or not g["expec_f"].requires_grad
    if with_mask:
        mk = g["query_image_mask"].flatten(-2)                                  # [B, L]
        assert float(g["conf_matrix"].detach()[(mk == 0)[:, None, :].expand_as(g["conf_matrix"])].abs().max()) < 1e-30
    loss.backward()
    n = 0
    for name, p in model.named_parameters():
        if not fine and name.startswith("loftr_fine."):
            assert p.grad is None
            continue
        if not fine and name.startswith(("backbone.layer1_outconv", "backbone.layer2_outconv")):
            # coarse only: the FPN fine branch has no consumer -> zero (not missing) gradients from the backbone node
            assert p.grad is not None and float(p.grad.abs().max()) == 0.0, name
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, name
        n += 1
    assert n > 100


@pytest.mark.parametrize("with_mask", [False, True], ids=["unmasked", "masked"])
def test_training_graph_vs_torch_autograd_at_an_odd_size(with_mask):
    """Whole training graph at a shape no fixture covers -- 104 x 40 image (L = 13 x 5 = 65 cells: not a multiple of 32, which the
    matcher's backward pads), N = 77 points, B = 2: conf_matrix / expec_f and every parameter gradient of the HIP nodes against
    torch.autograd of the functional restatement `differentiable_forward` evaluated ON THE DEVICE with plain torch operators (a
    checker here, never the product).  1e-2 of each tensor's largest entry: two fp32 evaluations may take different sides of a ReLU
    kink (see test_backbone_node_vs_autograd); the forward values (2e-5 on conf_matrix, 1e-4 on expec_f) are held against the same
    restatement in float64.  masked: the same under a `query_image_mask` that takes sample 0's last column and
    sample 1's last row of cells (built as `_train_variant` builds it: no ground truth on masked cells) -- the gradients of the masked
    branches, which test_training_graph_matches_the_fused_train_forward only asks to be finite."""
    from onepose_plus_plus_amd import train_autograd as TA
    from onepose_plus_plus_amd.config import default_config
    from onepose_plus_plus_amd.synthetic import make_inputs, make_state_dict
    from tests import hip_ops as ops
    cfg = default_config(thr=0.0)
    cfg["coarse_matching"]["train"] = {"train_padding": True, "train_coarse_percent": 0.3, "train_pad_num_gt_min": 5}
    sd = make_state_dict(cfg, 7)
    hw, n, B = (104, 40), 77, 2
    parts = [make_inputs(n, hw, 40 + b) for b in range(B)]
    data = {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}
    L = (hw[0] // 8) * (hw[1] // 8)
    g = torch.Generator().manual_seed(2)
    gt = torch.zeros(B, n, L, dtype=torch.int16)
    for b in range(B):
        gt[b, torch.randperm(n, generator=g)[:20], torch.randperm(L, generator=g)[:20]] = 1
    data["conf_matrix_gt"] = gt
    if with_mask:
        m = torch.ones(B, hw[0] // 8, hw[1] // 8)
        m[0, :, -1] = 0                                   # sample 0: the last column of cells
        m[1, -1, :] = 0                                   # sample 1: the last row of cells
        data["query_image_mask"] = m
        gtv = gt.view(B, n, hw[0] // 8, hw[1] // 8)
        gtv[0, :, :, -1] = 0                              # no ground truth on padding
        gtv[1, :, -1, :] = 0
        assert int(gt.sum()) > 20
    model = ops.make_model(cfg, sd)
    model.train()
    model.train_randint = lambda high, size, device=None, **kw: (torch.arange(size[0]) * 7 % high).to(device)
    d = {k: v.cuda() for k, v in data.items()}
    model(d)
    if with_mask:
        dead = (d["query_image_mask"].flatten(-2) == 0)[:, None, :].expand_as(d["conf_matrix"])
        assert float(d["conf_matrix"].detach()[dead].abs().max()) == 0.0
    wc = torch.rand(d["conf_matrix"].shape, generator=g).cuda()
    we = torch.randn(d["expec_f"].shape, generator=g).cuda()
    ((d["conf_matrix"] * wc).sum() + (d["expec_f"] * we).sum()).backward()
    got = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    # the checker: same parameters, same matches, torch operators on the device
    p = {k: v.detach().clone().requires_grad_(True) for k, v in model.named_parameters()}
    inputs = {k: d[k] for k in ("query_image", "keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
    inputs["query_image_mask"] = d["query_image_mask"].flatten(-2).float() if with_mask else None
    pe = model.dense_pos_encoding.pe.cuda()
    from tests.torch_graph_ref import differentiable_forward
    conf, expec = differentiable_forward(p, cfg, inputs, (d["b_ids"], d["i_ids"], d["j_ids"]), pe)
    # The two forward bars are held against the SAME restatement evaluated in float64 on the device, no longer against the float32 one:
    # torch's float32 convolutions do not repeat from process to process here (measured on one MI355X, three processes, unmasked:
    # |torch32 - torch64| 1.15e-5, 1.20e-5, 1.33e-5 on conf), while the HIP graph does (|hip - torch64| 1.397e-5 each time), so
    # |hip - torch32| came out 1.67e-5, 1.80e-5, 2.12e-5 around the 2e-5 bar.  Same bars, a more exact checker; the gradients below
    # are compared with the float32 restatement as before (its 1e-5 of noise is far inside their bars).
    with torch.no_grad():
        p64 = {k: v.detach().double() for k, v in p.items()}
        in64 = {k: (v.double() if v is not None else None) for k, v in inputs.items()}
        conf64, expec64 = differentiable_forward(p64, cfg, in64, (d["b_ids"], d["i_ids"], d["j_ids"]), pe.double())
    e_conf = float((conf64 - d["conf_matrix"].detach().double()).abs().max())
    e_expec = float((expec64 - d["expec_f"].detach().double()).abs()[:, :2].max())
    print("odd size, mask %s: |conf - f64| = %.3e (torch fp32: %.3e), |expec_f - f64| = %.3e (torch fp32: %.3e)" % (
        with_mask, e_conf, float((conf.detach().double() - conf64).abs().max()), e_expec, float((expec.detach().double() - expec64).abs()[:, :2].max())))
    assert e_conf < 2e-5
    assert e_expec < 1e-4
    ((conf * wc).sum() + (expec * we).sum()).backward()
    torch.cuda.synchronize()
    bad = []
    for k, v in p.items():
        err = float((got[k] - v.grad).abs().max()) / float(v.grad.abs().max())
        cos = float(torch.nn.functional.cosine_similarity(got[k].flatten().double(), v.grad.flatten().double(), dim=0))
        # everything behind the feature maps (transformers, keypoint encoder): entry-wise.  Backbone: the 1/8-resolution maps of this
        # image have 65 pixels, so ONE pre-activation that lands on the other side of a ReLU kink in the two fp32 evaluations moves a
        # gradient by several per cent of its largest entry (the exact check of the backbone backward, with the device's own kink sides,
        # is test_backbone_node_vs_autograd at 3e-5): direction and size of every tensor must still agree
        if (err > 1e-2 and not k.startswith("backbone.")) or err > 0.25 or cos < 0.98:
            bad.append((k, err, cos))
    assert len(got) == 144 and not bad, sorted(bad, key=lambda t: -t[1])[:6]


def test_training_graph_with_a_frozen_pretrained_backbone(tmp_path):
    """`loftr_backbone.pretrained` + `pretrained_fix = True` (OnePosePlusModel.py:78-94, :109-113): the backbone keeps requires_grad = False
    and runs in eval mode (folded BatchNorm, running statistics untouched) while every other parameter trains.  The gradient graph then
    needs the BatchNorm-folded packing (pack scope 0; round-4 advisor finding: scope 1 made this configuration raise).  Values and the
    gradients of everything behind the feature maps against torch.autograd of the plain-torch restatement with eval-mode BatchNorm."""
    from onepose_plus_plus_amd import OnePosePlus_model
    from onepose_plus_plus_amd.config import default_config
    from onepose_plus_plus_amd.synthetic import make_inputs, make_state_dict
    from tests.torch_graph_ref import differentiable_forward
    cfg = default_config(thr=0.0)
    cfg["coarse_matching"]["train"] = {"train_padding": True, "train_coarse_percent": 0.3, "train_pad_num_gt_min": 5}
    sd = make_state_dict(cfg, 7)
    g = torch.Generator().manual_seed(3)
    for k in sd:                                    # non-trivial running statistics: eval-mode BatchNorm must be the one that runs
        if k.endswith("running_mean"):
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
        if k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(sd[k].shape, generator=g)
    ck = {"matcher.backbone." + k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}
    path = tmp_path / "loftr.ckpt"
    torch.save({"state_dict": ck}, path)
    cfg["loftr_backbone"]["pretrained"] = str(path)
    cfg["loftr_backbone"]["pretrained_fix"] = True
    model = OnePosePlus_model(cfg)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().train()
    hw, n, B = (96, 64), 90, 2
    parts = [make_inputs(n, hw, 50 + b) for b in range(B)]
    data = {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}
    L = (hw[0] // 8) * (hw[1] // 8)
    gt = torch.zeros(B, n, L, dtype=torch.int16)
    for b in range(B):
        gt[b, torch.randperm(n, generator=g)[:20], torch.randperm(L, generator=g)[:20]] = 1
    data["conf_matrix_gt"] = gt
    model.train_randint = lambda high, size, device=None, **kw: (torch.arange(size[0]) * 7 % high).to(device)
    d = {k: v.cuda() for k, v in data.items()}
    model(d)                                                       # gradients enabled, backbone frozen
    assert d["conf_matrix"].requires_grad and d["expec_f"].requires_grad
    wc = torch.rand(d["conf_matrix"].shape, generator=g).cuda()
    we = torch.randn(d["expec_f"].shape, generator=g).cuda()
    ((d["conf_matrix"] * wc).sum() + (d["expec_f"] * we).sum()).backward()
    for k, v in model.state_dict().items():                        # eval-mode backbone: running statistics as loaded
        if "running" in k or "num_batches" in k:
            assert torch.equal(v.cpu(), sd[k]), k
    got = {}
    for k, p in model.named_parameters():
        if k.startswith("backbone."):
            assert p.grad is None and not p.requires_grad, k
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
            got[k] = p.grad.detach().clone()
    p = {k: v.detach().clone().requires_grad_(not k.startswith("backbone.")) for k, v in model.named_parameters()}
    stats = {k[:-len(".running_mean")]: (model.state_dict()[k], model.state_dict()[k[:-len("mean")] + "var"])
             for k in model.state_dict() if k.endswith("running_mean")}
    inputs = {k: d[k] for k in ("query_image", "keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
    inputs["query_image_mask"] = None
    conf, expec = differentiable_forward(p, cfg, inputs, (d["b_ids"], d["i_ids"], d["j_ids"]), model.dense_pos_encoding.pe.cuda(), bn_eval_stats=stats)
    assert float((conf.detach() - d["conf_matrix"].detach()).abs().max()) < 2e-5
    assert float((expec.detach() - d["expec_f"].detach()).abs()[:, :2].max()) < 1e-4
    ((conf * wc).sum() + (expec * we).sum()).backward()
    bad = [(k, float((got[k] - p[k].grad).abs().max()) / float(p[k].grad.abs().max())) for k in got]
    bad = [t for t in bad if not t[1] < 1e-2]
    assert len(got) == 144 - 56 and not bad, sorted(bad, key=lambda t: -t[1])[:6]
    # the next eval forward repacks for inference (scope 0 was kept) and runs
    model.eval()
    with torch.no_grad():
        e = {k: d[k][:1] for k in data if k != "conf_matrix_gt"}
        model(e)
    assert torch.isfinite(e["conf_matrix"]).all()


@pytest.mark.parametrize("M,W", [(1, 5), (37, 5), (1203, 5), (10, 7), (6, 3)])
def test_fine_head_backward_vs_fp64(M, W):
    """`HipFineHead` (FineMatching._s2d_heatmap, utils/fine_matching.py:63-94 under autograd): expec_f and the gradients of the point / window
    tokens against fp64 autograd of the reference formula (softmax heatmap over the W x W cells, kornia's normalised grid, spatial expectation,
    summed sqrt(clamp(var, 1e-10))), incl. sharply peaked heatmaps whose variance sits on the clamp."""
    from onepose_plus_plus_amd.train_autograd import HipFineHead
    g = torch.Generator().manual_seed(M * 10 + W)
    C = 128
    f0 = torch.randn(M, C, generator=g)
    win = torch.randn(M, W * W, C, generator=g)
    if M > 2:
        win[0] *= 0.0                                   # uniform heatmap
        win[1, 3] = f0[1] * 40.0                        # one cell takes all the mass: var below the clamp
    ge = torch.randn(M, 3, generator=g)
    a, b = f0.cuda().requires_grad_(True), win.cuda().requires_grad_(True)
    out = HipFineHead.apply(a, b)
    (out * ge.cuda()).sum().backward()
    fd, wd = f0.double().requires_grad_(True), win.double().requires_grad_(True)
    heat = torch.softmax(torch.einsum("mc,mrc->mr", fd, wd) / C ** 0.5, dim=1)
    lin = (torch.linspace(0, W - 1, W, dtype=torch.float64) / (W - 1) - 0.5) * 2
    gx, gy = lin.view(1, W).expand(W, W).reshape(-1), lin.view(W, 1).expand(W, W).reshape(-1)
    coords = torch.stack([(gx * heat).sum(-1), (gy * heat).sum(-1)], dim=-1)
    grid = torch.stack([gx, gy], dim=-1)
    var = torch.sum(grid[None] ** 2 * heat[:, :, None], dim=1) - coords ** 2
    ref = torch.cat([coords, torch.sum(torch.sqrt(torch.clamp(var, min=1e-10)), -1)[:, None]], -1)
    (ref * ge.double()).sum().backward()
    assert float((out.detach().cpu().double() - ref.detach()).abs()[:, :2].max()) < 1e-5
    ok = var.detach().min(1).values > 1e-6              # rows on the clamp: the derivative of sqrt there is ~1e5 and discontinuous
    for got, want in ((a.grad.cpu().double(), fd.grad), (b.grad.cpu().double(), wd.grad)):
        scale = float(want[ok].abs().max()) if ok.any() else 1.0
        assert float((got[ok] - want[ok]).abs().max()) <= 2e-5 * max(scale, 1e-6), (M, W)
        assert torch.isfinite(got).all()


def test_backbone_backward_refuses_parameters_modified_in_place():
    """`HipBackbone` reads the image and the backbone parameters in place during the backward: an in-place update between forward and
    backward must raise like PyTorch's saved-tensor version check, not give gradients of another function (r04 advisor finding)."""
    from onepose_plus_plus_amd import train_autograd as TA
    from onepose_plus_plus_amd.config import default_config
    from onepose_plus_plus_amd.synthetic import make_state_dict
    from tests import hip_ops as ops
    cfg = default_config()
    model = ops.make_model(cfg, make_state_dict(cfg, 4))
    model.train()
    img = torch.rand(1, 1, 64, 64).cuda()
    lib, c = model._ensure_ready(torch.device("cuda:0"))
    fc, ff = TA.backbone_node(model, lib, c, img)
    with torch.no_grad():
        model.backbone.conv1.weight.mul_(1.01)               # e.g. an optimiser step before a delayed backward
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (fc.sum() + ff.sum()).backward()
    fc, ff = TA.backbone_node(model, lib, c, img)             # untouched: the backward runs
    (fc.sum() + ff.sum()).backward()
    assert torch.isfinite(model.backbone.conv1.weight.grad).all()
