"""GPU: `onepose_plus_plus_amd.optim.FusedAdam` (csrc/optim.hip: one gradient-norm launch + one clip / decay / moments / update launch
per parameter group) against the float64 restatement of tests/optim_reference.py, on small tensors at the sizes where the kernel
takes another path: 1, 3, 4, 5 (scalar tail only / one float4 / float4 + tail), 255, 256, 257 (around one workgroup), C - 1, C,
C + 1, 2 C + 3 (partial chunk, the full-chunk path, more than one chunk per tensor; C = OPP_OPTIM_CHUNK).

Every comparison is max|x - x64| / max|x64| per tensor and per kind (p, m, v) in units of 2^-24 against `BAR_UNITS` = four times
the distance of torch's own fp32 CPU run from the restatement (p 110, m 64, v 27 units; measured 26.3, 15.8, 6.7).  The
hyper-parameters are exaggerated so that the smallest semantic slip (weight decay applied after the update) moves p by 5.8e3
units -- tests/test_optim_cpu.py checks both numbers without a device."""
import functools

import pytest
import torch

from tests import optim_reference as R

pytestmark = pytest.mark.gpu

LAYOUTS = ("plain", "flat_grads", "flat_params_and_grads")


@functools.lru_cache(maxsize=None)
def _case(steps):
    return R.make_case(steps)


def _flat_views(tensors, lead=0):
    """views at cumulative offsets into one buffer (`sharding.GradientAverager`'s layout) behind `lead` elements.  With SIZES and lead 0
    the 3, 255, C - 1 and 2 C + 3 tensors start off a 16-byte boundary (the others land on one again: 1 + 3 = 4, ...); with lead 1
    every tensor does"""
    flat = torch.zeros(lead + sum(t.numel() for t in tensors), device="cuda")
    views, off = [], lead
    for t in tensors:
        views.append(flat[off:off + t.numel()])
        off += t.numel()
    return flat, views


class _Run:
    """device parameters in one of LAYOUTS and a way to hand them a step's gradients"""

    def __init__(self, params, layout="plain"):
        self.layout = layout
        if layout == "flat_params_and_grads":
            self.pflat, views = _flat_views(params, lead=1)
            assert all(v.data_ptr() % 16 != 0 for v in views)
            self.ps = [torch.nn.Parameter(v) for v in views]
            with torch.no_grad():
                for p, src in zip(self.ps, params):
                    p.copy_(src)
        else:
            self.ps = [torch.nn.Parameter(p.cuda()) for p in params]
        if layout != "plain":
            self.gflat, self.gviews = _flat_views(params)
            assert sum(v.data_ptr() % 16 != 0 for v in self.gviews) == 4 and self.gviews[-1].data_ptr() % 16 != 0

    def set_grads(self, step):
        for i, (p, g) in enumerate(zip(self.ps, step)):
            if g is None:
                p.grad = None
            elif self.layout == "plain":
                p.grad = g.cuda()
            else:
                self.gviews[i].copy_(g)
                p.grad = self.gviews[i]


def _kinds(ps, opt):
    return {"p": [p.detach() for p in ps], "m": [opt.state[p]["exp_avg"] for p in ps], "v": [opt.state[p]["exp_avg_sq"] for p in ps]}


def _assert_within_bar(ps, opt, ref, where):
    worst = R.worst_units(_kinds(ps, opt), ref)
    print("%s: worst tensor, units of 2^-24: %s (bar %s)" % (where, {k: round(u, 2) for k, u in worst.items()}, R.BAR_UNITS))
    for kind, u in worst.items():
        assert u <= R.BAR_UNITS[kind], (where, kind, u)


def _assert_norm(opt, ref, where):
    got = float(opt.last_grad_norm.item())
    units = abs(got - ref.last_norm) / ref.last_norm / R.UNIT
    print("%s: last_grad_norm %.9g, float64 %.9g, %.2f units" % (where, got, ref.last_norm, units))
    assert units <= R.NORM_BAR_UNITS, (where, got, ref.last_norm)


def _fused(ps, decoupled, clip=True, scale=1.0, **kw):
    from onepose_plus_plus_amd.optim import FusedAdam
    return FusedAdam(ps, decoupled=decoupled, max_grad_norm=R.MAX_NORM if clip else None, grad_scale=scale, **dict(R.HYPER, **kw))


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("steps", [1, 10])
def test_steps_match_the_restatement(steps, decoupled, clip, scale):
    """Adam and AdamW, clipping on and off, grad_scale 1 and 0.5, one and ten steps: p, m, v of every tensor within the bar, the
    norm the kernel stores within 4 units of the float64 norm (in the ten-step run the third step does not clip, the others do)"""
    from onepose_plus_plus_amd import _lib
    assert _lib.load().opp_optim_chunk_elems() == R.CHUNK
    params, grads = _case(steps)
    run = _Run(params)
    opt = _fused(run.ps, decoupled, clip, scale)
    ref = R.ReferenceAdam(R.one_group(params, decoupled), max_grad_norm=R.MAX_NORM if clip else None, grad_scale=scale)
    where = "%s, clip %s, grad_scale %s" % ("AdamW" if decoupled else "Adam", clip, scale)
    for k, step in enumerate(grads):
        run.set_grads(step)
        opt.step()
        ref.step([step])
        if clip:
            _assert_norm(opt, ref, "%s, step %d" % (where, k + 1))
    _assert_within_bar(run.ps, opt, ref, "%s, %d steps" % (where, steps))
    assert all(float(opt.state[p]["step"]) == steps and not opt.state[p]["step"].is_cuda for p in run.ps)


@pytest.mark.parametrize("layout", LAYOUTS[1:])
@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("steps", [1, 10])
def test_unaligned_views_match_the_restatement(steps, decoupled, layout):
    """every `p.grad` a view into one flat buffer at cumulative offsets (four tensors, the multi-chunk one among them, take the 4-byte
    path), then every parameter such a view as well, one element further (every tensor takes it, full chunks included); same bar,
    clipping on, grad_scale 0.5"""
    params, grads = _case(steps)
    run = _Run(params, layout)
    opt = _fused(run.ps, decoupled, True, 0.5)
    ref = R.ReferenceAdam(R.one_group(params, decoupled), max_grad_norm=R.MAX_NORM, grad_scale=0.5)
    for step in grads:
        run.set_grads(step)
        opt.step()
        ref.step([step])
    _assert_norm(opt, ref, layout)
    _assert_within_bar(run.ps, opt, ref, "%s, decoupled %s, %d steps" % (layout, decoupled, steps))
    if layout == "flat_params_and_grads":                 # nothing was written between or beyond the views
        assert float(run.pflat[0]) == 0 and torch.equal(run.pflat[1:], torch.cat([p.detach().reshape(-1) for p in run.ps]))


@pytest.mark.parametrize("layout", LAYOUTS[:2])
def test_gradients_are_left_untouched(layout):
    """clipping and grad_scale act inside the update: every `.grad` is bit-identical after `step()`"""
    params, grads = _case(1)
    run = _Run(params, layout)
    opt = _fused(run.ps, True, True, 0.5)
    run.set_grads(grads[0])
    before = [p.grad.clone() for p in run.ps]
    ptrs = [p.grad.data_ptr() for p in run.ps]
    opt.step()
    torch.cuda.synchronize()
    assert float(opt.last_grad_norm) > 10 * R.MAX_NORM           # (it did clip)
    for p, g, ptr in zip(run.ps, before, ptrs):
        assert p.grad.data_ptr() == ptr and torch.equal(p.grad, g)


def test_same_inputs_give_the_same_bits():
    params, grads = _case(10)
    outs = []
    for _ in range(2):
        run = _Run(params, "flat_grads")
        opt = _fused(run.ps, True)
        for step in grads[:3]:
            run.set_grads(step)
            opt.step()
        outs.append((_kinds(run.ps, opt), opt.last_grad_norm.clone()))
    (a, na), (b, nb) = outs
    assert torch.equal(na, nb)
    for kind in ("p", "m", "v"):
        for x, y in zip(a[kind], b[kind]):
            assert torch.equal(x, y), kind


def test_a_gradient_of_none_skips_that_parameter():
    """the second step has no gradient for the C - 1 tensor: it and its state do not move (its step count stays behind, so the
    third step runs it with its own bias corrections, in a launch of its own), the others match the restatement in every step"""
    params, grads = _case(10)
    skip = R.SIZES.index(R.CHUNK - 1)
    run = _Run(params)
    opt = _fused(run.ps, True)
    ref = R.ReferenceAdam(R.one_group(params, True), max_grad_norm=R.MAX_NORM)
    for k in range(3):
        step = list(grads[k])
        if k == 1:
            step[skip] = None
            held = [run.ps[skip].detach().clone(), opt.state[run.ps[skip]]["exp_avg"].clone(), opt.state[run.ps[skip]]["exp_avg_sq"].clone()]
        run.set_grads(step)
        opt.step()
        ref.step([step])
        _assert_norm(opt, ref, "step %d" % (k + 1))
        _assert_within_bar(run.ps, opt, ref, "gradient of None in step 2, after step %d" % (k + 1))
        if k == 1:
            st = opt.state[run.ps[skip]]
            assert torch.equal(run.ps[skip].detach(), held[0]) and torch.equal(st["exp_avg"], held[1]) and torch.equal(st["exp_avg_sq"], held[2])
            assert float(st["step"]) == 1
    assert [float(opt.state[p]["step"]) for p in run.ps] == [2.0 if i == skip else 3.0 for i in range(len(run.ps))]
    assert len(opt._segments) == 2


def test_two_parameter_groups_share_one_norm():
    params, grads = _case(10)
    first = dict(lr=2e-2, weight_decay=0.1)
    half = len(params) // 2
    for decoupled in (False, True):
        run = _Run(params, "flat_grads")
        opt = _fused([dict(params=run.ps[:half], **first), dict(params=run.ps[half:])], decoupled)
        ref = R.ReferenceAdam(R.split_groups(params, decoupled, first=first), max_grad_norm=R.MAX_NORM)
        for step in grads[:3]:
            run.set_grads(step)
            opt.step()
            ref.step(R.split_grads(step))
        _assert_norm(opt, ref, "two groups")
        _assert_within_bar(run.ps, opt, ref, "two groups, decoupled %s" % decoupled)


def test_state_dict_round_trip_with_torch():
    """3 steps of torch.optim.AdamW on the device, `FusedAdam.load_state_dict`, 3 more steps: 6 steps of the restatement; then the
    other way round.  The loaded moments live in the flat buffers; the dict FusedAdam writes has torch's layout."""
    params, grads = _case(10)
    hyper = dict(R.HYPER)

    def torch_steps(opt, run, steps):
        for step in steps:
            run.set_grads(step)
            torch.nn.utils.clip_grad_norm_(run.ps, R.MAX_NORM)
            opt.step()

    def fused_steps(opt, run, steps):
        for step in steps:
            run.set_grads(step)
            opt.step()

    ref = R.ReferenceAdam(R.one_group(params, True), max_grad_norm=R.MAX_NORM)
    for step in grads[:6]:
        ref.step([step])
    # torch -> fused
    run = _Run(params)
    t_opt = torch.optim.AdamW(run.ps, **hyper)
    torch_steps(t_opt, run, grads[:3])
    opt = _fused(run.ps, True)
    opt.load_state_dict(t_opt.state_dict())
    m_flat, v_flat = opt._blocks[0]
    for p in run.ps:
        st = opt.state[p]
        assert m_flat.data_ptr() <= st["exp_avg"].data_ptr() < m_flat.data_ptr() + m_flat.numel() * 4
        assert v_flat.data_ptr() <= st["exp_avg_sq"].data_ptr() < v_flat.data_ptr() + v_flat.numel() * 4
        assert float(st["step"]) == 3 and torch.equal(st["exp_avg"], t_opt.state[p]["exp_avg"])
    fused_steps(opt, run, grads[3:6])
    _assert_within_bar(run.ps, opt, ref, "torch 3 steps -> FusedAdam 3 steps")
    # fused -> torch
    run = _Run(params)
    opt = _fused(run.ps, True)
    fused_steps(opt, run, grads[:3])
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and sorted(sd["state"]) == list(range(len(run.ps)))
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values())
    t_opt = torch.optim.AdamW(run.ps, lr=1.0, weight_decay=0.0)        # every hyper-parameter comes from the loaded groups
    t_opt.load_state_dict(sd)
    torch_steps(t_opt, run, grads[3:6])
    _assert_within_bar(run.ps, t_opt, ref, "FusedAdam 3 steps -> torch 3 steps")


def test_scheduler_changes_the_step_actually_applied():
    """MultiStepLR (through `build_scheduler`) over FusedAdam with betas = (0, 0) and constant gradients: m = g, v = g^2, both bias
    corrections 1, so a step moves p by lr g / (|g| + eps); at gamma = 0.5 the second step is half the first"""
    from onepose_plus_plus_amd.optim import FusedAdam, build_scheduler
    gen = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter((0.25 * torch.randn(n, generator=gen)).cuda()) for n in (5, 257, R.CHUNK + 1)]
    gs = [(torch.rand(p.numel(), generator=gen) + 0.5).cuda() for p in ps]
    opt = FusedAdam(ps, lr=1e-2, betas=(0.0, 0.0), eps=1e-8)
    trainer = {"scheduler": "MultiStepLR", "scheduler_invervel": "step", "mslr_milestones": [1], "mslr_gamma": 0.5}
    sched = build_scheduler({"trainer": trainer}, opt)["scheduler"]
    seen = [[p.detach().double().clone() for p in ps]]
    for _ in range(2):
        for p, g in zip(ps, gs):
            p.grad = g
        opt.step()
        sched.step()
        seen.append([p.detach().double().clone() for p in ps])
    assert opt.param_groups[0]["lr"] == pytest.approx(5e-3)
    for p0, p1, p2 in zip(*seen):
        d1, d2 = p1 - p0, p2 - p1
        assert (d1 + 1e-2).abs().max() < 5e-7                      # |p| < 2: an fp32 rounding of p is at most 1.2e-7
        assert (d2 - 0.5 * d1).abs().max() < 5e-7


def test_zero_grad_keeps_the_gradients_and_fills_a_flat_buffer_once():
    params, grads = _case(1)
    for layout in LAYOUTS[:2]:
        run = _Run(params, layout)
        opt = _fused(run.ps, True)
        run.set_grads(grads[0])
        ptrs = [p.grad.data_ptr() for p in run.ps]
        opt.zero_grad()
        assert (opt._zero_flat is not None) == (layout == "flat_grads")
        assert [p.grad.data_ptr() for p in run.ps] == ptrs and all(int(p.grad.count_nonzero()) == 0 for p in run.ps)
        if layout == "flat_grads":
            assert opt._zero_flat.data_ptr() == run.gflat.data_ptr() and opt._zero_flat.numel() == run.gflat.numel()
        opt.zero_grad(set_to_none=True)
        assert all(p.grad is None for p in run.ps)


def test_with_the_model_no_packed_weight_goes_stale():
    """the training shape of tests/test_e2e_gpu.py at its smallest (64 x 96, 100 points, B = 2): an eval forward on a resident
    object (fills the packed-weight and object-token caches), two training steps with `build_optimizer(..., max_grad_norm=0.5)`, an
    eval forward on the same tensors: it equals the eval forward of a fresh module loaded from the trained `state_dict()`"""
    from tests import helpers as H
    from tests import hip_ops as ops
    from onepose_plus_plus_amd.config import default_config
    from onepose_plus_plus_amd.optim import FusedAdam, build_optimizer
    from onepose_plus_plus_amd.synthetic import make_inputs, make_state_dict
    B, N, hw = 2, 100, (64, 96)
    L = (hw[0] // 8) * (hw[1] // 8)
    cfg = default_config(thr=0.0)
    cfg["coarse_matching"]["train"] = {"train_padding": True, "train_coarse_percent": 0.3, "train_pad_num_gt_min": 10}
    model = ops.make_model(cfg, make_state_dict(cfg, 0))
    parts = [make_inputs(N, hw, 40 + b) for b in range(B)]
    data = {k: torch.cat([p[k] for p in parts], 0).cuda() for k in parts[0]}
    g = torch.Generator().manual_seed(3)
    gt = torch.zeros(B, N, L, dtype=torch.int16)
    for b in range(B):
        gt[b, torch.randperm(N, generator=g)[:20], torch.randperm(L, generator=g)[:20]] = 1
    resident = {k: v[:1] for k, v in data.items()}
    with torch.no_grad():
        d0 = dict(resident)
        model(d0)
    hparams = {"trainer": {"optimizer": "adamw", "true_lr": 1e-5, "adamw_decay": 0.1}}       # small steps: the matcher keeps matching
    opt = build_optimizer(model, hparams, max_grad_norm=0.5)
    assert isinstance(opt, FusedAdam) and opt.module is model and opt.param_groups[0]["decoupled_weight_decay"]
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    model.train()
    torch.manual_seed(11)                                 # the train()-mode matcher draws its padding with torch.randint
    for _ in range(2):
        d = dict(data)
        d["conf_matrix_gt"] = gt.cuda()
        model(d)
        # the scalar of tests/test_e2e_gpu.py::test_training_step_gradients: every entry of both outputs weighs in, so every parameter
        # has a gradient that is not identically zero (a log-likelihood of a few planted pairs, clamped at 1e-6, can leave the whole
        # coarse level without one, and the keypoint encoder's last bias, zero by construction, then has nothing to move it)
        wc, we = H.train_loss_weights(d["conf_matrix"].shape, d["expec_f"].shape)
        loss = (d["conf_matrix"] * wc.cuda()).sum() + (d["expec_f"] * we.cuda()).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert torch.isfinite(loss)
    assert torch.isfinite(opt.last_grad_norm).all() and float(opt.last_grad_norm) > 0
    n = 0
    for k, p in model.named_parameters():
        if p.grad is not None:
            assert int(p.grad.count_nonzero()) > 0, "the test's loss leaves %s without a gradient" % k
            assert torch.isfinite(p).all() and not torch.equal(before[k], p.detach()), k
            n += 1
    assert n == 144
    model.eval()
    with torch.no_grad():
        d1 = dict(resident)
        model(d1)
        fresh = ops.make_model(cfg, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
        d2 = {k: v.clone() for k, v in resident.items()}
        fresh(d2)
    torch.cuda.synchronize()
    print("matches before / after training / fresh module: %d / %d / %d" % (len(d0["mconf"]), len(d1["mconf"]), len(d2["mconf"])))
    assert len(d1["mconf"]) > 0                                   # (so that the comparison of the matches below is not empty)
    assert not torch.equal(d0["conf_matrix"], d1["conf_matrix"])
    assert torch.equal(d1["conf_matrix"], d2["conf_matrix"])
    assert torch.equal(d1["i_ids"], d2["i_ids"]) and torch.equal(d1["mconf"], d2["mconf"])


def test_refusals():
    from onepose_plus_plus_amd.optim import FusedAdam
    with pytest.raises(ValueError, match="fp32"):
        FusedAdam([torch.nn.Parameter(torch.zeros(8, device="cuda", dtype=torch.float16))])
    with pytest.raises(ValueError, match="ROCm device"):
        FusedAdam([torch.nn.Parameter(torch.zeros(8))])
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdam([torch.nn.Parameter(torch.zeros(8, device="cuda"))], amsgrad=True)
    with pytest.raises(ValueError, match="contiguous"):
        FusedAdam([torch.nn.Parameter(torch.zeros(8, 4, device="cuda").t())])
    opt = FusedAdam([torch.nn.Parameter(torch.zeros(8, device="cuda"))])
    with pytest.raises(RuntimeError, match="closure"):
        opt.step(lambda: 0.0)
