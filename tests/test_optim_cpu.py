"""CPU: what the fused optimizer (onepose_plus_plus_amd/optim.py, csrc/optim.hip) rests on and that needs no device -- the float64
restatement against torch itself, the error bar against torch's fp32 run and against every semantic slip, the chunk plan
(a pure host function of the library), the reference's two builders and the drop-in registration.  The kernels are held to the
restatement on the device by tests/test_optim_gpu.py."""
import ctypes
import sys

import pytest
import torch

from tests import optim_reference as R


@pytest.mark.parametrize("steps", [1, 10])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("decoupled", [False, True])
def test_restatement_equals_torch_in_float64(decoupled, clip, steps):
    """`clip_grad_norm_` + torch.optim.Adam / AdamW in float64 on the CPU: p, m and v of every tensor to 1e-12 of its largest entry"""
    params, grads = R.make_case(steps)
    got = R.run_torch(params, grads, decoupled, clip, 1.0, dtype=torch.float64)
    worst = R.worst_units(got, R.run_reference(params, grads, decoupled, clip, 1.0))
    print("float64, decoupled %s clip %s, %d steps:" % (decoupled, clip, steps), {k: u * R.UNIT for k, u in worst.items()})
    assert all(u * R.UNIT <= 1e-12 for u in worst.values())


def test_case_clips_in_some_steps_and_not_in_others():
    """the shared inputs do what the tests need: coefficient < 1 in the first step (the one-step tests) and most others, a norm
    below MAX_NORM in the third, at both gradient scales; gradient scales differ by decades between tensors"""
    _, grads = R.make_case(10)
    for scale in (1.0, 0.5):
        norms = R.grad_norms(grads, scale)
        assert norms[0] > 10 * R.MAX_NORM and norms[2] < R.MAX_NORM and sum(n > R.MAX_NORM for n in norms) == 9
    rms = [float(g.double().pow(2).mean().sqrt()) for g in grads[0][6:]]
    assert max(rms) / min(rms) > 1e3


@pytest.mark.parametrize("steps", sorted(R.MEASURED_UNITS))
def test_bar_is_four_times_torch_fp32_distance(steps):
    """the committed bar: torch's own fp32 CPU run lies within a quarter of it (the instruction mix of the CPU kernels may differ
    between machines, so the re-measurement is held to the bar's quarter with the margin the rounding-up of the constants left,
    not to the recorded digits)"""
    got = R.measure_torch_fp32(steps)
    print("torch fp32 against the restatement after %d steps, units of 2^-24:" % steps, got, "recorded", R.MEASURED_UNITS[steps])
    for kind in ("p", "m", "v"):
        assert 4.0 * max(r[kind] for r in R.MEASURED_UNITS.values()) <= R.BAR_UNITS[kind]
        assert got[kind] <= R.BAR_UNITS[kind]


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_semantic_slip_exceeds_the_bar(mutation):
    """decay applied after the update, eps inside the bias-corrected root, bias corrections at t - 1, a missing clip, a clip per
    group: each moves p by > 10^3 units, i.e. far beyond BAR_UNITS["p"] = 110.  Smallest, from a CPU run: decay after the update,
    AdamW, one step, 5.8e3 units.  (Decay after the update is no slip for Adam's coupled decay, and t - 1 = 0 has no bias
    correction: those combinations are not mutations.)"""
    cases = [(10, True)]
    if mutation != "bias_correction_at_t_minus_1":
        cases.append((1, True))
    if mutation != "decay_after_update":
        cases.append((10, False))
    for steps, decoupled in cases:
        moved = R.mutation_units(steps, mutation, decoupled)
        print("%s, decoupled %s, %d steps: p moves by %.3g units" % (mutation, decoupled, steps, moved))
        assert moved > 1e3 and moved > 10 * R.BAR_UNITS["p"]


def test_chunk_plan_covers_every_element_once():
    """`opp_optim_plan` through the library, no device: every element of every tensor exactly once, no chunk across two tensors,
    none for the empty tensor, sum ceil(n / C) chunks"""
    from onepose_plus_plus_amd import _lib
    from onepose_plus_plus_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    C = lib.opp_optim_chunk_elems()
    assert C == R.CHUNK and C % 4 == 0
    counts = [1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3, 0, 7]
    numel = (ctypes.c_longlong * len(counts))(*counts)
    total = ctypes.c_longlong(-1)
    assert lib.opp_optim_plan(numel, len(counts), None, 0, ctypes.byref(total)) == 0
    assert total.value == sum((n + C - 1) // C for n in counts) == 12
    chunks = (_lib.OppOptimChunk * total.value)()
    assert lib.opp_optim_plan(numel, len(counts), chunks, total.value, ctypes.byref(total)) == 0
    seen = [[0] * n for n in counts]
    for c in chunks:
        assert 0 <= c.tensor < len(counts) and 1 <= c.len <= C and c.start % C == 0
        assert c.start + c.len <= counts[c.tensor]                      # within its one tensor
        for i in range(c.start, c.start + c.len):
            seen[c.tensor][i] += 1
    assert all(all(x == 1 for x in s) for s in seen)
    assert not any(c.tensor == 8 for c in chunks)
    assert [c.tensor for c in chunks] == sorted(c.tensor for c in chunks)
    # a table that is too small and a negative count are argument errors, reported through the C error channel
    assert lib.opp_optim_plan(numel, len(counts), chunks, total.value - 1, ctypes.byref(total)) != 0
    assert b"optim_plan" in lib.opp_last_error()
    numel[2] = -1
    assert lib.opp_optim_plan(numel, len(counts), None, 0, ctypes.byref(total)) != 0
    empty = ctypes.c_longlong(-1)
    assert lib.opp_optim_plan(None, 0, None, 0, ctypes.byref(empty)) == 0 and empty.value == 0


class _StubAdam(torch.optim.SGD):
    """stands in for the device optimizer: records what the builder passes"""

    def __init__(self, params, lr, **kw):
        self.received = dict(kw, lr=lr)
        super().__init__(params, lr=lr)


def _hparams(**trainer):
    base = {"optimizer": "adamw", "true_lr": 4e-4, "adam_decay": 0.0, "adamw_decay": 0.1, "scheduler": "MultiStepLR",
            "scheduler_invervel": "epoch", "mslr_milestones": [3, 6, 9, 12], "mslr_gamma": 0.5, "cosa_tmax": 30, "elr_gamma": 0.9}
    return {"trainer": dict(base, **trainer)}


def test_build_optimizer_plumbing(monkeypatch):
    from onepose_plus_plus_amd import optim
    monkeypatch.setattr(optim, "FusedAdam", _StubAdam)
    model = torch.nn.Linear(3, 2)
    opt = optim.build_optimizer(model, _hparams(), max_grad_norm=0.5, grad_scale=0.5)
    assert opt.received == dict(lr=4e-4, weight_decay=0.1, decoupled=True, module=model, max_grad_norm=0.5, grad_scale=0.5)
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in model.parameters()]
    opt = optim.build_optimizer(model, _hparams(optimizer="adam", adam_decay=0.03))
    assert opt.received == dict(lr=4e-4, weight_decay=0.03, decoupled=False, module=model)
    with pytest.raises(ValueError, match="TRAINER.OPTIMIZER = sgd is not a valid optimizer!"):
        optim.build_optimizer(model, _hparams(optimizer="sgd"))


def test_fused_adam_is_a_torch_optimizer_and_refuses_what_it_cannot_run():
    """no device needed to refuse: CPU and fp16 parameters and the unsupported options raise before anything is allocated"""
    from onepose_plus_plus_amd.optim import FusedAdam
    assert issubclass(FusedAdam, torch.optim.Optimizer)
    with pytest.raises(ValueError, match="ROCm device"):
        FusedAdam([torch.nn.Parameter(torch.zeros(4))])
    with pytest.raises(ValueError, match="fp32"):
        FusedAdam([torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))])
    for name in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(ValueError, match=name):
            FusedAdam([torch.nn.Parameter(torch.zeros(4))], **{name: True})
    with pytest.raises(ValueError):
        FusedAdam([torch.nn.Parameter(torch.zeros(4))], lr=-1.0)
    with pytest.raises(ValueError):
        FusedAdam([torch.nn.Parameter(torch.zeros(4))], max_grad_norm=0.0)


def test_build_scheduler_names_and_effect(monkeypatch):
    from torch.optim.lr_scheduler import CosineAnnealingLR, ExponentialLR, MultiStepLR
    from onepose_plus_plus_amd import optim
    monkeypatch.setattr(optim, "FusedAdam", _StubAdam)
    model = torch.nn.Linear(3, 2)

    def lrs(name, n, **trainer):
        hp = _hparams(scheduler=name, **trainer)
        opt = optim.build_optimizer(model, hp)
        out = optim.build_scheduler(hp, opt)
        assert set(out) == {"scheduler", "interval"} and out["interval"] == hp["trainer"]["scheduler_invervel"]
        seen = [opt.param_groups[0]["lr"]]
        for _ in range(n):
            opt.step()
            out["scheduler"].step()
            seen.append(opt.param_groups[0]["lr"])
        return out["scheduler"], seen

    s, seen = lrs("MultiStepLR", 4, mslr_milestones=[1, 3], mslr_gamma=0.5)
    assert isinstance(s, MultiStepLR) and seen == pytest.approx([4e-4, 2e-4, 2e-4, 1e-4, 1e-4])
    s, seen = lrs("CosineAnnealing", 4, cosa_tmax=4, scheduler_invervel="step")
    assert isinstance(s, CosineAnnealingLR) and s.T_max == 4 and seen[2] == pytest.approx(2e-4) and seen[4] == pytest.approx(0.0, abs=1e-12)
    s, seen = lrs("ExponentialLR", 2, elr_gamma=0.9)
    assert isinstance(s, ExponentialLR) and seen == pytest.approx([4e-4, 3.6e-4, 3.24e-4])
    with pytest.raises(NotImplementedError):
        optim.build_scheduler(_hparams(scheduler="OneCycle"), optim.build_optimizer(model, _hparams()))


def _without_src_modules():
    saved = {k: v for k, v in sys.modules.items() if k == "src" or k.startswith("src.")}
    for k in saved:
        sys.modules.pop(k, None)
    return saved


def _restore_src_modules(saved, saved_path):
    sys.path[:] = saved_path
    for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
        del sys.modules[k]
    sys.modules.update(saved)


def test_dropin_registers_the_builders_only_on_request():
    import types
    from onepose_plus_plus_amd import dropin, optim
    saved_path = list(sys.path)
    saved = _without_src_modules()
    try:
        done = dropin.install()
        assert set(done) == {"src.models.OnePosePlus.OnePosePlusModel", "src.models.OnePosePlus", "src.utils.metric_utils",
                             "src.lightning_model.losses", "src.models.OnePosePlus.utils.fine_supervision"}
        assert "src.models.OnePosePlus.optimizers.optimizers" not in sys.modules
    finally:
        _restore_src_modules(saved, saved_path)
    saved = _without_src_modules()
    try:
        # a Lightning module imported before install(): it bound the reference's builders already
        lm = types.ModuleType("src.lightning_model.OnePosePlus_lightning_model")
        lm.build_optimizer = lm.build_scheduler = lm.Loss = lm.fine_supervision = None
        dropin.install(pnp=False, loss=False)
        sys.modules[lm.__name__] = lm
        done = dropin.install(pnp=False, loss=False, optimizer=True)
        assert done["src.models.OnePosePlus.optimizers.optimizers"] == "build_optimizer, build_scheduler"
        assert done["src.lightning_model.OnePosePlus_lightning_model:build_optimizer"] == "build_optimizer, build_scheduler"
        from src.models.OnePosePlus.optimizers.optimizers import build_optimizer, build_scheduler
        assert build_optimizer is optim.build_optimizer and build_scheduler is optim.build_scheduler
        assert lm.build_optimizer is optim.build_optimizer and lm.build_scheduler is optim.build_scheduler
        assert lm.Loss is None                                   # loss=False: not touched
        import src.models.OnePosePlus as pkg
        assert pkg.optimizers.optimizers is sys.modules["src.models.OnePosePlus.optimizers.optimizers"]
    finally:
        _restore_src_modules(saved, saved_path)
