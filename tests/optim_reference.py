"""float64 restatement of one optimizer step as the reference runs it: `torch.nn.utils.clip_grad_norm_` (Lightning's
`gradient_clip_val`, train.yaml:32) then `torch.optim.Adam` / `AdamW` (optimizers/optimizers.py:4-13), written from the formulas:

    total_norm = sqrt(sum over ALL tensors of |g * grad_scale|^2),   coef = min(1, max_norm / (total_norm + 1e-6))
    g' = g * grad_scale * coef
    AdamW: p *= 1 - lr * wd            Adam: g' += wd * p
    m += (g' - m) * (1 - beta1)        v = v * beta2 + (1 - beta2) * g' * g'
    p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)

plus the inputs the optimizer tests share (`make_case`), the distance they measure (`distance_units`) and the error bar.

THE BAR.  torch's own fp32 run differs from float64 by thousands of ulps on single elements where `m` cancels, so every
comparison is max|x - x64| / max|x64| per tensor and per kind (p, m, v), in units of 2^-24.  The bar is measured, not chosen: the
distance of `torch.optim.Adam / AdamW(foreach=False)` in fp32 on the CPU from this restatement on the same inputs (`make_case`)
after 1, 3, 6 and 10 steps (the step counts the tests run), maximum over the tensors of `SIZES`, over the variants (Adam / AdamW x
clipping on / off x grad_scale 1 / 0.5) and over the four step counts, times four (FMA contraction and the rounding of division
and square root on the device, each at most one ulp per operation).
`MEASURED_UNITS` holds what `measure_torch_fp32()` gave when the constants were committed; tests/test_optim_cpu.py re-measures and
checks that it still lies under `BAR_UNITS`, and that every semantic slip of `MUTATIONS` lies far above it.
"""
import math

import torch

CHUNK = 8192                                             # OPP_OPTIM_CHUNK (include/opp_hip.h); the tests check the library agrees
SIZES = [1, 3, 4, 5, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
# exaggerated hyper-parameters: a semantic slip moves p by > 10^3 units, far above rounding
HYPER = dict(lr=5e-2, betas=(0.7, 0.9), eps=1e-3, weight_decay=0.5)
MAX_NORM = 1.0
UNIT = 2.0 ** -24
MUTATIONS = ("decay_after_update", "eps_inside_root", "bias_correction_at_t_minus_1", "no_clip", "clip_per_group")

# distance of torch's fp32 CPU run from the restatement, in units, by number of steps and kind (measure_torch_fp32());
# (the one- and three-element tensors set these values: with a single entry the measure is elementwise after all)
MEASURED_UNITS = {1: {"p": 26.32, "m": 4.25, "v": 6.68}, 3: {"p": 3.64, "m": 15.74, "v": 5.72},
                  6: {"p": 5.93, "m": 15.84, "v": 5.62}, 10: {"p": 21.87, "m": 13.41, "v": 6.32}}
# one bar per kind for every test of 1 to 10 steps: four times the largest entry of its column above, rounded up to two digits
BAR_UNITS = {"p": 110.0, "m": 64.0, "v": 27.0}
# the smallest semantic slip of MUTATIONS moves p by 5.8e3 units (decay after the update, AdamW, one step; mutation_units())
NORM_BAR_UNITS = 4.0                                     # last_grad_norm against the float64 norm


def distance_units(x, x64):
    """max|x - x64| / max|x64| in units of 2^-24"""
    x64 = x64.double().reshape(-1)
    scale = float(x64.abs().max())
    return float((x.detach().double().reshape(-1).cpu() - x64).abs().max()) / scale / UNIT


def make_case(steps, seed=0, sizes=None):
    """-> (params, grads): fp32 CPU tensors of `sizes` elements and, per step, one gradient per tensor.  Parameter and gradient
    scales vary by decades between tensors; the gradient norm lies far above MAX_NORM in every step but the third, where it
    lies below it (`grad_norms` confirms both)."""
    sizes = SIZES if sizes is None else sizes
    gen = torch.Generator().manual_seed(1234 + seed)
    params = [torch.randn(n, generator=gen) * 10.0 ** (i % 3) for i, n in enumerate(sizes)]
    grads = []
    for k in range(steps):
        level = 2e-4 if k == 2 else 1.0 + 0.5 * k
        grads.append([torch.randn(n, generator=gen) * (level * 10.0 ** (i % 5 - 3)) for i, n in enumerate(sizes)])
    return params, grads


def grad_norms(grads, grad_scale=1.0):
    """float64 global norm of every step's gradients"""
    return [math.sqrt(sum(float((g.double() * grad_scale).pow(2).sum()) for g in step if g is not None)) for step in grads]


class ReferenceAdam:
    """groups: list of dicts {"params": [tensors], lr, betas, eps, weight_decay, decoupled}; everything is held in float64.
    `step(grads)` takes one list of gradients per group (None = that parameter is skipped, its state does not move)."""

    def __init__(self, groups, max_grad_norm=None, grad_scale=1.0, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.groups = [dict(g, params=[p.detach().double().cpu().clone() for p in g["params"]]) for g in groups]
        self.m = [[torch.zeros_like(p) for p in g["params"]] for g in self.groups]
        self.v = [[torch.zeros_like(p) for p in g["params"]] for g in self.groups]
        self.t = [[0 for _ in g["params"]] for g in self.groups]
        self.max_grad_norm, self.grad_scale, self.mutation = max_grad_norm, grad_scale, mutation
        self.last_norm = None

    def _coef(self, grad_lists):
        sq = sum(float((g.double() * self.grad_scale).pow(2).sum()) for gl in grad_lists for g in gl if g is not None)
        norm = math.sqrt(sq)
        return min(1.0, self.max_grad_norm / (norm + 1e-6)), norm

    def step(self, grads):
        coefs = [1.0] * len(self.groups)
        if self.max_grad_norm is not None:
            coef, self.last_norm = self._coef(grads)
            coefs = [coef] * len(self.groups)
            if self.mutation == "no_clip":
                coefs = [1.0] * len(self.groups)
            if self.mutation == "clip_per_group":
                coefs = [self._coef([gl])[0] for gl in grads]
        for gi, group in enumerate(self.groups):
            lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            for i, g in enumerate(grads[gi]):
                if g is None:
                    continue
                p, m, v = group["params"][i], self.m[gi][i], self.v[gi][i]
                self.t[gi][i] += 1
                t = self.t[gi][i]
                g = g.detach().double().cpu() * self.grad_scale * coefs[gi]
                decay_now = wd != 0 and self.mutation != "decay_after_update"
                if decay_now and group["decoupled"]:
                    p = p * (1 - lr * wd)
                if wd != 0 and not group["decoupled"]:
                    g = g + wd * p
                m = m + (g - m) * (1 - b1)
                v = v * b2 + (1 - b2) * g * g
                tb = t - 1 if self.mutation == "bias_correction_at_t_minus_1" and t > 1 else t     # (t = 1 would divide by zero)
                bc1, bc2 = 1 - b1 ** tb, 1 - b2 ** tb
                if self.mutation == "eps_inside_root":
                    denom = (v.sqrt() + eps) / math.sqrt(bc2)
                else:
                    denom = v.sqrt() / math.sqrt(bc2) + eps
                p = p - (lr / bc1) * m / denom
                if wd != 0 and group["decoupled"] and not decay_now:
                    p = p * (1 - lr * wd)
                group["params"][i], self.m[gi][i], self.v[gi][i] = p, m, v

    def kinds(self):
        """-> {"p": [...], "m": [...], "v": [...]} flat over the groups"""
        return {"p": [p for g in self.groups for p in g["params"]], "m": [m for ml in self.m for m in ml],
                "v": [v for vl in self.v for v in vl]}


def one_group(params, decoupled, **over):
    return [dict(HYPER, params=params, decoupled=decoupled, **over)]


def worst_units(kinds, ref):
    """-> {"p": u, "m": u, "v": u}: the largest distance over the tensors; kinds: {"p": [...], "m": [...], "v": [...]}"""
    want = ref.kinds()
    return {k: max(distance_units(x, x64) for x, x64 in zip(kinds[k], want[k])) for k in ("p", "m", "v")}


VARIANTS = [(decoupled, clip, scale) for decoupled in (False, True) for clip in (True, False) for scale in (1.0, 0.5)]


def run_torch(params, grads, decoupled, clip, scale, dtype=torch.float32, device="cpu", **kw):
    """`clip_grad_norm_` + torch.optim.Adam / AdamW, one tensor at a time -> kinds"""
    ps = [torch.nn.Parameter(p.to(device=device, dtype=dtype).clone()) for p in params]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(ps, foreach=False, **dict(HYPER, **kw))
    for step in grads:
        for p, g in zip(ps, step):
            p.grad = g.to(device=device, dtype=dtype) * scale
        if clip:
            torch.nn.utils.clip_grad_norm_(ps, MAX_NORM, foreach=False)
        opt.step()
    return {"p": [p.detach() for p in ps], "m": [opt.state[p]["exp_avg"] for p in ps], "v": [opt.state[p]["exp_avg_sq"] for p in ps]}


def run_reference(params, grads, decoupled, clip, scale, mutation=None):
    ref = ReferenceAdam(one_group(params, decoupled), max_grad_norm=MAX_NORM if clip else None, grad_scale=scale, mutation=mutation)
    for step in grads:
        ref.step([step])
    return ref


def measure_torch_fp32(steps):
    """-> {"p": u, "m": u, "v": u}: torch's fp32 CPU run against the restatement, worst tensor of the worst variant"""
    params, grads = make_case(steps)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for decoupled, clip, scale in VARIANTS:
        got = worst_units(run_torch(params, grads, decoupled, clip, scale), run_reference(params, grads, decoupled, clip, scale))
        worst = {k: max(worst[k], got[k]) for k in worst}
    return worst


def split_groups(params, decoupled, first=None, second=None):
    """two parameter groups: the first half of the tensors and the rest, with HYPER overridden by `first` / `second`"""
    half = len(params) // 2
    return [dict(HYPER, params=params[:half], decoupled=decoupled, **(first or {})),
            dict(HYPER, params=params[half:], decoupled=decoupled, **(second or {}))]


def split_grads(step):
    half = len(step) // 2
    return [step[:half], step[half:]]


def mutation_units(steps, mutation, decoupled):
    """how far a semantic slip moves p: the mutated restatement against the right one (two groups, clipping on), measured like the
    bar -- the worst tensor's distance in units"""
    params, grads = make_case(steps)
    runs = []
    for mut in (None, mutation):
        ref = ReferenceAdam(split_groups(params, decoupled), max_grad_norm=MAX_NORM, mutation=mut)
        for step in grads:
            ref.step(split_grads(step))
        runs.append(ref.kinds()["p"])
    return max(distance_units(x, x64) for x, x64 in zip(runs[1], runs[0]))


if __name__ == "__main__":
    for n in sorted(MEASURED_UNITS):
        print(n, {k: round(u, 2) for k, u in measure_torch_fp32(n).items()})
    for mut in MUTATIONS:
        print(mut, {(n, dec): "%.3g" % mutation_units(n, mut, dec) for n in (1, 10) for dec in (False, True)})
