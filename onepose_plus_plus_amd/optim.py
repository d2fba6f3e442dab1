"""The parameter update of the training step on this package's own kernels, and the reference's optimizer / scheduler builders.

The reference trains with `torch.optim.AdamW` (src/models/OnePosePlus/optimizers/optimizers.py:4-13) under Lightning's
`gradient_clip_val: 0.5` (train.yaml:32), i.e. `clip_grad_norm_` + a foreach Adam: about a dozen multi-tensor launches
over the 144 parameter tensors.  `FusedAdam` does the same arithmetic in two launches of csrc/optim.hip
(include/opp_hip.h `opp_grad_sqnorm`, `opp_adam_step`): the global gradient norm, then clip + weight decay + both moments
+ the parameter update in one sweep, with no host synchronisation.

    from onepose_plus_plus_amd.optim import build_optimizer, build_scheduler
    opt = build_optimizer(model, hparams, max_grad_norm=0.5)          # in place of the reference's builder + clip_grad_norm_
    sched = build_scheduler(hparams, opt)["scheduler"]
    loss.backward(); opt.step(); opt.zero_grad(); sched.step()

There is no fallback: parameters the kernel cannot update (not fp32, not contiguous, not on a ROCm device) are refused.
"""
import ctypes

import torch
from torch.optim.lr_scheduler import CosineAnnealingLR, ExponentialLR, MultiStepLR

from . import _lib

# options of torch.optim.Adam that this optimizer refuses; the keys stay in `param_groups` (with torch's "off" values) so that
# a `state_dict()` written here loads into torch.optim.Adam / AdamW, whose load replaces its groups by the saved ones
_REFUSED = ("amsgrad", "maximize", "capturable", "differentiable")


class _Segment:
    """parameters of one group that share a step count: one update launch over the chunks [first, first + count)"""
    __slots__ = ("group", "first", "count", "t", "slots", "ones")


class FusedAdam(torch.optim.Optimizer):
    """Adam (`decoupled=False`) / AdamW (`decoupled=True`) with optional global-norm gradient clipping, as torch.optim.Adam /
    AdamW behind `torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm)` compute them, on csrc/optim.hip.

    * `max_grad_norm`: clip by the norm over the gradients of ALL groups (one norm launch, then one update launch per
      parameter group).  `.grad` is left untouched: the coefficient is applied inside the update, where `clip_grad_norm_`
      would have scaled the gradients in place.  `last_grad_norm` (one-element device tensor) receives the norm before
      clipping; the host never reads it.
    * `grad_scale` multiplies every gradient before the norm: `1 / accumulate_grad_batches` after summed backward passes,
      `1 / world_size` after a SUM all-reduce.
    * `module`: if it has `repack()`, `step()` calls it.  The kernel writes the parameters through raw pointers, which does
      not move `tensor._version`; `OnePosePlus_model` caches packed weights and object tokens that must follow the update.
    * State: `state[p]["exp_avg"]` / `["exp_avg_sq"]` are views into two flat fp32 buffers, `state[p]["step"]` a CPU fp32
      scalar as in torch; `state_dict()` has torch's layout and `load_state_dict()` takes one written by torch.optim.Adam /
      AdamW (the moments are copied into the flat views), and the other way round.
    * Parameters whose `.grad` is None are skipped, as torch skips them.
    * `zero_grad(set_to_none=False)`: note the default -- gradients are kept and zeroed (one fill when they form one
      contiguous buffer), so that `step()` finds the same addresses and reuses its device tables.

    Refused with an error: amsgrad, maximize, capturable, differentiable, sparse gradients, a closure."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, decoupled=False, max_grad_norm=None,
                 grad_scale=1.0, module=None, amsgrad=False, maximize=False, capturable=False, differentiable=False):
        for name, value in zip(_REFUSED, (amsgrad, maximize, capturable, differentiable)):
            if value:
                raise ValueError("FusedAdam does not support %s=True" % name)
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedAdam needs lr as a Python number (a tensor lr is torch's capturable path)")
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("Invalid beta parameters: %r" % (betas,))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be positive or None, got %r" % (max_grad_norm,))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_scale = float(grad_scale)
        self.module = module
        self._device = None
        self._blocks = []            # (m, v): flat moment buffers; one pair unless groups are added after construction
        self._slot = {}              # parameter -> (exp_avg view, exp_avg_sq view, index into _steps)
        self._steps = torch.zeros(0, dtype=torch.float32)
        self._key = None             # the (index, p.data_ptr(), p.grad.data_ptr()) tuple the device tables were built for
        self._tables = None
        self._segments = []
        self._stage, self._stage_next = [[None, None], [None, None]], 0      # pinned staging buffers of the tables + their copy events
        self._zero_key, self._zero_flat = None, None
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=bool(decoupled))
        super().__init__(params, defaults)
        self.last_grad_norm = torch.zeros(1, dtype=torch.float32, device=self._device)

    # ---- parameters and state -------------------------------------------------------------------
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            self._check_group(group)
            for p in group["params"]:
                self._check_param(p)
        except ValueError:
            self.param_groups.pop()
            raise
        self._allocate(group["params"])
        self._key = None

    @staticmethod
    def _check_group(group):
        for name in _REFUSED:
            if group.get(name):
                raise ValueError("FusedAdam does not support %s=True" % name)
        if isinstance(group["lr"], torch.Tensor):
            raise ValueError("FusedAdam needs lr as a Python number")

    def _check_param(self, p):
        if p.dtype != torch.float32:
            raise ValueError("FusedAdam updates fp32 parameters only, got %s" % p.dtype)
        if not p.is_cuda:
            raise ValueError("FusedAdam needs parameters on a ROCm device, got one on %s" % p.device)
        if p.is_sparse or not p.is_contiguous():
            raise ValueError("FusedAdam needs dense contiguous parameters (shape %s, stride %s)" % (tuple(p.shape), p.stride()))
        if self._device is None:
            self._device = p.device
        elif p.device != self._device:
            raise ValueError("FusedAdam needs all parameters on one device, got %s and %s" % (self._device, p.device))

    def _allocate(self, params):
        """moment views for `params`: one flat buffer each for m and v, every tensor at a multiple of 4 elements (16 bytes)"""
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4
        m = torch.zeros(total, dtype=torch.float32, device=self._device)
        v = torch.zeros(total, dtype=torch.float32, device=self._device)
        self._blocks.append((m, v))
        base = self._steps.numel()
        self._steps = torch.cat([self._steps, torch.zeros(len(params), dtype=torch.float32)])
        for i, (p, off) in enumerate(zip(params, offs)):
            n = p.numel()
            pm, pv = m[off:off + n].view_as(p), v[off:off + n].view_as(p)
            self._slot[p] = (pm, pv, base + i, n, pm.data_ptr(), pv.data_ptr())
        for p, entry in self._slot.items():               # _steps was reallocated: the step views of live states follow it
            slot = entry[2]
            if slot < base and "step" in self.state.get(p, {}):
                self.state[p]["step"] = self._steps[slot]

    def _attach(self, p, source=None):
        """state[p] = the flat views (filled from `source`, a state dict entry of torch's layout, when given)"""
        m, v, slot = self._slot[p][:3]
        if source is not None:
            for name, dst in (("exp_avg", m), ("exp_avg_sq", v)):
                if name not in source or tuple(source[name].shape) != tuple(dst.shape):
                    raise ValueError("loaded optimizer state has no %s of shape %s" % (name, tuple(dst.shape)))
                dst.copy_(source[name])
            self._steps[slot] = float(source["step"])
        self.state[p] = {"step": self._steps[slot], "exp_avg": m, "exp_avg_sq": v}

    def load_state_dict(self, state_dict):
        """also accepts a dict written by torch.optim.Adam / AdamW: the base class replaces the state tensors by casts of the
        loaded ones, then the moments are copied INTO the flat views and the views re-attached"""
        before = [g.get("decoupled_weight_decay", False) for g in self.param_groups]
        super().load_state_dict(state_dict)
        for group, decoupled in zip(self.param_groups, before):
            group.setdefault("decoupled_weight_decay", decoupled)       # torch before 2.7 had no such key: keep this optimizer's
            self._check_group(group)
        for group in self.param_groups:
            for p in group["params"]:
                loaded = self.state.get(p)
                if loaded:
                    self._attach(p, source=loaded)
                else:                                     # no state in the dict: the parameter starts afresh, as in torch
                    m, v, slot = self._slot[p][:3]
                    m.zero_()
                    v.zero_()
                    self._steps[slot] = 0.0
        self._key = None

    # ---- device tables --------------------------------------------------------------------------
    def _rebuild(self, key, entries):
        """entries: (group index, parameter) of every parameter with a gradient, in group order.  Runs when the addresses
        changed (every step under `zero_grad(set_to_none=True)` if the allocator hands out other blocks), so it avoids what costs
        host time: the two tables go to the device in ONE asynchronous copy from pinned memory, nothing waits for the device"""
        lib = _lib.load()
        chunk = lib.opp_optim_chunk_elems()
        steps = self._steps.tolist()
        keyed = []
        for gi, p in entries:
            g = p.grad
            m, v, slot, n, m_ptr, v_ptr = self._slot[p]
            if g.is_sparse:
                raise RuntimeError("FusedAdam does not support sparse gradients")
            if g.dtype != torch.float32 or g.device != self._device or not g.is_contiguous() or g.numel() != n:
                raise ValueError("FusedAdam needs fp32 contiguous gradients on the parameter's device (parameter of shape %s: gradient "
                                 "%s, %s, stride %s)" % (tuple(p.shape), g.dtype, g.device, g.stride()))
            st = self.state.get(p)
            if not st:
                self._attach(p)
            elif st["exp_avg"] is not m or st["exp_avg_sq"] is not v:
                raise RuntimeError("FusedAdam keeps the moments in its flat buffers: state[p]['exp_avg'] / ['exp_avg_sq'] were replaced "
                                   "(use load_state_dict, or write into the tensors in place)")
            keyed.append((gi, int(round(steps[slot])), len(keyed), p.data_ptr(), g.data_ptr(), m_ptr, v_ptr, n, slot))
        # within a group, parameters that skipped steps (gradient None) have another bias correction: one launch per step count
        keyed.sort(key=lambda e: e[:3])
        n_rows = len(keyed)
        rows = (_lib.OppOptimTensor * max(n_rows, 1))()
        numel = (ctypes.c_longlong * max(n_rows, 1))()
        segments, first = [], 0
        for row, (gi, t_now, _, p_ptr, g_ptr, m_ptr, v_ptr, n, slot) in enumerate(keyed):
            r = rows[row]
            r.p, r.g, r.m, r.v, r.n = p_ptr, g_ptr, m_ptr, v_ptr, n
            numel[row] = n
            if not segments or segments[-1].group != gi or segments[-1].t != t_now:
                seg = _Segment()
                seg.group, seg.first, seg.count, seg.t, seg.slots = gi, first, 0, t_now, []
                segments.append(seg)
            n_chunks = (n + chunk - 1) // chunk
            segments[-1].count += n_chunks
            segments[-1].slots.append(slot)
            first += n_chunks
        for seg in segments:
            seg.slots = torch.tensor(seg.slots, dtype=torch.int64)
            seg.ones = torch.ones(len(seg.slots), dtype=torch.float32)
        chunks = (_lib.OppOptimChunk * max(first, 1))()
        total = ctypes.c_longlong(0)
        _lib.check(lib.opp_optim_plan(numel, n_rows, chunks, first, ctypes.byref(total)), "opp_optim_plan")
        assert total.value == first
        # [tensor table | chunk table] through one of two pinned staging buffers (the copy of the step before may still be in flight)
        rows_bytes, chunks_bytes = ctypes.sizeof(rows), ctypes.sizeof(chunks)
        chunks_at = (rows_bytes + 255) // 256 * 256
        nbytes = chunks_at + chunks_bytes
        if self._stage[0][0] is None or self._stage[0][0].numel() < nbytes:
            room = (nbytes * 2 + 4095) // 4096 * 4096      # one pinned allocation (a slow call) for both halves, with room to grow
            pinned = torch.empty(2 * room, dtype=torch.uint8).pin_memory()
            self._stage = [[pinned[:room], None], [pinned[room:], None]]
        self._stage_next ^= 1
        stage = self._stage[self._stage_next]
        if stage[1] is not None:
            stage[1].synchronize()
        ctypes.memmove(stage[0].data_ptr(), rows, rows_bytes)
        ctypes.memmove(stage[0].data_ptr() + chunks_at, chunks, chunks_bytes)
        old = self._tables
        with torch.cuda.device(self._device):
            table = torch.empty(nbytes, dtype=torch.uint8, device=self._device)
            table.copy_(stage[0][:nbytes], non_blocking=True)
            stage[1] = torch.cuda.Event()
            stage[1].record(torch.cuda.current_stream(self._device))
        partials = old["partials"] if old is not None and old["partials"].numel() >= first else \
            torch.empty(max(first, 1), dtype=torch.float64, device=self._device)
        self._tables = {"table": table, "tensors": table.data_ptr(), "chunks": table.data_ptr() + chunks_at, "n_chunks": first,
                        "partials": partials}
        self._segments = segments
        self._key = key

    # ---- the step -------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise RuntimeError("FusedAdam.step() takes no closure: evaluate the loss and call backward() before the step")
        key, entries = [], []
        index = 0
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.grad is not None:
                    key.append((index, p.data_ptr(), p.grad.data_ptr()))
                    entries.append((gi, p))
                index += 1
        key = tuple(key)
        if key != self._key:
            self._rebuild(key, entries)
        tb = self._tables
        if tb["n_chunks"] == 0:
            return None
        lib = _lib.load()
        tensors, chunks, partials = tb["tensors"], tb["chunks"], tb["partials"].data_ptr()
        clip = self.max_grad_norm is not None
        with torch.cuda.device(self._device):
            stream = torch.cuda.current_stream(self._device).cuda_stream
            if clip:
                _lib.check(lib.opp_grad_sqnorm(tensors, chunks, tb["n_chunks"], self.grad_scale, partials, stream), "opp_grad_sqnorm")
            for seg in self._segments:
                group = self.param_groups[seg.group]
                seg.t += 1
                self._steps.index_add_(0, seg.slots, seg.ones)
                beta1, beta2 = group["betas"]
                _lib.check(lib.opp_adam_step(tensors, chunks + seg.first * ctypes.sizeof(_lib.OppOptimChunk), seg.count,
                                             partials if clip else None, tb["n_chunks"] if clip else 0,
                                             self.max_grad_norm if clip else 0.0, self.last_grad_norm.data_ptr() if clip else None,
                                             self.grad_scale, float(group["lr"]), beta1, beta2, float(group["eps"]), float(group["weight_decay"]),
                                             1 if group["decoupled_weight_decay"] else 0, 1.0 - beta1 ** seg.t, 1.0 - beta2 ** seg.t,
                                             stream), "opp_adam_step")
        if self.module is not None and hasattr(self.module, "repack"):
            self.module.repack()
        return None

    def zero_grad(self, set_to_none=False):
        """keeps the gradients by default (torch's default drops them).  Gradients that form ONE contiguous buffer in
        parameter order (`sharding.GradientAverager`'s layout) are zeroed by a single fill; otherwise the base class's loop"""
        if set_to_none:
            self._zero_key = self._zero_flat = None
            return super().zero_grad(set_to_none=True)
        grads = [p.grad for group in self.param_groups for p in group["params"] if p.grad is not None]
        key = tuple(g.data_ptr() for g in grads)
        if key != self._zero_key:
            self._zero_key, self._zero_flat = key, self._flat_view(grads)
        if self._zero_flat is None:
            return super().zero_grad(set_to_none=False)
        for g in grads:                                   # what the base class does besides zeroing
            if g.grad_fn is not None:
                g.detach_()
            else:
                g.requires_grad_(False)
        self._zero_flat.zero_()
        return None

    @staticmethod
    def _flat_view(grads):
        """one 1-D tensor over `grads` when they lie back to back in one storage, else None"""
        if len(grads) < 2:
            return None
        storage = grads[0].untyped_storage()
        end = grads[0].data_ptr()
        for g in grads:
            if (g.dtype != torch.float32 or not g.is_contiguous() or g.data_ptr() != end
                    or g.untyped_storage().data_ptr() != storage.data_ptr()):
                return None
            end += g.numel() * 4
        total = (end - grads[0].data_ptr()) // 4
        return torch.empty(0, dtype=torch.float32, device=grads[0].device).set_(storage, grads[0].storage_offset(), (total,))


def build_optimizer(model, config, **kw):
    """The reference's `build_optimizer(model, config)` (optimizers/optimizers.py:4-13) on `FusedAdam`:
    config["trainer"]["optimizer"] "adam" (coupled decay `adam_decay`) or "adamw" (decoupled decay `adamw_decay`) at
    `true_lr`.  Extra keywords (`max_grad_norm`, `grad_scale`) go to `FusedAdam`; the model is passed as `module`."""
    trainer = config["trainer"]
    name, lr = trainer["optimizer"], trainer["true_lr"]
    if name == "adam":
        return FusedAdam(model.parameters(), lr=lr, weight_decay=trainer["adam_decay"], decoupled=False, module=model, **kw)
    if name == "adamw":
        return FusedAdam(model.parameters(), lr=lr, weight_decay=trainer["adamw_decay"], decoupled=True, module=model, **kw)
    raise ValueError(f"TRAINER.OPTIMIZER = {name} is not a valid optimizer!")


def build_scheduler(config, optimizer):
    """The reference's `build_scheduler(config, optimizer)` (optimizers/optimizers.py:16-41): -> {"scheduler": ...,
    "interval": config["trainer"]["scheduler_invervel"]} (the key is spelt as upstream) for "MultiStepLR" (`mslr_milestones`,
    `mslr_gamma`), "CosineAnnealing" (`cosa_tmax`) or "ExponentialLR" (`elr_gamma`)."""
    trainer = config["trainer"]
    name = trainer["scheduler"]
    if name == "MultiStepLR":
        scheduler = MultiStepLR(optimizer, trainer["mslr_milestones"], gamma=trainer["mslr_gamma"])
    elif name == "CosineAnnealing":
        scheduler = CosineAnnealingLR(optimizer, trainer["cosa_tmax"])
    elif name == "ExponentialLR":
        scheduler = ExponentialLR(optimizer, trainer["elr_gamma"])
    else:
        raise NotImplementedError("scheduler %r" % (name,))
    return {"interval": trainer["scheduler_invervel"], "scheduler": scheduler}
