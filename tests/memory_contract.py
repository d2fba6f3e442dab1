"""The harness of the workspace contract ("The workspace contract"), shared by tests/test_memory_contract_cpu.py and
tests/test_memory_contract_gpu.py, and three fake stages in plain torch that show on any device that it bites.

A stage is a callable `run(bufs) -> dict of CPU tensors` that takes every byte of device memory from `bufs` (tests/hip_ops.py:
`Buffers`).  `fill_problems` runs it on a zero-filled, a NaN-filled and a left-over workspace and reports, in words, every output
that is not bit-identical to the zero-filled run, every guard band that changed and every read-only input that changed;
`refusal_problems` runs it with a workspace declared too small.  An empty list is a stage that keeps the contract.
"""
import torch

from tests import hip_ops as ops

ERR_WORKSPACE = -4           # OPP_ERR_WORKSPACE (csrc/opp_common.h)
_INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    """integer view of a tensor: NaN payloads and signed zeros count in a comparison"""
    t = t.contiguous()
    return t.view(_INT_OF[t.element_size()])


def _differs(name, got, want, close):
    """-> a sentence, or None when `got` equals `want` bit for bit (or, for the stages named in `close`, within that absolute bar)"""
    if got.shape != want.shape:
        return "output %s has shape %s, the zero-filled run %s" % (name, tuple(got.shape), tuple(want.shape))
    if name in close:
        err = float((got.double() - want.double()).abs().max()) if got.numel() else 0.0
        return None if err <= close[name] else "output %s is %.3e from the zero-filled run (bar %.1e)" % (name, err, close[name])
    d = bits(got) != bits(want)
    if not bool(d.any()):
        return None
    return "output %s differs from the zero-filled run in %d of %d elements (%d of them NaN)" % (
        name, int(d.sum()), d.numel(), int(torch.isnan(got[d]).sum()) if got.is_floating_point() else 0)


def fill_problems(run, run_larger, device="cuda", close=None):
    """run / run_larger: the stage at the shape under test and at a strictly larger one (the predecessor of the `leftover` fill).
    close: {output name: absolute bar} for the outputs of a stage that is order-dependent by design.  -> list of sentences"""
    close = close or {}
    problems, outs = [], {}
    for fill in ops.WS_FILLS:
        bufs = ops.GuardedBuffers(fill, device)
        if fill == "leftover":
            run_larger(bufs)
            problems += ["leftover, larger run: " + p for p in bufs.check()]
            bufs.new_call()
        outs[fill] = run(bufs)
        bufs.sync()
        problems += ["%s: %s" % (fill, p) for p in bufs.check()]
    for fill in ops.WS_FILLS[1:]:
        assert outs[fill].keys() == outs["zero"].keys()
        for k, want in outs["zero"].items():
            p = _differs(k, outs[fill][k], want, close)
            if p:
                problems.append("%s: %s" % (fill, p))
    return problems


def refusal_problems(run, device="cuda", may_write=()):
    """The stage with a workspace declared half as large as the size query says, and empty: the call must fail with the workspace error
    code and leave every output, the workspace and the guard bands as they were.  may_write: outputs of a call WITHOUT a workspace that the
    helper makes in front of the one under test (a forward whose statistics the backward takes)."""
    from onepose_plus_plus_amd._lib import OppError
    problems = []
    for label, given in (("half", lambda n: n // 2), ("empty", lambda n: 0)):
        bufs = ops.GuardedBuffers("zero", device, ws_given=given)
        try:
            run(bufs)
            problems.append("%s workspace: accepted (return codes %s)" % (label, bufs.rcs))
        except OppError as e:
            if bufs.rcs[-1] != ERR_WORKSPACE:
                problems.append("%s workspace: refused with %d, not the workspace code %d (%s)" % (label, bufs.rcs[-1], ERR_WORKSPACE, e))
        bufs.sync()
        problems += ["%s workspace: %s" % (label, p) for p in bufs.check()]
        problems += ["%s workspace: %s changed although the call was refused" % (label, n) for n in bufs.touched() if n not in may_write]
    return problems


# ---- three fake stages in plain torch ------------------------------------------------------------------------------------------
def fake_input(n, seed=0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def fake_clean(bufs, n):
    """out = 2 x through a scratch copy in the workspace: writes before it reads, stays inside"""
    x = bufs.input(fake_input(n), "x")
    out = bufs.output(n, name="out")
    ws = bufs.workspace(4 * n + 64).view(torch.float32)
    ws[:n] = x
    out.copy_(ws[:n] * 2)
    return {"out": out.cpu()}


def fake_read_before_write(bufs, n):
    """out = 2 x + 0 * ws[:n]: reads workspace words nothing in the call wrote"""
    x = bufs.input(fake_input(n), "x")
    out = bufs.output(n, name="out")
    ws = bufs.workspace(4 * n + 64).view(torch.float32)
    out.copy_(x * 2 + 0 * ws[:n])
    return {"out": out.cpu()}


def fake_overrun(bufs, n):
    """out = 2 x, and one element more: the store past the end lands in the allocation the output is a view of"""
    x = bufs.input(fake_input(n), "x")
    out = bufs.output(n, name="out")
    bufs.workspace(4 * n + 64)
    out.copy_(x * 2)
    out.as_strided((n + 1,), (1,), out.storage_offset())[n] = 1.0
    return {"out": out.cpu()}


FAKE_STAGES = {"clean": fake_clean, "read_before_write": fake_read_before_write, "overrun": fake_overrun}
