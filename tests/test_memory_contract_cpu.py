"""The buffer provider of tests/hip_ops.py and the harness of tests/memory_contract.py on CPU tensors ("The workspace
contract"): the canary sees one byte on either side of a view, a clean run is reported clean, the `leftover` fill hands a smaller call
the bytes of the larger one, the workspace view has the requested length and alignment -- and the three fake stages are classified as
clean, read-before-write and out-of-bounds, which is what shows that the GPU file (tests/test_memory_contract_gpu.py, which runs the
same fake stages on the device) bites without a mutated kernel."""
import pytest
import torch

from tests import hip_ops as ops
from tests import memory_contract as MC


def _raw_of(bufs, name):
    for rec in bufs._records:
        if rec[0] == name:
            return rec[2], rec[3], rec[4]
    raise KeyError(name)


@pytest.mark.parametrize("kind", ["workspace", "output", "input"])
@pytest.mark.parametrize("where", ["front", "behind"])
def test_canary_sees_one_byte(kind, where):
    bufs = ops.GuardedBuffers("zero", "cpu")
    if kind == "workspace":
        bufs.workspace(1000, "buf")
    elif kind == "output":
        bufs.output((7, 3), name="buf")
    else:
        bufs.input(torch.arange(21, dtype=torch.int64), "buf")
    bufs.output(5, name="other")
    assert bufs.check() == []
    raw, off, nbytes = _raw_of(bufs, "buf")
    raw[off - 1 if where == "front" else off + nbytes] ^= 0xFF
    got = bufs.check()
    assert got == ["buf: written %s the buffer" % ("in front of" if where == "front" else "behind")], got


def test_far_ends_of_the_guard_bands_count():
    bufs = ops.GuardedBuffers("nan", "cpu")
    bufs.workspace(512, "ws")
    raw, off, nbytes = _raw_of(bufs, "ws")
    assert off >= ops.GUARD_BYTES and raw.numel() - off - nbytes >= ops.GUARD_BYTES
    raw[0] = 0
    assert bufs.check() == ["ws: written in front of the buffer"]
    raw[0] = ops.CANARY
    raw[off + nbytes + ops.GUARD_BYTES - 1] = 0
    assert bufs.check() == ["ws: written behind the buffer"]


def test_input_changes_are_reported_and_output_changes_are_not():
    bufs = ops.GuardedBuffers("zero", "cpu")
    x = bufs.input(torch.ones(9), "x")
    out = bufs.output(9, name="out")
    out.fill_(3.0)
    assert bufs.check() == [] and bufs.touched() == ["out"]
    x[4] = -0.0 * x[4] + 1.0          # same value, same bits
    assert bufs.check() == []
    x[4] = 2.0
    assert bufs.check() == ["x: read-only input changed"]


@pytest.mark.parametrize("nbytes", [1, 255, 256, 1000, 4096, 70001])
@pytest.mark.parametrize("fill", ops.WS_FILLS)
def test_workspace_view_length_alignment_and_fill(fill, nbytes):
    bufs = ops.GuardedBuffers(fill, "cpu")
    ws = bufs.workspace(nbytes)
    assert ws.dtype == torch.uint8 and ws.numel() == nbytes and ws.is_contiguous()
    assert ws.data_ptr() % ops.GUARD_ALIGN == 0
    assert bufs.ws_bytes(ws) == nbytes
    words = ws[:nbytes // 4 * 4].view(torch.int32)
    if fill == "nan":
        assert bool((words == ops.NAN_WORD).all())
        assert nbytes < 4 or bool(torch.isnan(ws[:nbytes // 4 * 4].view(torch.float32)).all())
    else:
        assert bool((ws == 0).all())
    assert bufs.check() == []
    out = bufs.output((3, 5), torch.float64, name="o")
    assert out.data_ptr() % ops.GUARD_ALIGN == 0 and bool(torch.isnan(out).all())


def test_leftover_carries_the_larger_runs_bytes():
    bufs = ops.GuardedBuffers("leftover", "cpu")
    big = bufs.workspace(3000)
    big.copy_(torch.arange(3000) % 251)
    assert bufs.check() == []
    bufs.new_call()
    small = bufs.workspace(1000)
    assert small.numel() == 1000 and small.data_ptr() == big.data_ptr()
    assert torch.equal(small, (torch.arange(1000) % 251).to(torch.uint8))
    assert bufs.check() == []
    # the band behind the smaller view is live: the bytes the larger run left there no longer count as the call's to write
    big[1000] ^= 0xFF
    assert bufs.check() == ["ws: written behind the buffer"]
    with pytest.raises(AssertionError):
        bufs.new_call()
        bufs.workspace(3001)


def test_declared_size_of_a_refusal_run():
    bufs = ops.GuardedBuffers("zero", "cpu", ws_given=lambda n: n // 2)
    ws = bufs.workspace(1000)
    assert ws.numel() == 1000 and bufs.ws_bytes(ws) == 500
    assert bufs.touched() == []
    ws[999] = 1
    assert bufs.touched() == ["ws"]


def test_default_provider_is_the_plain_allocation():
    bufs = ops.Buffers("cpu")
    ws = bufs.workspace(100)
    assert ws.numel() == 100 and ws.dtype == torch.uint8 and bufs.ws_bytes(ws) == 100
    out = bufs.output((2, 3), name="o")
    assert out.shape == (2, 3) and bool(torch.isnan(out).all())
    assert bufs.output(4, torch.int64, None).dtype == torch.int64 and int(bufs.output(1, torch.int32, 0)[0]) == 0
    t = torch.arange(6.0).view(2, 3).t()
    assert bufs.input(t).is_contiguous() and torch.equal(bufs.input(t), t)
    x = torch.ones(3)
    y = bufs.inout(x)
    y += 1
    assert float(x[0]) == 1.0 and bufs.check() == []


# ---- the harness on the three fake stages (the GPU file runs the same three on the device) ------------------------------------
def check_fake_stages(device):
    n, big = 77, 300
    got = {name: MC.fill_problems(lambda b: f(b, n), lambda b: f(b, big), device) for name, f in MC.FAKE_STAGES.items()}
    assert got["clean"] == [], got["clean"]
    rbw = got["read_before_write"]
    assert rbw and all(p.startswith("nan: output out differs") for p in rbw), rbw
    assert "(%d of them NaN)" % n in rbw[0], rbw
    ovr = got["overrun"]
    assert ovr and all("out: written behind the buffer" in p for p in ovr), ovr
    assert {p.split(":")[0] for p in ovr} >= {"zero", "nan", "leftover"}, ovr
    return got


def test_fake_stages_are_classified():
    check_fake_stages("cpu")


def test_read_before_write_hides_behind_matching_leftovers():
    """what the caching allocator does to the suite: a stage that reads a word it never wrote passes when the run before left the right
    value there (here: zeros from the larger run), and only the poison finds it"""
    f = MC.FAKE_STAGES["read_before_write"]
    for fill, found in (("zero", False), ("leftover", False), ("nan", True)):
        bufs = ops.GuardedBuffers(fill, "cpu")
        if fill == "leftover":
            f(bufs, 300)
            bufs.new_call()
        out = f(bufs, 77)["out"]
        assert bool(torch.isnan(out).any()) == found, fill


def test_close_bar_for_an_order_dependent_output():
    want = torch.tensor([1.0, 2.0])
    assert MC._differs("g", want + 5e-6, want, {"g": 1e-5}) is None
    assert "1.0e-05" in MC._differs("g", want + 2e-5, want, {"g": 1e-5})
    assert MC._differs("g", torch.tensor([1.0, -0.0]), torch.tensor([1.0, 0.0]), {}) is not None      # signed zeros count
