"""CPU: the pure logic of the batched PnP-RANSAC (csrc/pnp_batch.h) built for the host with g++ -- the sample boundaries
from the matcher's batch ids and the per-sample mode table -- and the ctypes declarations of the three new entry points.
No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAIL, P3P_RANSAC, EPNP_ONE, EPNP_RANSAC = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pnp_batch") / "libpnp_batch_host.so")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "pnp_batch_host.cpp")])
    L = ctypes.CDLL(out)
    L.t_offsets.restype = None
    L.t_mode.restype = ctypes.c_int
    L.t_extent.restype = None
    return L


def _offsets(lib, ids, B):
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    off = np.full(B + 1, -99, np.int32)
    bad = ctypes.c_int(-1)
    lib.t_offsets(ids.ctypes.data_as(ctypes.c_void_p), int(ids.size), B, off.ctypes.data_as(ctypes.c_void_p), ctypes.byref(bad))
    return off, bad.value


@pytest.mark.parametrize("ids,B", [
    ([0, 0, 0, 1, 1, 2], 3),                 # every sample filled
    ([1, 1, 2, 2, 2], 3),                    # empty first sample
    ([0, 0, 2, 2, 2], 3),                    # empty middle sample
    ([0, 1, 1], 3),                          # empty last sample
    ([3, 3], 6),                             # several empty samples at both ends
    ([0, 3, 3, 5], 7),                       # empty ones in between and at the end
    ([0, 0, 0, 0], 1),                       # B = 1
    ([], 1),                                 # n_total = 0
    ([], 4),
    ([0], 1),
])
def test_offsets_match_searchsorted(lib, ids, B):
    off, bad = _offsets(lib, ids, B)
    ref = np.searchsorted(np.asarray(ids, dtype=np.int64), np.arange(B + 1), side="left")
    assert bad == 0
    assert np.array_equal(off, ref)
    assert off[0] == 0 and off[B] == len(ids) and (np.diff(off) >= 0).all()
    assert np.array_equal(np.diff(off), np.bincount(np.asarray(ids, dtype=np.int64), minlength=B))


def test_offsets_on_a_long_run(lib):
    rng = np.random.default_rng(0)
    ids = np.sort(rng.integers(0, 37, size=5000))
    ids = ids[(ids != 0) & (ids != 11) & (ids != 36)]
    off, bad = _offsets(lib, ids, 37)
    assert bad == 0 and np.array_equal(off, np.searchsorted(ids, np.arange(38), side="left"))


@pytest.mark.parametrize("ids,B", [
    ([0, 1, 0], 2),                          # a decreasing pair
    ([0, 0, 2, 1, 2], 3),
    ([0, 1, 2], 2),                          # an id == B
    ([-1, 0, 1], 2),                         # a negative id
    ([5], 1),
])
def test_bad_ids_are_flagged(lib, ids, B):
    off, bad = _offsets(lib, ids, B)
    assert bad == 1
    assert ((off >= 0) & (off <= len(ids))).all()          # whatever they are, they stay inside the array


def test_extent_of_unvalidated_offsets(lib):
    first, n = ctypes.c_int(), ctypes.c_int()
    for o0, o1, nt, want in ((2, 5, 9, (2, 3)), (5, 5, 9, (5, 0)), (0, 9, 9, (0, 9)), (5, 2, 9, (0, 0)), (-1, 3, 9, (0, 0)),
                             (3, 10, 9, (0, 0)), (0, 0, 0, (0, 0))):
        lib.t_extent(o0, o1, nt, ctypes.byref(first), ctypes.byref(n))
        assert (first.value, n.value) == want, (o0, o1, nt)


def _host_decisions(solver, n):
    """what opp_pnp_ransac_ex decided on the host from n_points before it read opp_pnp_mode, restated: (mode, m)"""
    sample = n >= 4 if solver == 0 else (n == 4 or n >= 6)
    if solver == 0:
        return (P3P_RANSAC if sample else FAIL), 4          # pnp_stop_kernel(..., 4, ...) / prm.iters = 0
    final_mode = 3 if n < 4 else (0 if n == 4 else (2 if n == 5 else 1))
    m = 4 if n == 4 else 5
    mode = {3: FAIL, 0: P3P_RANSAC, 2: EPNP_ONE, 1: EPNP_RANSAC}[final_mode]
    assert sample == (mode in (P3P_RANSAC, EPNP_RANSAC))
    return mode, m


@pytest.mark.parametrize("solver", [0, 1])
def test_mode_table(lib, solver):
    m = ctypes.c_int()
    for n in range(8):
        mode = lib.t_mode(solver, n, ctypes.byref(m))
        assert (mode, m.value) == _host_decisions(solver, n), (solver, n)
    # the table of the issue, written out
    want = {0: [FAIL] * 4 + [P3P_RANSAC] * 4, 1: [FAIL] * 4 + [P3P_RANSAC, EPNP_ONE, EPNP_RANSAC, EPNP_RANSAC]}[solver]
    assert [lib.t_mode(solver, n, ctypes.byref(m)) for n in range(8)] == want
    assert lib.t_mode(1, 4, ctypes.byref(m)) == P3P_RANSAC and m.value == 4
    assert lib.t_mode(1, 6, ctypes.byref(m)) == EPNP_RANSAC and m.value == 5
    assert lib.t_mode(solver, 100000, ctypes.byref(m)) == (P3P_RANSAC if solver == 0 else EPNP_RANSAC)


@pytest.mark.parametrize("solver", [0, 1])
def test_final_stage_mode(lib, solver):
    # pnp_epnp_final_body's mode as the host and the batched kernel derived it before they shared opp_pnp_final_mode
    lib.t_final_mode.restype = ctypes.c_int
    for n in (0, 3, 4, 5, 6, 7):
        want = 3 if n < 4 else (0 if n == 4 else (2 if n == 5 else 1))
        if solver == 0 and n >= 4:
            want = 0                                        # P3P hypotheses whatever n is (solver 0 never reaches that stage)
        assert lib.t_final_mode(solver, n) == want, (solver, n)


LAYOUT = ("hyp", "valid", "score", "score2", "pts", "hyp_stride", "int_stride", "bytes", "returned")


def _pnp_layout(lib, iterations, B, n_total):
    out = (ctypes.c_ulonglong * 9)()
    lib.t_pnp_layout.restype = None
    lib.t_pnp_layout(iterations, B, n_total, out)
    L = dict(zip(LAYOUT, (int(x) for x in out)))
    assert L["bytes"] == L["returned"]
    return L


def _align(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("iterations", [1, 63, 64, 2000, 10000])
@pytest.mark.parametrize("n", [0, 1, 4, 5, 6, 300])
def test_workspace_layout(lib, iterations, n):
    L = _pnp_layout(lib, iterations, 1, n)
    I, nn = max(iterations, 1), max(n, 1)
    # opp_pnp_ex_workspace_bytes and opp_pnp_workspace_bytes as they were written out before the layout
    assert L["bytes"] == _align(I * 96) + 3 * _align(I * 4) + _align(nn * 104) + 1024
    assert L["score2"] + 1024 == _align(I * 96) + 2 * _align(I * 4) + 1024
    assert _pnp_layout(lib, 0, 0, 0) == _pnp_layout(lib, 1, 1, 1)
    for B in (1, 3):
        L = _pnp_layout(lib, iterations, B, n)
        spans = []
        for name, stride, per_trial in (("hyp", "hyp_stride", 96), ("valid", "int_stride", 4), ("score", "int_stride", 4),
                                        ("score2", "int_stride", 4)):
            assert L[name] % 256 == 0 and L[stride] % 256 == 0 and L[stride] >= per_trial * iterations
            spans += [(L[name] + b * L[stride], L[name] + b * L[stride] + per_trial * iterations) for b in range(B)]
        assert L["pts"] % 256 == 0
        spans.append((L["pts"], L["pts"] + 104 * n))
        spans.sort()
        assert spans[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= L["bytes"]
        assert L["bytes"] == B * (_align(I * 96) + 3 * _align(I * 4)) + _align(nn * 104) + 1024       # opp_pnp_batch_workspace_bytes


def test_library_workspace_sizes_are_the_closed_forms():
    """the exported size functions themselves (they run on the host), at the sizes above and at the clamps"""
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    for I in (0, 1, 63, 64, 2000, 10000):
        assert lib.opp_pnp_workspace_bytes(I) == _align(I * 96) + 2 * _align(I * 4) + 1024           # this one never clamped
        for n in (0, 1, 4, 5, 6, 300):
            Ic, nc = max(I, 1), max(n, 1)
            slabs = _align(Ic * 96) + 3 * _align(Ic * 4)
            assert lib.opp_pnp_ex_workspace_bytes(I, n) == slabs + _align(nc * 104) + 1024
            for B in (0, 1, 3):
                assert lib.opp_pnp_batch_workspace_bytes(I, B, n) == max(B, 1) * slabs + _align(nc * 104) + 1024
            assert lib.opp_pnp_loransac_workspace_bytes(I, n) == lib.opp_pnp_loransac_batch_workspace_bytes(I, 1, n)


def _header_arg_counts():
    src = open(os.path.join(ROOT, "include", "opp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(opp_pnp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        out[name] = 0 if args.strip() in ("", "void") else args.count(",") + 1
    return out


def test_ctypes_table_declares_the_batch_entry_points():
    from onepose_plus_plus_amd import _lib
    counts = _header_arg_counts()
    for name, n_args in (("opp_pnp_batch_workspace_bytes", 3), ("opp_pnp_offsets", 6), ("opp_pnp_ransac_batch", 21)):
        assert counts.get(name) == n_args, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == n_args, name
    assert _lib.SIGNATURES["opp_pnp_batch_workspace_bytes"][0] is ctypes.c_size_t
    assert _lib.SIGNATURES["opp_pnp_offsets"][0] is ctypes.c_int and _lib.SIGNATURES["opp_pnp_ransac_batch"][0] is ctypes.c_int
