"""CPU: the pure logic of the batched LO-RANSAC (csrc/pnp_lo_batch.h) built for the host with g++ -- the per-sample mode, the
trials of the first pass, the workspace layout --, the ctypes declarations of the two new entry points, and the stop indices
the float64 restatement (tests/loransac_reference.py) gives for the batch of tests/test_loransac_batch_gpu.py.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import loransac_batch_cases as BC
from tests import loransac_cases as C
from tests import loransac_reference as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAIL, RUN = 0, 1
ARRAYS = ("hyp", "nmod", "cnt", "sum", "cand_idx", "cand_rc", "cand_rs", "cand_lc", "cand_ls", "cand_pose", "cand_taken", "ctl", "lo_pts",
          "fin_pts")
STRIDES = ("pose_stride", "i1_stride", "i4_stride", "d4_stride", "ctl_stride")
# array -> (its stride, the bytes a sample needs per trial): LoBuffers of csrc/pnp_lo_body.h
SLABS = {"hyp": ("pose_stride", 384), "nmod": ("i1_stride", 4), "cnt": ("i4_stride", 16), "sum": ("d4_stride", 32),
         "cand_idx": ("i4_stride", 16), "cand_rc": ("i4_stride", 16), "cand_rs": ("d4_stride", 32), "cand_lc": ("i4_stride", 16),
         "cand_ls": ("d4_stride", 32), "cand_pose": ("pose_stride", 384), "cand_taken": ("i4_stride", 16)}
LO_ROW, FIN_ROW = 32 * 13 * 8, 21 * 8          # bytes per match: OPP_LO_GRID workgroups of 13 doubles; X, uv and a 16-double LM row


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("loransac_batch") / "libloransac_batch_host.so")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "loransac_batch_host.cpp")])
    L = ctypes.CDLL(out)
    L.t_lo_mode.restype = ctypes.c_int
    L.t_lo_first_pass.restype = ctypes.c_int
    L.t_lo_layout.restype = None
    L.t_lo_point_regions.restype = None
    return L


def test_mode_is_the_host_decision_of_the_single_call(lib):
    # opp_pnp_loransac (csrc/pnp_lo.hip) asks it too: FAIL launches the final kernel in mode 2 alone
    assert [lib.t_lo_mode(n) for n in range(6)] == [FAIL, FAIL, FAIL, RUN, RUN, RUN]
    assert lib.t_lo_mode(100000) == RUN and lib.t_lo_mode(2 ** 31 - 1) == RUN


def test_first_pass_trials(lib):
    # t1 = min(max(min_trials, 1), iterations)
    for min_trials, iterations, want in ((0, 1500, 1), (1, 1500, 1), (300, 1500, 300), (1000, 10000, 1000), (1499, 1500, 1499),
                                         (1500, 1500, 1500), (1000, 600, 600), (0, 1, 1), (5, 1, 1)):
        assert lib.t_lo_first_pass(min_trials, iterations) == want == min(max(min_trials, 1), iterations)


def _layout(lib, iterations, B, n_total):
    out = (ctypes.c_ulonglong * 21)()
    lib.t_lo_layout(iterations, B, n_total, out)
    v = [int(x) for x in out]
    L = dict(zip(ARRAYS + STRIDES + ("bytes", "returned"), v))
    assert L["bytes"] == L["returned"]
    return L


def _regions(lib, iterations, B, n_total, o0, o1):
    out = (ctypes.c_ulonglong * 4)()
    lib.t_lo_point_regions(iterations, B, n_total, o0, o1, out)
    return [int(x) for x in out]


def _disjoint(spans):
    spans = sorted(s for s in spans if s[1] > s[0])
    return all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


@pytest.mark.parametrize("iterations,offsets", [(1500, [0, 300, 300, 302, 305, 309, 314, 384, 514]),      # the GPU test's batch
                                                (10000, [0, 300, 600]), (1, [0, 7]), (37, [0, 0, 0, 5]), (600, [0, 0])])
def test_layout_of_ragged_batches(lib, iterations, offsets):
    B, n_total = len(offsets) - 1, offsets[-1]
    L = _layout(lib, iterations, B, n_total)
    spans = []
    for name, (stride, per_trial) in SLABS.items():
        assert L[name] % 256 == 0 and L[stride] % 256 == 0 and L[stride] >= per_trial * iterations
        spans += [(L[name] + b * L[stride], L[name] + b * L[stride] + per_trial * iterations) for b in range(B)]
    assert L["ctl"] % 256 == 0 and L["ctl_stride"] >= 8 and L["ctl_stride"] % 4 == 0
    spans += [(L["ctl"] + b * L["ctl_stride"], L["ctl"] + b * L["ctl_stride"] + 8) for b in range(B)]
    assert L["lo_pts"] % 256 == 0 and L["fin_pts"] % 256 == 0
    for b in range(B):
        lo0, lo1, f0, f1 = _regions(lib, iterations, B, n_total, offsets[b], offsets[b + 1])
        n = offsets[b + 1] - offsets[b]
        assert lo0 % 8 == 0 and f0 % 8 == 0
        assert (lo0, lo1) == (L["lo_pts"] + LO_ROW * offsets[b], L["lo_pts"] + LO_ROW * offsets[b + 1]) and lo1 - lo0 == LO_ROW * n
        assert (f0, f1) == (L["fin_pts"] + FIN_ROW * offsets[b], L["fin_pts"] + FIN_ROW * offsets[b + 1]) and f1 - f0 == FIN_ROW * n
        assert L["lo_pts"] <= lo0 <= lo1 <= L["fin_pts"] and L["fin_pts"] <= f0 <= f1 <= L["bytes"]
        spans += [(lo0, lo1), (f0, f1)]
    assert _disjoint(spans) and all(0 <= s[0] <= s[1] <= L["bytes"] for s in spans)
    # the size the issue states: 948 bytes per trial and sample, 3496 per match, plus alignment
    assert L["bytes"] >= 948 * iterations * B + (LO_ROW + FIN_ROW) * n_total and LO_ROW + FIN_ROW == 3496
    assert L["bytes"] <= 948 * iterations * B + 3496 * max(n_total, 1) + 256 * (11 * B + 3) + 64 * B


def test_layout_of_invalid_offsets_stays_inside(lib):
    L = _layout(lib, 100, 3, 9)
    for o0, o1 in ((5, 2), (-1, 3), (3, 10), (-7, -2), (2 ** 31 - 1, 2 ** 31 - 1), (-2 ** 31, 4)):
        lo0, lo1, f0, f1 = _regions(lib, 100, 3, 9, o0, o1)
        assert (lo0, lo1, f0, f1) == (L["lo_pts"], L["lo_pts"], L["fin_pts"], L["fin_pts"]), (o0, o1)     # an empty sample
    lo0, lo1, f0, f1 = _regions(lib, 100, 3, 9, 0, 9)                                                     # the whole array
    assert lo1 <= L["fin_pts"] and f1 <= L["bytes"]
    assert _layout(lib, 0, 0, 0) == _layout(lib, 1, 1, 1)                                                  # never a zero-sized workspace


@pytest.mark.parametrize("iterations", [1, 63, 64, 2000, 10000])
@pytest.mark.parametrize("n", [0, 1, 4, 5, 6, 300])
def test_single_call_workspace_is_the_batch_layout_of_one_sample(lib, iterations, n):
    # opp_pnp_loransac_workspace_bytes as pnp_lo.hip wrote it out before it used the layout: fourteen 256-aligned blocks
    I, nn = max(iterations, 1), max(n, 1)
    blocks = [I * 48 * 8, I * 4, I * 16, I * 32, I * 16, I * 16, I * 32, I * 16, I * 32, I * 48 * 8, I * 16, 64, 32 * 13 * nn * 8, 21 * nn * 8]
    L = _layout(lib, iterations, 1, n)
    assert L["bytes"] == sum((x + 255) // 256 * 256 for x in blocks)
    off = 0
    for name, x in zip(ARRAYS, blocks):                     # and in the same order
        assert L[name] == off, name
        off += (x + 255) // 256 * 256


def test_workspace_grows_with_every_argument(lib):
    base = _layout(lib, 1000, 4, 500)["bytes"]
    assert _layout(lib, 1001, 4, 500)["bytes"] >= base and _layout(lib, 2000, 4, 500)["bytes"] > base
    assert _layout(lib, 1000, 5, 500)["bytes"] > base and _layout(lib, 1000, 4, 600)["bytes"] > base


_CTYPE = {"int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t, "unsigned": ctypes.c_uint}


def _header_prototypes():
    src = open(os.path.join(ROOT, "include", "opp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(size_t|int)\s+(opp_pnp_loransac_batch[a-z_]*)\s*\(([^)]*)\)\s*;", src):
        types = []
        for a in args.split(","):
            a = a.strip()
            types.append(ctypes.c_void_p if "*" in a else _CTYPE[a.split()[0]])
        out[name] = (_CTYPE[ret], types)
    return out


def test_ctypes_table_declares_the_batch_entry_points():
    from onepose_plus_plus_amd import _lib
    protos = _header_prototypes()
    assert sorted(protos) == ["opp_pnp_loransac_batch", "opp_pnp_loransac_batch_workspace_bytes"]
    assert len(protos["opp_pnp_loransac_batch"][1]) == 20 and len(protos["opp_pnp_loransac_batch_workspace_bytes"][1]) == 3
    for name, (restype, argtypes) in protos.items():
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is restype, name
        assert list(got_args) == argtypes, name


def test_python_entry_points():
    from onepose_plus_plus_amd import pose
    assert callable(pose.loransac_PnP_batch)
    K = np.array([[560.0, 0, 256.0], [0, 560.0, 250.0], [0, 0, 1]])[None]
    for kw in (dict(solver="loransac"), dict(solver="auto", use_pycolmap_ransac=True)):       # before anything touches a GPU
        with pytest.raises(NotImplementedError, match="ransac_PnP"):
            pose.ransac_PnP_batch(K, np.zeros((8, 2)), np.zeros((8, 3)), offsets=[0, 8], **kw)
    with pytest.raises(ValueError):
        pose.loransac_PnP_batch(K, np.zeros((8, 2)), np.zeros((8, 3)))                         # neither m_bids nor offsets
    with pytest.raises(ValueError):
        pose.loransac_PnP_batch(K, np.zeros((8, 2)), np.zeros((8, 3)), m_bids=np.zeros(8, np.int64), offsets=[0, 8])


def test_two_pass_setting_reaches_both_second_pass_branches(tmp_path):
    """iterations 1500, min_trials 300 on the batch of the GPU test, by the restatement with host-built P3P models: the
    70 %-outlier sample's loop runs past the first pass's 300 trials (3 log(1e-4) / log(1 - 0.3^3) is about 1010), so the second
    pass scores trials for it; the clean 130-match sample stops at 300, so its second candidates / LO stage is skipped"""
    out = str(tmp_path / "libloransac_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "loransac_host.cpp")])
    host = ctypes.CDLL(out)
    dp = ctypes.POINTER(ctypes.c_double)
    host.t_p3p.argtypes = [dp, dp, dp, dp]
    K, uvs, Xs, _ = BC.make_batch()
    kw = BC.SETTINGS["two_pass"]
    stops = {}
    for b in (0, 7):
        uv64, X64 = C.f64(uvs[b], Xs[b])
        K4 = np.array([K[b, 0, 0], K[b, 0, 0], K[b, 0, 2], K[b, 1, 2]])
        models, counts, sums = C.host_trials(host, LR, X64, uv64, K4, BC.THR, BC.SEEDS[b], kw["iterations"])
        r = LR.lo_ransac(models, counts, sums, X64, uv64, K4, BC.THR, confidence=0.9999, min_trials=kw["min_trials"], cap=kw["iterations"])
        assert r["state"]
        stops[b] = r["stop"]
    assert kw["min_trials"] + 100 < stops[0] < kw["iterations"], stops      # far from both ends: no rounding can move it across
    assert stops[7] == kw["min_trials"], stops
