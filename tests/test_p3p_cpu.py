"""CPU: the float64 restatement of the default P3P PnP-RANSAC (tests/p3p_reference.py) against the host build of the device's
math (csrc/pnp_math.h through tests/pnp_host.cpp, g++) on every hypothesis of every case of tests/p3p_cases.py, and the conditions
under which those cases were chosen: few undecided decisions, the special cases' properties, the bar on a hypothesis pose.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import p3p_cases as C
from tests import p3p_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("p3p") / "libpnp_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "pnp_host.cpp")])
    L = ctypes.CDLL(out)
    L.t_hypothesis.restype = ctypes.c_int
    L.t_hypothesis.argtypes = [DP, DP, DP, IP, ctypes.c_double, DP]
    L.t_score.restype = ctypes.c_int
    L.t_score.argtypes = [DP, DP, DP, DP, ctypes.c_int, ctypes.c_double, IP]
    L.t_refine_inliers.restype = ctypes.c_int
    L.t_refine_inliers.argtypes = [DP, DP, DP, DP, ctypes.c_int, ctypes.c_double, ctypes.c_int, IP]
    return L


def _dp(a):
    return a.ctypes.data_as(DP)


def _close(a, ref):
    return np.abs(a - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())


def _flat(pose):
    return np.concatenate([pose[:, :3].reshape(-1), pose[:, 3]])


def _unflat(p):
    return np.concatenate([p[:9].reshape(3, 3), p[9:, None]], 1)


@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_restatement_agrees_with_the_host_build(lib, case):
    """validity and score of every hypothesis, its pose within HYP_POSE_TOL, and the refinement (pose within 1e-9, final mask) from
    the selected hypothesis and from every 25th valid one"""
    K, uv, X, planted, uv64, X64, K4, out = C.reference(case)
    Xc, uvc = np.ascontiguousarray(X64), np.ascontiguousarray(uv64)
    worst_h = worst_r = 0.0
    valid = [h for h in range(case.iterations) if out["poses"][h] is not None]
    refined = set(valid[::25]) | ({out["best"]} if out["best"] >= 0 else set())
    for h in range(case.iterations):
        idx = np.array(out["samples"][h], dtype=np.int32)
        buf = np.zeros(12)
        ok = lib.t_hypothesis(_dp(Xc), _dp(uvc), _dp(K4), idx.ctypes.data_as(IP), C.THR2, _dp(buf))
        ref = out["poses"][h]
        assert bool(ok) == (ref is not None), (h, out["undecided"][h])
        if ref is None:
            continue
        assert lib.t_score(_dp(buf), _dp(K4), _dp(Xc), _dp(uvc), case.n, C.THR2, None) == out["scores"][h], h
        d = C.pose_distance(PR.out_pose(_unflat(buf), case.scale), PR.out_pose(ref, case.scale))
        if not out["undecided"][h]:
            worst_h = max(worst_h, d)
            assert d <= C.HYP_POSE_TOL, (h, d)
        if h in refined:
            margins = []
            want, want_mask = PR.refine(ref, X64, uv64, K4, C.THR2, case.refine_iters, case.scale, margins)
            got, mask = _flat(ref), np.zeros(case.n, dtype=np.int32)
            cnt = lib.t_refine_inliers(_dp(got), _dp(K4), _dp(Xc), _dp(uvc), case.n, C.THR2, case.refine_iters, mask.ctypes.data_as(IP))
            if any(m < C.MARGIN for _, m in margins):
                assert h != out["best"]
                continue                                   # an inlier on the threshold: the two may refine on different sets
            got = PR.out_pose(_unflat(got), case.scale)
            assert _close(got, want), (h, np.abs(got - want).max())
            assert cnt == want_mask.sum() and np.array_equal(mask.astype(bool), want_mask), h
            worst_r = max(worst_r, C.pose_distance(got, want))
    print("%s: %d hypotheses, %d valid; largest host-vs-restatement distance: hypothesis pose %.3g, refined pose %.3g (%d refined)"
          % (case.name, case.iterations, len(valid), worst_h, worst_r, len(refined)))


@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_few_decisions_are_undecided(case):
    """the condition the seeds were searched for, on the restatement alone"""
    out = C.reference(case)[-1]
    hyps, points, selected = C.undecided_shares(case, out)
    print("%s: undecided hypotheses %d of %d (%.2f %%), undecided scoring decisions %d of %d (%.3f %%)"
          % (case.name, int(np.sum(out["undecided"])), case.iterations, 100 * hyps, int(np.sum(out["point_undecided"])),
             case.iterations * case.n, 100 * points))
    assert hyps <= 0.01 and points <= 0.01
    assert not selected


def test_special_cases_have_their_properties():
    tie, stop, few, none = (C.BY_NAME[k] for k in ("tie", "stop", "few", "none"))
    out = C.reference(tie)[-1]
    t = C.tied(out)
    assert tie.n == 12 and tie.refine_iters == 0 and len(t) >= 2 and out["best"] == t[0]
    d = C.pose_distance(PR.out_pose(out["poses"][t[0]], tie.scale), PR.out_pose(out["poses"][t[1]], tie.scale))
    assert d > 1e-3
    assert C.pose_distance(PR.out_pose(out["poses"][t[0]], tie.scale), PR.out_pose(out["poses"][t[-1]], tie.scale)) > 1e-3
    print("tie: %d hypotheses share the score %d; the first two, %d and %d, are %.3g apart" % (len(t), out["scores"][t[0]], t[0], t[1], d))
    out = C.reference(stop)[-1]
    sc, s = out["scores"], out["stop"]
    assert stop.confidence == 0.99 and s < stop.iterations and sc[s:].max() > sc[:s].max()
    assert PR.select(sc) >= s and PR.select(sc) != out["best"]
    print("stop: stop index %d of %d, best score %d before it (hypothesis %d) and %d after it (hypothesis %d)"
          % (s, stop.iterations, sc[:s].max(), out["best"], sc[s:].max(), PR.select(sc)))
    K, uv, X, planted, uv64, X64, K4, out = C.reference(few)
    assert few.n == 50 and few.outliers == 1.0 and out["state"] and 0 <= out["scores"].max() < 4 and few.refine_iters > 0
    assert np.array_equal(out["pose"], PR.out_pose(out["poses"][out["best"]], few.scale))        # unrefined
    out = C.reference(none)[-1]
    assert (out["scores"] == -1).all() and not out["state"] and out["best"] == -1
    assert np.array_equal(out["pose"], np.eye(4)[:3]) and not out["inliers"].any()
    for name in ("n65_behind", "n700_behind"):                   # the planted matches: perfect pixels, behind the camera
        K, uv, X, planted, uv64, X64, K4, out = C.reference(C.BY_NAME[name])
        assert len(planted) >= 5 and not out["inliers"][planted].any()
        e, z = PR.residuals(np.concatenate([out["pose"][:, :3], out["pose"][:, 3:] * C.BY_NAME[name].scale], 1), X64, uv64, K4)
        assert (z[planted] < 0).all() and np.isinf(e[planted]).all()


def test_the_cases_hold_hypotheses_only_the_validity_bar_rejects():
    """4th-match errors between 4 thr^2 and 8 thr^2, decided: a bar off by a factor of two changes their validity"""
    between = 0
    for case in C.CASES:
        K, uv, X, planted, uv64, X64, K4, out = C.reference(case)
        for h in range(case.iterations):
            if out["poses"][h] is None and not out["undecided"][h]:
                loose, m = PR.hypothesis(X64, uv64, K4, out["samples"][h], 2.0 * C.THR2)
                between += loose is not None and not PR.undecided(m)
    print("%d hypotheses have a 4th-match error in (4 thr^2, 8 thr^2]" % between)
    assert between >= 5


def test_the_cases_cover_the_shapes():
    assert {c.n for c in C.CASES} >= {4, 5, 12, 63, 64, 65, 257, 700}
    assert {c.iterations for c in C.CASES} >= {1, 3, 255, 257, 601}
    assert {c.scale for c in C.CASES} == {1, 1000} and {c.refine_iters for c in C.CASES} == {0, 1, 8}
    assert {c.confidence for c in C.CASES} == {1.0, 0.99}


def test_hypothesis_pose_bar():
    """HYP_POSE_TOL = 16 x the restatement's own float64 noise: every decided valid hypothesis evaluated a second time in long
    double with polished roots; the recorded noise must be the measured one (rounded up, by a quarter at most)"""
    assert np.finfo(np.longdouble).eps < 1e-18                    # the second evaluation needs the extended format
    noise, where, total = 0.0, None, 0
    per_scene = {}
    for case in C.CASES + C.single_cases():
        K, uv, X, planted, uv64, X64, K4, out = C.reference(case)
        worst = per_scene.get(case.name, 0.0)
        for h in range(case.iterations):
            if out["poses"][h] is None or out["undecided"][h]:
                continue
            second, _ = PR.hypothesis(X64, uv64, K4, out["samples"][h], C.THR2, precise=True)
            assert second is not None, (case.name, h)
            d = C.pose_distance(PR.out_pose(out["poses"][h], case.scale), PR.out_pose(second.astype(np.float64), case.scale))
            worst = max(worst, d)
            total += 1
            if d > noise:
                noise, where = d, (case.name, h)
        per_scene[case.name] = worst
    for name, worst in per_scene.items():
        print("%s: float64 noise of the restatement's hypothesis poses %.3g" % (name, worst))
    print("measured conditioning noise %.4g at %s over %d hypotheses; recorded %.4g; HYP_POSE_TOL = 16 x = %.4g"
          % (noise, where, total, C.HYP_POSE_NOISE, C.HYP_POSE_TOL))
    assert C.HYP_POSE_TOL == 16 * C.HYP_POSE_NOISE and C.HYP_POSE_TOL < 1e-6
    assert noise <= C.HYP_POSE_NOISE <= 1.25 * noise
