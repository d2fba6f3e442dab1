"""CPU: the deciding pieces of the LO-RANSAC estimator shared with the HIP kernels (csrc/pnp_math.h, built for the host with
g++: tests/loransac_host.cpp) against the float64 restatement (tests/loransac_reference.py): support order, the bound on the
trials, the sequential walk over candidate models, the Cauchy Levenberg-Marquardt refinement; the decision margins of the
replay cases of tests/test_loransac_gpu.py; dropin routing of pnp="loransac" / "auto".  No GPU."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import loransac_cases as C
from tests import loransac_reference as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K4 = np.array([560.0, 560.0, 256.0, 250.0])
dp = ctypes.POINTER(ctypes.c_double)
ip = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("loransac") / "libloransac_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "loransac_host.cpp")])
    L = ctypes.CDLL(out)
    L.t_lo_better.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_double]
    L.t_lo_dyn.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.t_lo_resolve.argtypes = [ip, ip, dp, ip, dp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, ip, ip]
    L.t_lm_refine.argtypes = [dp, dp, ctypes.c_int, dp, dp, dp]
    L.t_gn_refine.argtypes = [dp, dp, ctypes.c_int, dp, dp, ctypes.c_int]
    L.t_p3p.argtypes = [dp, dp, dp, dp]
    return L


def _p(a):
    return a.ctypes.data_as(dp)


def _flat(pose):
    return np.ascontiguousarray(np.concatenate([pose[:, :3].reshape(-1), pose[:, 3]]))


def _unflat(p):
    return np.concatenate([p[:9].reshape(3, 3), p[9:, None]], 1)


def _pose_err(pose, R, t):
    """rotation angle (radians, from the chord) + relative translation error"""
    return 2 * np.arcsin(min(1.0, np.linalg.norm(pose[:, :3] - R) / (2 * np.sqrt(2)))) + np.linalg.norm(pose[:, 3] - t) / np.linalg.norm(t)


def _lm_scene(rng, n, noise):
    """a simple-pinhole scene in metres and a start pose a little off the truth"""
    Ksp, uv, X, R, t, _ = C.sp_scene(rng, n, 0.0, noise)
    assert Ksp[0, 0] == K4[0] and Ksp[1, 1] == K4[1]
    start = np.concatenate([LR._rodrigues(rng.normal(size=3) * 0.004) @ R, (t + rng.normal(size=3) * 0.002)[:, None]], 1)
    return np.ascontiguousarray(X), np.ascontiguousarray(uv), R, t, start


def _host_lm(lib, X, uv, start):
    p, cost = _flat(start), np.zeros(1)
    iters = lib.t_lm_refine(_p(X), _p(uv), len(X), _p(K4), _p(p), _p(cost))
    return _unflat(p), iters, cost[0]


def test_support_order(lib):
    # more inliers wins whatever the sums; with as many, the smaller sum; equal supports are not better
    for a, b, want in (((5, 9.0), (4, 0.1), 1), ((4, 0.1), (5, 9.0), 0), ((5, 1.0), (5, 2.0), 1), ((5, 2.0), (5, 1.0), 0),
                       ((5, 2.0), (5, 2.0), 0), ((0, 0.0), (0, LR.NOSUM), 1), ((1, 3.0), (0, LR.NOSUM), 1)):
        assert lib.t_lo_better(a[0], a[1], b[0], b[1]) == want == int(LR.better(a, b))


def test_dyn_at_hand_checked_points(lib):
    assert lib.t_lo_dyn(0.9999, 100, 100, 10000) == 0 == LR.dyn_trials(0.9999, 100, 100, 10000)         # r = 1
    # r = 0.5: 3 ln(1e-4) / ln(0.875) = 3 * 9.21034 / 0.133531 = 206.9 -> 207
    assert lib.t_lo_dyn(0.9999, 50, 100, 10000) == 207 == LR.dyn_trials(0.9999, 50, 100, 10000)
    assert lib.t_lo_dyn(0.9999, 1, 10 ** 6, 10000) == 10000 == LR.dyn_trials(0.9999, 1, 10 ** 6, 10000)  # 1 - r^3 rounds to 1
    assert lib.t_lo_dyn(0.9999, 0, 100, 10000) == 10000 == LR.dyn_trials(0.9999, 0, 100, 10000)
    assert lib.t_lo_dyn(0.9999, 3, 100, 500) == 500 == LR.dyn_trials(0.9999, 3, 100, 500)                # above the cap
    assert lib.t_lo_dyn(1.0, 50, 100, 10000) == 10000 == LR.dyn_trials(1.0, 50, 100, 10000)              # confidence 1: never early
    rng = np.random.default_rng(2)
    for _ in range(500):
        n = int(rng.integers(3, 2000))
        cnt, cap, conf = int(rng.integers(0, n + 1)), int(rng.integers(1, 20000)), [0.9999, 0.99, 0.5, 1.0][int(rng.integers(0, 4))]
        assert lib.t_lo_dyn(conf, cnt, n, cap) == LR.dyn_trials(conf, cnt, n, cap)


def test_resolve_matches_restatement(lib):
    rng = np.random.default_rng(9)
    seen_drop = seen_end = 0
    for trial in range(300):
        n = int(rng.integers(6, 500))
        cap = int(rng.integers(1, 3000))
        min_trials = int(rng.integers(0, 1500))
        conf = [0.9999, 0.5, 0.99, 1.0][trial % 4]
        ncand = int(rng.integers(0, 30))
        idx = np.sort(rng.choice(cap * 4, size=min(ncand, cap * 4), replace=False)).astype(np.int32)
        ncand = len(idx)
        # raw supports: prefix records, as the candidate kernel lists them; LO supports at least as good
        rc = np.sort(rng.integers(0, n + 1, size=ncand)).astype(np.int32)
        rs = rng.uniform(0, 50, size=ncand)
        for c in range(1, ncand):
            if rc[c] == rc[c - 1]:
                rs[c] = rs[c - 1] * rng.uniform(0.1, 0.9)
        lc = np.array([int(rng.integers(c0, n + 1)) if rng.random() < 0.6 else c0 for c0 in rc], dtype=np.int32)
        ls = np.array([rs[c] * rng.uniform(0.1, 1.0) if lc[c] == rc[c] else rng.uniform(0, 50) for c in range(ncand)])
        best, taken = ctypes.c_int(0), np.full(max(ncand, 1), 7, dtype=np.int32)
        stop = lib.t_lo_resolve(idx.ctypes.data_as(ip), rc.ctypes.data_as(ip), _p(rs), lc.ctypes.data_as(ip), _p(ls), ncand, n, conf,
                                min_trials, cap, ctypes.byref(best), taken.ctypes.data_as(ip))
        ref_stop, ref_best, ref_taken = LR.resolve(idx, list(zip(rc.tolist(), rs.tolist())), list(zip(lc.tolist(), ls.tolist())), n, conf,
                                                   min_trials, cap)
        assert (stop, best.value, taken[:ncand].tolist()) == (ref_stop, ref_best, ref_taken)
        assert stop <= cap and (conf < 1.0 or stop == cap)
        seen_drop += int(0 in ref_taken[:max(ref_best, 0)])
        seen_end += int(ncand > 0 and (idx[-1] >> 2) >= stop)
    assert seen_drop > 20 and seen_end > 20      # candidates overtaken by an earlier LO, and candidates past the stop, both occur


@pytest.mark.parametrize("noise", [0.0, 0.5])
def test_lm_matches_restatement(lib, noise):
    rng = np.random.default_rng(17 + int(noise * 10))
    for n in (6, 40, 300):
        X, uv, R, t, start = _lm_scene(rng, n, noise)
        pose, iters, cost = _host_lm(lib, X, uv, start)
        m = []
        ref, ref_iters, cost0, ref_cost = LR.cauchy_lm(start, X, uv, K4, m)
        assert LR.smallest_margin(m) >= C.MARGIN
        assert iters == ref_iters and 1 <= iters < LR.LM_ITERS
        assert np.abs(pose - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), np.abs(pose - ref).max()
        assert abs(cost - ref_cost) <= 1e-9 * max(1.0, ref_cost) and cost <= cost0
        assert abs(cost - LR.robust_cost(pose, X, uv, K4)) <= 1e-9 * max(1.0, cost)
        err = _pose_err(pose, R, t)
        print("n=%d noise=%.1f: %d iterations, cost %.6g -> %.6g, pose error %.3g (start %.3g)" % (n, noise, iters, cost0, cost, err,
                                                                                                 _pose_err(start, R, t)))
        if noise == 0.0:
            # exact data: the minimum is the truth, and near it g = H delta for the 6-vector delta between the two.  The
            # refinement stops at |g|_inf <= 1, so |delta|_2 <= sqrt(6) / lambda_min(H); the error measure adds the angle
            # (<= |delta|) and |dt| / |t| (<= |delta| / |t|, dt also carries the rotation of t: a factor 2 covers it)
            H, _ = LR._normal_equations(np.concatenate([R, t[:, None]], 1), X, uv, K4)
            bound = 2.0 * (1.0 + 1.0 / np.linalg.norm(t)) * np.sqrt(6.0) * LR.LM_GTOL / np.linalg.eigvalsh(H)[0]
            assert err < bound, (err, bound)
        # with noise the minimiser of the robust cost is not the truth: the error is printed, the cost must not rise (above)


def test_lm_cauchy_beats_gauss_newton_on_displaced_inliers(lib):
    """10 % of the points displaced by 3-6 px (inside a 7 px RANSAC threshold, so they would be 'inliers'): the robust
    refinement must end closer to the truth than the unweighted Gauss-Newton of opp_gn_accumulate on the same points"""
    rng = np.random.default_rng(33)
    for trial in range(5):
        n = 200
        X, uv, R, t, start = _lm_scene(rng, n, 0.5)
        bad = rng.choice(n, n // 10, replace=False)
        ang = rng.uniform(0, 2 * np.pi, size=len(bad))
        uv[bad] += (rng.uniform(3.0, 6.0, size=len(bad)) * np.stack([np.cos(ang), np.sin(ang)]))[:, :].T
        pose, iters, cost = _host_lm(lib, X, uv, start)
        ref, ref_iters, _, _ = LR.cauchy_lm(start, X, uv, K4)
        assert iters == ref_iters and np.abs(pose - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
        g = _flat(start)
        lib.t_gn_refine(_p(X), _p(uv), n, _p(K4), _p(g), 8)
        e_lm, e_gn = _pose_err(pose, R, t), _pose_err(_unflat(g), R, t)
        print("trial %d: Cauchy LM %.3g, Gauss-Newton %.3g" % (trial, e_lm, e_gn))
        assert e_lm < e_gn, (e_lm, e_gn)


def test_lm_degenerate_inputs_stay_finite(lib):
    rng = np.random.default_rng(5)
    X, uv, R, t, start = _lm_scene(rng, 30, 0.5)
    for n in (0, 1, 2):                       # under-determined: the damping overflows or the gradient is small; no NaN
        pose, iters, cost = _host_lm(lib, X[:n].copy(), uv[:n].copy(), start)
        assert np.all(np.isfinite(pose)) and iters <= LR.LM_ITERS
    behind = start.copy()
    behind[2, 3] = -start[2, 3]               # every point behind the camera: zero weights, nothing to do
    pose, iters, cost = _host_lm(lib, X, uv, behind)
    assert np.array_equal(pose, behind) and iters == 0


@pytest.mark.parametrize("case", C.REPLAY_CASES)
def test_replay_cases_have_decision_margin(lib, case):
    """the scenes / seeds of test_loransac_gpu.py::test_loransac_matches_restatement, with host-built P3P models: every decision
    of the restatement (support comparisons, LM accept / reject, |g|_inf against 1) has a relative margin >= 1e-6"""
    n, outl, conf, iters, scene_seed, seed = case
    K, uv, X, R, t, _ = C.sp_scene(np.random.default_rng(scene_seed), n, outl, 0.5)
    uv64, X64 = C.f64(uv, X)
    trials = iters if conf >= 1.0 else 1100    # with confidence < 1 these scenes stop long before (asserted)
    models, counts, sums = C.host_trials(lib, LR, X64, uv64, K4, C.THR, seed, trials)
    m = []
    out = LR.estimate(models, counts, sums, X64, uv64, K4, C.THR, margins=m, confidence=conf, min_trials=1000, cap=iters if conf < 1.0 else trials)
    assert out["state"] and out["stop"] <= trials
    assert LR.smallest_margin(m) >= C.MARGIN, sorted(m, key=lambda x: x[1])[:3]
    # the walk over the candidate list with the LO supports gives what the literal loop gave
    cands = out["candidates"]
    raw = [(int(counts[c >> 2][c & 3]), float(sums[c >> 2][c & 3])) for c in cands]
    lo = [l if l is not None else r for l, r in zip(out["lo"], raw)]
    stop, b, taken = LR.resolve(cands, raw, lo, n, conf, 1000, iters if conf < 1.0 else trials)
    assert stop == out["stop"] and taken == out["taken"] and (cands[b] >> 2, cands[b] & 3) == out["best"]


def test_dropin_routes_loransac(monkeypatch):
    import onepose_plus_plus_amd.dropin as dropin
    from onepose_plus_plus_amd import pose
    saved = {k: v for k, v in sys.modules.items() if k == "src" or k.startswith("src.")}
    try:
        for k in saved:
            monkeypatch.delitem(sys.modules, k)
        for name in ("src", "src.utils"):
            m = types.ModuleType(name)
            m.__path__ = []
            monkeypatch.setitem(sys.modules, name, m)
        mu = types.ModuleType("src.utils.metric_utils")
        mu.ransac_PnP = None
        monkeypatch.setitem(sys.modules, "src.utils.metric_utils", mu)
        sys.modules["src.utils"].metric_utils = mu
        for name in ("loransac", "auto"):
            done = dropin.install(pnp=name, loss=False)
            assert done["src.utils.metric_utils"] == "ransac_PnP (%s)" % name
            f = mu.ransac_PnP
            assert f is not pose.ransac_PnP and f.func is pose.ransac_PnP and f.keywords == {"solver": name}
        dropin.install(pnp=True, loss=False)
        assert mu.ransac_PnP is pose.ransac_PnP
        with pytest.raises(ValueError):
            dropin.install(pnp="dls", loss=False)
    finally:
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_unknown_solver_raises():
    from onepose_plus_plus_amd.pose import ransac_PnP, ransac_PnP_ex
    K = np.array([[560.0, 0, 256.0], [0, 560.0, 250.0], [0, 0, 1]])
    with pytest.raises(ValueError):
        ransac_PnP(K, np.zeros((8, 2)), np.zeros((8, 3)), solver="nope")
    with pytest.raises(ValueError):
        ransac_PnP_ex(K, np.zeros((8, 2)), np.zeros((8, 3)), solver="auto")     # "auto" needs the flag: ransac_PnP only
