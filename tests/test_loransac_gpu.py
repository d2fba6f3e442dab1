"""GPU: LO-RANSAC with robust refinement (csrc/pnp_lo.hip through opp_pnp_loransac and pose.ransac_PnP(solver="loransac"), the
reference's pycolmap branch) on synthetic scenes: against ground truth, and against the float64 restatement
(tests/loransac_reference.py) replayed on the recorded models and supports of the same run."""
import ctypes

import numpy as np
import pytest
import torch

from tests import loransac_cases as C
from tests import loransac_reference as LR
from tests.test_pnp_gpu import _scene

pytestmark = pytest.mark.gpu
THR = C.THR
FAIL = (np.eye(4)[:3], np.eye(4))


def _errs(pose, R, t):
    """rotation angle (degrees, from the chord: exact near zero) and translation error (cm; the scenes are in metres)"""
    ang = np.rad2deg(2 * np.arcsin(min(1.0, np.linalg.norm(pose[:, :3] - R) / (2 * np.sqrt(2)))))
    return ang, np.linalg.norm(pose[:, 3] - t) * 100.0


def _K4(K, simple=True):
    return np.array([K[0, 0], K[0, 0] if simple else K[1, 1], K[0, 2], K[1, 2]])


def _ex(K, uv, X, **kw):
    from onepose_plus_plus_amd.pose import ransac_PnP_ex
    kw.setdefault("pnp_reprojection_error", THR)
    return ransac_PnP_ex(K, uv, X, solver="loransac", **kw)


def _replay(r, uv, X, K4, thr=THR, margins=None, **kw):
    """the restatement on the models and supports the device recorded"""
    uv64, X64 = C.f64(uv, X)
    m = r["models"]
    models = np.concatenate([m[..., :9].reshape(m.shape[0], 4, 3, 3), m[..., 9:, None]], -1)
    out = LR.estimate(models, r["counts"], r["sums"], X64, uv64, K4, thr, margins=margins, **kw)
    assert (r["samples"][:out["stop"]] >= 0).all()          # every trial the loop ran was drawn (and scored) on the device
    return out, uv64, X64


def _close(a, ref):
    return np.abs(a - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())


def _is_failure(res):
    pose, homo, inl, ok = res
    return (not ok) and np.array_equal(pose, FAIL[0]) and np.array_equal(homo, FAIL[1]) and inl.size == 0


@pytest.mark.parametrize("n,outliers,noise,planar", [(300, 0.0, 0.0, False), (1500, 0.5, 0.5, False), (200, 0.7, 1.0, False),
                                                      (500, 0.4, 0.5, True), (12, 0.25, 0.3, False)])
def test_loransac_recovers_pose(n, outliers, noise, planar):
    from onepose_plus_plus_amd.pose import ransac_PnP
    rng = np.random.default_rng(200 + n + int(outliers * 100))
    for trial in range(4):
        K, uv, X, R, t, out_idx = C.sp_scene(rng, n, outliers, noise, planar)
        pose, homo, inl, ok = ransac_PnP(K, uv, X, scale=1000.0, pnp_reprojection_error=THR, img_hw=[512, 512], use_pycolmap_ransac=True,
                                         seed=trial, solver="loransac")
        assert ok and pose.shape == (3, 4) and homo.shape == (4, 4) and inl.ndim == 2 and inl.shape[1] == 1
        assert np.array_equal(homo[:3], pose) and np.array_equal(homo[3], [0, 0, 0, 1])
        inl_set = set(inl[:, 0].tolist())
        true_in = set(range(n)) - set(out_idx.tolist())
        assert len(inl_set & true_in) >= 0.85 * len(true_in)
        assert len(inl_set - true_in) <= 0.05 * n + 2
        ang, tcm = _errs(pose, R, t)
        if noise == 0:
            assert ang < 1e-6 and tcm < 1e-6, (ang, tcm)
        # the same run, recorded, against the restatement of it
        r = _ex(K, uv, X, seed=trial, record=True)
        assert np.array_equal(r["pose"], pose) and np.array_equal(r["inliers"], inl[:, 0])
        out, _, _ = _replay(r, uv, X, _K4(K))
        assert out["state"] and r["stop"] == out["stop"]
        assert _close(r["pose"], out["pose_refined"]), np.abs(r["pose"] - out["pose_refined"]).max()
        print("n=%d outliers=%.2f noise=%.1f seed=%d: device %.3g deg %.3g cm, restatement %.3g deg %.3g cm, stop %d, %d LM iterations"
              % ((n, outliers, noise, trial, ang, tcm) + _errs(out["pose_refined"], R, t) + (r["stop"], r["lm_iters"])))


@pytest.mark.parametrize("case", C.REPLAY_CASES)
def test_loransac_matches_restatement(case):
    """candidate list, surviving candidates, stop index, best (trial, model), inlier set, LO supports, pose before and after the
    refinement -- all against the restatement replayed on the recorded per-model supports.  The scenes / seeds are those whose
    smallest decision margin is >= 1e-6 (tests/test_loransac_cpu.py checks that without a GPU; asserted again here)."""
    n, outl, conf, iters, scene_seed, seed = case
    K, uv, X, R, t, _ = C.sp_scene(np.random.default_rng(scene_seed), n, outl, 0.5)
    r = _ex(K, uv, X, iterations=iters, seed=seed, confidence=conf, record=True)
    K4, thr2, margins = _K4(K), THR * THR, []
    out, uv64, X64 = _replay(r, uv, X, K4, margins=margins, confidence=conf, cap=iters)
    assert LR.smallest_margin(margins) >= C.MARGIN, sorted(margins, key=lambda x: x[1])[:3]
    assert r["state"] and out["state"]
    smp = r["samples"][:out["stop"]]
    assert smp.shape[1] == 3 and (smp < n).all() and all(len(set(s)) == 3 for s in smp[:50].tolist())
    assert r["cand_idx"].tolist() == out["candidates"]
    assert r["cand_taken"].tolist() == out["taken"]
    assert r["stop"] == out["stop"] and (conf < 1.0 or r["stop"] == iters)
    best = r["cand_idx"][np.nonzero(r["cand_taken"])[0][-1]]
    assert (best >> 2, best & 3) == out["best"]
    for c, idx in enumerate(out["candidates"]):
        tr, m = idx >> 2, idx & 3
        # the scoring kernel: the recorded support of the candidate model is the restatement's support of the recorded model
        model = np.concatenate([r["models"][tr, m, :9].reshape(3, 3), r["models"][tr, m, 9:, None]], 1)
        cnt, s, _, e = LR.support(model, X64, uv64, K4, thr2)
        near = int((np.abs(e - thr2) < 1e-6).sum())       # a point on the threshold may round either way
        assert abs(cnt - r["counts"][tr, m]) <= near and abs(s - r["sums"][tr, m]) <= 1e-9 * max(1.0, s) + near * thr2
        if out["taken"][c]:                                # the LO kernel: the support after local optimisation
            lc, ls = out["lo"][c]
            assert lc == r["cand_cnt"][c] and abs(ls - r["cand_sum"][c]) <= 1e-9 * max(1.0, ls), (c, lc, ls, r["cand_cnt"][c], r["cand_sum"][c])
    e = LR.residuals(out["pose"], X64, uv64, K4)
    excused = set(np.nonzero(np.abs(e - thr2) < 1e-6)[0].tolist())
    assert set(r["inliers"].tolist()) ^ set(out["inliers"].tolist()) <= excused
    assert _close(r["ransac_pose"], out["pose"]), np.abs(r["ransac_pose"] - out["pose"]).max()
    assert _close(r["pose"], out["pose_refined"]), np.abs(r["pose"] - out["pose_refined"]).max()
    assert r["lm_iters"] == out["lm_iters"]
    print("n=%d: stop %d, %d candidates, %d taken, best %s, %d inliers, %d LM iterations, smallest margin %.3g; pose distance to the "
          "restatement %.3g before / %.3g after the refinement" % (n, r["stop"], len(out["candidates"]), sum(out["taken"]), out["best"],
                                                                   len(r["inliers"]), r["lm_iters"], LR.smallest_margin(margins),
                                                                   np.abs(r["ransac_pose"] - out["pose"]).max(),
                                                                   np.abs(r["pose"] - out["pose_refined"]).max()))


def test_refinement_does_not_raise_the_robust_cost():
    # a refinement that takes steps without checking the cost (plain Gauss-Newton on a robustified system) can end above it
    rng = np.random.default_rng(51)
    for trial in range(3):
        K, uv, X, R, t, _ = C.sp_scene(rng, 300, 0.4, 1.0)
        r = _ex(K, uv, X, seed=trial, record=True, pnp_reprojection_error=7.0)
        uv64, X64 = C.f64(uv, X)
        inl = r["inliers"]
        before = LR.robust_cost(r["ransac_pose"], X64[inl], uv64[inl], _K4(K))
        after = LR.robust_cost(r["pose"], X64[inl], uv64[inl], _K4(K))
        assert r["state"] and after <= before and r["lm_iters"] >= 1, (before, after)


def test_stop_rule():
    rng = np.random.default_rng(8)
    K, uv, X, R, t, _ = C.sp_scene(rng, 500, 0.0, 0.0)
    # all inliers: dyn = 0 after the first model, so the loop runs exactly min_trials trials (no adaptive stop: 10000; a
    # min_trials that is ignored: 1)
    r = _ex(K, uv, X)
    assert r["state"] and r["stop"] == 1000 and len(r["inliers"]) == 500
    assert _ex(K, uv, X, min_trials=300)["stop"] == 300
    # min_trials = 1: over after the first trial that yields a model (a stop that waits for min_trials' default: 1000)
    assert 1 <= _ex(K, uv, X, min_trials=1)["stop"] <= 5
    # confidence 1: every trial (an adaptive stop that ignores it: 1000)
    assert _ex(K, uv, X, confidence=1.0, iterations=3000)["stop"] == 3000
    # the cap below min_trials
    assert _ex(K, uv, X, iterations=200)["stop"] == 200
    ang, tcm = _errs(r["pose"], R, t)
    assert ang < 1e-6 and tcm < 1e-6


def test_determinism_device_inputs_and_scale():
    from onepose_plus_plus_amd.pose import ransac_PnP
    rng = np.random.default_rng(31)
    K, uv, X, R, t, _ = C.sp_scene(rng, 800, 0.5, 0.5)
    kw = dict(pnp_reprojection_error=THR, seed=3, solver="loransac")
    a = ransac_PnP(K, torch.from_numpy(uv).float().cuda(), torch.from_numpy(X).float().cuda(), **kw)
    b = ransac_PnP(K, uv, X, **kw)
    c = ransac_PnP(K, uv, X, **kw)
    d = ransac_PnP(K, uv, X, scale=1000.0, **kw)      # the pycolmap branch does not rescale (applied: t 1000 times larger)
    for x in (b, c, d):                               # bit-identical: a second call, numpy inputs, another scale
        assert a[3] and x[3] and a[0].tobytes() == x[0].tobytes() and np.array_equal(a[2], x[2])


def test_simple_pinhole_switch():
    # a scene built with fx = 560, fy = 555: exact with both focal lengths; with fx on both axes (the reference's camera) the
    # residuals of exact data are up to 0.9 % of |v - cy|, so the pose cannot be exact (a switch that is ignored: both equal)
    rng = np.random.default_rng(61)
    K, uv, X, R, t, _ = _scene(rng, 300, 0.0, 0.0)
    assert K[0, 0] != K[1, 1]
    two = _ex(K, uv, X, simple_pinhole=False)
    one = _ex(K, uv, X)
    assert two["state"] and max(_errs(two["pose"], R, t)) < 1e-6
    assert one["state"] and max(_errs(one["pose"], R, t)) > 1e-3


def test_small_inputs():
    from onepose_plus_plus_amd.pose import ransac_PnP
    rng = np.random.default_rng(12)
    K, uv, X, R, t, _ = C.sp_scene(rng, 30, 0.0, 0.0)
    for k in (0, 1, 2):
        assert _is_failure(ransac_PnP(K, uv[:k], X[:k], solver="loransac"))
        r = _ex(K, uv[:k], X[:k], record=True)
        assert not r["state"] and r["stop"] == 0 and r["inliers"].size == 0
    # n = 3: P3P models with 3 inliers each, no LO; state and pose as the restatement says
    r = _ex(K, uv[:3], X[:3], iterations=50, record=True)
    out, _, _ = _replay(r, uv[:3], X[:3], _K4(K), cap=50)
    assert r["state"] == out["state"] and r["stop"] == out["stop"]
    if out["state"]:
        assert r["inliers"].tolist() == out["inliers"].tolist() and _close(r["pose"], out["pose_refined"])
        assert np.array_equal(r["cand_cnt"], [r["counts"][i >> 2, i & 3] for i in r["cand_idx"]])
    else:
        assert _is_failure(ransac_PnP(K, uv[:3], X[:3], iterations=50, solver="loransac"))
    # n = 4: LO needs more than 4 inliers, so every candidate keeps its raw support bit for bit (LO from 4 inliers: EPnP on the
    # four would replace the sums)
    r = _ex(K, uv[:4], X[:4], iterations=200, record=True)
    assert r["state"] and len(r["cand_idx"]) >= 1 and r["counts"].max() <= 4
    for c, i in enumerate(r["cand_idx"]):
        assert r["cand_cnt"][c] == r["counts"][i >> 2, i & 3] and r["cand_sum"][c] == r["sums"][i >> 2, i & 3]
    assert _errs(r["pose"], R, t)[0] < 1e-3
    # pure outliers: a handful of chance inliers, below 20 % of 50 -> failure (without the ratio test: state True)
    junk = rng.uniform(0, 512, (50, 2))
    assert _is_failure(ransac_PnP(K, junk, X[:30].repeat(2, 0)[:50] + rng.normal(size=(50, 3)) * 0.05, pnp_reprojection_error=THR,
                                  min_inlier_ratio=0.2, solver="loransac"))


def test_workspace_one_byte_short_launches_nothing():
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(3)
    K, uv, X, R, t, _ = C.sp_scene(rng, 100, 0.2, 0.5)
    p2, p3 = torch.from_numpy(uv).float().cuda(), torch.from_numpy(X).float().cuda()
    K4 = (ctypes.c_double * 4)(*_K4(K))
    nb = lib.opp_pnp_loransac_workspace_bytes(500, 100)
    assert nb > lib.opp_pnp_loransac_workspace_bytes(500, 50) > 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    out = torch.full((12,), 7.0, dtype=torch.float64, device="cuda")
    mask = torch.full((100,), 7, dtype=torch.int32, device="cuda")
    cnt = torch.full((3,), 7, dtype=torch.int32, device="cuda")
    args = [p2.data_ptr(), p3.data_ptr(), 100, K4, THR, 500, 1, 0.9999, 1000, 0.01, out.data_ptr(), mask.data_ptr(), cnt.data_ptr(),
            cnt.data_ptr() + 4, cnt.data_ptr() + 8, None, ws.data_ptr()]
    s = torch.cuda.current_stream().cuda_stream
    assert lib.opp_pnp_loransac(*args, nb - 1, s) != 0 and b"workspace" in lib.opp_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (mask == 7).all() and (cnt == 7).all()       # nothing was launched
    assert lib.opp_pnp_loransac(*args, nb, s) == 0
    torch.cuda.synchronize()
    assert cnt[1].item() == 1 and cnt[2].item() == 500 and not (out == 7.0).any()


def test_routing():
    from onepose_plus_plus_amd.pose import ransac_PnP
    rng = np.random.default_rng(71)
    K, uv, X, R, t, _ = C.sp_scene(rng, 400, 0.4, 0.5)

    def same(a, b):
        return a[3] == b[3] and a[0].tobytes() == b[0].tobytes() and np.array_equal(a[2], b[2])

    kw = dict(scale=1000.0, pnp_reprojection_error=7, img_hw=[512, 512], seed=2)
    lo = ransac_PnP(K, uv, X, solver="loransac", **kw)
    ep = ransac_PnP(K, uv, X, solver="epnp", **kw)
    p3 = ransac_PnP(K, uv, X, solver="p3p", **kw)
    assert same(ransac_PnP(K, uv, X, use_pycolmap_ransac=True, solver="auto", **kw), lo)
    assert same(ransac_PnP(K, uv, X, use_pycolmap_ransac=False, solver="auto", **kw), ep)
    assert same(ransac_PnP(K, uv, X, **kw), p3)                                     # the default is still P3P ...
    assert same(ransac_PnP(K, uv, X, use_pycolmap_ransac=True, **kw), p3)           # ... and ignores the flag
    assert same(ransac_PnP(K, uv, X, use_pycolmap_ransac=True, solver="epnp", **kw), ep)
    assert not same(lo, ep) and not same(lo, p3)
