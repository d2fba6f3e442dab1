"""GPU: EPnP PnP-RANSAC (csrc/pnp.hip through opp_pnp_ransac_ex and pose.ransac_PnP(solver="epnp")) on synthetic scenes,
against ground truth and against the float64 restatement (tests/epnp_reference.py) on the reported samples and scores."""
import numpy as np
import pytest
import torch

from tests import epnp_reference as ER
from tests.test_pnp_gpu import _scene


def _errs(pose, R, t):
    """rotation angle (degrees, from the chord: exact near zero) and translation error (cm)"""
    ang = np.rad2deg(2 * np.arcsin(min(1.0, np.linalg.norm(pose[:, :3] - R) / (2 * np.sqrt(2)))))
    return ang, np.linalg.norm(pose[:, 3] - t) * 100.0

pytestmark = pytest.mark.gpu
SCALE = 1000.0
THR = 3.3


def _K4(K):
    return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])


def _f64(uv, X):
    return uv.astype(np.float32).astype(np.float64), X.astype(np.float32).astype(np.float64) * SCALE


@pytest.mark.parametrize("n,outliers,noise,planar", [(300, 0.0, 0.0, False), (1500, 0.5, 0.5, False), (200, 0.7, 1.0, False),
                                                      (500, 0.4, 0.5, True), (12, 0.25, 0.3, False)])
def test_epnp_recovers_pose(n, outliers, noise, planar):
    from onepose_plus_plus_amd.pose import ransac_PnP
    rng = np.random.default_rng(100 + n + int(outliers * 100))
    for trial in range(4):
        K, uv, X, R, t, out_idx = _scene(rng, n, outliers, noise, planar)
        pose, homo, inl, ok = ransac_PnP(K, uv, X, scale=SCALE, pnp_reprojection_error=THR, seed=trial, solver="epnp")
        assert ok and pose.shape == (3, 4) and homo.shape == (4, 4) and inl.ndim == 2 and inl.shape[1] == 1
        ang, tcm = _errs(pose, R, t)
        tol_a, tol_t = (1e-6, 1e-6) if noise == 0 else ((2.0, 2.0) if n < 50 else (0.8, 1.0))
        assert ang < tol_a and tcm < tol_t, (ang, tcm)
        inl_set = set(inl[:, 0].tolist())
        true_in = set(range(n)) - set(out_idx.tolist())
        assert len(inl_set & true_in) >= 0.85 * len(true_in)
        assert len(inl_set - true_in) <= 0.05 * n + 2


def test_epnp_matches_restatement():
    """hypotheses, stop index, best hypothesis and the final refit against the numpy restatement"""
    from onepose_plus_plus_amd.pose import ransac_PnP_ex
    rng = np.random.default_rng(21)
    for n, outl, conf, iters in ((120, 0.5, 0.99, 300), (60, 0.3, 1.0, 300), (400, 0.7, 0.99, 4000)):
        K, uv, X, R, t, _ = _scene(rng, n, outl, 0.5)
        r = ransac_PnP_ex(K, uv, X, scale=SCALE, pnp_reprojection_error=THR, iterations=iters, seed=5, solver="epnp",
                          confidence=conf, record=True)
        uv64, X64 = _f64(uv, X)
        K4 = _K4(K)
        sc, smp = r["scores"], r["samples"]
        assert smp.shape == (iters, 5) and (smp >= 0).all() and (smp < n).all()
        stop, best = ER.ransac_stop(sc, n, 5, conf)
        assert r["stop"] == stop and best >= 0
        checked = 0
        for h in sorted(set(range(0, min(iters, 400), 37)) | {best}):
            idx = smp[h]
            if len(set(idx.tolist())) < 5:
                continue
            ref, _ = ER.epnp(X64[idx], uv64[idx], K4)
            if ref is None:
                assert sc[h] == -1
                continue
            ref = ref.copy()
            ref[:, 3] /= SCALE
            # the device's hypothesis, re-scored through its inliers: the count the scoring kernel reported
            Xc = X64 @ ref[:, :3].T + ref[:, 3] * SCALE
            e2 = (K4[0] * Xc[:, 0] / Xc[:, 2] + K4[2] - uv64[:, 0]) ** 2 + (K4[1] * Xc[:, 1] / Xc[:, 2] + K4[3] - uv64[:, 1]) ** 2
            cnt = int(((e2 <= THR * THR) & (Xc[:, 2] > 1e-12)).sum())
            assert abs(cnt - sc[h]) <= 1, (h, cnt, sc[h])       # a point exactly on the threshold may round either way
            checked += 1
            if h == best:
                inl_ref = np.nonzero((e2 <= THR * THR) & (Xc[:, 2] > 1e-12))[0]
                assert set(r["inliers"].tolist()) ^ set(inl_ref.tolist()) <= set(np.nonzero(np.abs(e2 - THR * THR) < 1e-6)[0].tolist())
        assert checked >= 5
        # the final pose: EPnP on the returned inliers
        inl = r["inliers"]
        ref, _ = ER.epnp(X64[inl], uv64[inl], K4)
        ref[:, 3] /= SCALE
        assert np.abs(r["pose"] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), np.abs(r["pose"] - ref).max()


def test_epnp_hypothesis_pose_matches_restatement():
    """one hypothesis' pose straight from the device (iterations = 1: the refit is skipped only when it has < 5 inliers, so
    take an all-outlier scene where the best hypothesis's pose itself is returned)"""
    from onepose_plus_plus_amd.pose import ransac_PnP_ex
    rng = np.random.default_rng(4)
    n = 40
    K = np.array([[560.0, 0, 256.0], [0, 555.0, 250.0], [0, 0, 1]])
    for trial in range(6):
        X = rng.uniform(-0.15, 0.15, size=(n, 3))
        uv = rng.uniform(0, 512, size=(n, 2))
        r = ransac_PnP_ex(K, uv, X, scale=SCALE, pnp_reprojection_error=0.01, iterations=1, seed=trial, solver="epnp", record=True)
        if r["scores"][0] < 0:
            assert not r["state"]
            continue
        assert r["state"] and r["inliers"].size == 0 and r["stop"] == 1
        uv64, X64 = _f64(uv, X)
        ref, _ = ER.epnp(X64[r["samples"][0]], uv64[r["samples"][0]], _K4(K))
        ref[:, 3] /= SCALE
        assert np.abs(r["pose"] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())


def test_epnp_clean_scene_stops_early():
    from onepose_plus_plus_amd.pose import ransac_PnP_ex
    rng = np.random.default_rng(8)
    K, uv, X, R, t, _ = _scene(rng, 500, 0.0, 0.0)
    r = ransac_PnP_ex(K, uv, X, scale=SCALE, pnp_reprojection_error=THR, solver="epnp", record=True)
    assert r["state"] and r["stop"] <= 5 and len(r["inliers"]) == 500
    off = ransac_PnP_ex(K, uv, X, scale=SCALE, pnp_reprojection_error=THR, solver="epnp", confidence=1.0)
    assert off["stop"] == 10000
    ang, tcm = _errs(r["pose"], R, t)
    assert ang < 1e-6 and tcm < 1e-6


def test_epnp_small_inputs():
    from onepose_plus_plus_amd.pose import ransac_PnP, ransac_PnP_ex
    rng = np.random.default_rng(12)
    K, uv, X, R, t, _ = _scene(rng, 30, 0.0, 0.0)
    # n = 5: one EPnP solve on all five, all inliers
    r = ransac_PnP_ex(K, uv[:5], X[:5], scale=SCALE, pnp_reprojection_error=THR, solver="epnp")
    assert r["state"] and r["inliers"].tolist() == [0, 1, 2, 3, 4] and r["stop"] == 0
    uv64, X64 = _f64(uv[:5], X[:5])
    ref, _ = ER.epnp(X64, uv64, _K4(K))
    ref[:, 3] /= SCALE
    assert np.abs(r["pose"] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
    assert _errs(r["pose"], R, t)[0] < 1e-4
    # n = 4: P3P hypotheses (OpenCV's switch)
    pose, homo, inl, ok = ransac_PnP(K, uv[:4], X[:4], scale=SCALE, pnp_reprojection_error=THR, solver="epnp")
    assert ok and sorted(inl[:, 0].tolist()) == [0, 1, 2, 3] and _errs(pose, R, t)[0] < 1e-3
    # n < 4: the reference's failure convention
    for k in (0, 1, 3):
        pose, homo, inl, ok = ransac_PnP(K, uv[:k], X[:k], solver="epnp")
        assert not ok and np.array_equal(pose, np.eye(4)[:3]) and inl.size == 0


def test_epnp_determinism_and_device_inputs():
    from onepose_plus_plus_amd.pose import ransac_PnP
    rng = np.random.default_rng(31)
    K, uv, X, R, t, _ = _scene(rng, 800, 0.5, 0.5)
    a = ransac_PnP(K, torch.from_numpy(uv).float().cuda(), torch.from_numpy(X).float().cuda(), scale=SCALE, seed=3, solver="epnp")
    b = ransac_PnP(K, uv, X, scale=SCALE, seed=3, solver="epnp")
    c = ransac_PnP(K, uv, X, scale=SCALE, seed=3, solver="epnp")
    for x in (b, c):
        assert np.array_equal(a[0], x[0]) and np.array_equal(a[2], x[2]) and a[3] == x[3]


def test_p3p_through_ex_is_identical():
    import ctypes
    from onepose_plus_plus_amd import _lib
    from onepose_plus_plus_amd.pose import ransac_PnP, ransac_PnP_ex
    lib = _lib.load()
    rng = np.random.default_rng(41)
    for n in (2, 4, 12, 700):
        K, uv, X, R, t, _ = _scene(rng, max(n, 4), 0.4, 0.5)
        uv, X = uv[:n], X[:n]
        old = ransac_PnP(K, uv, X, scale=SCALE, seed=9, iterations=2000)
        new = ransac_PnP(K, uv, X, scale=SCALE, seed=9, iterations=2000, confidence=1.0)
        assert np.array_equal(old[0], new[0]) and np.array_equal(old[2], new[2]) and old[3] == new[3]
        # the raw outputs as well (pose doubles, mask, counts)
        p2 = torch.from_numpy(uv).float().cuda().reshape(-1, 2)
        p3 = torch.from_numpy(X).float().cuda().reshape(-1, 3)
        K4 = (ctypes.c_double * 4)(*_K4(K))
        outs = []
        for ex in (False, True):
            out = torch.empty(12, dtype=torch.float64, device="cuda")
            mask = torch.full((max(n, 1),), 7, dtype=torch.int32, device="cuda")
            cnt = torch.zeros(3, dtype=torch.int32, device="cuda")
            s = torch.cuda.current_stream().cuda_stream
            if ex:
                nb = lib.opp_pnp_ex_workspace_bytes(2000, n)
                ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
                _lib.check(lib.opp_pnp_ransac_ex(p2.data_ptr(), p3.data_ptr(), n, K4, 3.3, SCALE, 2000, 9, 8, 0, 1.0, out.data_ptr(),
                                                 mask.data_ptr(), cnt.data_ptr(), cnt.data_ptr() + 4, cnt.data_ptr() + 8, None, None,
                                                 ws.data_ptr(), nb, s), "ex")
            else:
                nb = lib.opp_pnp_workspace_bytes(2000)
                ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
                _lib.check(lib.opp_pnp_ransac(p2.data_ptr(), p3.data_ptr(), n, K4, 3.3, SCALE, 2000, 9, 8, out.data_ptr(),
                                              mask.data_ptr(), cnt.data_ptr(), cnt.data_ptr() + 4, ws.data_ptr(), nb, s), "old")
            outs.append((out.cpu().numpy().tobytes(), mask[:n].cpu().numpy().tobytes(), cnt[:2].cpu().numpy().tobytes()))
        assert outs[0] == outs[1]
    # p3p samples reported by the ex entry: 4 indices and -1
    r = ransac_PnP_ex(K, uv, X, scale=SCALE, iterations=50, record=True)
    assert (r["samples"][:, 4] == -1).all() and (r["samples"][:, :4] >= 0).all() and r["stop"] == 50
