"""GPU: `opp_pose_metrics` (csrc/pose_metrics.hip) and `onepose_plus_plus_amd.metrics` against the fixtures the reference's own
functions produced (tests/golden/pose_metrics_*.npz; inputs rebuilt from the seeds of tests/golden/pose_metrics_cases.py).

Bars, from float64 rounding (eps = 2.2e-16), not fitted:
  * t_err, mean_dist, proj2D: 1e-10 * max(1, |ref|) -- at least two orders above the (P + 20) * eps a sum over P = 2500 terms and
    its ~20 roundings per term can move;
  * R_err: rad2deg(min(sqrt(16 eps), 8 eps / sin(theta))) + 1e-12 * theta, theta the reference angle in radians: the trace of
    Rp Rg^T carries up to 8 eps from either side's rounding, acos turns that into 8 eps / sin(theta), and next to theta = 0 into
    sqrt(16 eps), about 3.4e-6 degrees -- the identical-pose cases are held to exactly that;
  * the add_metric booleans: exact (the generator keeps every mean distance 1e-6 away from its threshold)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.golden import pose_metrics_cases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.2e-16


def _r_bar(ref_deg):
    theta = np.deg2rad(ref_deg)
    s = np.sin(theta)
    return np.rad2deg(min(np.sqrt(16 * EPS), 8 * EPS / s if s > 0 else np.inf)) + 1e-12 * theta


def _bar(ref):
    return 1e-10 * max(1.0, abs(ref))


@pytest.fixture(scope="module")
def single():
    g = np.load(os.path.join(GOLDEN, "pose_metrics_single.npz"))
    assert list(g["names"]) == list(C.SINGLE_CASES)
    return {k: g[k] for k in g.files}


def _raw(model, preds, gts, Ks=None, syn=None, valid=None, t_to_cm=100.0, ws_short=0):
    """one call of the C entry point -> (status, out [B,4] numpy)"""
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    pts = torch.from_numpy(np.ascontiguousarray(model, np.float32)).to(dev)
    pp = torch.from_numpy(np.ascontiguousarray(preds, np.float64)).to(dev)
    pg = torch.from_numpy(np.ascontiguousarray(gts, np.float64)).to(dev)
    kd = None if Ks is None else torch.from_numpy(np.ascontiguousarray(Ks, np.float64)).to(dev)
    sd = None if syn is None else torch.from_numpy(np.asarray(syn, np.uint8)).to(dev)
    vd = None if valid is None else torch.from_numpy(np.asarray(valid, np.uint8)).to(dev)
    B, P = len(preds), len(model)
    out = torch.full((B, 4), -7.0, dtype=torch.float64, device=dev)
    nbytes = lib.opp_pose_metrics_workspace_bytes(B, P)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = lib.opp_pose_metrics(pts.data_ptr(), P, pp.data_ptr(), pg.data_ptr(), kd.data_ptr() if kd is not None else None,
                              sd.data_ptr() if sd is not None else None, vd.data_ptr() if vd is not None else None, B,
                              ctypes.c_double(t_to_cm), out.data_ptr(), ws.data_ptr(), nbytes - ws_short,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _check(out, g, i, si, u, where):
    """out [4] against row i of a fixture: syn index si, unit index u"""
    print("%s syn=%d unit=%s: dR %.3e (bar %.3e)  dt %.3e  dmean %.3e  dproj %.3e" % (
        where, si, C.UNITS[u], abs(out[0] - g["R_err"][i]), _r_bar(g["R_err"][i]), abs(out[1] - g["t_err"][i][u]),
        abs(out[2] - g["mean_dist"][i][si]), abs(out[3] - g["proj2D"][i])))
    assert abs(out[0] - g["R_err"][i]) <= _r_bar(g["R_err"][i]), where
    assert abs(out[1] - g["t_err"][i][u]) <= _bar(g["t_err"][i][u]), where
    assert abs(out[2] - g["mean_dist"][i][si]) <= _bar(g["mean_dist"][i][si]), where
    assert abs(out[3] - g["proj2D"][i]) <= _bar(g["proj2D"][i]), where
    for di, diameter in enumerate(C.DIAMETERS):
        assert bool(out[2] < diameter * 0.1) == bool(g["add"][i][di][si]), (where, diameter)


@pytest.mark.parametrize("name", list(C.SINGLE_CASES))
def test_c_entry_point_matches_fixture(single, name):
    i = list(C.SINGLE_CASES).index(name)
    model, pred, gt, K = C.single_inputs(name)
    for si in (0, 1):
        u = (i + si) % 3
        rc, out = _raw(model, pred[None], gt[None], K[None], syn=[si] if si else None, t_to_cm=(100.0, 1.0, 0.1)[u])
        assert rc == 0
        _check(out[0], single, i, si, u, name)
    u = (i + 2) % 3                                                       # the third unit: one more launch without the ADD-S sweep
    rc, out = _raw(model, pred[None], gt[None], K[None], t_to_cm=(100.0, 1.0, 0.1)[u])
    assert rc == 0
    _check(out[0], single, i, 0, u, name)


def test_mixed_batch_in_one_call():
    g = np.load(os.path.join(GOLDEN, "pose_metrics_batch.npz"))
    model, preds, gts, Ks, syn, valid = C.batch_inputs()
    rc, out = _raw(model, preds, gts, Ks, syn=syn, valid=valid)
    assert rc == 0
    assert np.all(np.isposinf(out[1]))                                   # the invalid row
    for b in (0, 2):
        _check(out[b], g, b, int(syn[b]), 0, "batch row %d" % b)
        rc, one = _raw(model, preds[b:b + 1], gts[b:b + 1], Ks[b:b + 1], syn=syn[b:b + 1])
        assert rc == 0 and out[b].tobytes() == one[0].tobytes()          # bit for bit the B = 1 result
    rc, again = _raw(model, preds, gts, Ks, syn=syn, valid=valid)         # run to run
    assert rc == 0 and again.tobytes() == out.tobytes()


def test_two_runs_are_bit_identical():
    model, pred, gt, K = C.single_inputs("p2500_small")
    preds, gts, Ks = np.stack([pred, gt, pred]), np.stack([gt, gt, gt]), np.stack([K, K, K])
    a = _raw(model, preds, gts, Ks, syn=[1, 1, 0])[1]
    b = _raw(model, preds, gts, Ks, syn=[1, 1, 0])[1]
    assert np.all(np.isfinite(a)) and a.tobytes() == b.tobytes()


def test_no_intrinsics_and_no_points():
    """K = NULL: no 2D error (NaN in the raw output, no key in Python); no model: only the 3x3 / translation metrics"""
    from onepose_plus_plus_amd.metrics import pose_metrics, query_pose_error
    model, pred, gt, K = C.single_inputs("p65_small")
    rc, out = _raw(model, pred[None], gt[None])
    rc2, full = _raw(model, pred[None], gt[None], K[None])
    assert rc == 0 and rc2 == 0 and np.isnan(out[0, 3]) and out[0, :3].tobytes() == full[0, :3].tobytes()
    res = pose_metrics(model, pred[None], gt[None])
    assert "proj2D" not in res and res["mean_dist"][0] == full[0, 2]
    r, t = query_pose_error(pred, gt, unit="cm")
    assert r == full[0, 0] and abs(t * 100.0 - full[0, 1]) <= 1e-12 * full[0, 1]


def test_numpy_host_and_device_inputs_give_the_same_bits(single):
    from onepose_plus_plus_amd.metrics import add_metric, pose_metrics, projection_2d_error
    model, preds, gts, Ks, syn, valid = C.batch_inputs()
    homo = np.tile(np.eye(4), (3, 1, 1))
    homo[:, :3] = preds                                                   # [B,4,4]: the last row is dropped
    a = pose_metrics(model, homo, gts, K=Ks, syn=syn, valid=valid, unit="mm")
    b = pose_metrics(torch.from_numpy(model), torch.from_numpy(preds), torch.from_numpy(gts), K=torch.from_numpy(Ks),
                     syn=list(syn), valid=torch.from_numpy(valid), unit="mm")
    resident = torch.from_numpy(model).cuda()
    c = pose_metrics(resident, torch.from_numpy(preds).cuda(), torch.from_numpy(gts).cuda(), K=torch.from_numpy(Ks).cuda(), syn=syn,
                     valid=valid, unit="mm")
    raw = _raw(model, preds, gts, Ks, syn=syn, valid=valid, t_to_cm=0.1)[1]
    for r in (a, b, c):
        assert sorted(r) == ["R_errs", "mean_dist", "proj2D", "t_errs"]
        got = np.stack([r["R_errs"], r["t_errs"], r["mean_dist"], r["proj2D"]], axis=1)
        assert got.dtype == np.float64 and got.tobytes() == raw.tobytes()
    # the reference-signature wrappers are B = 1 calls of the same kernel
    i = list(C.SINGLE_CASES).index("p257_small")
    m1, pred, gt, K = C.single_inputs("p257_small")
    for si, s in enumerate((False, True)):
        for di, diameter in enumerate(C.DIAMETERS):
            res = add_metric(m1, diameter, pred, gt, syn=s)
            assert isinstance(res, bool) and res == bool(single["add"][i][di][si])
    p2d = projection_2d_error(resident.new_tensor(m1), pred, gt, K)
    assert abs(p2d - single["proj2D"][i]) <= _bar(single["proj2D"][i])


def test_short_workspace_is_refused_before_any_launch():
    from onepose_plus_plus_amd import _lib
    model, pred, gt, K = C.single_inputs("p257_small")
    rc, out = _raw(model, pred[None], gt[None], K[None], syn=[1], ws_short=1)
    assert rc < 0 and b"workspace" in _lib.load().opp_last_error()
    assert np.all(out == -7.0)                                            # nothing was written


def _planted(rng, n, K, pose):
    X = rng.uniform(-0.1, 0.1, size=(n, 3))
    Xc = X @ pose[:, :3].T + pose[:, 3]
    uv = np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], 1)
    return X.astype(np.float32), uv.astype(np.float32)


def test_compute_query_pose_errors_batch_of_two():
    """sample 0: 200 planted matches under a known pose; sample 1: 3 matches, so its pose fails"""
    from onepose_plus_plus_amd.metrics import compute_query_pose_errors, query_pose_error
    rng = np.random.default_rng(3)
    K = C.intrinsics()
    model = C.vertices(300, rng)
    gts = np.stack([np.concatenate([C.gt_pose(rng), [[0.0, 0.0, 0.0, 1.0]]]) for _ in range(2)])
    X0, uv0 = _planted(rng, 200, K, gts[0, :3])
    X1, uv1 = _planted(rng, 3, K, gts[1, :3])
    data = {"m_bids": torch.tensor([0] * 200 + [1] * 3), "mkpts_3d_db": torch.from_numpy(np.concatenate([X0, X1])).cuda(),
            "mkpts_query_f": torch.from_numpy(np.concatenate([uv0, uv1])).cuda(), "q_hw_i": (480, 640),
            "query_image_scale": torch.ones(2, 2), "query_intrinsic": torch.from_numpy(np.stack([K, K])),
            "query_intrinsic_origin": torch.from_numpy(np.stack([K, K])), "query_pose_gt": torch.from_numpy(gts),
            "query_image_path": "/data/lm/0810-obj/seq-1/color/0.png"}
    data["m_bids"] = data["m_bids"].cuda()
    configs = {"point_cloud_rescale": 1000, "pnp_reprojection_error": 3.3, "use_pycolmap_ransac": False, "eval_ADD_metric": True,
               "model_unit": "m"}
    compute_query_pose_errors(data, configs, model_vertices=model, diameter=C.DIAMETER_PASS)
    for k in ("R_errs", "t_errs", "inliers", "ADD"):
        assert len(data[k]) == 2, k
    assert data["R_errs_c"] == [] and data["t_errs_c"] == [] and data["inliers_c"] == []
    assert len(data["proj2D"]) == 1                                        # no entry for the failed sample
    assert data["pose_pred"].shape == (2, 4, 4) and np.array_equal(data["pose_pred"][1], np.eye(4))
    assert data["R_errs"][1] == np.inf and data["t_errs"][1] == np.inf and data["ADD"][1] is False
    assert data["inliers"][1].dtype == bool and data["inliers"][1].size == 0
    r, t = query_pose_error(data["pose_pred"][0], gts[0])
    assert data["R_errs"][0] == r and data["t_errs"][0] == t
    assert r < 0.05 and t < 0.05 and data["ADD"][0] is True and data["proj2D"][0] < 0.5 and len(data["inliers"][0]) >= 190
    # training, or no vertices: no ADD / proj2D keys
    for kwargs in ({"training": True, "model_vertices": model, "diameter": 0.3}, {}):
        d2 = {k: v for k, v in data.items() if k not in ("ADD", "proj2D", "R_errs", "t_errs", "inliers", "pose_pred")}
        compute_query_pose_errors(d2, configs, solver="epnp", **kwargs)
        assert "ADD" not in d2 and "proj2D" not in d2 and len(d2["R_errs"]) == 2 and d2["R_errs"][1] == np.inf


def test_compute_query_pose_errors_with_another_estimator():
    """`ransac_PnP=`: what the drop-in passes with `pnp=False` -- the estimator gets numpy matches and the reference's keywords,
    its poses are the ones scored"""
    from onepose_plus_plus_amd.metrics import compute_query_pose_errors, query_pose_error
    rng = np.random.default_rng(4)
    K = C.intrinsics()
    gt = np.concatenate([C.gt_pose(rng), [[0.0, 0.0, 0.0, 1.0]]])
    pred = np.concatenate([C.perturbed(gt[:3], "small", rng), [[0.0, 0.0, 0.0, 1.0]]])
    seen = []

    def estimator(Kq, pts_2d, pts_3d, scale=1, pnp_reprojection_error=5, img_hw=None, use_pycolmap_ransac=False):
        seen.append((type(pts_2d), type(pts_3d), pts_2d.shape, scale, pnp_reprojection_error, tuple(img_hw), use_pycolmap_ransac))
        return pred[:3], pred, np.arange(5).reshape(-1, 1), True

    data = {"m_bids": torch.zeros(7, dtype=torch.long).cuda(), "mkpts_3d_db": torch.zeros(7, 3).cuda(),
            "mkpts_query_f": torch.zeros(7, 2).cuda(), "q_hw_i": (480, 640), "query_image_scale": torch.ones(1, 2),
            "query_intrinsic": torch.from_numpy(K[None]), "query_pose_gt": torch.from_numpy(gt[None])}
    configs = {"point_cloud_rescale": 1000, "pnp_reprojection_error": 7, "use_pycolmap_ransac": True}
    compute_query_pose_errors(data, configs, ransac_PnP=estimator)
    assert seen == [(np.ndarray, np.ndarray, (7, 2), 1000, 7, (480.0, 640.0), True)]
    assert np.array_equal(data["pose_pred"], pred[None]) and len(data["inliers"][0]) == 5 and "ADD" not in data
    r, t = query_pose_error(pred, gt)
    assert data["R_errs"] == [r] and data["t_errs"] == [t] and abs(r - np.rad2deg(0.03)) < 1e-6 and abs(t - 1.0) < 1e-6
