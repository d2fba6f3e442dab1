"""Fixtures of the pose metrics (tests/golden/pose_metrics_*.npz), produced by the REFERENCE'S OWN functions: `query_pose_error`,
`add_metric`, `projection_2d_error` and `aggregate_metrics` of src/utils/metric_utils.py, imported read-only from the reference
checkout (OPP_REFERENCE_ROOT, default /root/reference) with empty stand-ins for cv2, open3d, plyfile and loguru, which the four
functions never touch.  Runs only where the reference is present:

    python tests/golden/gen_pose_metrics_golden.py

Inputs come from the seeds of pose_metrics_cases.py, so only results are stored.  `add_metric` returns a boolean; the mean
distance it compares is recomputed here by the function's own lines (:75-83, scipy's cKDTree included) and the boolean derived
from it is asserted to equal the function's return value.  The generator refuses to write a fixture when
  * a stored mean distance lies within 1e-6 (relative) of a `diameter * 0.1` threshold -- the boolean is then shared by any two
    correct float64 evaluations;
  * a rotation error lies within 1e-3 rad of pi -- upstream has no lower clamp, acos may return NaN there."""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden import pose_metrics_cases as C  # noqa: E402

REF = os.environ.get("OPP_REFERENCE_ROOT", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))


def load_reference_metric_utils():
    if not os.path.isdir(os.path.join(REF, "src", "utils")):
        raise RuntimeError("reference tree not found at %s" % REF)
    for name in ("cv2", "open3d", "plyfile", "loguru"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["plyfile"].PlyData = getattr(sys.modules["plyfile"], "PlyData", None)
    sys.modules["loguru"].logger = getattr(sys.modules["loguru"], "logger", None)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    return importlib.import_module("src.utils.metric_utils")


def mean_dist_by_the_functions_own_lines(mu, model_3D_pts, pose_pred, pose_target, syn):
    """metric_utils.py:75-83"""
    model_pred = np.dot(model_3D_pts, pose_pred[:, :3].T) + pose_pred[:, 3]
    model_target = np.dot(model_3D_pts, pose_target[:, :3].T) + pose_target[:, 3]
    if syn:
        mean_dist, _ = mu.spatial.cKDTree(model_pred).query(model_target, k=1)
        return np.mean(mean_dist)
    return np.mean(np.linalg.norm(model_pred - model_target, axis=-1))


def score(mu, model, pred, gt, K):
    """-> R_err, t_err [3 units], mean_dist [ADD, ADD-S], proj2D, add booleans [2 diameters][ADD, ADD-S]"""
    R_err = None
    t_err = []
    for unit in C.UNITS:
        r, t = mu.query_pose_error(pred, gt, unit=unit)
        assert R_err is None or r == R_err
        R_err = r
        t_err.append(t)
    cos = (np.trace(pred[:, :3] @ gt[:, :3].T) - 1.0) / 2.0
    assert np.isfinite(R_err) and abs(np.arccos(np.clip(cos, -1, 1)) - np.pi) > 1e-3, "rotation error next to pi"
    mean_dist = [mean_dist_by_the_functions_own_lines(mu, model, pred, gt, syn) for syn in (False, True)]
    add = np.zeros((2, 2), bool)
    for di, diameter in enumerate(C.DIAMETERS):
        for si, syn in enumerate((False, True)):
            thr = diameter * 0.1
            assert abs(mean_dist[si] - thr) >= 1e-6 * thr, "mean distance on the threshold"
            add[di, si] = mu.add_metric(model, diameter, pred, gt, syn=syn)
            assert add[di, si] == bool(mean_dist[si] < thr)
    return R_err, np.array(t_err), np.array(mean_dist), mu.projection_2d_error(model, pred, gt, K), add


def main():
    mu = load_reference_metric_utils()
    names = list(C.SINGLE_CASES)
    rows = [score(mu, *C.single_inputs(n)) for n in names]
    for P in C.P_LIST:      # for every vertex count one ADD that passes and one that fails
        adds = np.stack([r[4][:, 0] for n, r in zip(names, rows) if C.SINGLE_CASES[n][0] == P])
        assert adds.any() and not adds.all(), P
    np.savez(os.path.join(OUT, "pose_metrics_single.npz"), names=np.array(names), R_err=np.array([r[0] for r in rows]),
             t_err=np.stack([r[1] for r in rows]), mean_dist=np.stack([r[2] for r in rows]), proj2D=np.array([r[3] for r in rows]),
             add=np.stack([r[4] for r in rows]), units=np.array(C.UNITS), diameters=np.array(C.DIAMETERS))
    model, preds, gts, Ks, syn, valid = C.batch_inputs()
    rows = [score(mu, model, preds[b], gts[b], Ks[b]) for b in range(len(preds))]
    np.savez(os.path.join(OUT, "pose_metrics_batch.npz"), R_err=np.array([r[0] for r in rows]), t_err=np.stack([r[1] for r in rows]),
             mean_dist=np.stack([r[2] for r in rows]), proj2D=np.array([r[3] for r in rows]), add=np.stack([r[4] for r in rows]),
             units=np.array(C.UNITS), diameters=np.array(C.DIAMETERS))
    agg = mu.aggregate_metrics(C.aggregate_inputs())
    agg_no_add = mu.aggregate_metrics({k: v for k, v in C.aggregate_inputs().items() if k in ("R_errs", "t_errs")}, pose_thres=[2, 4])
    np.savez(os.path.join(OUT, "pose_metrics_aggregate.npz"), keys=np.array(list(agg)), values=np.array([agg[k] for k in agg]),
             keys_pose_only=np.array(list(agg_no_add)), values_pose_only=np.array([agg_no_add[k] for k in agg_no_add]))
    print("wrote %d single cases, 1 batch case, the aggregate case" % len(names))


if __name__ == "__main__":
    main()
