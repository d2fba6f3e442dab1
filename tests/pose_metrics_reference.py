"""numpy restatement of the reference's four pose metrics (src/utils/metric_utils.py:31-118), TEST INFRASTRUCTURE ONLY: the same
numpy operations in the same order, with a brute-force nearest neighbour in place of scipy's cKDTree (the GPU machine has neither
the reference nor, necessarily, scipy).  Pinned against the reference's own results by tests/test_pose_metrics_cpu.py."""
import numpy as np


def _rows3(pose):
    return pose[:3] if pose.shape[0] == 4 else pose


_CM_PER_UNIT = {"m": lambda d: d * 100, "cm": lambda d: d, "mm": lambda d: d / 10}      # the operations upstream applies, bit for bit


def query_pose_error(pose_pred, pose_gt, unit="m"):
    """-> (degrees, cm), :91-118; the trace is clamped from above only"""
    if unit not in _CM_PER_UNIT:
        raise NotImplementedError
    pose_pred, pose_gt = _rows3(pose_pred), _rows3(pose_gt)
    t_cm = _CM_PER_UNIT[unit](np.linalg.norm(pose_pred[:, 3] - pose_gt[:, 3]))
    trace = np.trace(np.dot(pose_pred[:, :3], pose_gt[:, :3].T))
    trace = trace if trace <= 3 else 3            # upstream's form: a NaN trace becomes 3 as well
    return np.rad2deg(np.arccos((trace - 1.0) / 2.0)), t_cm


def nearest_distances(model_pred, model_target, block=256):
    """for every TARGET point the distance to the nearest PREDICTED point (cKDTree(model_pred).query(model_target, k=1))"""
    out = np.empty(len(model_target))
    for s in range(0, len(model_target), block):
        d = model_target[s:s + block, None, :] - model_pred[None, :, :]
        out[s:s + block] = np.sqrt(np.min(np.sum(d * d, axis=-1), axis=1))
    return out


def add_mean_dist(model_3D_pts, pose_pred, pose_target, syn=False):
    """the `mean_dist` of add_metric, :75-83"""
    pose_pred, pose_target = _rows3(pose_pred), _rows3(pose_target)
    model_pred = np.dot(model_3D_pts, pose_pred[:, :3].T) + pose_pred[:, 3]
    model_target = np.dot(model_3D_pts, pose_target[:, :3].T) + pose_target[:, 3]
    if syn:
        return np.mean(nearest_distances(model_pred, model_target))
    return np.mean(np.linalg.norm(model_pred - model_target, axis=-1))


def add_metric(model_3D_pts, diameter, pose_pred, pose_target, percentage=0.1, syn=False):
    return bool(add_mean_dist(model_3D_pts, pose_pred, pose_target, syn) < diameter * percentage)


def projection_2d_error(model_3D_pts, pose_pred, pose_targets, K):
    """:31-53; divides by z without a guard"""
    def project(xyz, K, RT):
        xyz = np.dot(xyz, RT[:, :3].T) + RT[:, 3:].T
        xyz = np.dot(xyz, K.T)
        return xyz[:, :2] / xyz[:, 2:]

    pose_pred, pose_targets = _rows3(pose_pred), _rows3(pose_targets)
    return np.mean(np.linalg.norm(project(model_3D_pts, K, pose_pred) - project(model_3D_pts, K, pose_targets), axis=-1))


def score(model, pose_pred, pose_gt, K, syn, unit="m"):
    """-> [4] float64 in the order of the device output: R_err (deg), t_err (cm), mean_dist, proj2D"""
    r, t = query_pose_error(pose_pred, pose_gt, unit)
    return np.array([r, t, add_mean_dist(model, pose_pred, pose_gt, syn), projection_2d_error(model, pose_pred, pose_gt, K)])
