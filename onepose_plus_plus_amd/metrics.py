"""Pose-error metrics on the GPU: mirror of the scoring half of the reference's `compute_query_pose_errors`
(src/utils/metric_utils.py:207-292) on top of `opp_pose_metrics` (csrc/pose_metrics.hip).

`pose_metrics` scores a batch of poses of one model in one enqueue and one device-to-host copy: rotation error (degrees),
translation error (cm), ADD or ADD-S mean distance, mean 2D projection error.  `query_pose_error`, `projection_2d_error` and
`add_metric` keep the reference's signatures and return types (each is a batch of one); `compute_query_pose_errors` estimates
the batch's poses (`pose.ransac_PnP_batch` / `pose.loransac_PnP_batch`, or `pose.ransac_PnP` per sample) and scores the whole batch in one call; `aggregate_metrics` is the dataset-level summary.  All
arithmetic is float64, as the reference's numpy is (float32 vertices times float64 poses promote to float64).  No CPU fallback.

Formulas as written upstream: the trace of Rp Rg^T is clamped from above only (:116), so a rotation error next to 180 degrees
may come out NaN there and here alike; ADD-S takes for every TARGET point the nearest PREDICTED point (:79-81); the projection
divides by z without a guard (:41).
"""
import warnings

import numpy as np
import torch

from . import _lib

_T_TO_CM = {"m": 100.0, "cm": 1.0, "mm": 0.1}


def _f64(a, device, tail):
    """numpy / torch, host / device -> contiguous float64 device tensor [B, *tail]; a trailing homogeneous row is dropped"""
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() == len(tail):
        t = t[None]
    if tail == (3, 4) and t.shape[-2] == 4:        # the reference's "dim check" (:99-102)
        t = t[..., :3, :]
    if tuple(t.shape[1:]) != tail:
        raise ValueError("expected [B, %s], got %s" % (", ".join(str(d) for d in tail), tuple(t.shape)))
    return t.to(device=device, dtype=torch.float64).contiguous()


def _flags(v, n):
    """scalar or length-B sequence -> host bool array [B]"""
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    v = np.asarray(v).astype(bool)
    if v.ndim and v.shape != (n,):
        raise ValueError("expected a scalar or %d flags, got shape %s" % (n, v.shape))
    return np.broadcast_to(v, (n,))


def pose_metrics(model_pts, pose_pred, pose_gt, K=None, syn=False, valid=None, unit="m", device=None):
    """model_pts [P,3] (float32 on the device; a CUDA tensor stays resident across calls) or None (no point metrics);
    pose_pred / pose_gt [B,3,4] or [B,4,4]; K [B,3,3] or None; syn / valid: scalars or length-B sequences; unit of the model:
    'm', 'cm' or 'mm'.  -> dict of float64 numpy arrays [B]: R_errs (degrees), t_errs (cm), mean_dist (ADD where syn is false,
    ADD-S where true; model units), proj2D (pixels; absent when K is None).  A pose with valid = False gets +inf everywhere."""
    if unit not in _T_TO_CM:
        raise NotImplementedError
    lib = _lib.load()
    if device is None:
        for a in (model_pts, pose_pred, pose_gt):
            if torch.is_tensor(a) and a.is_cuda:
                device = a.device
                break
        else:
            device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    pp = _f64(pose_pred, device, (3, 4))
    pg = _f64(pose_gt, device, (3, 4))
    B = int(pp.shape[0])
    if pg.shape[0] != B:
        raise ValueError("pose_pred has %d poses, pose_gt %d" % (B, pg.shape[0]))
    Kd = None
    if K is not None:
        Kd = _f64(K, device, (3, 3))
        if Kd.shape[0] != B:
            raise ValueError("K has %d matrices for %d poses" % (Kd.shape[0], B))
    if model_pts is None:
        pts, P = None, 0
    else:
        pts = model_pts if torch.is_tensor(model_pts) else torch.from_numpy(np.ascontiguousarray(model_pts))
        pts = pts.to(device=device, dtype=torch.float32).reshape(-1, 3).contiguous()
        P = int(pts.shape[0])
    syn_h = _flags(syn, B)
    valid_h = None if valid is None else _flags(valid, B)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        syn_d = torch.from_numpy(syn_h.astype(np.uint8)).to(device) if syn_h.any() else None
        valid_d = torch.from_numpy(valid_h.astype(np.uint8)).to(device) if valid_h is not None and not valid_h.all() else None
        out = torch.empty((B, 4), dtype=torch.float64, device=device)
        nbytes = lib.opp_pose_metrics_workspace_bytes(B, P)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _lib.check(lib.opp_pose_metrics(pts.data_ptr() if P else None, P, pp.data_ptr(), pg.data_ptr(),
                                        Kd.data_ptr() if Kd is not None else None,
                                        syn_d.data_ptr() if syn_d is not None else None,
                                        valid_d.data_ptr() if valid_d is not None else None, B, _T_TO_CM[unit], out.data_ptr(),
                                        ws.data_ptr(), nbytes, stream), "opp_pose_metrics")
        host = out.cpu().numpy()                                         # the one D2H copy
    res = {"R_errs": host[:, 0].copy(), "t_errs": host[:, 1].copy(), "mean_dist": host[:, 2].copy()}
    if K is not None:
        res["proj2D"] = host[:, 3].copy()
    return res


def query_pose_error(pose_pred, pose_gt, unit="m"):
    """-> (angular distance in degrees, translation distance in cm), metric_utils.py:91-118"""
    r = pose_metrics(None, pose_pred, pose_gt, unit=unit)
    return r["R_errs"][0], r["t_errs"][0]


def projection_2d_error(model_3D_pts, pose_pred, pose_targets, K):
    """-> mean pixel distance of the projected model vertices, metric_utils.py:31-53"""
    return pose_metrics(model_3D_pts, pose_pred, pose_targets, K=K)["proj2D"][0]


def add_metric(model_3D_pts, diameter, pose_pred, pose_target, percentage=0.1, syn=False, model_unit="m"):
    """-> bool: ADD (ADD-S with `syn`) mean distance < diameter * percentage, metric_utils.py:55-87 (`model_unit` is unused
    there as well)"""
    mean_dist = pose_metrics(model_3D_pts, pose_pred, pose_target, syn=syn)["mean_dist"][0]
    return bool(mean_dist < diameter * percentage)


def _np(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _batch_poses(data, configs, query_K, pnp_kwargs, batch_loransac=False):
    """The poses of the whole batch from ONE batch call on data['m_bids'] -- `pose.ransac_PnP_batch` for "p3p" / "epnp",
    `pose.loransac_PnP_batch` for "loransac" (named, or what "auto" resolves to) when `batch_loransac` is set -- or None where the
    per-sample loop has to run: "loransac" without `batch_loransac`, or ids that are not in the matcher's order (non-decreasing, in
    [0, B)), which the loop's `m_bids == bs` selection does not need.  The order is checked on the device and read back with the
    poses, so such ids pay for the batch pass AND the loop; a RuntimeWarning says so."""
    from . import pose
    options = dict(scale=configs["point_cloud_rescale"], **pnp_kwargs)
    found = pose._batch_call(options, configs["use_pycolmap_ransac"], batch_loransac)
    if found is None or query_K.shape[0] > 1024:   # 1024: the batch passes' limit on B
        return None
    call, kw = found
    try:
        return call(query_K, data["mkpts_query_f"], data["mkpts_3d_db"], m_bids=data["m_bids"],
                    pnp_reprojection_error=configs["pnp_reprojection_error"], **kw)
    except pose.BatchIdsError:
        warnings.warn("compute_query_pose_errors: m_bids is not non-decreasing in [0, B); the batch pass was discarded and the "
                      "poses are estimated per sample", RuntimeWarning, stacklevel=3)
        return None


@torch.no_grad()
def compute_query_pose_errors(data, configs, training=False, model_vertices=None, diameter=None, syn=None, **pnp_kwargs):
    """Mirror of metric_utils.py:207-292: reads m_bids, mkpts_3d_db, mkpts_query_f, q_hw_i, query_image_scale, query_intrinsic,
    query_pose_gt (and query_intrinsic_origin, query_image_path for ADD) from `data`, estimates the poses with
    configs' point_cloud_rescale / pnp_reprojection_error / use_pycolmap_ransac (`pnp_kwargs`, e.g. solver=, are passed through):
    ONE `pose.ransac_PnP_batch` call for the solvers "p3p" and "epnp"; for "loransac" `pose.ransac_PnP` per sample, or ONE
    `pose.loransac_PnP_batch` call with `batch_loransac=True` (same bytes; off by default); `pose.ransac_PnP` per sample for ids that
    are not in the matcher's order and for `ransac_PnP=`, which names another estimator with the reference's signature and
    return tuple and gets numpy matches (the batch call and the loop give the same bytes),
    scores the whole batch in ONE `pose_metrics` call and writes R_errs, t_errs, inliers, the empty *_c lists and pose_pred
    [B,4,4]; ADD and proj2D when configs['eval_ADD_metric'] is set, the call is not training and `model_vertices` (with
    `diameter`) is given -- the reference loads both from the object's directory, `dropin.install(metrics=True)` does the same.
    syn None: the reference's rule, '0810-' or '0811-' in data['query_image_path'].
    A failed pose (`ransac_PnP` state False) follows the convention upstream writes down: np.inf errors, an empty bool array
    for the inliers, ADD False, NO proj2D entry for that sample, the identity as pose_pred.
    query_pose_gt and the intrinsics are converted to float64 before scoring; where a caller's tensors are float32 the
    reference evaluates part of the sums in float32, and the results then agree to float32 rounding only."""
    ransac_PnP = pnp_kwargs.pop("ransac_PnP", None)
    batch_loransac = bool(pnp_kwargs.pop("batch_loransac", False))
    host_matches = ransac_PnP is not None           # another estimator gets numpy matches, as the reference's own does
    if ransac_PnP is None:
        from .pose import ransac_PnP
    model_unit = configs["model_unit"] if "model_unit" in configs else "m"
    m_bids = data["m_bids"]
    mkpts_3d = data["mkpts_3d_db"]
    mkpts_query = data["mkpts_query_f"]
    img_orig_size = np.asarray(torch.tensor(data["q_hw_i"]).numpy() * _np(data["query_image_scale"]))   # B*2
    query_K = _np(data["query_intrinsic"])
    query_pose_gt = _np(data["query_pose_gt"]).astype(np.float64)   # B*4*4
    B = query_K.shape[0]

    data.update({"R_errs": [], "t_errs": [], "inliers": []})
    data.update({"R_errs_c": [], "t_errs_c": [], "inliers_c": []})
    eval_add = bool("eval_ADD_metric" in configs and configs["eval_ADD_metric"] and not training and model_vertices is not None)
    query_K_origin = None
    if eval_add:
        if diameter is None:
            raise ValueError("compute_query_pose_errors: model_vertices needs its diameter")
        if syn is None:
            image_path = data["query_image_path"]
            syn = ("0810-" in image_path) or ("0811-" in image_path)       # symmetric objects of LINEMOD
        query_K_origin = _np(data["query_intrinsic_origin"]).astype(np.float64)
        data.update({"ADD": [], "proj2D": []})

    batch = None if host_matches or not B else _batch_poses(data, configs, query_K, pnp_kwargs, batch_loransac)
    if batch is not None:
        valid = [bool(s) for s in batch["state"]]
        pose_pred = [batch["pose_homo"][bs] if valid[bs] else np.eye(4) for bs in range(B)]
        inliers = list(batch["inliers"])
    else:
        pose_pred, inliers, valid = [], [], []
        for bs in range(B):
            mask = m_bids == bs
            pts_2d, pts_3d = mkpts_query[mask], mkpts_3d[mask]
            if host_matches:
                pts_2d, pts_3d = _np(pts_2d), _np(pts_3d)
            _, pose_homo, inl, state = ransac_PnP(query_K[bs], pts_2d, pts_3d, scale=configs["point_cloud_rescale"],
                                                  img_hw=img_orig_size[bs].tolist(),
                                                  pnp_reprojection_error=configs["pnp_reprojection_error"],
                                                  use_pycolmap_ransac=configs["use_pycolmap_ransac"], **pnp_kwargs)
            pose_pred.append(pose_homo if state else np.eye(4))
            inliers.append(inl if state else np.array([]).astype(bool))
            valid.append(bool(state))
    pose_pred = np.stack(pose_pred) if B else np.zeros((0, 4, 4))   # [B*4*4]
    if B:
        res = pose_metrics(model_vertices if eval_add else None, pose_pred, query_pose_gt, K=query_K_origin, syn=bool(syn) if eval_add else False,
                           valid=valid, unit=model_unit)
    for bs in range(B):
        data["R_errs"].append(res["R_errs"][bs] if valid[bs] else np.inf)
        data["t_errs"].append(res["t_errs"][bs] if valid[bs] else np.inf)
        data["inliers"].append(inliers[bs])
        if eval_add:
            data["ADD"].append(bool(res["mean_dist"][bs] < diameter * 0.1) if valid[bs] else False)
            if valid[bs]:
                data["proj2D"].append(res["proj2D"][bs])
    data.update({"pose_pred": pose_pred})


def aggregate_metrics(metrics, pose_thres=[1, 3, 5], proj2d_thres=5):
    """Dataset-level summary with the keys of metric_utils.py:295-315: the share of frames under each "<k>cm@<k>degree" bar, and,
    when the per-frame ADD results are there ("ADD_metric", "proj2D_metric"), "ADD metric" and "proj2D metric" (the share of
    scored frames under `proj2d_thres` pixels)"""
    R = np.asarray(metrics["R_errs"])
    t = np.asarray(metrics["t_errs"])
    out = {"%scm@%sdegree" % (k, k): np.mean((R < k) & (t < k)) for k in pose_thres}
    if "ADD_metric" in metrics:
        out["ADD metric"] = np.mean(metrics["ADD_metric"])
        out["proj2D metric"] = np.mean(np.asarray(metrics["proj2D_metric"]) < proj2d_thres)
    return out
