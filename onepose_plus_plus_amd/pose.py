"""Pose from 2D-3D matches on the GPU: mirror of the reference's `ransac_PnP`
(/root/reference/src/utils/metric_utils.py:121-204) on top of `opp_pnp_ransac` (csrc/pnp.hip).

Same call signature and return tuple `(pose [3,4], pose_homo [4,4], inliers, state)`; the
matches may be CUDA tensors (they then never leave the device until the 12-number pose is read)
or numpy arrays.  Deterministic for a given `seed`.  No CPU fallback.

Two minimal solvers (`solver=`):
  * "epnp": the reference's estimator, OpenCV 4.x `solvePnPRansac(flags=SOLVEPNP_EPNP)` as we read it (OpenCV's source is
    not available here, so no OpenCV fixtures: "parity unpinned"): EPnP on 5-match samples (P3P when there are exactly 4
    matches, one EPnP solve on all of them when there are exactly 5), inlier when the squared reprojection error <= thr^2,
    a new best only above max(best count, 4), OpenCV's adaptive stop at `confidence` (default 0.99, the reference's), an
    EPnP refit on the best hypothesis's inliers, and those RANSAC inliers returned.  Where it may differ from OpenCV:
      - samples come from a hash of (seed, hypothesis), not cv::RNG; all hypotheses run in parallel and the result is that
        of the sequential loop over hypotheses 0, 1, ... (see `stop` of `ransac_PnP_ex`);
      - errors are evaluated in float64 (OpenCV's RANSAC callback projects in float32); (1 - eps)^m is a product, not pow;
      - EPnP works on pixel coordinates with fx, fy, cx, cy (the paper and OpenCV's `epnp` class); the three beta
        initialisations are solved by Householder QR (OpenCV: SVD; the same least-squares solution for full-rank L);
        the eigenvectors of M^T M and the 3x3 SVDs come from fixed-sweep cyclic Jacobi solves; the barycentric
        coordinates use the pseudo-inverse of the control-point offsets (a vanishing principal axis gets alpha 0);
      - a degenerate refit keeps the best hypothesis's pose; a degenerate 5-match input is reported as a failure;
  * "p3p" (default, unchanged): Grunert P3P on 3 matches + a 4th for disambiguation, Gauss-Newton refinement
    (`refine_iters`) on the inliers, instead of EPnP; every one of the `iterations` hypotheses is evaluated unless a
    `confidence` < 1 is given.
Both: failure convention -- fewer than 4 matches, or no hypothesis producing a model, returns the reference's own
`cv2.error` branch (identity pose, empty inliers, state False, metric_utils.py:197-204); with "p3p", when no hypothesis
gathers 4 inliers the best one is returned with state True and whatever inliers it has; with "epnp", when none gathers 5
the best valid hypothesis's pose is returned with state True and empty inliers (the reference's `inliers is None` branch).
The pycolmap branch (`use_pycolmap_ransac=True`) is not reproduced: the argument is accepted and ignored.
"""
import ctypes

import numpy as np
import torch

from . import _lib


def _dev_f32(a, device):
    if torch.is_tensor(a):
        t = a
    else:
        t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=device, dtype=torch.float32).contiguous()


_SOLVERS = {"p3p": 0, "epnp": 1}


def ransac_PnP_ex(K, pts_2d, pts_3d, scale=1, pnp_reprojection_error=5, iterations=10000, refine_iters=8, seed=0, device=None,
                  solver="p3p", confidence=None, record=False):
    """`opp_pnp_ransac_ex` -> dict(pose [3,4], inliers [k] int, state, stop, and with `record` the per-hypothesis
    `samples` [iterations, 5] and `scores` [iterations]).  confidence None: 0.99 for "epnp", off for "p3p"."""
    if solver not in _SOLVERS:
        raise ValueError("solver must be 'p3p' or 'epnp', got %r" % (solver,))
    if confidence is None:
        confidence = 0.99 if solver == "epnp" else 1.0
    lib = _lib.load()
    if device is None:
        device = pts_2d.device if torch.is_tensor(pts_2d) and pts_2d.is_cuda else torch.device("cuda", torch.cuda.current_device())
    Kn = K.detach().cpu().numpy() if torch.is_tensor(K) else np.asarray(K)
    Kn = Kn.astype(np.float64)
    K4 = (ctypes.c_double * 4)(Kn[0, 0], Kn[1, 1], Kn[0, 2], Kn[1, 2])
    p2 = _dev_f32(pts_2d, device).reshape(-1, 2)
    p3 = _dev_f32(pts_3d, device).reshape(-1, 3)
    n = int(p2.shape[0])
    iterations = int(iterations)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        out = torch.empty(12, dtype=torch.float64, device=device)
        mask = torch.empty(max(n, 1), dtype=torch.int32, device=device)
        cnt = torch.zeros(3, dtype=torch.int32, device=device)          # n_inliers, ok, stop
        samples = torch.full((iterations, 5), -1, dtype=torch.int32, device=device) if record else None
        scores = torch.full((iterations,), -1, dtype=torch.int32, device=device) if record else None
        nbytes = lib.opp_pnp_ex_workspace_bytes(iterations, n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _lib.check(lib.opp_pnp_ransac_ex(p2.data_ptr(), p3.data_ptr(), n, K4, float(pnp_reprojection_error), float(scale),
                                         iterations, int(seed) & 0xFFFFFFFF, int(refine_iters), _SOLVERS[solver], float(confidence),
                                         out.data_ptr(), mask.data_ptr(), cnt.data_ptr(), cnt.data_ptr() + 4, cnt.data_ptr() + 8,
                                         samples.data_ptr() if record else None, scores.data_ptr() if record else None,
                                         ws.data_ptr(), nbytes, stream),
                   "opp_pnp_ransac_ex")
        host = torch.cat([out, cnt.double()]).cpu().numpy()              # one D2H copy
        res = {"pose": host[:12].reshape(3, 4).copy(), "state": bool(host[13] != 0), "stop": int(host[14])}
        res["inliers"] = torch.nonzero(mask[:n]).to(torch.int32).cpu().numpy().reshape(-1) if res["state"] else \
            np.zeros(0, np.int32)
        if record:
            res["samples"] = samples.cpu().numpy()
            res["scores"] = scores.cpu().numpy()
    return res


def ransac_PnP(K, pts_2d, pts_3d, scale=1, pnp_reprojection_error=5, img_hw=None, use_pycolmap_ransac=False,
               iterations=10000, refine_iters=8, seed=0, device=None, solver="p3p", confidence=None):
    """K [3,3]; pts_2d [M,2] pixels; pts_3d [M,3].  `img_hw` / `use_pycolmap_ransac` are accepted for
    signature compatibility (the pycolmap branch of the reference is not reproduced).  solver: "p3p" (default) or "epnp"
    (the reference's); confidence: None = the solver's default (off for "p3p", 0.99 for "epnp"); refine_iters: "p3p" only."""
    if solver not in _SOLVERS:
        raise ValueError("solver must be 'p3p' or 'epnp', got %r" % (solver,))
    if solver != "p3p" or confidence is not None:
        r = ransac_PnP_ex(K, pts_2d, pts_3d, scale, pnp_reprojection_error, iterations, refine_iters, seed, device, solver,
                          confidence)
        if not r["state"]:
            return np.eye(4)[:3], np.eye(4), np.array([]).astype(bool), False
        pose = r["pose"]
        pose_homo = np.concatenate([pose, np.array([[0.0, 0.0, 0.0, 1.0]])], axis=0)
        return pose, pose_homo, r["inliers"].reshape(-1, 1), True
    lib = _lib.load()
    if device is None:
        device = pts_2d.device if torch.is_tensor(pts_2d) and pts_2d.is_cuda else torch.device("cuda", torch.cuda.current_device())
    Kn = K.detach().cpu().numpy() if torch.is_tensor(K) else np.asarray(K)
    Kn = Kn.astype(np.float64)
    K4 = (ctypes.c_double * 4)(Kn[0, 0], Kn[1, 1], Kn[0, 2], Kn[1, 2])
    p2 = _dev_f32(pts_2d, device).reshape(-1, 2)
    p3 = _dev_f32(pts_3d, device).reshape(-1, 3)
    n = int(p2.shape[0])
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        out = torch.empty(12, dtype=torch.float64, device=device)
        mask = torch.empty(max(n, 1), dtype=torch.int32, device=device)
        cnt = torch.zeros(2, dtype=torch.int32, device=device)          # n_inliers, ok
        nbytes = lib.opp_pnp_workspace_bytes(int(iterations))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _lib.check(lib.opp_pnp_ransac(p2.data_ptr(), p3.data_ptr(), n, K4, float(pnp_reprojection_error), float(scale),
                                      int(iterations), int(seed) & 0xFFFFFFFF, int(refine_iters), out.data_ptr(),
                                      mask.data_ptr(), cnt.data_ptr(), cnt.data_ptr() + 4, ws.data_ptr(), nbytes, stream),
                   "opp_pnp_ransac")
        host = torch.cat([out, cnt.double()]).cpu().numpy()              # one D2H copy
    pose = host[:12].reshape(3, 4).copy()
    state = bool(host[13] != 0)
    pose_homo = np.concatenate([pose, np.array([[0.0, 0.0, 0.0, 1.0]])], axis=0)
    if not state:
        return np.eye(4)[:3], np.eye(4), np.array([]).astype(bool), False
    inliers = torch.nonzero(mask[:n]).to(torch.int32).cpu().numpy().reshape(-1, 1)   # OpenCV returns [n_inl, 1] indices
    return pose, pose_homo, inliers, True
