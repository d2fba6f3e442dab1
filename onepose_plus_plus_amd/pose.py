"""Pose from 2D-3D matches on the GPU: mirror of the reference's `ransac_PnP`
(/root/reference/src/utils/metric_utils.py:121-204) on top of `opp_pnp_ransac` (csrc/pnp.hip).

Same call signature and return tuple `(pose [3,4], pose_homo [4,4], inliers, state)`; the
matches may be CUDA tensors (they then never leave the device until the 12-number pose is read)
or numpy arrays.  Deterministic for a given `seed`.  No CPU fallback.  `ransac_PnP_batch` ("p3p" and "epnp", csrc/pnp_batch.hip)
and `loransac_PnP_batch` ("loransac", csrc/pnp_lo_batch.hip) estimate the poses of a whole batch in one pass, each sample
bit-identical to its single call.

Three estimators (`solver=`):
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
"epnp" and "p3p": failure convention -- fewer than 4 matches, or no hypothesis producing a model, returns the reference's own
`cv2.error` branch (identity pose, empty inliers, state False, metric_utils.py:197-204); with "p3p", when no hypothesis
gathers 4 inliers the best one is returned with state True and whatever inliers it has; with "epnp", when none gathers 5
the best valid hypothesis's pose is returned with state True and empty inliers (the reference's `inliers is None` branch).
  * "loransac": the reference's pycolmap branch (`use_pycolmap_ransac=True`: pycolmap.absolute_pose_estimation, i.e. COLMAP 3.8
    EstimateAbsolutePose = LORANSAC<P3PEstimator, EPNPEstimator> + RefineAbsolutePose, with pycolmap's defaults) as we read it
    (pycolmap is not available here, so no pycolmap fixtures: "parity unpinned"; csrc/pnp_lo.hip).  As the reference's branch does:
    a SIMPLE_PINHOLE camera [K[0,0], cx, cy] (fx serves both axes), `scale` NOT applied, `img_hw` unused.  Trial t draws 3 matches,
    P3P gives 0..4 models and every one is scored (no 4th disambiguation match): residual = squared reprojection error, a point at
    depth <= 0 is never an inlier, inlier when residual <= thr^2, support = (inliers, sum of their residuals), better = more
    inliers, or as many and a smaller sum.  A model that beats the best support with more than 4 inliers is locally optimised: EPnP
    on the best model's inliers, kept when better, repeated while the inlier count grows, at most 10 times.  After every new best
    dyn = ceil(3 log(1 - confidence) / log(1 - r^3)), r = inliers / n (r = 1: 0; log(1 - r^3) = 0: the cap); the loop ends at the
    first trial t >= dyn and >= min_trials (`confidence` 0.9999, `min_trials` 1000, `iterations` the cap).  Failure (identity pose,
    empty inliers, state False): fewer than 3 matches, no model, a best inlier count of 0 or below `min_inlier_ratio` (0.01) * n.
    The pose is then refined on the best model's inliers by Levenberg-Marquardt on sum log(1 + residual) (Cauchy, scale 1 px):
    weights 1 / (1 + s), a step accepted only when the robust cost decreases (by at least 1e-3 of the decrease the linearised
    model predicts, Ceres' min_relative_decrease), damping x10 / :10, stop at |gradient|_inf <= 1
    (COLMAP's gradient_tolerance), after 100 iterations or when the damping overflows.  The inliers returned are the RANSAC
    inliers of the best model before the refinement, as pycolmap returns them.  Where it may differ from COLMAP:
      - samples come from the hash of (seed, trial), not COLMAP's RandomSampler; all trials run in parallel and the result is that
        of the sequential loop over trials 0, 1, ... (see `stop` of `ransac_PnP_ex`);
      - the cap on the trials is `iterations` (default 10000; COLMAP's max_num_trials is 100000); confidence >= 1 runs them all;
      - P3P is Grunert's (COLMAP: Kneip-style P3P), EPnP is the one of "epnp" above (COLMAP's own EPnP port);
      - the refinement is a plain Levenberg-Marquardt on the 6-vector pose update (damping scaled by the diagonal, a fixed factor),
        not Ceres' trust-region strategy with its step-quality ratio, function / parameter tolerances and inner iterations; the
        robust loss enters by its first derivative only (no second-order Triggs correction); the focal length is not refined;
      - a depth below 1e-12 counts as "behind the camera".
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


_SOLVERS = {"p3p": 0, "epnp": 1}                                   # the C calls' solver numbers
_SOLVER_NAMES = ("p3p", "epnp", "loransac")
_CONFIDENCE = {"p3p": 1.0, "epnp": 0.99, "loransac": 0.9999}        # confidence=None; 1.0: every hypothesis is evaluated
# the options of `ransac_PnP` a solver has no use for, which its batch call therefore does not take
_NOT_TAKEN = {"p3p": ("min_trials", "min_inlier_ratio"), "epnp": ("min_trials", "min_inlier_ratio"), "loransac": ("scale", "refine_iters")}


def _resolve_solver(solver, use_pycolmap_ransac=False, auto=True):
    """the estimator's name; with `auto`, "auto" = what the reference would run.  Any other name raises ValueError"""
    if auto and solver == "auto":
        return "loransac" if use_pycolmap_ransac else "epnp"
    if solver not in _SOLVER_NAMES:
        allowed = _SOLVER_NAMES + (("auto",) if auto else ())
        raise ValueError("solver must be one of %s, got %r" % (", ".join(repr(a) for a in allowed), solver))
    return solver


def _confidence(solver, confidence):
    return _CONFIDENCE[solver] if confidence is None else confidence


def _device(pts_2d, device):
    if device is not None:
        return device
    return pts_2d.device if torch.is_tensor(pts_2d) and pts_2d.is_cuda else torch.device("cuda", torch.cuda.current_device())


def _homo(pose):
    """[3,4] -> [4,4], [B,3,4] -> [B,4,4]"""
    out = np.zeros(pose.shape[:-2] + (4, 4))
    out[..., :3, :] = pose
    out[..., 3, 3] = 1.0
    return out


def _failure():
    """the reference's `cv2.error` branch"""
    return np.eye(4)[:3], np.eye(4), np.array([]).astype(bool), False


def _single(K, pts_2d, pts_3d, device, n_cnt, ws_bytes, call, simple_pinhole=False, record_bufs=None):
    """One single-sample C call and its device-to-host copy.  cnt = n_inliers, ok(, stop(, the caller's)) is `n_cnt` ints;
    ws_bytes(lib, n) sizes the workspace; record_bufs(device) -> dict of the caller's extra device tensors;
    call(lib, p2, p3, n, K4, out, mask, cnt, bufs, ws, nbytes, stream) -- pointers but for n, bufs and nbytes -- -> (return code, name).
    -> (dict(pose [3,4], state, n_inliers (the raw count), inliers [k] int32(, stop)), cnt on the host as float64, bufs)"""
    lib = _lib.load()
    device = _device(pts_2d, device)
    Kn = K.detach().cpu().numpy() if torch.is_tensor(K) else np.asarray(K)
    Kn = Kn.astype(np.float64)
    K4 = (ctypes.c_double * 4)(Kn[0, 0], Kn[0, 0] if simple_pinhole else Kn[1, 1], Kn[0, 2], Kn[1, 2])
    p2 = _dev_f32(pts_2d, device).reshape(-1, 2)
    p3 = _dev_f32(pts_3d, device).reshape(-1, 3)
    n = int(p2.shape[0])
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        out = torch.empty(12, dtype=torch.float64, device=device)
        mask = torch.empty(max(n, 1), dtype=torch.int32, device=device)
        cnt = torch.zeros(n_cnt, dtype=torch.int32, device=device)
        bufs = record_bufs(device) if record_bufs else {}
        nbytes = ws_bytes(lib, n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _lib.check(*call(lib, p2.data_ptr(), p3.data_ptr(), n, K4, out.data_ptr(), mask.data_ptr(), cnt.data_ptr(), bufs, ws.data_ptr(),
                         nbytes, stream))
        host = torch.cat([out, cnt.double()]).cpu().numpy()              # one D2H copy
        res = {"pose": host[:12].reshape(3, 4).copy(), "state": bool(host[13] != 0), "n_inliers": int(host[12])}
        if n_cnt > 2:
            res["stop"] = int(host[14])
        res["inliers"] = torch.nonzero(mask[:n]).to(torch.int32).cpu().numpy().reshape(-1) if res["state"] else \
            np.zeros(0, np.int32)
    return res, host[12:], bufs


def _loransac(K, pts_2d, pts_3d, pnp_reprojection_error, iterations, seed, device, confidence, min_trials, min_inlier_ratio,
              simple_pinhole, record):
    """`opp_pnp_loransac` -> the dict of `ransac_PnP_ex`"""
    iterations = int(iterations)

    def record_bufs(device):
        i32, f64 = torch.int32, torch.float64
        return {"samples": torch.full((iterations, 3), -1, dtype=i32, device=device),
                "counts": torch.full((iterations, 4), -1, dtype=i32, device=device),
                "sums": torch.zeros((iterations, 4), dtype=f64, device=device),
                "models": torch.zeros((iterations, 4, 12), dtype=f64, device=device),
                "cand_idx": torch.full((iterations * 4,), -1, dtype=i32, device=device),
                "cand_cnt": torch.full((iterations * 4,), -1, dtype=i32, device=device),
                "cand_sum": torch.zeros((iterations * 4,), dtype=f64, device=device),
                "cand_taken": torch.zeros((iterations * 4,), dtype=i32, device=device),
                "ransac_pose": torch.zeros(12, dtype=f64, device=device)}

    def call(lib, p2, p3, n, K4, out, mask, cnt, bufs, ws, nbytes, stream):
        rec = _lib.OppLoRecord(n_cand=cnt + 12, lm_iters=cnt + 16, **{k: v.data_ptr() for k, v in bufs.items()}) if record else None
        return lib.opp_pnp_loransac(p2, p3, n, K4, float(pnp_reprojection_error), iterations, int(seed) & 0xFFFFFFFF, float(confidence),
                                    int(min_trials), float(min_inlier_ratio), out, mask, cnt, cnt + 4, cnt + 8,
                                    ctypes.addressof(rec) if record else None, ws, nbytes, stream), "opp_pnp_loransac"

    res, cnt, bufs = _single(K, pts_2d, pts_3d, device, 5, lambda lib, n: lib.opp_pnp_loransac_workspace_bytes(iterations, n), call,
                             simple_pinhole, record_bufs if record else None)          # cnt: n_inliers, ok, stop, n_cand, lm_iters
    if record:
        nc = int(cnt[3])
        res["lm_iters"] = int(cnt[4])
        for k in ("samples", "counts", "sums", "models"):
            res[k] = bufs[k].cpu().numpy()
        for k in ("cand_idx", "cand_cnt", "cand_sum", "cand_taken"):
            res[k] = bufs[k][:nc].cpu().numpy()
        res["ransac_pose"] = bufs["ransac_pose"].cpu().numpy().reshape(3, 4)
    return res


def ransac_PnP_ex(K, pts_2d, pts_3d, scale=1, pnp_reprojection_error=5, iterations=10000, refine_iters=8, seed=0, device=None,
                  solver="p3p", confidence=None, record=False, min_trials=1000, min_inlier_ratio=0.01, simple_pinhole=True):
    """`opp_pnp_ransac_ex` -> dict(pose [3,4], inliers [k] int, n_inliers (the kernel's own count), state, stop, and with `record` the per-hypothesis
    `samples` [iterations, 5] and `scores` [iterations]).  confidence None: 0.99 for "epnp", off for "p3p", 0.9999 for "loransac".
    solver "loransac" (`opp_pnp_loransac`; `scale` and `refine_iters` unused, `min_trials` / `min_inlier_ratio` / `simple_pinhole`
    for it alone: simple_pinhole False uses fx and fy instead of fx for both axes): `stop` = trials the sequential loop runs, and
    with `record`: `samples` [iterations, 3], per-model `counts` / `sums` [iterations, 4] (-1: no model, or a trial past the bound
    that was never scored) and `models` [iterations, 4, 12] (R row-major | t), the candidate list `cand_idx` (4 * trial + model of
    every model that beats all earlier ones), its supports after local optimisation `cand_cnt` / `cand_sum`, `cand_taken` (the
    candidates that became the best in the sequential loop; the last one is the result), `ransac_pose` [3,4] before the
    refinement and `lm_iters`."""
    solver = _resolve_solver(solver, auto=False)
    confidence = _confidence(solver, confidence)
    if solver == "loransac":
        return _loransac(K, pts_2d, pts_3d, pnp_reprojection_error, iterations, seed, device, confidence, min_trials, min_inlier_ratio,
                         simple_pinhole, record)
    iterations = int(iterations)

    def record_bufs(device):
        return {"samples": torch.full((iterations, 5), -1, dtype=torch.int32, device=device),
                "scores": torch.full((iterations,), -1, dtype=torch.int32, device=device)}

    def call(lib, p2, p3, n, K4, out, mask, cnt, bufs, ws, nbytes, stream):
        return lib.opp_pnp_ransac_ex(p2, p3, n, K4, float(pnp_reprojection_error), float(scale), iterations, int(seed) & 0xFFFFFFFF,
                                     int(refine_iters), _SOLVERS[solver], float(confidence), out, mask, cnt, cnt + 4, cnt + 8,
                                     bufs["samples"].data_ptr() if record else None, bufs["scores"].data_ptr() if record else None,
                                     ws, nbytes, stream), "opp_pnp_ransac_ex"

    res, _, bufs = _single(K, pts_2d, pts_3d, device, 3, lambda lib, n: lib.opp_pnp_ex_workspace_bytes(iterations, n), call,
                           record_bufs=record_bufs if record else None)                # cnt: n_inliers, ok, stop
    for k in bufs:
        res[k] = bufs[k].cpu().numpy()
    return res


class BatchIdsError(ValueError):
    """`ransac_PnP_batch`: the batch ids are not non-decreasing, or not all in [0, B)"""


def _batch_call(options, use_pycolmap_ransac=False, batch_loransac=True):
    """options: keyword arguments as `ransac_PnP` takes them (solver, scale, seed, ...) -> (the batch call that runs that solver, the
    options it takes), or None where no batch call is to run: a solver name that `ransac_PnP` refuses, or "loransac" (named, or what
    "auto" resolves to) without `batch_loransac`"""
    try:
        solver = _resolve_solver(options.get("solver", "p3p"), use_pycolmap_ransac)
    except ValueError:
        return None
    if solver == "loransac" and not batch_loransac:
        return None
    kw = {k: v for k, v in options.items() if k not in ("solver",) + _NOT_TAKEN[solver]}
    if solver == "loransac":
        return loransac_PnP_batch, kw
    return ransac_PnP_batch, dict(kw, solver=solver)


def _batch_seeds(name, seed, B):
    """seed: an int for every sample, or B of them -> [B] int64 in [0, 2^32)"""
    seeds = np.broadcast_to(np.asarray(seed, dtype=np.int64) & 0xFFFFFFFF, (B,)) if np.ndim(seed) == 0 else \
        np.asarray(seed, dtype=np.int64).reshape(-1) & 0xFFFFFFFF
    if seeds.shape != (B,):
        raise ValueError("%s: seed must be an int or %d ints" % (name, B))
    return seeds


def _seeds_to_device(seeds, device):
    """[B] int64 in [0, 2^32) -> the device array of unsigned the batch calls read (carried as int32 bits)"""
    return torch.from_numpy(seeds.astype(np.uint32).view(np.int32).copy()).to(device)


def _batch_prepare(name, K, pts_2d, pts_3d, m_bids, offsets, batch_size, seed, device):
    """the argument checks and host-side inputs the batch calls share -> (device, K [B,3,3] float64, seeds [B], p2, p3)"""
    if (m_bids is None) == (offsets is None):
        raise ValueError("%s: give exactly one of m_bids and offsets" % name)
    device = _device(pts_2d, device)
    Kn = K.detach().cpu().numpy() if torch.is_tensor(K) else np.asarray(K)
    Kn = Kn.astype(np.float64).reshape(-1, 3, 3)
    B = int(Kn.shape[0])
    if batch_size is not None and int(batch_size) != B:
        raise ValueError("%s: K holds %d matrices, batch_size is %d" % (name, B, int(batch_size)))
    if not 1 <= B <= 1024:
        raise ValueError("%s: 1 to 1024 samples, got %d" % (name, B))
    seeds = _batch_seeds(name, seed, B)
    p2 = _dev_f32(pts_2d, device).reshape(-1, 2)
    p3 = _dev_f32(pts_3d, device).reshape(-1, 3)
    if int(p3.shape[0]) != int(p2.shape[0]):
        raise ValueError("%s: %d 2D points, %d 3D points" % (name, int(p2.shape[0]), int(p3.shape[0])))
    return device, Kn, seeds, p2, p3


def _batch_offsets(name, lib, m_bids, offsets, B, n, bad_ptr, device, stream):
    """offsets [B+1] int32 on the device: from the ids (`opp_pnp_offsets`, which also sets the flag at `bad_ptr`), or the caller's"""
    if m_bids is not None:
        ids = m_bids if torch.is_tensor(m_bids) else torch.from_numpy(np.ascontiguousarray(m_bids))
        ids = ids.to(device=device, dtype=torch.int64).reshape(-1).contiguous()
        if int(ids.shape[0]) != n:
            raise ValueError("%s: %d batch ids for %d matches" % (name, int(ids.shape[0]), n))
        off = torch.empty(B + 1, dtype=torch.int32, device=device)
        _lib.check(lib.opp_pnp_offsets(ids.data_ptr(), n, B, off.data_ptr(), bad_ptr, stream), "opp_pnp_offsets")
        return off
    off = offsets if torch.is_tensor(offsets) else torch.from_numpy(np.ascontiguousarray(offsets))
    off = off.to(device=device, dtype=torch.int32).reshape(-1).contiguous()
    if int(off.shape[0]) != B + 1:
        raise ValueError("%s: offsets needs %d entries, got %d" % (name, B + 1, int(off.shape[0])))
    return off


def _batch_result(name, out, cnt, off, mask, B, n):
    """the two device-to-host copies of a batch call and the dict it returns; cnt = n_inliers [B], ok [B], stop [B], bad ids"""
    host = torch.cat([out.reshape(-1), cnt.double(), off.double()]).cpu().numpy()   # D2H copy 1 of 2
    if host[12 * B + 3 * B] != 0:
        raise BatchIdsError("%s: m_bids must be non-decreasing with values in [0, %d)" % (name, B))
    mask_h = mask[:n].cpu().numpy()                                               # D2H copy 2 of 2
    pose = host[:12 * B].reshape(B, 3, 4).copy()
    state = host[13 * B:14 * B] != 0
    stop = host[14 * B:15 * B].astype(np.int64)
    off_h = host[15 * B + 1:].astype(np.int64)
    inliers = []
    for b in range(B):
        lo, hi = int(off_h[b]), int(off_h[b + 1])
        if state[b] and 0 <= lo <= hi <= n:
            inliers.append(np.nonzero(mask_h[lo:hi])[0].astype(np.int32).reshape(-1, 1))
        else:
            inliers.append(np.array([]).astype(bool))
    return {"pose": pose, "pose_homo": _homo(pose), "state": state, "stop": stop, "inliers": inliers, "pose_dev": out}


def _batch_run(name, device, Kn, fy, seeds, p2, p3, m_bids, offsets, chunk, ws_bytes, call):
    """The device buffers of a batch call, its C calls over `chunk` samples at a time through one workspace (ws_bytes(lib, n) sizes
    it) and `_batch_result`.  Offsets are absolute, so a chunk is the same call further on:
    call(lib, p2, p3, off, nb, n, K4, seeds, out, mask, n_inl, ok, stop, ws, nbytes, stream) -- pointers but for nb, n and nbytes,
    those of the per-sample arrays at the chunk's first sample -- -> (return code, name)"""
    lib = _lib.load()
    B, n = int(Kn.shape[0]), int(p2.shape[0])
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        K4 = torch.from_numpy(np.ascontiguousarray(np.stack([Kn[:, 0, 0], fy, Kn[:, 0, 2], Kn[:, 1, 2]], axis=1))).to(device)
        seeds_d = _seeds_to_device(seeds, device)
        cnt = torch.zeros(3 * B + 1, dtype=torch.int32, device=device)   # n_inliers [B], ok [B], stop [B], bad ids
        off = _batch_offsets(name, lib, m_bids, offsets, B, n, cnt.data_ptr() + 12 * B, device, stream)
        out = torch.empty((B, 3, 4), dtype=torch.float64, device=device)
        mask = torch.empty(max(n, 1), dtype=torch.int32, device=device)
        nbytes = ws_bytes(lib, n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        for b0 in range(0, B, chunk):
            _lib.check(*call(lib, p2.data_ptr(), p3.data_ptr(), off.data_ptr() + 4 * b0, min(chunk, B - b0), n, K4.data_ptr() + 32 * b0,
                             seeds_d.data_ptr() + 4 * b0, out.data_ptr() + 96 * b0, mask.data_ptr(), cnt.data_ptr() + 4 * b0,
                             cnt.data_ptr() + 4 * (B + b0), cnt.data_ptr() + 4 * (2 * B + b0), ws.data_ptr(), nbytes, stream))
        return _batch_result(name, out, cnt, off, mask, B, n)


def ransac_PnP_batch(K, pts_2d, pts_3d, m_bids=None, offsets=None, batch_size=None, scale=1, pnp_reprojection_error=5,
                     iterations=10000, refine_iters=8, seed=0, solver="p3p", confidence=None, device=None,
                     use_pycolmap_ransac=False):
    """`ransac_PnP_ex` for B samples in one pass (`opp_pnp_ransac_batch`, csrc/pnp_batch.hip): sample b's results are bit for bit
    those of `ransac_PnP_ex(K[b], <its matches>, seed=seed[b], ...)`.  K [B,3,3]; pts_2d [M,2] and pts_3d [M,3] hold the matches of
    all samples concatenated in sample order (CUDA tensors stay on the device); give exactly one of `m_bids` [M] (the matcher's
    batch ids, non-decreasing, in [0, B)) and `offsets` [B+1] (sample b = matches offsets[b]:offsets[b+1]); seed: an int for every
    sample, or B of them; solver "p3p", "epnp" or "auto" (with `use_pycolmap_ransac`, as in `ransac_PnP`; "loransac" raises
    NotImplementedError: `loransac_PnP_batch` is its batch pass); confidence None: the solver's default, as in `ransac_PnP_ex`.
    -> dict: pose [B,3,4] and pose_homo [B,4,4] float64, state [B] bool, stop [B], inliers: B arrays [k,1] int32 of indices LOCAL to
    the sample (an empty bool array where state is False), pose_dev: the [B,3,4] float64 CUDA tensor.  Two device-to-host copies
    whatever B is (poses + counts + offsets, and the mask); ids that break the contract raise ValueError after the first."""
    name = "ransac_PnP_batch"
    solver = _resolve_solver(solver, use_pycolmap_ransac)
    if solver == "loransac":
        raise NotImplementedError('ransac_PnP_batch runs "p3p" and "epnp"; LO-RANSAC has a batch pass of its own, loransac_PnP_batch '
                                  '(or call ransac_PnP(solver="loransac") / ransac_PnP_ex for each sample)')
    device, Kn, seeds, p2, p3 = _batch_prepare(name, K, pts_2d, pts_3d, m_bids, offsets, batch_size, seed, device)
    confidence, iterations = _confidence(solver, confidence), int(iterations)

    def call(lib, p2, p3, off, nb, n, K4, seeds, out, mask, n_inl, ok, stop, ws, nbytes, stream):
        return lib.opp_pnp_ransac_batch(p2, p3, off, nb, n, K4, seeds, float(pnp_reprojection_error), float(scale), iterations,
                                        int(refine_iters), _SOLVERS[solver], float(confidence), out, mask, n_inl, ok, stop, ws, nbytes,
                                        stream), "opp_pnp_ransac_batch"

    B = int(Kn.shape[0])
    return _batch_run(name, device, Kn, Kn[:, 1, 1], seeds, p2, p3, m_bids, offsets, B,
                      lambda lib, n: lib.opp_pnp_batch_workspace_bytes(iterations, B, n), call)


def loransac_PnP_batch(K, pts_2d, pts_3d, m_bids=None, offsets=None, batch_size=None, pnp_reprojection_error=5, iterations=10000,
                       seed=0, confidence=None, min_trials=1000, min_inlier_ratio=0.01, simple_pinhole=True, max_batch=128,
                       device=None):
    """`ransac_PnP_ex(solver="loransac")` for B samples in one pass (`opp_pnp_loransac_batch`, csrc/pnp_lo_batch.hip): sample b's
    results are bit for bit those of `ransac_PnP_ex(K[b], <its matches>, seed=seed[b], solver="loransac", ...)`.  The inputs, the
    errors raised and the dict returned are those of `ransac_PnP_batch`; confidence None: 0.9999; `min_trials`, `min_inlier_ratio`
    and `simple_pinhole` as in `ransac_PnP_ex` (simple_pinhole True puts K[b,0,0] on both axes, as the reference's pycolmap branch
    does; that branch applies no `scale`, so there is none here).  A focal length <= 0 raises ValueError.
    max_batch: samples per C call.  The workspace of a call over b samples and M matches takes about
    948 * iterations * b + 3496 * M bytes (9.5 MB per sample at 10000 trials: 128 samples -> 1.2 GB), so larger batches run as
    chunks of `max_batch` samples through the one workspace, enqueued back to back on the same offsets, outputs and mask: no
    host sync is added and no byte of the result changes.  Two device-to-host copies whatever B and `max_batch` are."""
    name = "loransac_PnP_batch"
    device, Kn, seeds, p2, p3 = _batch_prepare(name, K, pts_2d, pts_3d, m_bids, offsets, batch_size, seed, device)
    fy = Kn[:, 0, 0] if simple_pinhole else Kn[:, 1, 1]
    if not ((Kn[:, 0, 0] > 0).all() and (fy > 0).all()):
        raise ValueError("%s: focal lengths must be positive" % name)
    if int(max_batch) < 1:
        raise ValueError("%s: max_batch must be at least 1, got %d" % (name, int(max_batch)))
    confidence, iterations = _confidence("loransac", confidence), int(iterations)
    chunk = min(int(max_batch), int(Kn.shape[0]))

    def call(lib, p2, p3, off, nb, n, K4, seeds, out, mask, n_inl, ok, stop, ws, nbytes, stream):
        return lib.opp_pnp_loransac_batch(p2, p3, off, nb, n, K4, seeds, float(pnp_reprojection_error), iterations, float(confidence),
                                          int(min_trials), float(min_inlier_ratio), out, mask, n_inl, ok, stop, ws, nbytes,
                                          stream), "opp_pnp_loransac_batch"

    return _batch_run(name, device, Kn, fy, seeds, p2, p3, m_bids, offsets, chunk,
                      lambda lib, n: lib.opp_pnp_loransac_batch_workspace_bytes(iterations, chunk, n), call)


def ransac_PnP(K, pts_2d, pts_3d, scale=1, pnp_reprojection_error=5, img_hw=None, use_pycolmap_ransac=False,
               iterations=10000, refine_iters=8, seed=0, device=None, solver="p3p", confidence=None, min_trials=1000,
               min_inlier_ratio=0.01):
    """K [3,3]; pts_2d [M,2] pixels; pts_3d [M,3].  solver: "p3p" (default), "epnp" (the reference's OpenCV branch), "loransac"
    (the reference's pycolmap branch) or "auto" = what the reference would run: "loransac" when `use_pycolmap_ransac` is true,
    "epnp" otherwise.  With "p3p" / "epnp" `use_pycolmap_ransac` is ignored; `img_hw` is accepted and unused, as in the reference.
    confidence: None = the solver's default (off for "p3p", 0.99 for "epnp", 0.9999 for "loransac"); refine_iters: "p3p" only;
    min_trials / min_inlier_ratio: "loransac" only, which also leaves `scale` unapplied (the reference's pycolmap branch does)."""
    solver = _resolve_solver(solver, use_pycolmap_ransac)
    if solver != "p3p" or confidence is not None:
        r = ransac_PnP_ex(K, pts_2d, pts_3d, scale, pnp_reprojection_error, iterations, refine_iters, seed, device, solver,
                          confidence, min_trials=min_trials, min_inlier_ratio=min_inlier_ratio)
    else:                                        # every hypothesis, no stop stage: `opp_pnp_ransac`, one launch fewer
        def call(lib, p2, p3, n, K4, out, mask, cnt, bufs, ws, nbytes, stream):
            return lib.opp_pnp_ransac(p2, p3, n, K4, float(pnp_reprojection_error), float(scale), int(iterations), int(seed) & 0xFFFFFFFF,
                                      int(refine_iters), out, mask, cnt, cnt + 4, ws, nbytes, stream), "opp_pnp_ransac"

        r, _, _ = _single(K, pts_2d, pts_3d, device, 2, lambda lib, n: lib.opp_pnp_workspace_bytes(int(iterations)), call)
    if not r["state"]:
        return _failure()
    return r["pose"], _homo(r["pose"]), r["inliers"].reshape(-1, 1), True        # OpenCV returns [n_inl, 1] indices
