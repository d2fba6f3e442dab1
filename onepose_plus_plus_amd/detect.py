"""The object's 2D box from 2D-2D matches: the estimator half of the reference's first-frame detector on the device.

`LocalFeatureObjectDetector.match_worker` / `detect_by_matching` (src/local_feature_object_detector/local_feature_2D_detector.py:
74-131) match the query frame against each of `n_ref_view` database images with LoFTR and then, per view, fit an affine map with
`cv2.estimateAffine2D(mkpts0, mkpts1, method=cv2.RANSAC, ransacReprojThreshold=6)`, map the view's four image corners through it,
truncate them to int32, take min / max, and keep the box of the view with the most inliers.  The LoFTR matcher needs a submodule the
reference checkout does not carry and is not provided; everything behind it is here, as one device call for all views
(`opp_affine2d_ransac_batch`, csrc/affine.hip) instead of 15 sequential OpenCV calls behind a device-to-host copy each.

The estimator is OpenCV 4.x's RANSAC point-set registrator with modelPoints = 3 as we read `ptsetreg.cpp` (OpenCV's source and
binaries are not available here, so there are no OpenCV fixtures: "parity unpinned"; tests/affine_reference.py restates the
arithmetic in float64 numpy): a sample is rejected when its SOURCE points are collinear by `haveCollinearPoints`, the model is the
closed-form map through 3 matches, a match is an inlier when its squared transfer error <= thr^2, a new best needs more than
max(best, 2) inliers, OpenCV's adaptive stop runs at `confidence`, and the inliers returned are those of the best RANSAC model.
Where it departs from OpenCV:
  - samples come from the hash of (seed, hypothesis) the PnP estimators use, not cv::RNG; a degenerate sample counts as an iteration
    (OpenCV draws again, up to 10000 times); all hypotheses run in parallel and the result is that of the sequential loop;
  - errors are evaluated in float64 on the float32 inputs (OpenCV: float32);
  - the refinement is the linear least-squares fit on the inliers, solved by the normal equations in coordinates centred on the
    inlier mean.  OpenCV runs 10 Levenberg-Marquardt iterations on the same problem; it is linear, so its minimiser is this fit;
  - a view whose mapped corners are not finite or do not fit int32 fails (numpy's cast is undefined there).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import pose as _pose

__all__ = ["estimate_affine_2d_batch", "estimate_affine_2d", "detect_box", "AffineBoxDetector"]

_NAME = "estimate_affine_2d_batch"


def _shape2(name, which, p):
    n = int(np.prod(tuple(p.shape))) if len(tuple(p.shape)) else 1
    if n % 2 or (len(p.shape) and n and int(p.shape[-1]) != 2):
        raise ValueError("%s: %s must be [n, 2], got shape %s" % (name, which, tuple(p.shape)))
    return n // 2


def _as_arraylike(a):
    return a if torch.is_tensor(a) else np.asarray(a)


def estimate_affine_2d_batch(pts0, pts1, view_ids=None, offsets=None, n_views=None, corners=None, ransac_reproj_threshold=6.0,
                             max_iters=2000, confidence=0.99, refine=True, seed=0, fallback_box=None, device=None, record=False):
    """`cv2.estimateAffine2D(pts0, pts1, method=cv2.RANSAC)` for V views in one device call, and the boxes behind it.

    pts0 [n,2] (points in each view's image) and pts1 [n,2] (their matches in the query frame) hold the matches of all views
    concatenated in view order; CUDA tensors stay on the device.  Give at most one of `view_ids` [n] (non-decreasing, in [0, V);
    `n_views` or `corners` then says what V is) and `offsets` [V+1] (view v = matches offsets[v]:offsets[v+1]; a pair that is no
    segment of [0, n] makes an empty view); neither: one view.  corners [V,4,2]: the points whose mapped, truncated min / max is
    the view's box -- the reference's (0,0), (W,0), (0,H), (W,H) of the view's image; None: zeros.  seed: an int for every view,
    or V of them.  fallback_box: the four ints a view without a model gets (the reference's image centre +- 500); None: zeros.
    confidence >= 1 evaluates all `max_iters` hypotheses.

    -> dict of DEVICE tensors, nothing synchronised: affine [V,2,3] float64, inliers [n] int32 (0/1), n_inliers, ok, stop [V],
    boxes [V,4], best_view [1] (the view with the most inliers among those with ok = 1, the first on ties; -1 if none), best_box
    [4] int32, offsets [V+1], and with `view_ids` bad_ids [1] (1: the ids break their contract); with `record` also samples
    [V,max_iters,3] and scores [V,max_iters] (-1: no model / not evaluated).  A failed view (fewer than 3 matches, no hypothesis
    above 2 inliers, an unrepresentable box) has the identity map, no inliers, ok = 0 and the fallback box."""
    name = _NAME
    if view_ids is not None and offsets is not None:
        raise ValueError("%s: give at most one of view_ids and offsets" % name)
    pts0, pts1 = _as_arraylike(pts0), _as_arraylike(pts1)
    n = _shape2(name, "pts0", pts0)
    if _shape2(name, "pts1", pts1) != n:
        raise ValueError("%s: %d points in pts0, %d in pts1" % (name, n, _shape2(name, "pts1", pts1)))
    if corners is not None:
        corners = _as_arraylike(corners)
        if len(corners.shape) != 3 or tuple(corners.shape[1:]) != (4, 2):
            raise ValueError("%s: corners must be [V, 4, 2], got shape %s" % (name, tuple(corners.shape)))
    if offsets is not None:
        V = int(np.prod(tuple(_as_arraylike(offsets).shape))) - 1
    elif n_views is not None:
        V = int(n_views)
    elif corners is not None:
        V = int(corners.shape[0])
    elif view_ids is None:
        V = 1
    else:
        raise ValueError("%s: view_ids needs n_views (or corners)" % name)
    if n_views is not None and int(n_views) != V:
        raise ValueError("%s: offsets describe %d views, n_views is %d" % (name, V, int(n_views)))
    if corners is not None and int(corners.shape[0]) != V:
        raise ValueError("%s: corners of %d views, %d views" % (name, int(corners.shape[0]), V))
    if not 1 <= V <= 1024:
        raise ValueError("%s: 1 to 1024 views, got %d" % (name, V))
    iterations = int(max_iters)
    if not (1 <= iterations <= 1 << 20 and float(ransac_reproj_threshold) > 0 and float(confidence) > 0):
        raise ValueError("%s: max_iters must be in [1, 2^20], the threshold and the confidence positive" % name)
    seeds = _pose._batch_seeds(name, seed, V)
    fb = np.zeros(4, np.int64) if fallback_box is None else np.asarray(fallback_box).reshape(-1)
    if fb.shape != (4,) or not np.array_equal(fb, np.trunc(fb)) or (np.abs(fb) >= 2 ** 31).any():
        raise ValueError("%s: fallback_box must be four integers" % name)
    fb_c = (ctypes.c_int * 4)(*[int(x) for x in fb])

    lib = _lib.load()
    device = _pose._device(pts0, device)
    p0 = _pose._dev_f32(pts0, device).reshape(-1, 2)
    p1 = _pose._dev_f32(pts1, device).reshape(-1, 2)
    i32, f64 = torch.int32, torch.float64
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        seeds_d = _pose._seeds_to_device(seeds, device)
        bad = torch.zeros(1, dtype=i32, device=device)
        if view_ids is None and offsets is None:
            offsets = np.array([0, n], np.int32)
        off = _pose._batch_offsets(name, lib, view_ids, offsets, V, n, bad.data_ptr(), device, stream)
        if corners is None:
            cor = torch.zeros((V, 4, 2), dtype=f64, device=device)
        else:
            cor = (corners if torch.is_tensor(corners) else torch.from_numpy(np.ascontiguousarray(corners))).to(device=device, dtype=f64).contiguous()
        out = {"affine": torch.empty((V, 2, 3), dtype=f64, device=device), "inliers": torch.empty(max(n, 1), dtype=i32, device=device),
               "n_inliers": torch.empty(V, dtype=i32, device=device), "ok": torch.empty(V, dtype=i32, device=device),
               "stop": torch.empty(V, dtype=i32, device=device), "boxes": torch.empty((V, 4), dtype=i32, device=device),
               "best_view": torch.empty(1, dtype=i32, device=device), "best_box": torch.empty(4, dtype=i32, device=device)}
        if record:
            out["samples"] = torch.empty((V, iterations, 3), dtype=i32, device=device)
            out["scores"] = torch.empty((V, iterations), dtype=i32, device=device)
        nbytes = lib.opp_affine2d_batch_workspace_bytes(iterations, V, n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _lib.check(lib.opp_affine2d_ransac_batch(
            p0.data_ptr(), p1.data_ptr(), off.data_ptr(), V, n, seeds_d.data_ptr(), cor.data_ptr(), float(ransac_reproj_threshold),
            iterations, float(confidence), 1 if refine else 0, fb_c, out["affine"].data_ptr(), out["inliers"].data_ptr(),
            out["n_inliers"].data_ptr(), out["ok"].data_ptr(), out["stop"].data_ptr(), out["boxes"].data_ptr(),
            out["best_view"].data_ptr(), out["best_box"].data_ptr(), out["samples"].data_ptr() if record else None,
            out["scores"].data_ptr() if record else None, ws.data_ptr(), nbytes, stream), "opp_affine2d_ransac_batch")
    out["inliers"] = out["inliers"][:n]
    out["offsets"] = off
    if view_ids is not None:
        out["bad_ids"] = bad
    return out


def estimate_affine_2d(pts0, pts1, ransac_reproj_threshold=3.0, max_iters=2000, confidence=0.99, refine=True, seed=0, device=None):
    """`cv2.estimateAffine2D(pts0, pts1, method=cv2.RANSAC, ...)` with OpenCV's defaults and return convention:
    (2 x 3 float64 ndarray, or None when there is no model; inlier mask uint8 [n,1]).  One device call, one device-to-host copy."""
    r = estimate_affine_2d_batch(pts0, pts1, ransac_reproj_threshold=ransac_reproj_threshold, max_iters=max_iters, confidence=confidence,
                                 refine=refine, seed=seed, device=device)
    n = int(r["inliers"].shape[0])
    host = torch.cat([r["affine"].reshape(-1), r["ok"].double(), r["inliers"].double()]).cpu().numpy()
    mask = host[7:].astype(np.uint8).reshape(n, 1)
    return (host[:6].reshape(2, 3).copy() if host[6] != 0 else None), mask


def _hw_list(ref_hw, V):
    hw = np.asarray(ref_hw, np.int64)
    if hw.shape == (2,):
        hw = np.broadcast_to(hw, (V, 2))
    if hw.shape != (V, 2):
        raise ValueError("detect_box: ref_hw must be (h, w) or one (h, w) per view")
    return hw


def detect_box(matches, ref_hw, query_hw, min_matches=6, ransac_reproj_threshold=6.0, max_iters=2000, confidence=0.99, refine=True,
               seed=0, device=None):
    """The reference's `match_worker` + `detect_by_matching` behind the matcher.

    matches: one (mkpts0 [k,2] in the view's image, mkpts1 [k,2] in the query frame) per database view (numpy arrays or
    tensors; CUDA tensors are concatenated on the device); ref_hw: (h, w) of the views' images, or one pair per view; query_hw:
    (h, w) of the query frame.  A view with fewer than `min_matches` (6) matches gets no estimate: the box of the frame centre
    (w // 2, h // 2) +- 500 and zero inliers, as every view without a model does.  One device call for all views, one
    device-to-host copy.  -> (box int32 [4] = x0, y0, x1, y1 of the view with the most inliers, the first one on ties; that view's
    index, -1 when no view has a model and the box is the centre box; its number of inliers)."""
    V = len(matches)
    if V < 1:
        raise ValueError("detect_box: no views")
    hw = _hw_list(ref_hw, V)
    qh, qw = int(query_hw[0]), int(query_hw[1])
    cx, cy = qw // 2, qh // 2
    fallback = [cx - 500, cy - 500, cx + 500, cy + 500]
    corners = np.zeros((V, 4, 2))
    corners[:, 1, 0] = corners[:, 3, 0] = hw[:, 1]
    corners[:, 2, 1] = corners[:, 3, 1] = hw[:, 0]
    offsets, kept0, kept1 = [0], [], []
    for v, (m0, m1) in enumerate(matches):
        m0, m1 = _as_arraylike(m0), _as_arraylike(m1)
        k = _shape2("detect_box", "mkpts0 of view %d" % v, m0)
        if _shape2("detect_box", "mkpts1 of view %d" % v, m1) != k:
            raise ValueError("detect_box: view %d has %d and %d points" % (v, k, _shape2("detect_box", "mkpts1", m1)))
        if k >= int(min_matches):
            kept0.append(m0)
            kept1.append(m1)
        offsets.append(offsets[-1] + (k if k >= int(min_matches) else 0))
    device = _pose._device(kept0[0] if kept0 else None, device)

    def cat(parts):
        if not parts:
            return torch.zeros((0, 2), dtype=torch.float32, device=device)
        return torch.cat([_pose._dev_f32(p, device).reshape(-1, 2) for p in parts])

    r = estimate_affine_2d_batch(cat(kept0), cat(kept1), offsets=np.asarray(offsets, np.int32), corners=corners,
                                 ransac_reproj_threshold=ransac_reproj_threshold, max_iters=max_iters, confidence=confidence, refine=refine,
                                 seed=seed, fallback_box=fallback, device=device)
    host = torch.cat([r["best_box"], r["best_view"], r["n_inliers"]]).cpu().numpy()          # the one device-to-host copy
    view = int(host[4])
    return host[:4].astype(np.int32), view, (int(host[5 + view]) if view >= 0 else 0)


class AffineBoxDetector:
    """A first-frame detector for `PoseTracker(detector=...)`: `(frame_u8, K) -> [x0, y0, x1, y1]`.

    matcher(ref_image, frame) -> (mkpts0 [k,2], mkpts1 [k,2]) is the caller's 2D-2D matcher (the reference uses LoFTR), called once
    per reference view; ref_images: the database views ([h, w] arrays or tensors, kept as given).  The class holds the views and
    their corner tables and runs `detect_box` on what the matcher returns; the remaining keyword arguments are `detect_box`'s.
    `last` = (view index, inliers) of the latest call."""

    def __init__(self, matcher, ref_images, min_matches=6, **detect_kwargs):
        self.matcher, self.ref_images = matcher, list(ref_images)
        if not self.ref_images:
            raise ValueError("AffineBoxDetector: no reference views")
        self.ref_hw = np.array([[int(im.shape[-2]), int(im.shape[-1])] for im in self.ref_images], np.int64)
        self.min_matches, self.detect_kwargs, self.last = int(min_matches), detect_kwargs, None

    def __call__(self, frame_u8, K=None):
        matches = [self.matcher(ref, frame_u8) for ref in self.ref_images]
        box, view, n_inl = detect_box(matches, self.ref_hw, tuple(frame_u8.shape[-2:]), self.min_matches, **self.detect_kwargs)
        self.last = (view, n_inl)
        return box
