"""Pose tracking: the loop of the reference's demo (demo.py:98-134) with the frame kept on the device.

The reference needs a 2D box on the first frame only; afterwards it projects the object's 3D box with the previous frame's pose,
crops the frame to 512 x 512 around it, matches, and estimates the pose with the pycolmap branch of `ransac_PnP`:

    previous_pose_detect    src/local_feature_object_detector/local_feature_2D_detector.py:200-227
    crop_img_by_bbox        local_feature_2D_detector.py:133-159   (cv2.imread + two cv2.warpAffine on the CPU, fp32 upload)
    get_K_crop_resize       src/utils/data_utils.py:258-280
    reproj                  src/utils/vis_utils.py:10-37

Here the decoded 8-bit frame is uploaded once and `opp_crop_warp_u8` (csrc/track.hip) produces the crop(s) on the device; the
box and the cropped intrinsics are 8 points and a 3 x 3 product and stay on the host in float64, where the pose already is
after PnP.  Decoding the file stays with the caller.  OpenCV's source is not available here: parity of the crop with
cv2.warpAffine is unpinned (tests/crop_reference.py restates the arithmetic in two forms).

The first-frame detector of the reference (`LocalFeatureObjectDetector.detect`) is LoFTR matching against the SfM database images
and, behind it, an affine RANSAC per view whose best view gives the box.  The estimator is built: `detect.AffineBoxDetector` runs it
on the device for all views at once (parity with `cv2.estimateAffine2D` unpinned: OpenCV is not installed here).  The LoFTR matcher
is not: the reference checkout does not carry that submodule, so the detector takes the caller's 2D-2D matcher.  `PoseTracker` takes
any callable `detector(frame_u8, K) -> [x0, y0, x1, y1]` -- an `AffineBoxDetector` is one -- or an explicit `box=` per frame.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import pose as _pose

__all__ = ["TrackingLost", "box_from_pose", "crop_K", "crop_by_box", "PoseTracker"]

_COORD_LIMIT = 32767            # OpenCV keeps warp coordinates in `short`


class TrackingLost(RuntimeError):
    """a frame needs the detector (first frame, too few inliers, unusable projected box) and there is none"""


def _np64(a):
    return (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float64)


def box_from_pose(K, pose, bbox3d):
    """2D box of the object's 3D box under `pose` (previous_pose_detect, :213-217): `reproj`, min / max over the 8 corners,
    `.astype(np.int32)` (truncation towards zero).  K [3,3] or [3,4]; pose [3,4] or [4,4]; bbox3d [8,3].  float64 on the host.

    Returns (box int32 [4] = x0, y0, x1, y1, valid).  `valid` is False -- and the box then all zeros when it cannot be
    represented -- when a projection is not finite, a corner has depth <= 0 (the reference does not check: its box is then
    meaningless), or the box is empty (x1 - x0 < 1 or y1 - y0 < 1)."""
    K, pose = _np64(K), _np64(pose)
    pts = _np64(bbox3d).reshape(-1, 3)
    if K.shape not in ((3, 3), (3, 4)) or pose.shape not in ((3, 4), (4, 4)):
        raise ValueError("box_from_pose: K must be [3,3] or [3,4], pose [3,4] or [4,4]")
    K_homo = np.concatenate([K, np.zeros((3, 1))], axis=1) if K.shape == (3, 3) else K
    pose_homo = np.concatenate([pose, np.array([[0, 0, 0, 1]])], axis=0) if pose.shape == (3, 4) else pose
    pts_homo = np.concatenate([pts, np.ones((pts.shape[0], 1))], axis=1).T
    proj = K_homo @ pose_homo @ pts_homo
    depth = proj[2].copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        proj = (proj[:] / proj[2:])[:2, :].T
    if not np.isfinite(proj).all() or np.abs(proj).max() >= 2.0 ** 31:
        return np.zeros(4, np.int32), False
    x0, y0 = np.min(proj, axis=0)
    x1, y1 = np.max(proj, axis=0)
    box = np.array([x0, y0, x1, y1]).astype(np.int32)
    valid = bool((depth > 0).all() and box[2] - box[0] >= 1 and box[3] - box[1] >= 1)
    return box, valid


def _check_box(box):
    box = np.asarray(box)
    if box.shape != (4,):
        raise ValueError("a box is [x0, y0, x1, y1]")
    if box[2] - box[0] < 1 or box[3] - box[1] < 1:
        raise ValueError("empty box %s" % (box.tolist(),))
    return box


def crop_K(box, K, crop_size=512):
    """Intrinsics of the crop (the two `get_K_crop_resize` calls of crop_img_by_bbox): T2 @ (T1 @ K) in float64, with T1 the
    translation by (-x0, -y0) and T2 = [[s, 0, 0], [0, s, S/2 - s h/2], [0, 0, 1]], s = S / w (upstream takes the scale
    from the width only).  K [3,3] -> [3,3]."""
    box = _check_box(box)
    K = _np64(K)
    if K.shape != (3, 3):
        raise ValueError("crop_K: K must be [3,3]")
    x0, y0 = float(box[0]), float(box[1])
    w, h = float(box[2]) - x0, float(box[3]) - y0
    S = float(crop_size)
    s = S / w
    T1 = np.array([[1.0, 0.0, -x0], [0.0, 1.0, -y0], [0.0, 0.0, 1.0]])
    T2 = np.array([[s, 0.0, 0.0], [0.0, s, S / 2.0 - s * h / 2.0], [0.0, 0.0, 1.0]])
    return T2 @ (T1 @ K)


def _check_crop_args(boxes, frame_hw, crop_size):
    """the refusals of opp_crop_warp_u8, raised before anything is uploaded"""
    S = int(crop_size)
    if S != crop_size or S < 64 or S > 1024 or S & (S - 1):
        raise ValueError("crop_size must be a power of two in [64, 1024], got %r" % (crop_size,))
    boxes = np.asarray(boxes.detach().cpu().numpy() if torch.is_tensor(boxes) else boxes)
    if boxes.ndim not in (1, 2) or boxes.size == 0 or boxes.shape[-1] != 4:
        raise ValueError("boxes must be [4] or [B,4] = x0, y0, x1, y1")
    boxes = boxes.reshape(-1, 4).astype(np.float64)
    if not (np.isfinite(boxes).all() and (boxes == np.trunc(boxes)).all()):
        raise ValueError("boxes must hold integers")
    if (np.abs(boxes) >= _COORD_LIMIT).any() or max(frame_hw) >= _COORD_LIMIT:
        raise ValueError("box coordinates and frame sides must stay below %d" % _COORD_LIMIT)
    boxes = np.ascontiguousarray(boxes.astype(np.int32))
    for b in boxes:
        _check_box(b)
    return boxes, S


def crop_by_box(frame_u8, boxes, K=None, crop_size=512, device=None, stream=None):
    """`crop_img_by_bbox` + `/ 255` on the device, for B boxes of one frame in one launch.

    frame_u8: [h, w] uint8 -- numpy array, CPU tensor (uploaded; pinned memory makes the copy async) or device tensor (any row
    stride).  boxes: [B,4] or [4] integers x0, y0, x1, y1 (numpy, list or tensor); they may overhang the frame (zeros there).
    Returns the crops as a DEVICE tensor [B,1,S,S] float32 in [0, 1] and, when `K` [3,3] is given, K_crop [B,3,3] float64
    numpy (`crop_K`).  Raises ValueError, before any launch, for a crop_size that is not a power of two in [64, 1024], an
    empty box, or a box coordinate / frame side at or beyond 32767."""
    lib = _lib.load()
    if isinstance(frame_u8, np.ndarray):
        frame_u8 = torch.from_numpy(np.ascontiguousarray(frame_u8))
    if not torch.is_tensor(frame_u8) or frame_u8.dtype != torch.uint8 or frame_u8.dim() != 2:
        raise ValueError("crop_by_box expects a [h, w] uint8 frame")
    h, w = frame_u8.shape
    if h < 1 or w < 1:
        raise ValueError("empty frame")
    boxes, S = _check_crop_args(boxes, (h, w), crop_size)
    K_crop = None if K is None else np.stack([crop_K(b, K, S) for b in boxes])
    if device is None:
        device = frame_u8.device if frame_u8.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("the crop kernel runs on the GPU only (no CPU fallback)")
    B = boxes.shape[0]
    with torch.cuda.device(device):
        st = torch.cuda.current_stream(device) if stream is None else stream
        with torch.cuda.stream(st):
            src = frame_u8.to(device, non_blocking=True)
            if src.stride(1) != 1:
                src = src.contiguous()
            boxes_dev = torch.from_numpy(boxes).to(device, non_blocking=True)
            out = torch.empty(B, 1, S, S, dtype=torch.float32, device=device)
            _lib.check(lib.opp_crop_warp_u8(src.data_ptr(), h, w, src.stride(0), boxes_dev.data_ptr(),
                                            boxes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), B, S, out.data_ptr(), None,
                                            st.cuda_stream), "opp_crop_warp_u8")
            src.record_stream(st)
            boxes_dev.record_stream(st)
    return out if K is None else (out, K_crop)


class PoseTracker:
    """The demo's tracking loop (demo.py:98-134) around a matcher and a resident object bank.

    model: `OnePosePlus_model` (any callable that fills `mkpts_query_f` [M,2] and `mkpts_3d_db` [M,3] of the data dict);
    bank: `ObjectBank`; K [3,3]: intrinsics of the full frame; bbox3d [8,3]: corners of the object's 3D box;
    detector: optional callable `detector(frame_u8, K) -> [x0, y0, x1, y1]`, e.g. `detect.AffineBoxDetector(matcher, ref_images)`
    (the reference's detector behind its LoFTR matcher; the matcher itself needs a submodule the checkout does not carry).  PnP runs with the demo's arguments (demo.py:132:
    scale 1000, reprojection error 7, the pycolmap branch = solver "auto" -> "loransac"); `pnp_kwargs` override them.

    >>> tracker = PoseTracker(model, bank, K, bbox3d, detector=my_detector)
    >>> for frame in frames:                      # [h, w] uint8, numpy or tensor
    ...     r = tracker.step(frame)
    ...     r["pose"], r["inliers"], r["bbox"]
    """

    def __init__(self, model, bank, K, bbox3d, detector=None, crop_size=512, min_inliers=20, seed=0, **pnp_kwargs):
        self.model, self.bank, self.detector = model, bank, detector
        self.K = _np64(K)
        self.bbox3d = _np64(bbox3d).reshape(-1, 3)
        if self.K.shape != (3, 3) or self.bbox3d.shape != (8, 3):
            raise ValueError("PoseTracker: K must be [3,3], bbox3d [8,3]")
        self.crop_size, self.min_inliers = int(crop_size), int(min_inliers)
        self.pnp_kwargs = dict(scale=1000, pnp_reprojection_error=7, use_pycolmap_ransac=True, solver="auto", seed=seed)
        self.pnp_kwargs.update(pnp_kwargs)
        self.pnp_kwargs.setdefault("img_hw", [self.crop_size, self.crop_size])
        self.reset()

    def reset(self):
        """forgets the previous pose: the next frame takes the detector (or an explicit box)"""
        self._prev = None           # (pose [3,4], number of inliers) of the last frame

    def _choose_box(self, frame_u8, box):
        if box is not None:
            return np.asarray(box.detach().cpu().numpy() if torch.is_tensor(box) else box).reshape(4), "given"
        if self._prev is not None and self._prev[1] >= self.min_inliers:      # demo.py:111 `len(inliers) < 20` -> detector
            pbox, valid = box_from_pose(self.K, self._prev[0], self.bbox3d)
            if valid:
                return pbox, "previous_pose"
        if self.detector is None:
            raise TrackingLost("no usable previous pose (first frame, fewer than %d inliers or an invalid projected box) and "
                               "no detector: pass detector= or step(frame, box=...)" % self.min_inliers)
        return np.asarray(self.detector(frame_u8, self.K)).reshape(4), "detector"

    def step(self, frame_u8, box=None, device=None, stream=None):
        """One frame [h, w] uint8.  Returns dict(pose [3,4], pose_homo [4,4], inliers, state, bbox int32 [4], K_crop [3,3],
        source "detector" | "previous_pose" | "given", data = the matcher's dict; the matches stay on the device)."""
        bbox, source = self._choose_box(frame_u8, box)
        crop, K_crop = crop_by_box(frame_u8, bbox, self.K, self.crop_size, device=device, stream=stream)
        bbox = np.asarray(bbox).astype(np.int32)
        K_crop = K_crop[0]
        data = self.bank.data(crop, K_crop=K_crop, bbox=bbox)
        with torch.no_grad():
            self.model(data)
        pose, pose_homo, inliers, state = _pose.ransac_PnP(K_crop, data["mkpts_query_f"], data["mkpts_3d_db"], **self.pnp_kwargs)
        self._prev = (pose, len(inliers))
        return {"pose": pose, "pose_homo": pose_homo, "inliers": inliers, "state": state, "bbox": bbox, "K_crop": K_crop,
                "source": source, "data": data}
