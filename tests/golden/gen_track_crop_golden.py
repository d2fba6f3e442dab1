"""Fixture of the tracker's host arithmetic (tests/golden/track_crop.npz), produced by the REFERENCE'S OWN functions: `reproj`
(src/utils/vis_utils.py) and `get_affine_transform` / `get_K_crop_resize` (src/utils/data_utils.py), called the way
`previous_pose_detect` and `crop_img_by_bbox` call them (src/local_feature_object_detector/local_feature_2D_detector.py:133-159,
:213-217; that module itself needs LoFTR and pytorch_lightning and is not imported).  The reference checkout is read-only
(OPP_REFERENCE_ROOT, default /root/reference); natsort, loguru and wis3d get empty stand-ins, and cv2 is a stand-in with
`getAffineTransform` ALONE, as a float64 solve of the 6 x 6 system of the three point pairs (cv2 is not installed; OpenCV solves
the same system in double).  Runs only where the reference is present:

    python tests/golden/gen_track_crop_golden.py

Stored: the inputs (K, bbox3d, poses, the hand-picked boxes with their crop sizes) and the reference's results (projected boxes,
K_crop).  Data only."""
import importlib
import os
import sys
import types

import numpy as np

REF = os.environ.get("OPP_REFERENCE_ROOT", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))

# hand-picked boxes (x0, y0, x1, y1, crop_size): odd widths, h != w, overhanging the frame, w = 1, other crop sizes
EXTRA_BOXES = [(100, 200, 612, 712, 512), (101, 200, 612, 633, 512), (7, 9, 340, 1200, 512), (-50, -20, 251, 97, 512),
               (1300, 1800, 1501, 2001, 512), (10, 10, 11, 12, 512), (3, 5, 68, 64, 64), (0, 0, 1440, 1920, 1024),
               (17, 23, 530, 360, 256), (400, 300, 527, 555, 128)]


def _get_affine_transform(src, dst):
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    A = np.zeros((6, 6))
    b = np.zeros(6)
    for i in range(3):
        A[i, 0:3] = [src[i, 0], src[i, 1], 1.0]
        A[i + 3, 3:6] = [src[i, 0], src[i, 1], 1.0]
        b[i], b[i + 3] = dst[i, 0], dst[i, 1]
    return np.linalg.solve(A, b).reshape(2, 3)


def load_reference():
    if not os.path.isdir(os.path.join(REF, "src", "utils")):
        raise RuntimeError("reference tree not found at %s" % REF)
    for name in ("cv2", "natsort", "loguru", "wis3d"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["cv2"].getAffineTransform = _get_affine_transform
    sys.modules["loguru"].logger = getattr(sys.modules["loguru"], "logger", None)
    sys.modules["wis3d"].Wis3D = getattr(sys.modules["wis3d"], "Wis3D", None)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    return importlib.import_module("src.utils.data_utils"), importlib.import_module("src.utils.vis_utils")


def k_crop_by_the_functions_own_lines(du, bbox, K, crop_size):
    """crop_img_by_bbox, local_feature_2D_detector.py:144-156 (the image half left out)"""
    x0, y0 = bbox[0], bbox[1]
    x1, y1 = bbox[2], bbox[3]
    resize_shape = np.array([y1 - y0, x1 - x0])
    K_crop, _ = du.get_K_crop_resize(bbox, K, resize_shape)
    bbox_new = np.array([0, 0, x1 - x0, y1 - y0])
    resize_shape = np.array([crop_size, crop_size])
    K_crop, _ = du.get_K_crop_resize(bbox_new, K_crop, resize_shape)
    return K_crop


def rodrigues(rvec):
    th = np.linalg.norm(rvec)
    k = rvec / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def main():
    du, vu = load_reference()
    rng = np.random.default_rng(20)
    K = np.array([[1477.3, 0.0, 721.6], [0.0, 1480.9, 958.2], [0.0, 0.0, 1.0]])
    ext = np.array([0.071, 0.043, 0.112])
    bbox3d = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * ext
    poses, boxes, k_crops = [], [], []
    for i in range(20):
        R = rodrigues(rng.normal(size=3) * 1.2)
        t = np.array([rng.uniform(-0.12, 0.12), rng.uniform(-0.15, 0.15), rng.uniform(0.35, 1.1)])
        pose = np.concatenate([R, t[:, None]], axis=1)
        proj = vu.reproj(K, pose if i % 4 else np.concatenate([pose, np.array([[0, 0, 0, 1.0]])]), bbox3d)   # [3,4] and [4,4]
        x0, y0 = np.min(proj, axis=0)                                                        # previous_pose_detect :215-217
        x1, y1 = np.max(proj, axis=0)
        bbox = np.array([x0, y0, x1, y1]).astype(np.int32)
        poses.append(pose)
        boxes.append(bbox)
        k_crops.append(k_crop_by_the_functions_own_lines(du, bbox, K, 512))
    boxes = np.stack(boxes)
    w, h = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    assert (w >= 1).all() and (h >= 1).all() and (w % 2 == 1).any() and (w % 2 == 0).any() and (w != h).all()
    assert (boxes[:, :2] < 0).any(), "one projected box should overhang the frame"
    extra = np.array(EXTRA_BOXES, np.int32)
    extra_k = np.stack([k_crop_by_the_functions_own_lines(du, e[:4], K, int(e[4])) for e in extra])
    np.savez(os.path.join(OUT, "track_crop.npz"), K=K, bbox3d=bbox3d, poses=np.stack(poses), boxes=boxes, K_crop=np.stack(k_crops),
             extra_boxes=extra[:, :4], extra_crop_size=extra[:, 4], extra_K_crop=extra_k)
    print("wrote %d projected boxes, %d hand-picked boxes" % (len(boxes), len(extra)))


if __name__ == "__main__":
    main()
