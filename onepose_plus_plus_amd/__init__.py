"""MI355X-native (gfx950) implementation of the OnePose++ 2D-3D matching forward.

Public surface mirrors the reference package `src.models.OnePosePlus`
(/root/reference/src/models/OnePosePlus/__init__.py:1): `OnePosePlus_model`.
"""
from . import pointcloud  # noqa: F401
from .config import default_config  # noqa: F401
from .detect import AffineBoxDetector, detect_box, estimate_affine_2d, estimate_affine_2d_batch  # noqa: F401
from .metrics import (add_metric, aggregate_metrics, compute_query_pose_errors, pose_metrics, projection_2d_error,  # noqa: F401
                      query_pose_error)
from .loftr import LoFTRMatcher  # noqa: F401
from .model import OnePosePlus_model  # noqa: F401
from .tracking import PoseTracker, TrackingLost, box_from_pose, crop_K, crop_by_box  # noqa: F401

__all__ = ["OnePosePlus_model", "default_config", "pose_metrics", "query_pose_error", "projection_2d_error", "add_metric",
           "compute_query_pose_errors", "aggregate_metrics", "PoseTracker", "TrackingLost", "box_from_pose", "crop_K",
           "crop_by_box", "pointcloud", "estimate_affine_2d", "estimate_affine_2d_batch", "detect_box", "AffineBoxDetector", "LoFTRMatcher"]
