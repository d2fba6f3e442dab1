"""CPU: the host half of the tracker (onepose_plus_plus_amd/tracking.py) -- the projected box and the cropped intrinsics against
the reference's own functions (tests/golden/track_crop.npz, written by gen_track_crop_golden.py), the two forms of the crop
arithmetic against each other (tests/crop_reference.py), the `valid` flag, every refusal and `TrackingLost`.  Nothing here
touches the device: the refusals are raised before anything is uploaded."""
import os

import numpy as np
import pytest
import torch

from tests import crop_reference as CR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track_crop.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _close(a, ref):
    """1e-9 relative to the matrix's largest entry (the bound of test_loransac_gpu.py): upstream gets its 2 x 3 matrices from a
    linear solve, which leaves rounding of that size where the exact entry is 0"""
    return np.abs(a - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())


def _random_box(rng, fh, fw):
    """boxes of all kinds: inside, overhanging, outside, thin, wide, w = 1"""
    kind = rng.integers(0, 6)
    w = int(rng.integers(1, 2 * fw)) if kind else 1
    h = int(rng.integers(1, 2 * fh))
    if kind == 1:
        h = w
    x0 = int(rng.integers(-w - 3, fw + 3))
    y0 = int(rng.integers(-h - 3, fh + 3))
    return [x0, y0, x0 + w, y0 + h]


@pytest.mark.parametrize("S", [64, 256, 512])
def test_closed_form_equals_generic_warp(S):
    rng = np.random.default_rng(S)
    n = {64: 200, 256: 100, 512: 60}[S]
    for i in range(n):
        fh, fw = int(rng.integers(1, 90)), int(rng.integers(1, 90))
        frame = rng.integers(0, 256, (fh, fw), dtype=np.uint8)
        box = _random_box(rng, fh, fw)
        assert np.array_equal(CR.warp_closed(frame, box, S), CR.warp_generic(frame, box, S)), (S, i, (fh, fw), box)


def test_closed_form_known_crops():
    rng = np.random.default_rng(1)
    frame = rng.integers(0, 256, (45, 61), dtype=np.uint8)
    # w == S: the window itself, vertically centred (h = 40 < S = 64: 12 zero rows above and below)
    out = CR.warp_closed(frame, [-2, 3, 62, 43], 64)
    want = np.zeros((64, 64), np.uint8)
    want[12:52, 2:63] = frame[3:43, 0:61]
    assert np.array_equal(out, want)
    assert not CR.warp_closed(frame, [100, 100, 130, 130], 64).any()          # entirely outside
    assert CR.to_float(out).dtype == np.float32 and CR.to_float(out).max() <= 1.0


def test_box_from_pose_equals_the_reference(gold):
    from onepose_plus_plus_amd.tracking import box_from_pose
    K, bbox3d = gold["K"], gold["bbox3d"]
    for i, (pose, want) in enumerate(zip(gold["poses"], gold["boxes"])):
        box, valid = box_from_pose(K, pose, bbox3d)
        assert valid and box.dtype == np.int32 and np.array_equal(box, want), i
        homo = np.concatenate([pose, [[0, 0, 0, 1]]])
        box4, _ = box_from_pose(np.concatenate([K, np.zeros((3, 1))], 1), torch.from_numpy(homo), bbox3d)
        assert np.array_equal(box4, want), i


def test_crop_K_equals_the_reference(gold):
    from onepose_plus_plus_amd.tracking import crop_K
    K = gold["K"]
    for box, want in zip(gold["boxes"], gold["K_crop"]):
        assert _close(crop_K(box, K, 512), want), box
    for box, S, want in zip(gold["extra_boxes"], gold["extra_crop_size"], gold["extra_K_crop"]):
        got = crop_K(box, K, int(S))
        assert got.dtype == np.float64 and got.shape == (3, 3) and _close(got, want), (box, S)
    with pytest.raises(ValueError):
        crop_K([5, 5, 5, 9], K)


def test_box_from_pose_valid_flag(gold):
    from onepose_plus_plus_amd.tracking import box_from_pose
    K, bbox3d = gold["K"], gold["bbox3d"]
    pose = np.concatenate([np.eye(3), [[0.0], [0.0], [0.6]]], axis=1)
    assert box_from_pose(K, pose, bbox3d)[1]
    behind = pose.copy()
    behind[2, 3] = -0.6                                                       # every corner behind the camera
    assert not box_from_pose(K, behind, bbox3d)[1]
    straddle = pose.copy()
    straddle[2, 3] = 0.05                                                     # half of the corners behind it
    assert not box_from_pose(K, straddle, bbox3d)[1]
    on_plane = pose.copy()
    on_plane[2, 3] = float(bbox3d[0, 2]) * -1.0                               # a corner at depth 0: division by zero
    box, valid = box_from_pose(K, on_plane, bbox3d)
    assert not valid and box.dtype == np.int32
    nan_pose = pose.copy()
    nan_pose[0, 0] = np.nan
    assert not box_from_pose(K, nan_pose, bbox3d)[1]
    far = pose.copy()
    far[2, 3] = 1e6                                                           # projects into one pixel: w < 1
    box, valid = box_from_pose(K, far, bbox3d)
    assert not valid and box[2] - box[0] < 1
    with pytest.raises(ValueError):
        box_from_pose(K[:2], pose, bbox3d)


BAD_CALLS = [  # boxes, frame shape, crop_size
    ([0, 0, 10, 10], (20, 20), 500),            # not a power of two
    ([0, 0, 10, 10], (20, 20), 32),             # below 64
    ([0, 0, 10, 10], (20, 20), 2048),           # above 1024
    ([0, 0, 10, 10], (20, 20), 128.5),
    ([5, 0, 5, 10], (20, 20), 64),              # w = 0
    ([5, 0, 4, 10], (20, 20), 64),              # w < 0
    ([0, 7, 10, 7], (20, 20), 64),              # h = 0
    ([0, 0, 32767, 10], (20, 20), 64),          # coordinate at the limit
    ([-32767, 0, 10, 10], (20, 20), 64),
    ([0, 0, 10, 40000], (20, 20), 64),
    ([[0, 0, 10, 10], [3, 3, 3, 9]], (20, 20), 64),      # one bad box of two
    ([0, 0, 10], (20, 20), 64),                 # not a box
    ([0.5, 0, 10, 10], (20, 20), 64),           # not integers
    (np.zeros((0, 4), np.int32), (20, 20), 64),
]


@pytest.mark.parametrize("boxes,hw,S", BAD_CALLS)
def test_crop_by_box_refusals_need_no_device(boxes, hw, S):
    """every refusal is raised on the host before any upload or launch: they pass without a GPU"""
    from onepose_plus_plus_amd.tracking import crop_by_box
    frame = np.zeros(hw, np.uint8)
    with pytest.raises(ValueError):
        crop_by_box(frame, boxes, crop_size=S)


def test_crop_by_box_refuses_bad_frames():
    from onepose_plus_plus_amd.tracking import crop_by_box
    with pytest.raises(ValueError):
        crop_by_box(np.zeros((20, 20), np.float32), [0, 0, 10, 10], crop_size=64)
    with pytest.raises(ValueError):
        crop_by_box(np.zeros((3, 20, 20), np.uint8), [0, 0, 10, 10], crop_size=64)
    with pytest.raises(ValueError):
        crop_by_box(torch.zeros(1, 32767, dtype=torch.uint8), [0, 0, 10, 10], crop_size=64)       # frame side at the limit


def test_c_abi_refuses_before_any_device_work():
    """The C entry point checks its host arguments first: with null device pointers replaced by dummies it returns an error
    without touching the device (no GPU here)."""
    import ctypes
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.addressof(dummy)

    def call(h, w, stride, box, S, n=1):
        hb = (ctypes.c_int * 4)(*box)
        return lib.opp_crop_warp_u8(p, h, w, stride, p, hb, n, S, p, None, None)

    assert call(20, 20, 20, [0, 0, 10, 10], 96) != 0 and b"power of two" in lib.opp_last_error()
    assert call(20, 20, 20, [0, 0, 10, 10], 32) != 0
    assert call(20, 20, 20, [0, 0, 10, 10], 2048) != 0
    assert call(20, 20, 20, [4, 0, 4, 10], 64) != 0 and b"empty" in lib.opp_last_error()
    assert call(20, 20, 20, [0, 9, 10, 8], 64) != 0
    assert call(20, 20, 20, [0, 0, 32767, 10], 64) != 0 and b"16-bit" in lib.opp_last_error()
    assert call(20, 20, 20, [0, -32767, 10, 10], 64) != 0
    assert call(32767, 20, 20, [0, 0, 10, 10], 64) != 0
    assert call(20, 32767, 32767, [0, 0, 10, 10], 64) != 0
    assert call(20, 20, 19, [0, 0, 10, 10], 64) != 0                          # stride < w
    assert call(20, 20, 20, [0, 0, 10, 10], 64, n=0) != 0
    assert lib.opp_crop_warp_u8(p, 20, 20, 20, p, None, 1, 64, p, None, None) != 0
    assert lib.opp_crop_warp_u8(p, 20, 20, 20, p, (ctypes.c_int * 4)(0, 0, 10, 10), 1, 64, None, None, None) != 0


def test_tracking_lost_without_detector(gold):
    from onepose_plus_plus_amd import PoseTracker, TrackingLost
    import onepose_plus_plus_amd as pkg
    assert issubclass(TrackingLost, RuntimeError)
    for name in ("PoseTracker", "TrackingLost", "box_from_pose", "crop_K", "crop_by_box"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    called = []
    tracker = PoseTracker(lambda d: called.append(1), None, gold["K"], gold["bbox3d"])
    assert tracker.pnp_kwargs["scale"] == 1000 and tracker.pnp_kwargs["pnp_reprojection_error"] == 7
    assert tracker.pnp_kwargs["use_pycolmap_ransac"] is True and tracker.pnp_kwargs["solver"] == "auto"
    frame = np.zeros((30, 40), np.uint8)
    with pytest.raises(TrackingLost):
        tracker.step(frame)                                                   # first frame, no detector, no box
    tracker._prev = (gold["poses"][0], 19)                                    # a pose with fewer than min_inliers inliers
    with pytest.raises(TrackingLost):
        tracker.step(frame)
    behind = gold["poses"][0].copy()
    behind[2, 3] = -1.0
    tracker._prev = (behind, 500)                                             # enough inliers, unusable projected box
    with pytest.raises(TrackingLost):
        tracker.step(frame)
    assert not called
    box, source = tracker._choose_box(frame, [1, 2, 30, 40])
    assert source == "given" and box.tolist() == [1, 2, 30, 40]
    tracker._prev = (gold["poses"][0], 20)
    box, source = tracker._choose_box(frame, None)
    assert source == "previous_pose" and np.array_equal(box, gold["boxes"][0])
    tracker.reset()
    with pytest.raises(TrackingLost):
        tracker.step(frame)
    with pytest.raises(ValueError):
        PoseTracker(None, None, gold["K"], gold["bbox3d"][:4])
