"""GPU: `opp_crop_warp_u8` (csrc/track.hip) bit-exact against the closed form of tests/crop_reference.py, and `PoseTracker`
(onepose_plus_plus_amd/tracking.py): the box logic of demo.py:104-123 with a stub matcher, and one frame through the real model."""
import ctypes

import numpy as np
import pytest
import torch

from tests import crop_reference as CR

pytestmark = pytest.mark.gpu

FH, FW, S = 45, 61, 64

BOXES = {  # on the 45 x 61 frame, S = 64
    "inside_square": [10, 8, 40, 38],
    "wide": [5, 12, 55, 30],                     # w > h: zero rows above and below
    "tall": [20, 2, 35, 44],                     # h > w: cut vertically
    "odd_w_odd_h": [7, 9, 40, 36],               # 33 x 27
    "odd_w_even_h": [7, 9, 40, 35],
    "over_left": [-13, 5, 20, 30],
    "over_top": [10, -11, 42, 20],
    "over_right": [40, 10, 75, 41],
    "over_bottom": [15, 25, 50, 63],
    "over_all_sides": [-9, -7, 70, 52],
    "outside": [80, 60, 110, 95],                # all zeros
    "outside_negative": [-50, -40, -10, -5],
    "w_1": [30, 20, 31, 29],
    "w_1_h_1": [60, 44, 61, 45],
    "w_eq_S": [-2, -10, 62, 54],                 # an exact copy of the window
    "w_lt_S": [12, 6, 43, 40],                   # magnified
    "w_gt_S": [-20, -15, 109, 110],              # w = 129 > S: minified
}


@pytest.fixture(scope="module")
def frame():
    """a 45 x 61 window of a wider buffer: row stride 80"""
    full = np.random.default_rng(11).integers(0, 256, (50, 80), dtype=np.uint8)
    return full, torch.from_numpy(full).cuda()[3:3 + FH, 7:7 + FW]


def _crop_raw(view, boxes, size, want_u8=True, fill=None):
    """opp_crop_warp_u8 directly -> (float output, uint8 output, return code)"""
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    boxes = np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(-1, 4))
    B = boxes.shape[0]
    dev_boxes = torch.from_numpy(boxes).cuda()
    out = torch.full((B, size, size), -7.0 if fill is None else fill, dtype=torch.float32, device="cuda")
    out8 = torch.full((B, size, size), 201, dtype=torch.uint8, device="cuda")
    rc = lib.opp_crop_warp_u8(view.data_ptr(), view.shape[0], view.shape[1], view.stride(0), dev_boxes.data_ptr(),
                              boxes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), B, size, out.data_ptr(),
                              out8.data_ptr() if want_u8 else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out8.cpu().numpy(), rc


@pytest.mark.parametrize("name", list(BOXES))
def test_crop_bit_exact_small_frame(frame, name):
    full, view = frame
    assert view.stride(0) == 80 and not view.is_contiguous()
    img = full[3:3 + FH, 7:7 + FW]
    box = BOXES[name]
    ref = CR.warp_closed(img, box, S)
    out, out8, rc = _crop_raw(view, box, S)
    assert rc == 0
    assert np.array_equal(out8[0], ref)
    assert np.array_equal(out[0], CR.to_float(ref))                     # bit-exact, including the / 255
    if name.startswith("outside"):
        assert not ref.any()
    if name == "w_eq_S":
        want = np.zeros((S, S), np.uint8)
        want[10:55, 2:63] = img
        assert np.array_equal(ref, want)
    # the public entry point on the same strided device view
    from onepose_plus_plus_amd.tracking import crop_by_box
    crop = crop_by_box(view, box, crop_size=S)
    assert crop.is_cuda and crop.dtype == torch.float32 and tuple(crop.shape) == (1, 1, S, S)
    assert np.array_equal(crop.cpu().numpy()[0, 0], CR.to_float(ref))


def test_crop_bit_exact_vga_512():
    from onepose_plus_plus_amd.tracking import crop_by_box, crop_K
    img = np.random.default_rng(5).integers(0, 256, (480, 640), dtype=np.uint8)
    K = np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1]])
    boxes = [[150, 90, 451, 370], [-40, 200, 700, 520]]
    for frame_in in (img, torch.from_numpy(img)):                          # numpy and CPU tensor are uploaded
        crop, K_crop = crop_by_box(frame_in, boxes, K=K, crop_size=512)
        torch.cuda.synchronize()
        assert tuple(crop.shape) == (2, 1, 512, 512) and K_crop.shape == (2, 3, 3)
        for b, box in enumerate(boxes):
            assert np.array_equal(crop[b, 0].cpu().numpy(), CR.to_float(CR.warp_closed(img, box, 512)))
            assert np.array_equal(K_crop[b], crop_K(box, K, 512))
    out, out8, rc = _crop_raw(torch.from_numpy(img).cuda(), boxes[0], 512)
    assert rc == 0 and np.array_equal(out8[0], CR.warp_closed(img, boxes[0], 512))


def test_batched_boxes_equal_single_calls(frame):
    _, view = frame
    names = ["odd_w_odd_h", "over_right", "w_gt_S"]
    boxes = [BOXES[n] for n in names]
    out, out8, rc = _crop_raw(view, boxes, S)
    assert rc == 0
    for b, box in enumerate(boxes):
        o1, o8, rc1 = _crop_raw(view, box, S)
        assert rc1 == 0 and np.array_equal(out[b], o1[0]) and np.array_equal(out8[b], o8[0])
    only_f, untouched8, rc = _crop_raw(view, boxes, S, want_u8=False)      # the uint8 output is optional
    assert rc == 0 and np.array_equal(only_f, out) and (untouched8 == 201).all()


@pytest.mark.parametrize("box,size", [([5, 5, 5, 20], 64), ([5, 5, 20, 4], 64), ([0, 0, 32767, 10], 64), ([0, 0, 20, 20], 96),
                                      ([0, 0, 20, 20], 32), ([[0, 0, 20, 20], [9, 9, 9, 30]], 64)])
def test_refused_call_launches_nothing(frame, box, size):
    _, view = frame
    out, out8, rc = _crop_raw(view, box, size)
    assert rc != 0
    assert (out == -7.0).all() and (out8 == 201).all()                     # the sentinels are intact


class _Detector:
    def __init__(self, box):
        self.box, self.calls = box, 0

    def __call__(self, frame_u8, K):
        self.calls += 1
        return np.array(self.box)


class _PlantedMatcher:
    """Stands in for the model: plants noise-free matches of a known, moving pose into the data dict, on the device.  Random
    weights give almost no matches, and the box logic under test does not depend on where the matches come from."""

    def __init__(self, poses, counts, pts3d):
        self.poses, self.counts, self.pts3d, self.frame = poses, counts, pts3d, 0

    def __call__(self, data):
        pose, n = self.poses[self.frame], self.counts[self.frame]
        self.frame += 1
        X = self.pts3d[:n]
        cam = X @ pose[:, :3].T + pose[:, 3]
        uv = cam @ np.asarray(data["K_crop"]).T
        uv = uv[:, :2] / uv[:, 2:]
        data["mkpts_query_f"] = torch.from_numpy(uv.astype(np.float32)).cuda()
        data["mkpts_3d_db"] = torch.from_numpy(X.astype(np.float32)).cuda()
        return data


def test_tracker_follows_the_demo_box_logic():
    from onepose_plus_plus_amd import PoseTracker, box_from_pose
    from onepose_plus_plus_amd.bank import ObjectBank
    from onepose_plus_plus_amd.pose import ransac_PnP
    rng = np.random.default_rng(2)
    K = np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1]])       # fx == fy: the pycolmap branch's SIMPLE_PINHOLE is exact
    ext = np.array([0.07, 0.045, 0.1])
    bbox3d = np.array([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], np.float64) * ext
    pts3d = rng.uniform(-1, 1, (200, 3)) * ext
    th = 0.4
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    poses = [np.concatenate([R, np.array([[0.01 * i - 0.02], [0.005 * i], [0.6 + 0.01 * i]])], axis=1) for i in range(5)]
    counts = [200, 200, 200, 10, 200]                                      # frame 3: fewer than min_inliers matches
    bank = ObjectBank(pts3d, np.zeros((128, 200), np.float32))
    det_box, _ = box_from_pose(K, poses[0], bbox3d)
    detector = _Detector(det_box)
    matcher = _PlantedMatcher(poses, counts, pts3d)
    tracker = PoseTracker(matcher, bank, K, bbox3d, detector=detector, crop_size=128)
    frames = rng.integers(0, 256, (5, 480, 640), dtype=np.uint8)
    results = [tracker.step(frames[i]) for i in range(5)]
    assert [r["source"] for r in results] == ["detector", "previous_pose", "previous_pose", "previous_pose", "detector"]
    assert detector.calls == 2
    for i, r in enumerate(results):
        assert r["state"] and len(r["inliers"]) == counts[i], i            # noise-free matches: all of them are inliers
        assert r["data"]["query_image"].is_cuda and tuple(r["data"]["query_image"].shape) == (1, 1, 128, 128)
        assert r["data"]["mkpts_query_f"].is_cuda and r["pose"].shape == (3, 4) and r["pose_homo"].shape == (4, 4)
        direct = ransac_PnP(r["K_crop"], r["data"]["mkpts_query_f"], r["data"]["mkpts_3d_db"], **tracker.pnp_kwargs)
        assert np.array_equal(r["pose"], direct[0]) and np.array_equal(r["inliers"], direct[2]), i
        if r["source"] == "previous_pose":
            want, valid = box_from_pose(K, results[i - 1]["pose"], bbox3d)
            assert valid and np.array_equal(r["bbox"], want), i
        else:
            assert np.array_equal(r["bbox"], det_box)
        assert np.array_equal(r["data"]["query_image"][0, 0].cpu().numpy(), CR.to_float(CR.warp_closed(frames[i], r["bbox"], 128)))
    assert len(results[3]["inliers"]) < tracker.min_inliers
    matcher.frame = 0
    given = tracker.step(frames[0], box=[100, 100, 300, 260])
    assert given["source"] == "given" and given["bbox"].tolist() == [100, 100, 300, 260]
    tracker.reset()
    matcher.frame = 0
    assert tracker.step(frames[0])["source"] == "detector" and detector.calls == 3


def test_tracker_step_through_the_real_model(tmp_path):
    """step() on a frame == the model called on crop_reference's crop of the same frame (128 x 128 crop, 400-point bank)."""
    from onepose_plus_plus_amd import PoseTracker
    from onepose_plus_plus_amd.bank import ObjectBank
    from onepose_plus_plus_amd.config import default_config
    from onepose_plus_plus_amd.synthetic import make_state_dict, make_inputs
    from tests import hip_ops as ops
    cfg = default_config(thr=0.0)
    sd = make_state_dict(cfg, 0)
    base = make_inputs(400, (128, 128), 3)
    path = str(tmp_path / "anno_3d_average.npz")
    ObjectBank.save_npz(path, base["keypoints3d"][0].double().numpy(), base["descriptors3d_db"][0].numpy(),
                        np.ones((400, 1), np.float32), base["descriptors3d_coarse_db"][0].numpy())
    bank = ObjectBank.from_npz(path, shape3d=15000)
    frame = np.random.default_rng(9).integers(0, 256, (150, 200), dtype=np.uint8)
    box = [31, -12, 188, 131]                                              # odd width, overhangs the top
    K = np.array([[300.0, 0, 100.0], [0, 300.0, 75.0], [0, 0, 1]])
    bbox3d = np.array([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], np.float64) * 0.5
    tracker = PoseTracker(ops.make_model(cfg, sd), bank, K, bbox3d, crop_size=128, iterations=2000)
    r = tracker.step(frame, box=box)
    ref = {k: v for k, v in base.items() if k != "query_image_scale"}
    ref["query_image"] = torch.from_numpy(CR.to_float(CR.warp_closed(frame, box, 128)))[None, None]
    out = ops.run_model(ops.make_model(cfg, sd), ref)
    assert out["i_ids"].numel() > 0
    for k in ("i_ids", "j_ids", "mconf", "mkpts_query_f"):
        assert torch.equal(r["data"][k], out[k]), k
    assert r["source"] == "given" and r["pose"].shape == (3, 4) and isinstance(r["state"], bool)
