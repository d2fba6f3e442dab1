"""Per-frame time of the tracking loop (onepose_plus_plus_amd/tracking.py) on one 1920 x 1440 8-bit frame stream: upload, crop,
forward, PnP.  Random weights, a synthetic 5000-point bank, crop 512 x 512.

  upload / crop / forward   HIP events around each stage's enqueue on the current stream (pinned host frame -> device; opp_crop_warp_u8
                            with its box upload; OnePosePlus_model on the resident bank), read after the frame's synchronize
  pnp                       wall clock of `ransac_PnP` (it ends with the D2H copy of the pose, so it is synchronous) with the demo's
                            arguments.  Random weights give no usable matches, so the matches handed to PnP are PLANTED: --matches
                            projections of bank points under a slowly moving pose, 0.5 px Gaussian noise, 20 % outliers, on the device
  step                      wall clock of `PoseTracker.step` as a whole (same forward, same planted matches, box from the previous pose)
  crop / ingest launches    the crop kernel beside ingest_u8_kernel (1920 x 1440 -> 512 x 384) on the same device-resident frame:
                            --launches back-to-back launches between two events, divided by their number

Medians over --frames frames after --warmup.  Prints a table and one JSON line.
    python tools/track_probe.py [--frames 20] [--warmup 3] [--matches 600] [--launches 50]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from onepose_plus_plus_amd import OnePosePlus_model, PoseTracker, box_from_pose, crop_by_box, default_config  # noqa: E402
from onepose_plus_plus_amd import _lib, ingest  # noqa: E402
from onepose_plus_plus_amd.bank import ObjectBank  # noqa: E402
from onepose_plus_plus_amd.pose import ransac_PnP  # noqa: E402
from onepose_plus_plus_amd.synthetic import make_inputs, make_state_dict  # noqa: E402

H, W, S = 1920, 1440, 512


class PlantedAfterForward:
    """the real forward, then the planted matches in place of the (random-weight) ones"""

    def __init__(self, model, pts3d, n, rng):
        self.model, self.pts3d, self.n, self.rng, self.pose = model, pts3d, n, rng, None

    def plant(self, K_crop):
        idx = self.rng.choice(len(self.pts3d), self.n, replace=False)
        X = self.pts3d[idx]
        cam = X @ self.pose[:, :3].T + self.pose[:, 3]
        uv = cam @ np.asarray(K_crop).T
        uv = uv[:, :2] / uv[:, 2:] + self.rng.normal(0, 0.5, (self.n, 2))
        out = self.rng.random(self.n) < 0.2
        uv[out] = self.rng.uniform(0, S, (int(out.sum()), 2))
        return torch.from_numpy(uv.astype(np.float32)).cuda(), torch.from_numpy(X.astype(np.float32)).cuda()

    def __call__(self, data):
        self.model(data)
        data["mkpts_query_f"], data["mkpts_3d_db"] = self.plant(data["K_crop"])
        return data


def pose_at(i):
    th = 0.3 + 0.01 * i
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    return np.concatenate([R, np.array([[0.002 * i], [-0.001 * i], [0.55 + 0.003 * i]])], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--matches", type=int, default=600)
    ap.add_argument("--launches", type=int, default=50)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    cfg = default_config()
    model = OnePosePlus_model(cfg).eval()
    model.load_state_dict(make_state_dict(cfg, 0), strict=True)
    model = model.cuda()
    base = make_inputs(5000, (S, S), 3)
    pts3d = base["keypoints3d"][0].double().numpy() * 0.2                  # a 20 cm object
    bank = ObjectBank(pts3d, base["descriptors3d_db"][0], base["descriptors3d_coarse_db"][0])
    bbox3d = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) * 0.1
    K = np.array([[1480.0, 0, W / 2.0], [0, 1480.0, H / 2.0], [0, 0, 1]])
    n_total = a.warmup + a.frames
    frames = [torch.from_numpy(rng.integers(0, 256, (H, W), dtype=np.uint8)).pin_memory() for _ in range(4)]
    matcher = PlantedAfterForward(model, pts3d, a.matches, rng)
    pnp_kwargs = dict(scale=1000, pnp_reprojection_error=7, img_hw=[S, S], use_pycolmap_ransac=True, solver="auto")

    # stage by stage
    rows = {"upload": [], "crop": [], "forward": [], "pnp": []}
    pose = pose_at(0)
    inliers = []
    for i in range(n_total):
        box, valid = box_from_pose(K, pose, bbox3d)
        assert valid
        matcher.pose = pose_at(i)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        dev = frames[i % 4].to("cuda", non_blocking=True)
        ev[1].record()
        crop, K_crop = crop_by_box(dev, box, K, S)
        ev[2].record()
        data = bank.data(crop, K_crop=K_crop[0], bbox=box)
        with torch.no_grad():
            model(data)
        ev[3].record()
        torch.cuda.synchronize()
        p2, p3 = matcher.plant(K_crop[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pose, _, inl, state = ransac_PnP(K_crop[0], p2, p3, **pnp_kwargs)
        t_pnp = (time.perf_counter() - t0) * 1e3
        assert state
        if i >= a.warmup:
            rows["upload"].append(ev[0].elapsed_time(ev[1]))
            rows["crop"].append(ev[1].elapsed_time(ev[2]))
            rows["forward"].append(ev[2].elapsed_time(ev[3]))
            rows["pnp"].append(t_pnp)
            inliers.append(len(inl))

    # the whole step
    tracker = PoseTracker(matcher, bank, K, bbox3d, detector=lambda f, k: box_from_pose(K, pose_at(0), bbox3d)[0], crop_size=S)
    step_ms, sources = [], []
    for i in range(n_total):
        matcher.pose = pose_at(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = tracker.step(frames[i % 4])
        torch.cuda.synchronize()
        if i >= a.warmup:
            step_ms.append((time.perf_counter() - t0) * 1e3)
            sources.append(r["source"])

    # crop kernel beside the ingest kernel, launches only
    lib = _lib.load()
    dev = frames[0].cuda()
    box, _ = box_from_pose(K, pose_at(0), bbox3d)
    launch_us = {}
    box = np.ascontiguousarray(box, np.int32)
    box_dev = torch.from_numpy(box).cuda()
    box_host = box.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    out = torch.empty(S, S, dtype=torch.float32, device="cuda")
    w_new, h_new = ingest.process_resize(W, H, [S], 8)
    st = torch.cuda.current_stream().cuda_stream
    for name, fn in (("crop_warp_u8_kernel", lambda: lib.opp_crop_warp_u8(dev.data_ptr(), H, W, W, box_dev.data_ptr(), box_host, 1, S,
                                                                          out.data_ptr(), None, st)),
                     ("ingest_u8_kernel", lambda: lib.opp_image_ingest_u8(dev.data_ptr(), H, W, W, h_new, w_new, out.data_ptr(), w_new,
                                                                          None, st))):
        _lib.check(fn(), name)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        launch_us[name] = e0.elapsed_time(e1) * 1e3 / a.launches

    med = {k: float(np.median(v)) for k, v in rows.items()}
    print("| stage | median ms over %d frames |" % a.frames)
    print("|---|---|")
    for k in ("upload", "crop", "forward", "pnp"):
        print("| %s | %.3f |" % (k, med[k]))
    print("| PoseTracker.step (wall) | %.3f |" % float(np.median(step_ms)))
    for k, v in launch_us.items():
        print("| %s, us per launch | %.1f |" % (k, v))
    print(json.dumps({"frame_hw": [H, W], "crop_size": S, "frames": a.frames, "warmup": a.warmup, "matches": a.matches,
                      "median_ms": med, "step_wall_ms": float(np.median(step_ms)), "launch_us": launch_us,
                      "box_wh": [int(box[2] - box[0]), int(box[3] - box[1])], "median_inliers": float(np.median(inliers)),
                      "sources": sorted(set(sources))}))


if __name__ == "__main__":
    main()
