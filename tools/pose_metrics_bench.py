"""Device time of the pose metrics: opp_pose_metrics (csrc/pose_metrics.hip) at P = 1000 / 5000 / 20000 model vertices, B = 1 / 8
poses, ADD (syn off) and ADD-S (syn on, every pose), 2D error included.  HIP events around the enqueue (inputs and workspace already
on the device), median of --reps after one warm-up.  Beside each row, as information: the wall time of the numpy restatement
(tests/pose_metrics_reference.py: brute-force nearest neighbour, one thread pool of numpy's own) for ONE pose on the same host.
    python tools/pose_metrics_bench.py [--reps 5] [--no-host]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from onepose_plus_plus_amd import _lib  # noqa: E402
from tests import pose_metrics_reference as R  # noqa: E402
from tests.golden import pose_metrics_cases as C  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    lib = _lib.load()
    rng = np.random.default_rng(0)
    s = torch.cuda.current_stream().cuda_stream
    print("| P | B | syn | device ms | numpy restatement, one pose, ms |")
    print("|---|---|---|---|---|")
    for P in (1000, 5000, 20000):
        model = C.vertices(P, rng)
        gt = C.gt_pose(rng)
        pred = C.perturbed(gt, "small", rng)
        K = C.intrinsics()
        pts = torch.from_numpy(model).cuda()
        for syn in (0, 1):
            host_ms = float("nan")
            if not a.no_host:
                t0 = time.perf_counter()
                R.score(model, pred, gt, K, bool(syn))
                host_ms = (time.perf_counter() - t0) * 1e3
            for B in (1, 8):
                pp = torch.from_numpy(np.stack([pred] * B)).cuda()
                pg = torch.from_numpy(np.stack([gt] * B)).cuda()
                kd = torch.from_numpy(np.stack([K] * B)).cuda()
                sd = torch.ones(B, dtype=torch.uint8, device="cuda") if syn else None
                out = torch.empty((B, 4), dtype=torch.float64, device="cuda")
                nb = lib.opp_pose_metrics_workspace_bytes(B, P)
                ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
                times = []
                for r in range(a.reps + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    _lib.check(lib.opp_pose_metrics(pts.data_ptr(), P, pp.data_ptr(), pg.data_ptr(), kd.data_ptr(),
                                                    sd.data_ptr() if syn else None, None, B, 100.0, out.data_ptr(), ws.data_ptr(), nb, s),
                               "opp_pose_metrics")
                    e1.record()
                    torch.cuda.synchronize()
                    if r:
                        times.append(e0.elapsed_time(e1))
                print("| %d | %d | %s | %.3f | %.1f |" % (P, B, "on" if syn else "off", float(np.median(times)), host_ms), flush=True)


if __name__ == "__main__":
    main()
