"""Pose-step device time per solver: opp_pnp_ransac_ex (csrc/pnp.hip) on synthetic scenes at n = 300 / 1000 / 3000 matches and
0 / 50 / 70 % outliers, 10000 hypotheses, adaptive stop on (confidence 0.99) and off.  Times with HIP events around the launches
(inputs already on the device), median of --reps after one warm-up.
    python tools/pnp_bench.py [--reps 5]
    python tools/pnp_bench.py --loransac     # opp_pnp_loransac (csrc/pnp_lo.hip) beside solver "epnp": n = 300 / 1500, 50 % outliers"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from onepose_plus_plus_amd import _lib  # noqa: E402


def scene(rng, n, outl):
    K4 = np.array([560.0, 555.0, 256.0, 250.0])
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    X = rng.uniform(-0.15, 0.15, size=(n, 3))
    t = np.array([0.01, -0.02, 0.8])
    Xc = X @ R.T + t
    uv = np.stack([K4[0] * Xc[:, 0] / Xc[:, 2] + K4[2], K4[1] * Xc[:, 1] / Xc[:, 2] + K4[3]], 1) + rng.normal(size=(n, 2)) * 0.5
    k = int(outl * n)
    uv[rng.choice(n, k, replace=False)] = rng.uniform(0, 512, size=(k, 2))
    return K4, uv, X


def _time(call, reps):
    times = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def loransac_rows(lib, a):
    """the same call with the two estimators of the reference, each with its own defaults (epnp: confidence 0.99; loransac:
    confidence 0.9999, min_trials 1000, SIMPLE_PINHOLE, no scale)"""
    rng = np.random.default_rng(0)
    s = torch.cuda.current_stream().cuda_stream
    print("| n | outliers | solver | stop index | inliers | device ms |")
    print("|---|---|---|---|---|---|")
    for n in (300, 1500):
        K4n, uv, X = scene(rng, n, 0.5)
        p2 = torch.from_numpy(uv).float().cuda().contiguous()
        p3 = torch.from_numpy(X).float().cuda().contiguous()
        out = torch.empty(12, dtype=torch.float64, device="cuda")
        mask = torch.empty(n, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(3, dtype=torch.int32, device="cuda")
        K4 = (ctypes.c_double * 4)(*K4n)
        nb = lib.opp_pnp_ex_workspace_bytes(a.iterations, n)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        ms = _time(lambda: _lib.check(lib.opp_pnp_ransac_ex(p2.data_ptr(), p3.data_ptr(), n, K4, 3.3, 1000.0, a.iterations, 1, 8, 1, 0.99,
                                                            out.data_ptr(), mask.data_ptr(), cnt.data_ptr(), cnt.data_ptr() + 4,
                                                            cnt.data_ptr() + 8, None, None, ws.data_ptr(), nb, s), "pnp_ex"), a.reps)
        c = cnt.cpu().numpy()
        print("| %d | 50 %% | epnp | %d | %d | %.3f |" % (n, c[2], c[0], ms), flush=True)
        K4 = (ctypes.c_double * 4)(K4n[0], K4n[0], K4n[2], K4n[3])
        nb = lib.opp_pnp_loransac_workspace_bytes(a.iterations, n)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        ms = _time(lambda: _lib.check(lib.opp_pnp_loransac(p2.data_ptr(), p3.data_ptr(), n, K4, 3.3, a.iterations, 1, 0.9999, 1000, 0.01,
                                                           out.data_ptr(), mask.data_ptr(), cnt.data_ptr(), cnt.data_ptr() + 4,
                                                           cnt.data_ptr() + 8, None, ws.data_ptr(), nb, s), "pnp_loransac"), a.reps)
        c = cnt.cpu().numpy()
        print("| %d | 50 %% | loransac | %d | %d | %.3f |" % (n, c[2], c[0], ms), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=10000)
    ap.add_argument("--loransac", action="store_true")
    a = ap.parse_args()
    lib = _lib.load()
    if a.loransac:
        return loransac_rows(lib, a)
    rng = np.random.default_rng(0)
    s = torch.cuda.current_stream().cuda_stream
    print("| n | outliers | solver | confidence | stop index | inliers | device ms |")
    print("|---|---|---|---|---|---|---|")
    for n in (300, 1000, 3000):
        for outl in (0.0, 0.5, 0.7):
            K4n, uv, X = scene(rng, n, outl)
            p2 = torch.from_numpy(uv).float().cuda().contiguous()
            p3 = torch.from_numpy(X).float().cuda().contiguous()
            K4 = (ctypes.c_double * 4)(*K4n)
            nb = lib.opp_pnp_ex_workspace_bytes(a.iterations, n)
            ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
            out = torch.empty(12, dtype=torch.float64, device="cuda")
            mask = torch.empty(n, dtype=torch.int32, device="cuda")
            cnt = torch.zeros(3, dtype=torch.int32, device="cuda")
            for solver, name in ((0, "p3p"), (1, "epnp")):
                for conf in (0.99, 1.0):
                    times = []
                    for r in range(a.reps + 1):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        _lib.check(lib.opp_pnp_ransac_ex(p2.data_ptr(), p3.data_ptr(), n, K4, 3.3, 1000.0, a.iterations, 1, 8, solver,
                                                         conf, out.data_ptr(), mask.data_ptr(), cnt.data_ptr(), cnt.data_ptr() + 4,
                                                         cnt.data_ptr() + 8, None, None, ws.data_ptr(), nb, s), "pnp_ex")
                        e1.record()
                        torch.cuda.synchronize()
                        if r:
                            times.append(e0.elapsed_time(e1))
                    c = cnt.cpu().numpy()
                    print("| %d | %d %% | %s | %s | %d | %d | %.3f |" % (n, round(outl * 100), name, "0.99" if conf < 1 else "off", c[2], c[0],
                                                                      float(np.median(times))), flush=True)


if __name__ == "__main__":
    main()
