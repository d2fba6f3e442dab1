"""The estimator of the 2D detector at the reference's size: 15 views of 2000 matches (30 % outliers, 0.5 px noise, threshold 6 px),
2000 hypotheses, `confidence` 0.99 and 1.0.
  device   one `estimate_affine_2d_batch` call on device tensors (`opp_affine2d_ransac_batch`, csrc/affine.hip): HIP-event time
           from before the call to after its last kernel, one warm-up call, then the median of --reps calls; and the wall-clock
           time of the same call with a synchronise behind it;
  host     the wall-clock time of the float64 numpy restatement (tests/affine_reference.py) of the same 15 views, one pass.  It is
           not OpenCV, which is not installed here: the reference's 15 `cv2.estimateAffine2D` calls are not measured.
The numbers are recorded; nothing is asserted.  With --parity the case list of tests/affine_cases.py runs through the device and
the restatement and the largest displacement of an image corner between their final maps is written as well.
    python tools/affine_bench.py [--reps 30] [--out profiles/affine_bench.txt] [--parity profiles/affine_parity.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from onepose_plus_plus_amd import estimate_affine_2d_batch  # noqa: E402
from tests import affine_cases as AC  # noqa: E402
from tests import affine_reference as AR  # noqa: E402


def _write(path, text):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


def bench(a):
    V, n, iters = a.views, a.matches, a.iterations
    scenes = [AC.scene(300 + v, n, 0.3) for v in range(V)]
    p0 = torch.from_numpy(np.concatenate([s[0] for s in scenes])).cuda()
    p1 = torch.from_numpy(np.concatenate([s[1] for s in scenes])).cuda()
    off = torch.arange(V + 1, dtype=torch.int32).cuda() * n
    corners = torch.from_numpy(np.tile(AC.corners_of(AC.REF_HW), (V, 1, 1))).cuda()
    seeds = list(range(1, V + 1))
    lines = ["%d views of %d matches, 30 %% outliers, %d hypotheses, threshold %g px; %s; device: median of %d calls after a warm-up" %
             (V, n, iters, AC.THR, torch.cuda.get_device_name(0), a.reps),
             "| confidence | device event ms | device wall ms (call + synchronise) | stop index min / max | numpy restatement wall ms | same best view |",
             "|---|---|---|---|---|---|"]
    for conf in (0.99, 1.0):
        def call():
            return estimate_affine_2d_batch(p0, p1, offsets=off, corners=corners, ransac_reproj_threshold=AC.THR, max_iters=iters,
                                            confidence=conf, seed=seeds, fallback_box=AC.FALLBACK)
        call()
        torch.cuda.synchronize()
        ev, wall = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            r = call()
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
        stop = r["stop"].cpu().numpy()
        t0 = time.perf_counter()
        _, best_view, _, _ = AR.estimate_batch([(s[0], s[1]) for s in scenes], seeds, iters, AC.THR, conf, True, corners.cpu().numpy(), AC.FALLBACK)
        host_ms = (time.perf_counter() - t0) * 1e3
        lines.append("| %g | %.3f | %.3f | %d / %d | %.1f | %s |" % (conf, np.median(ev), np.median(wall), stop.min(), stop.max(), host_ms,
                                                                     "yes" if int(r["best_view"][0]) == best_view else "NO"))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        _write(a.out, text)


def parity(path):
    from tests.test_affine_gpu import compare_groups, corner_gap
    rows = compare_groups(AC.GPU_CASES)
    lines = ["final affine map, device against the float64 restatement: largest displacement of an image corner (640 x 480), px; %s" %
             torch.cuda.get_device_name(0),
             "| n | outliers | iterations | confidence | inliers | condition number | corner displacement px |", "|---|---|---|---|---|---|---|"]
    worst, undecided = 0.0, 0
    for r in rows:
        ref, dev = r["ref"], r["dev"]
        undecided += bool(ref["undecided"])
        if ref["undecided"] or not ref["ok"]:
            continue
        cond = ref["cond"] if ref["cond"] is not None else ref["sample_cond"]
        gap = corner_gap(dev["affine"], ref["affine"])
        worst = max(worst, gap) if cond <= 1e3 else worst
        lines.append("| %d | %g | %d | %g | %d | %.3g%s | %.3e |" % (r["case"][0], r["case"][1], r["case"][2], r["case"][3], ref["n_inliers"], cond,
                                                                   "" if ref["cond"] is not None else " (sample, no refit)", gap))
    lines.append("largest over the cases with a condition number <= 1e3: %.3e px (bar 1e-6 px); undecided cases: %d of %d" %
                 (worst, undecided, len(rows)))
    text = "\n".join(lines) + "\n"
    print(text)
    _write(path, text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--views", type=int, default=15)
    ap.add_argument("--matches", type=int, default=2000)
    ap.add_argument("--iterations", type=int, default=2000)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--parity", default=None, help="write the parity table of the test case list to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("affine_bench needs a GPU: there is nothing to measure without one")
    bench(a)
    if a.parity:
        parity(a.parity)


if __name__ == "__main__":
    main()
