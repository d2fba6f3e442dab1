"""The LO-RANSAC pose step of a batch, per-sample loop against one batched pass: B samples of 300 matches, 40 % outliers, 0.5 px
noise, threshold 3.3 px, the estimator's defaults (10000 trials cap, min_trials 1000, confidence 0.9999), B = 8, 1 and 32.
  (a) the loop compute_query_pose_errors runs for "loransac": per sample `m_bids == b` selects the matches and one
      `pose.ransac_PnP_ex(solver="loransac")` call estimates the pose (its own workspace, launches and blocking copies);
  (b) one `pose.loransac_PnP_batch` call on the same device tensors.
Timed as in tools/pnp_batch_bench.py (whole Python calls with their host syncs, wall clock and HIP events, the two alternating,
medians of --reps after a warm-up of each); host syncs are counted in one extra, untimed call of each.  One process, one GPU.
    python tools/pnp_lo_batch_bench.py [--reps 20] [--out FILE]
    python tools/pnp_lo_batch_bench.py --one-call            # a warm-up and ONE batch call at --batch: the span a kernel trace covers
    python tools/pnp_lo_batch_bench.py --trace-csv FILE      # per-kernel sums of a kernel-trace CSV of such a run (no GPU)"""
import argparse
import csv
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def trace_table(path):
    """the LO-RANSAC launches of the LAST batch call in a kernel-trace CSV (columns Kernel_Name, Start_Timestamp, End_Timestamp,
    Grid_Size_X / _Y), i.e. those from the last `pnp_offsets_kernel` on, in launch order: kernel, grid in threads, microseconds"""
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    last = max((i for i, r in enumerate(rows) if "pnp_offsets_kernel" in r["Kernel_Name"]), default=0)
    lines = ["| # | kernel | grid (threads) | us |", "|---|---|---|---|"]
    total = 0.0
    for k, r in enumerate(rows[last:]):
        m = re.search(r"(\w+_kernel)\b", r["Kernel_Name"])
        name = m.group(1) if m else r["Kernel_Name"]
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "loransac_batch" in name or "pnp_offsets" in name:
            total += us
            lines.append("| %d | %s | %s x %s | %.1f |" % (k, name, r.get("Grid_Size_X", "?"), r.get("Grid_Size_Y", "?"), us))
    lines.append("| | sum of the LO-RANSAC kernels | | %.1f |" % total)
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--matches", type=int, default=300)
    ap.add_argument("--iterations", type=int, default=10000)
    ap.add_argument("--one-call", action="store_true")
    ap.add_argument("--trace-csv", default=None)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if a.trace_csv:
        print(trace_table(a.trace_csv))
        return
    import torch
    from onepose_plus_plus_amd import pose
    from tools.pnp_batch_bench import SyncCounter, measure_pair
    from tools.pnp_bench import scene

    n = a.matches
    kw = dict(pnp_reprojection_error=3.3, iterations=a.iterations, seed=1)

    def inputs(B):
        rng = np.random.default_rng(0)
        Ks, uvs, Xs = [], [], []
        for _ in range(B):
            K4, uv, X = scene(rng, n, 0.4)
            Ks.append(np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]]))
            uvs.append(uv)
            Xs.append(X)
        return (np.stack(Ks), torch.from_numpy(np.concatenate(uvs)).float().cuda().contiguous(),
                torch.from_numpy(np.concatenate(Xs)).float().cuda().contiguous(), torch.from_numpy(np.repeat(np.arange(B), n)).cuda())

    if a.one_call:
        K, p2, p3, ids = inputs(a.batch)
        pose.loransac_PnP_batch(K, p2, p3, m_bids=ids, **kw)
        torch.cuda.synchronize()
        r = pose.loransac_PnP_batch(K, p2, p3, m_bids=ids, **kw)
        print("one loransac_PnP_batch call, B = %d: stops %s" % (a.batch, r["stop"].tolist()))
        return
    lines = ["samples of %d matches, 40 %% outliers, cap %d trials, the estimator's defaults; %s; median of %d after a warm-up" %
             (n, a.iterations, torch.cuda.get_device_name(0), a.reps),
             "| B | loop wall ms | batch wall ms | wall ratio | loop event ms | batch event ms | event ratio | loop syncs | batch syncs | same bytes | stops |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for B in (a.batch, 1, 32):
        K, p2, p3, ids = inputs(B)

        def loop():
            out = []
            for b in range(B):
                m = ids == b
                out.append(pose.ransac_PnP_ex(K[b], p2[m], p3[m], solver="loransac", **kw))
            return out

        def batch():
            return pose.loransac_PnP_batch(K, p2, p3, m_bids=ids, **kw)

        (lw, le), (bw, be) = measure_pair(loop, batch, a.reps)
        with SyncCounter() as c:
            ref = loop()
        loop_syncs = c.n
        with SyncCounter() as c:
            got = batch()
        same = all(got["pose"][b].tobytes() == ref[b]["pose"].tobytes() and int(got["stop"][b]) == ref[b]["stop"] and
                   np.array_equal(got["inliers"][b][:, 0], ref[b]["inliers"]) for b in range(B))
        stops = sorted(set(got["stop"].tolist()))
        lines.append("| %d | %.3f | %.3f | %.2f | %.3f | %.3f | %.2f | %d | %d | %s | %s |" %
                     (B, lw, bw, lw / bw, le, be, le / be, loop_syncs, c.n, "yes" if same else "NO",
                      "%d..%d" % (stops[0], stops[-1]) if len(stops) > 1 else str(stops[0])))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
