"""What the close-point merge of the SfM post-processing costs (filter_points.merge, run.py:363) on the clustered cloud of
tests/golden/pointcloud_cases.py (isolated seeds, satellites, chains; threshold 1e-3) at n = 2 000 and n = 15 000 -- every shipped
`max_num_kp3d` is 10 000 or 15 000:

  (a) `pointcloud.merge`: host arrays in, the reference's return values out (upload, five launches, two read-backs, download,
      the {cluster: ids} dictionary) -- host clock around the call, which ends in a device-to-host copy;
  (b) `pointcloud.merge_csr` on points already on the device -- host clock around the call + a synchronise;
  (c) the kernels alone, each between one pair of events (pair count, pair fill, selection, emit), with the pair tests per second of the
      two search passes (n^2 tests each);
  (d) the float64 numpy restatement of tests/pointcloud_reference.py on the host of the same run (one run: it takes seconds).

(a)-(c) are medians after warm-up.  The device result is compared with (d) bit for bit at both sizes before anything is printed.
The reference's own `merge` (scipy pdist + squareform + a Python row walk) was timed on the CPU of the build machine, not in this run:
0.82 s at n = 2 000 and 19.35 s at n = 15 000, where its distance matrix takes 1.8 GB; those two numbers are quoted below as given.

    python tools/pointcloud_bench.py [--reps 20] [--warmup 3] > profiles/pointcloud_bench.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REFERENCE_CPU_SECONDS = {2000: 0.82, 15000: 19.35}      # the reference's merge on the build machine's CPU (not measured here)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def time_host(fn, dev, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        out.append((time.perf_counter() - t0) * 1e3)
    return median(out), min(out), max(out)


def time_kernels(xyzs, ids, thr, dev, reps):
    """the five launches of merge_csr, one event pair each -> {name: median ms}, pairs, clusters"""
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    n = len(ids)
    pts = torch.from_numpy(xyzs).to(dev)
    idd = torch.from_numpy(ids).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.check(lib.opp_pc_neighbor_count(pts.data_ptr(), n, thr, counts.data_ptr(), stream), "opp_pc_neighbor_count")
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, dtype=torch.int64, out=offsets[1:])
    pairs = int(offsets[n].item())
    ws_bytes = int(lib.opp_pc_workspace_bytes(n, pairs))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    sel = torch.empty(n, dtype=torch.int32, device=dev)
    selcnt = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def count():
        _lib.check(lib.opp_pc_neighbor_count(pts.data_ptr(), n, thr, counts.data_ptr(), stream), "opp_pc_neighbor_count")

    def fill():
        _lib.check(lib.opp_pc_neighbor_fill(pts.data_ptr(), n, thr, offsets.data_ptr(), pairs, ws.data_ptr(), ws_bytes, stream), "opp_pc_neighbor_fill")

    def select():
        _lib.check(lib.opp_pc_select(offsets.data_ptr(), n, pairs, sel.data_ptr(), selcnt.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes,
                                     stream), "opp_pc_select")
    fill()
    select()
    rank = torch.cumsum(sel, 0, dtype=torch.int64)
    mem_end = torch.cumsum(selcnt, 0, dtype=torch.int64)
    n_clusters, n_members = int(rank[-1].item()), int(mem_end[-1].item())
    assert int(status.item()) == 0
    ret_points = torch.empty((n_clusters, 3), dtype=torch.float64, device=dev)
    cl_offsets = torch.zeros(n_clusters + 1, dtype=torch.int64, device=dev)
    members = torch.empty(n_members, dtype=torch.int64, device=dev)

    def emit():
        _lib.check(lib.opp_pc_emit(pts.data_ptr(), idd.data_ptr(), n, pairs, offsets.data_ptr(), sel.data_ptr(), rank.data_ptr(), mem_end.data_ptr(),
                                   n_clusters, n_members, ret_points.data_ptr(), cl_offsets.data_ptr(), members.data_ptr(), ws.data_ptr(), ws_bytes,
                                   stream), "opp_pc_emit")
    out = {}
    for name, fn in (("pc_neighbor_kernel<count>", count), ("pc_neighbor_kernel<fill>", fill), ("pc_select_kernel", select), ("pc_emit_kernel", emit)):
        fn()
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize(dev)
            ms.append(e0.elapsed_time(e1))
        out[name] = median(ms)
    return out, pairs, n_clusters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 15000])
    args = ap.parse_args()
    from onepose_plus_plus_amd import pointcloud as P
    from tests import pointcloud_reference as R
    from tests.golden import pointcloud_cases as C
    dev = torch.device("cuda:0")
    print("device: %s, torch %s" % (torch.cuda.get_device_name(dev), torch.__version__))
    print("cloud: tests/golden/pointcloud_cases.mixed_cloud(n, seed = n), dist_threshold %g; medians of %d after %d warm-up calls" %
          (C.THR, args.reps, args.warmup))
    for n in args.sizes:
        xyzs, ids = C.mixed_cloud(n, n)
        xyzs = np.ascontiguousarray(xyzs)
        t0 = time.perf_counter()
        want_points, want_idxs = R.merge(xyzs, ids, C.THR)
        host_s = time.perf_counter() - t0
        got_points, got_idxs = P.merge(xyzs, ids, C.THR)
        same = (got_points.shape == want_points.shape and np.array_equal(got_points.view(np.int64), want_points.view(np.int64))
                and all(np.array_equal(got_idxs[c], want_idxs[c]) for c in want_idxs))
        if not same:
            raise SystemExit("n = %d: the device result differs from the restatement" % n)
        d_pts, d_ids = torch.from_numpy(xyzs).to(dev), torch.from_numpy(ids).to(dev)
        a = time_host(lambda: P.merge(xyzs, ids, C.THR), dev, args.reps, args.warmup)
        b = time_host(lambda: P.merge_csr(d_pts, d_ids, C.THR), dev, args.reps, args.warmup)
        kernels, pairs, clusters = time_kernels(xyzs, ids, C.THR, dev, args.reps)
        multi = sum(len(v) > 1 for v in want_idxs.values())
        print("\nn = %d: %d pairs below the threshold (%.2f per point), %d clusters (%d multi-member); device result == restatement, bit for bit" %
              (n, pairs, pairs / n, clusters, multi))
        print("  %-64s %10.3f ms   (min %.3f, max %.3f)" % ("(a) pointcloud.merge, host arrays in, dictionary out", a[0], a[1], a[2]))
        print("  %-64s %10.3f ms   (min %.3f, max %.3f)" % ("(b) pointcloud.merge_csr, points on the device", b[0], b[1], b[2]))
        for name, ms in kernels.items():
            rate = "   %7.1f G pair tests/s" % (n * n / ms * 1e-6) if "neighbor" in name else ""
            print("  (c) %-60s %10.3f ms%s" % (name, ms, rate))
        print("  %-64s %10.1f ms" % ("(d) numpy restatement on this host, one run", host_s * 1e3))
        if n in REFERENCE_CPU_SECONDS:
            print("  %-64s %10.1f ms   (CPU of the build machine, not measured in this run)" %
                  ("    the reference's own merge (scipy pdist + Python walk)", REFERENCE_CPU_SECONDS[n] * 1e3))


if __name__ == "__main__":
    main()
