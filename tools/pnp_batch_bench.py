"""The pose step of a batch, per-sample loop against one batched pass: B = 8 samples of 300 matches, 40 % outliers, 0.5 px noise,
threshold 3.3 px, 10000 hypotheses, solvers "p3p" and "epnp", `confidence` at the solver's default and at 1.0.
  (a) the loop compute_query_pose_errors ran before the batch pass: per sample `m_bids == b` selects the matches and one
      `pose.ransac_PnP_ex` call estimates the pose (its own workspace, launches, and two blocking device-to-host copies);
  (b) one `pose.ransac_PnP_batch` call on the same device tensors.
Both are whole Python calls, host synchronisation included, because that is what (b) removes: wall-clock time from a
synchronised start to the last result on the host, and the HIP-event time over the same span; one warm-up call of each, then
the medians of --reps calls of each, the two alternating.  Host syncs are counted in one extra, untimed call of each:
`Tensor.cpu()`, `torch.nonzero` and boolean-mask indexing each block the host once.  One process, one GPU.
    python tools/pnp_batch_bench.py [--reps 20] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from onepose_plus_plus_amd import pose  # noqa: E402
from tools.pnp_bench import scene  # noqa: E402


class SyncCounter:
    """counts the calls that block the host while it is active"""

    def __enter__(self):
        self.n = 0
        self._cpu, self._nonzero, self._getitem = torch.Tensor.cpu, torch.nonzero, torch.Tensor.__getitem__

        def cpu(t, *a, **k):
            self.n += 1 if t.is_cuda else 0
            return self._cpu(t, *a, **k)

        def nonzero(t, *a, **k):
            self.n += 1 if t.is_cuda else 0
            return self._nonzero(t, *a, **k)

        def getitem(t, idx):
            self.n += 1 if torch.is_tensor(idx) and idx.dtype == torch.bool and idx.is_cuda else 0
            return self._getitem(t, idx)

        torch.Tensor.cpu, torch.nonzero, torch.Tensor.__getitem__ = cpu, nonzero, getitem
        return self

    def __exit__(self, *exc):
        torch.Tensor.cpu, torch.nonzero, torch.Tensor.__getitem__ = self._cpu, self._nonzero, self._getitem


def _once(call):
    """-> (wall ms, event ms) of one `call`, which returns with its results on the host"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)


def measure_pair(a, b, reps):
    """medians (wall ms, event ms) of `a` and of `b`, the two alternating so that both see the same machine"""
    a()
    b()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(_once(a))
        tb.append(_once(b))
    return tuple(np.median(np.array(ta), axis=0)), tuple(np.median(np.array(tb), axis=0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--matches", type=int, default=300)
    ap.add_argument("--iterations", type=int, default=10000)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    B, n = a.batch, a.matches
    Ks, uvs, Xs = [], [], []
    for _ in range(B):
        K4, uv, X = scene(rng, n, 0.4)
        Ks.append(np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]]))
        uvs.append(uv)
        Xs.append(X)
    K = np.stack(Ks)
    p2 = torch.from_numpy(np.concatenate(uvs)).float().cuda().contiguous()
    p3 = torch.from_numpy(np.concatenate(Xs)).float().cuda().contiguous()
    ids = torch.from_numpy(np.repeat(np.arange(B), n)).cuda()
    kw = dict(scale=1000, pnp_reprojection_error=3.3, iterations=a.iterations, seed=1)
    lines = ["B = %d samples of %d matches, 40 %% outliers, %d hypotheses; %s; median of %d after a warm-up" %
             (B, n, a.iterations, torch.cuda.get_device_name(0), a.reps),
             "| solver | confidence | loop wall ms | batch wall ms | wall ratio | loop event ms | batch event ms | event ratio | loop syncs | batch syncs | same poses |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for solver in ("p3p", "epnp"):
        for conf in (None, 1.0):
            def loop():
                out = []
                for b in range(B):
                    m = ids == b
                    out.append(pose.ransac_PnP_ex(K[b], p2[m], p3[m], solver=solver, confidence=conf, **kw))
                return out

            def batch():
                return pose.ransac_PnP_batch(K, p2, p3, m_bids=ids, solver=solver, confidence=conf, **kw)

            (lw, le), (bw, be) = measure_pair(loop, batch, a.reps)
            with SyncCounter() as c:
                ref = loop()
            loop_syncs = c.n
            with SyncCounter() as c:
                got = batch()
            same = all(got["pose"][b].tobytes() == ref[b]["pose"].tobytes() for b in range(B))
            name = "default (%s)" % ("0.99" if solver == "epnp" else "off") if conf is None else "1.0"
            lines.append("| %s | %s | %.3f | %.3f | %.2f | %.3f | %.3f | %.2f | %d | %d | %s |" %
                         (solver, name, lw, bw, lw / bw, le, be, le / be, loop_syncs, c.n, "yes" if same else "NO"))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
