"""What building one training batch costs: 4 samples of 512 x 512, an object of 9000 points cut to shape3d = 7000, k = 1500 pairs over
2000 2D keypoints -- without warp and with every sample warped:

  (a) onepose_plus_plus_amd.train_sample.make_train_batch: annotation arrays and the device-resident image in, everything made on the
      device (csrc/train_sample.hip + opp_build_assignmatrix).  Per batch: wall time of the call up to a device synchronisation (it
      contains the host's index bookkeeping and the uploads of the descriptor banks) and the device span between two events.
  (b) the host restatement of the reference's loader code (tests/train_sample_reference.py: torch / numpy on the CPU threads torch is
      given, the warp through F.grid_sample) followed by the upload of the collated batch, as a training loop on the reference has
      to do it: wall time up to the synchronisation.

Medians of `--steps` batches after `--warmup`.  The numbers are recorded, not asserted: this is HBM-bound byte work and a few thousand
items of index logic; the point of the module is a complete device-resident sample builder, not a kernel speed-up.

    python tools/train_sample_bench.py [--steps 10] [--warmup 3] [--out profiles/train_sample_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HW, N_OBJECT, SHAPE3D, K_PAIRS, N2D, BATCH = (512, 512), 9000, 7000, 1500, 2000, 4


def median(xs):
    return sorted(xs)[len(xs) // 2]


def time_device_batch(samples, dev, steps, warmup):
    from onepose_plus_plus_amd.train_sample import make_train_batch
    wall, pairs = [], []
    for i in range(warmup + steps):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        batch = make_train_batch(samples)
        e1.record()
        torch.cuda.synchronize(dev)
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
            pairs.append(e0.elapsed_time(e1))
    return median(wall), median(pairs), batch


def time_host_batch(inputs, dev, steps, warmup):
    from tests import train_sample_reference as TR
    keys = ("query_image", "keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db", "scores3d_db", "conf_matrix_gt", "fine_location_matrix_gt")
    build, total = [], []
    for i in range(warmup + steps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        outs = [TR.read_anno_train(inp, diagnostics=False) for inp in inputs]
        host = {k: torch.stack([o[k] for o in outs]) for k in keys}
        t1 = time.perf_counter()
        batch = {k: v.to(dev) for k, v in host.items()}
        torch.cuda.synchronize(dev)
        if i >= warmup:
            build.append((t1 - t0) * 1e3)
            total.append((time.perf_counter() - t0) * 1e3)
    return median(build), median(total), batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_sample_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_sample_bench measures on the GPU: no device found")
    from tests import train_sample_reference as TR
    dev = torch.device("cuda:0")
    lines = ["device: %s, torch %s, %d CPU threads for the host restatement" % (torch.cuda.get_device_name(dev), torch.__version__, torch.get_num_threads()),
             "batch: %d samples of %d x %d, object of %d points -> shape3d %d, k = %d pairs over %d 2D keypoints; medians of %d batches after %d" %
             (BATCH, HW[0], HW[1], N_OBJECT, SHAPE3D, K_PAIRS, N2D, args.steps, args.warmup)]
    for warp in (False, True):
        inputs = [TR.make_inputs(HW, N_OBJECT, SHAPE3D, K_PAIRS, N2D, warp, 70 + b, 700 + b, 3 + b, fine_dim=128, coarse_dim=256) for b in range(BATCH)]
        samples = []
        for inp in inputs:
            homo = None
            if warp:
                np.random.seed(inp["np_seed"])
                homo = TR.sample_homography_sap(*HW)
            samples.append(dict(query_image=inp["query_image"].to(dev), keypoints3d=inp["keypoints3d"], descriptors3d=inp["descriptors3d"],
                                scores3d=inp["scores3d"], coarse_descriptors3d=inp["coarse_descriptors3d"], assign_matrix=inp["assign_matrix"],
                                keypoints2d_coarse=inp["keypoints2d_coarse"], pose_gt=inp["pose_gt"], K_crop=inp["K_crop"],
                                query_img_scale=inp["query_img_scale"], warp=warp, homography=homo, shape3d=SHAPE3D))
        wall, span, dbatch = time_device_batch(samples, dev, args.steps, args.warmup)
        build, total, hbatch = time_host_batch(inputs, dev, args.steps, args.warmup)
        kept = [int(v) for v in dbatch["n_pairs"].flatten()]
        ones = [int(v) for v in hbatch["conf_matrix_gt"].sum((1, 2))]
        lines += ["", "warp = %s   (pairs kept per sample: (a) %s, (b) %s)" % (warp, kept, ones),
                  "  (a) make_train_batch on the device:      %8.2f ms wall to synchronisation, %8.2f ms device span" % (wall, span),
                  "  (b) host restatement + upload:           %8.2f ms wall to synchronisation (%8.2f ms building on the CPU, the rest uploading "
                  "%.0f MB)" % (total, build, sum(v.numel() * v.element_size() for v in hbatch.values()) / 1e6)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
