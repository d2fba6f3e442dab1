"""What one parameter update of the training step costs, on the real model's 144 parameter tensors (10.2 M floats) with random
gradients:

  (a) torch.nn.utils.clip_grad_norm_(0.5) + torch.optim.AdamW, foreach default -- what the reference's Lightning loop runs
  (b) the same with AdamW(fused=True), if torch constructs it on this device
  (c) onepose_plus_plus_amd.optim.FusedAdam(max_grad_norm=0.5): csrc/optim.hip, two launches

each with plain gradients (one tensor per parameter) and with `sharding.GradientAverager`'s flat views.  Per update: host wall
time of the call(s) (enqueue only: the device is idle when the call starts and is not waited for) and device time (an event
before and after, read after a synchronisation; for a host-bound variant this is the span its launches are spread over).  Then the
two kernels of (c) alone, back to back between one event pair, against the bytes the algorithm moves (norm: 4 n; update: reads
p, g, m, v and writes p, m, v = 28 n).  Back-to-back launches re-read a 286 MB working set, which exceeds the 256 MiB last-level cache
only just: the GB/s are an upper estimate of what a step between a backward pass and a forward pass sees.

    python tools/optim_bench.py [--steps 50] [--warmup 10] > profiles/optim_step_bench.txt
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_NORM = 0.5
HYPER = dict(lr=1e-6, weight_decay=0.1)          # train.yaml: AdamW, decay 0.1; a small lr keeps the 60 updates of a run harmless


def make_model(dev, flat):
    from onepose_plus_plus_amd import OnePosePlus_model, default_config
    from onepose_plus_plus_amd.sharding import GradientAverager
    from onepose_plus_plus_amd.synthetic import make_state_dict
    cfg = default_config(thr=0.2)
    model = OnePosePlus_model(cfg).to(dev)
    model.load_state_dict(make_state_dict(cfg, 0), strict=True)
    gen = torch.Generator(device=dev).manual_seed(7)
    if flat:
        avg = GradientAverager(model, sync_initial=False)
        avg.flat.copy_(torch.randn(avg.flat.numel(), generator=gen, device=dev) * 1e-2)
        assert avg.attached()
    else:
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=gen, device=dev) * 1e-2
    return model


def variants(model, flat):
    from onepose_plus_plus_amd.optim import FusedAdam
    params = list(model.parameters())
    out = []
    opt_a = torch.optim.AdamW(params, **HYPER)

    def step_a():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        opt_a.step()
    out.append(("(a) clip_grad_norm_ + torch AdamW (foreach)", step_a))
    try:
        opt_b = torch.optim.AdamW(params, fused=True, **HYPER)

        def step_b():
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
            opt_b.step()
        out.append(("(b) clip_grad_norm_ + torch AdamW (fused=True)", step_b))
    except Exception as e:                          # torch refuses the fused implementation on this device / build
        out.append(("(b) clip_grad_norm_ + torch AdamW (fused=True): not constructed (%s)" % str(e).splitlines()[0], None))
    opt_c = FusedAdam(params, decoupled=True, max_grad_norm=MAX_NORM, **HYPER)
    out.append(("(c) FusedAdam(max_grad_norm=0.5)", opt_c.step))
    if not flat:
        # gradients at other addresses in every step (what zero_grad(set_to_none=True) can lead to): the device tables are rebuilt
        sets = [[p.grad for p in params], [p.grad.clone() for p in params]]
        turn = [0]

        def step_c_moved():
            turn[0] ^= 1
            for p, g in zip(params, sets[turn[0]]):
                p.grad = g
            opt_c.step()
        out.append(("(c) FusedAdam, gradients moved: tables rebuilt", step_c_moved))
    return out, opt_c


def time_variant(fn, dev, steps, warmup):
    """-> (host ms, device ms) per update, medians"""
    for _ in range(warmup):
        fn()
    host, pairs = [], []
    for _ in range(steps):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t0) * 1e3)
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize(dev)
    device = sorted(a.elapsed_time(b) for a, b in pairs)
    return sorted(host)[len(host) // 2], device[len(device) // 2]


def time_kernels(opt, dev, n_floats, reps=20):
    """the two kernels of FusedAdam alone: `reps` launches back to back between one event pair"""
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    tb = opt._tables
    tensors, chunks, partials, n = tb["tensors"], tb["chunks"], tb["partials"].data_ptr(), tb["n_chunks"]
    stream = torch.cuda.current_stream(dev).cuda_stream
    group = opt.param_groups[0]

    def norm():
        _lib.check(lib.opp_grad_sqnorm(tensors, chunks, n, 1.0, partials, stream), "opp_grad_sqnorm")

    def update():
        _lib.check(lib.opp_adam_step(tensors, chunks, n, partials, n, MAX_NORM, opt.last_grad_norm.data_ptr(), 1.0, group["lr"], 0.9, 0.999,
                                     group["eps"], group["weight_decay"], 1, 1.0 - 0.9 ** 100, 1.0 - 0.999 ** 100, stream), "opp_adam_step")

    out = []
    for name, fn, nbytes in (("opp_grad_sqnorm", norm, 4 * n_floats), ("opp_adam_step", update, 28 * n_floats)):
        fn()
        fn()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        us = e0.elapsed_time(e1) / reps * 1e3
        out.append((name, n, us, nbytes, nbytes / us * 1e-3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device: %s, torch %s" % (torch.cuda.get_device_name(dev), torch.__version__))
    for flat in (False, True):
        model = make_model(dev, flat)
        params = list(model.parameters())
        n_floats = sum(p.numel() for p in params)
        unaligned = sum(p.grad.data_ptr() % 16 != 0 for p in params)
        print("\n%s gradients: %d tensors, %d floats, %d gradient tensors off a 16-byte boundary" %
              ("GradientAverager's flat" if flat else "plain", len(params), n_floats, unaligned))
        print("  %-52s %12s %12s" % ("per update, median of %d" % args.steps, "host ms", "device ms"))
        rows, opt_c = variants(model, flat)
        for name, fn in rows:
            if fn is None:
                print("  " + name)
                continue
            host_ms, dev_ms = time_variant(fn, dev, args.steps, args.warmup)
            print("  %-52s %12.3f %12.3f" % (name, host_ms, dev_ms))
        for name, grid, us, nbytes, gbs in time_kernels(opt_c, dev, n_floats):
            print("  kernel %-16s grid %5d: %8.1f us per launch, %6.1f MB -> %7.1f GB/s" % (name, grid, us, nbytes / 1e6, gbs))


if __name__ == "__main__":
    main()
