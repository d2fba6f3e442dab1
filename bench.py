#!/usr/bin/env python
"""Throughput bench of the 2D-3D matching forward on MI355X (BASELINE.json metric).

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR]     (N > 1: spawns one rank per GPU itself)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1]): one object, 512x512 query image x 5000-point cloud,
coarse-match only (`fine_matching.enable=False`), B=1 per forward, synthetic image/bank and
seeded random weights (no datasets or checkpoints are available offline).  A step is a fixed batch of
IMAGES_PER_STEP = 16 B=1 `OnePosePlus_model(data)` forwards per GPU through the HIP path with image and descriptor
banks already resident in HBM (so that the driver's `--steps 20` times >= 0.5 s, not 45 ms); `value` stays images/s.  With N GPUs every rank owns a different synthetic object (per-object sharding,
SURVEY.md §8e): weights are broadcast once from rank 0 over RCCL, then there is no collective in
the data path ("scaling": "weak").  Rank 0 prints ONE JSON line.

Arithmetic: the module default `bf16x3` -- fp32 in / fp32 accumulate / fp32 out, GEMM operands carried
EXACTLY as hi + mid + lo bf16 triples (24 significant bits, fp32 exponent range): not narrower than the
reference's fp32.  `--precision fp32` runs the exact-fp32 MFMA instead; the narrower `fp16x2*` fast modes
are reported as secondary legs only.

Extra legs (rank 0, N=1 only):
  (a step of the "roofline" pass below is ONE forward)
  roofline     - HIP-event timing (events recorded on the launch stream by libopp_hip.so) of every
                 launch of each profiled kernel symbol: the implicit-GEMM conv / dense / score GEMM
                 tiles (bound "mfma", algorithmic FLOPs with unpadded channel counts) and the
                 bandwidth-bound attention gather / apply and dual-softmax passes (bound "hbm",
                 algorithmic bytes).  The symbol with the largest time per forward is `roofline`.
  fine_leg     - the full coarse-to-fine forward on a bank with ~1500 confident matches.
  cpu_baseline - the CPU oracle (oracle/onepose_oracle.py, a port of the reference PyTorch
                 path) timed on the host cores over a bounded sample of the same workload.
"""
import argparse
import ctypes
import json
import os
import socket
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_F16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: BF16/FP16 MFMA ~2.5 PF dense (32x32x16)
PEAK_HBM_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s peak
# MFMA peak in ALGORITHMIC TFLOP/s per arithmetic: products issued per algorithmic multiply-add
MFMA_PEAK = {"fp32": PEAK_F32_MFMA_TFLOPS, "bf16x3": PEAK_F16_MFMA_TFLOPS / 6.0,
             "fp16x2": PEAK_F16_MFMA_TFLOPS / 3.0, "fp16x2_all": PEAK_F16_MFMA_TFLOPS / 3.0}
DTYPE = {"fp32": "f32",
         "bf16x3": "f32 (GEMM operands carried exactly as hi+mid+lo bf16 triples, 6 bf16 MFMAs per product, fp32 accumulate)",
         "fp16x2": "f32 (GEMM operands as hi+lo fp16 pairs [22-bit mantissa, narrower than fp32], fp32 accumulate; score GEMM fp32)",
         "fp16x2_all": "f32 (GEMM operands as hi+lo fp16 pairs [22-bit mantissa, narrower than fp32], fp32 accumulate)"}
PREC_ID = {"fp32": 0, "fp16x2": 1, "fp16x2_all": 1, "bf16x3": 2}
# candidate kernel symbols: (tile cfg, kind, template tile args, description).  kind 1 = implicit-GEMM conv,
# 0 = dense GEMM, 2 = coarse score GEMM with the fused dual-softmax statistics.  Only symbols the model actually
# launches for the arithmetic in use show up (launches > 0).
GEMM_SYMBOLS = [
    (20, 1, "256, 128, 4, 2, true", "implicit-GEMM conv, 256x128 tile, 8 waves"),
    (22, 1, "128, 256, 2, 4, true", "implicit-GEMM conv, 128x256 tile, 8 waves"),
    (27, 1, "128, 224, 4, 2, true", "implicit-GEMM conv, 128x224 tile on four fragment sets, 8 waves: the 196(->224)-column layers on grids of >= one full round (latency tile policy)"),
    (24, 1, "128, 192, 4, 2, true", "implicit-GEMM conv, 128x192 tile, 8 waves: the 192-column body of the 196-channel layers (last 4 columns: conv_tail_kernel)"),
    (25, 1, "128, 128, 4, 2, true", "implicit-GEMM conv, 128x128 tile, 8 waves"),
    (26, 1, "64, 128, 2, 4, true", "implicit-GEMM conv, 64x128 tile, 8 waves"),
    (11, 1, "128, 128, 2, 2, true", "implicit-GEMM conv, 128x128 tile, 4 waves, prefetch depth 4"),
    (10, 1, "128, 128, 2, 2, true", "implicit-GEMM conv, 128x128 tile, 4 waves, prefetch depth 3"),
    (0, 1, "128, 128, 2, 2, true", "implicit-GEMM conv, 128x128 tile, 4 waves"),
    (1, 1, "64, 128, 2, 2, true", "implicit-GEMM conv, 64x128 tile, 4 waves"),
    (2, 1, "64, 64, 2, 2, true", "implicit-GEMM conv, 64x64 tile, 4 waves"),
    (20, 0, "256, 128, 4, 2, false", "dense GEMM, 256x128 tile, 8 waves"),
    (22, 0, "128, 256, 2, 4, false", "dense GEMM, 128x256 tile, 8 waves"),
    (25, 0, "128, 128, 4, 2, false", "dense GEMM (QKV, mlp.0, stem), 128x128 tile, 8 waves"),
    (0, 0, "128, 128, 2, 2, false", "dense GEMM (QKV, mlp.0, stem), 128x128 tile, 4 waves"),
    (26, 0, "64, 128, 2, 4, false", "dense GEMM, 64x128 tile, 8 waves"),
    (1, 0, "64, 128, 2, 2, false", "dense GEMM, 64x128 tile, 4 waves"),
    (2, 0, "64, 64, 2, 2, false", "dense GEMM, 64x64 tile, 4 waves"),
    (30, 0, "64, 256, 2, 4, false", "dense GEMM + fused LayerNorm (merge, mlp.2), 64x256 tile, 8 waves"),
    (20, 2, "256, 128, 4, 2, false", "coarse score GEMM + fused dual-softmax statistics, 256x128 tile, 8 waves"),
    (25, 2, "128, 128, 4, 2, false", "coarse score GEMM + fused dual-softmax statistics, 128x128 tile, 8 waves"),
    (0, 2, "128, 128, 2, 2, false", "coarse score GEMM + fused dual-softmax statistics, 128x128 tile, 4 waves"),
]
DEPTH_OF_CFG = {10: 3, 11: 4}
IMAGES_PER_STEP = 16
# MFMA-bound kernels outside opp_gemm_kernel: (profile symbol, kernel name, description); work = algorithmic FLOPs
MFMA_SYMBOLS = [
    (1009, "enc_layer64_kernel", "one encoder layer behind the QKV projection in ONE launch: attention apply, merge, norm1, mlp.0, ReLU, "
                                 "mlp.2, norm2, residual on 64-token tiles held in LDS (enc_chain_kernel on 32-token tiles when "
                                 "encoder_fusion = 1); 2 x T x (7 C^2 + 32 C) FLOP"),
    (1012, "gemm_ss_kernel<3>", "coarse score GEMM on operands pre-split once, LDS-DMA staged, + dual-softmax statistics + score matrix "
                                "(gemm_ss_res3_kernel in the kernel trace since r06: three resident workgroups per CU)"),
    (1010, "gemm_ss_kernel<1>", "coarse score GEMM sweep 1 (statistics only; two-sweep matcher)"),
    (1011, "gemm_ss_kernel<2>", "coarse score GEMM sweep 2 (confidences written once; two-sweep matcher)"),
    (1014, "opp_gemm_kernel<128, 128, 4, 2, true> x 4 K slices", "3x3 convolutions of the 1/8-resolution stage (4096 pixels, K = 1792 .. 2304) as "
                                                                  "four K slices on 8-wave tiles: 256 workgroups instead of 64 four-wave ones"),
]
EMPTY_KERNEL_US = 3.6        # fallback only: duration of opp_empty_kernel in the rocprofv3 kernel trace of round 4; the run measures its own (roofline_leg)
HBM_SYMBOLS = [
    (1000, "linattn_kv_mfma_kernel", "linear-attention gather: sum_s phi(K_s)^T V_s (K, V read once + chunk partials written)"),
    (1001, "linattn_apply_pair_kernel", "linear-attention apply (Q read, message written)"),
    (1002, "conf_reg_kernel", "dual-softmax product over the N x L score matrix (read + written once)"),
    (1015, "splitk_epilogue_kernel", "K slices of a split convolution summed in slice order + bias / residual / activation"),
    (1017, "conv_tail_kernel", "columns 192 .. 223 of the 196-channel convolutions: 4 fp32 FMA chains per pixel on the vector ALU + the zero padding "
                               "channels (input read once, one 128-byte line per pixel written)"),
    (1016, "linattn_reduce_pair_kernel", "fixed-order sum of the attention gather's chunk partials (partials read, KV / Ksum written)"),
]
# launch shapes that are ONE kernel symbol in a rocprofv3 trace: (symbol of the entry that absorbs, symbol absorbed).  The K slices of the
# 1/8-resolution convolutions run the same template instance as the 128x128 convolutions of the 1/4-resolution stage.
SAME_SYMBOL = [("128, 128, 4, 2, true, 0, 2, 2", "opp_gemm_kernel<128, 128, 4, 2, true> x 4 K slices")]


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40, help="timed steps; one step = --images-per-step forwards per GPU")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--images-per-step", type=int, default=IMAGES_PER_STEP)
    ap.add_argument("--n-points", type=int, default=5000)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--fine", action="store_true", help="full coarse-to-fine forward instead of configs[1]")
    ap.add_argument("--thr", type=float, default=0.1)
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="budget of the cpu_baseline leg (0 = skip)")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-legs", action="store_true", help="skip the other-arithmetic and fine-stage legs")
    ap.add_argument("--precision", default=None, choices=["bf16x3", "fp32", "fp16x2", "fp16x2_all"],
                    help="GEMM arithmetic (default: the module default bf16x3 / OPP_GEMM_PRECISION)")
    ap.add_argument("--tile-policy", default="auto", choices=["auto", "latency", "throughput"],
                    help="automatic GEMM / conv tile choice of the timed region (opp_config.tile_policy); auto = what serving.MatcherPool does: "
                         "throughput (least CU time per launch) with several forwards in flight, latency (every launch sized to fill the chip) "
                         "with one; the other one is reported as a leg.  The per-kernel roofline pass is single-stream and always uses the latency tiles.")
    ap.add_argument("--fpn-overlap", default="auto", choices=["auto", "on", "off"],
                    help="FPN fine branch on a side HIP stream (opp_config.fpn_overlap); auto = on for one forward in flight, off for "
                         "several (the other forwards are the overlap; extra streams only crowd the hardware queues)")
    ap.add_argument("--streams", type=int, default=int(os.environ.get("OPP_BENCH_STREAMS", "4")),
                    help="B=1 forwards kept in flight per GPU on separate HIP streams (the reference runs "
                         "2 Ray workers per GPU, inference_OnePosePlus.py:18-26); measured with the throughput tiles (r05, one box): "
                         "2 / 3 / 4 / 5 streams = 493 / 523 / 530 / 530 images/s")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the forwards of the last timed step returned as DIR/<name>.npy (float32 / float64; "
                         "matrices above %d elements as a fixed seeded sample) so that two builds can be compared output for output"
                         % DUMP_FULL_MAX)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    return args


def main():
    args = parse_args()
    if args.gpus > 1 and "RANK" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher -- one rank per GPU over RCCL, the same command
        # line the driver uses (src/inference.py:83-106 fans objects out to GPUs the same way, with Ray)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        raise SystemExit(subprocess.call(cmd, env=env))
    if os.environ.get("OPP_BENCH_DRY_RUN") == "1":
        return run_dry(args)
    run(args)


def timed_region(run_steps, n, barrier, sync):
    """The contract's timed region: barrier + device sync, EXACTLY n forwards, device sync, barrier.
    -> (last result, this rank's own time before the closing barrier, time including it)"""
    barrier()
    t0 = time.perf_counter()
    last = run_steps(n)
    sync()
    own_elapsed = time.perf_counter() - t0      # this rank alone (before the closing barrier): per-rank rate
    barrier()
    return last, own_elapsed, time.perf_counter() - t0


def gather_ranks(dist, torch, dev, elapsed, info):
    """-> (MAX of `elapsed` over the ranks, every rank's `info` record in rank order, ranks seen); dist = None: single process"""
    if dist is None:
        return elapsed, [info], 1
    t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    devs = [None] * dist.get_world_size()
    dist.all_gather_object(devs, info)
    return float(t.item()), devs, dist.get_world_size()


def per_rank_summary(devs):
    per_rank = [d["images_per_s"] for d in devs]
    return {"min": min(per_rank), "max": max(per_rank), "sum": round(sum(per_rank), 2)}


def run_dry(args):
    """OPP_BENCH_DRY_RUN=1 (tests/test_bench_dry_cpu.py): the multi-rank skeleton of this file -- launcher, RANK / WORLD_SIZE
    handling, weight broadcast, barriers, max-over-ranks timing, per-rank gather, the one JSON line of rank 0 -- over gloo on
    CPU tensors with a stand-in for the forward (a sleep whose length depends on the rank), so that the code the first
    multi-GPU lease will execute has run somewhere.  Not a measurement: the line says so."""
    import torch
    import torch.distributed as dist
    from onepose_plus_plus_amd import OnePosePlus_model, default_config
    from onepose_plus_plus_amd.sharding import broadcast_weights
    from onepose_plus_plus_amd.synthetic import make_state_dict
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    dev = torch.device("cpu")
    d = None
    if "RANK" in os.environ:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        d = dist
    cfg = default_config(thr=args.thr, fine=args.fine)
    model = OnePosePlus_model(cfg).eval()
    sd = make_state_dict(cfg, 0) if rank == 0 else None
    if d is not None:
        broadcast_weights(model, sd, src=0)
    else:
        model.load_state_dict(sd, strict=True)
    checksum = float(sum(float(v.double().sum()) for v in model.state_dict().values() if v.is_floating_point()))
    ips = max(1, args.images_per_step)

    def run_steps(n):
        time.sleep(n * 0.001 * (1.0 + 0.5 * rank))          # rank r is 1 + r / 2 times slower: max-over-ranks must show
        return {"mconf": torch.zeros(0)}

    def barrier():
        if d is not None:
            d.barrier()
    run_steps(max(args.warmup, 1) * ips)
    last, own, elapsed = timed_region(run_steps, args.steps * ips, barrier, lambda: None)
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    elapsed, devs, seen = gather_ranks(d, torch, dev, elapsed, {"rank": rank, "local_rank": local_rank, "pid": os.getpid(),
                                                              "device": local_rank,        # what run() hands torch.cuda.set_device
                                                              "visible": os.environ.get("HIP_VISIBLE_DEVICES"),
                                                              "host_affinity": "dry run: %d cpus allowed" % len(os.sched_getaffinity(0)),
                                                              "images_per_s": round(args.steps * ips / own, 2), "weights_checksum": checksum})
    if rank == 0:
        total = args.steps * ips * world
        print(bounded_dumps({"metric": "DRY RUN (no GPU work): multi-rank skeleton of bench.py over gloo", "value": round(total / elapsed, 3),
                          "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                          "data": "none", "config": {"workload": "dry run", "images_per_step": ips, "per_rank_images_per_s": per_rank_summary(devs),
                                                     "n_ranks_seen": seen, "rank_devices": devs}}), flush=True)
    if d is not None:
        d.destroy_process_group()


def pin_to_gpu_numa_node(torch, dev):
    """Best effort: restrict this rank's host threads (the stream feeders) to the CPUs of the NUMA node its GPU hangs off, so
    that an 8-rank run does not explain a non-linearity by cross-socket launches.  Returns a short description."""
    try:
        bus = torch.cuda.get_device_properties(dev).pci_bus_id if hasattr(torch.cuda.get_device_properties(dev), "pci_bus_id") else None
        dom = getattr(torch.cuda.get_device_properties(dev), "pci_domain_id", 0)
        devid = getattr(torch.cuda.get_device_properties(dev), "pci_device_id", 0)
        if bus is None:
            return "unknown (no pci id)"
        path = "/sys/bus/pci/devices/%04x:%02x:%02x.0/numa_node" % (dom, bus, devid)
        node = int(open(path).read().strip())
        if node < 0:
            return "numa_node -1 (single node)"
        cpus = []
        for part in open("/sys/devices/system/node/node%d/cpulist" % node).read().strip().split(","):
            a, _, b = part.partition("-")
            cpus += list(range(int(a), int(b or a) + 1))
        allowed = sorted(set(cpus) & set(os.sched_getaffinity(0)))
        if allowed:
            os.sched_setaffinity(0, allowed)
            return "numa node %d (%d cpus)" % (node, len(allowed))
        return "numa node %d (no allowed cpu)" % node
    except Exception as e:      # sysfs layout differs / not permitted: run unpinned
        return "unpinned (%s)" % type(e).__name__


def run(args):
    import torch
    from onepose_plus_plus_amd import OnePosePlus_model, default_config, _lib
    from onepose_plus_plus_amd.synthetic import make_state_dict, make_inputs

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    affinity = pin_to_gpu_numa_node(torch, dev) if (world > 1 or os.environ.get("OPP_BENCH_PIN")) else "not pinned (single rank)"
    ips = max(1, args.images_per_step)
    dist = None
    if "RANK" in os.environ:     # launched by torch.distributed.run: one rank per GPU over RCCL
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    cfg = default_config(thr=args.thr, fine=args.fine)
    model = OnePosePlus_model(cfg).eval()
    if args.precision:
        model.set_gemm_precision(args.precision)
    precision = model.gemm_precision
    sd = make_state_dict(cfg, 0) if rank == 0 else None
    model = model.to(dev)
    if dist is not None:
        from onepose_plus_plus_amd.sharding import broadcast_weights
        broadcast_weights(model, sd, src=0)       # ONE broadcast of the flat weight buffer (RCCL over xGMI)
    else:
        model.load_state_dict(sd, strict=True)
    n_streams = max(1, args.streams)
    # scheduling switches (bit-identical results either way).  Tiles follow the number of forwards in flight, as serving.MatcherPool
    # sets them: with several forwards in flight other forwards' kernels take the CUs a launch leaves idle, so the tiles with the
    # least CU time per launch win (`throughput`: +4 % images/s at 3 streams in rounds 3 / 4, where it was a leg); with one forward
    # in flight -- and in the per-kernel roofline pass, which is single-stream -- every launch is sized to fill the chip on its own
    # (`latency`), so a symbol's stand-alone duration is a meaningful roofline figure.  The other policy is reported as a leg.  Side
    # stream of the FPN fine branch: on for one forward in flight, off for several (the other forwards are the overlap; more streams
    # only crowd the hardware queues: -0.7 % with the latency tiles, -3 % with the throughput tiles).
    policy = args.tile_policy
    if policy == "auto":
        policy = "throughput" if n_streams > 1 else "latency"
    overlap = (n_streams == 1) if args.fpn_overlap == "auto" else args.fpn_overlap == "on"
    if args.fpn_overlap == "auto" and "OPP_FPN_OVERLAP" in os.environ:
        overlap = os.environ["OPP_FPN_OVERLAP"] != "0"
    model.set_tile_policy(policy).set_fpn_overlap(overlap)
    models = [model]
    for _ in range(1, n_streams):        # one module (own workspace / outputs) per in-flight forward
        m = OnePosePlus_model(cfg).eval().set_gemm_precision(precision).set_tile_policy(policy).set_fpn_overlap(overlap).to(dev)
        m.load_state_dict(model.state_dict(), strict=True)
        models.append(m)
    streams = [torch.cuda.Stream(device=dev) for _ in range(n_streams)] if n_streams > 1 else [None]

    # one synthetic object per rank (seed = rank), a small pool of query images resident in HBM
    n_img = 4
    datas = []
    for i in range(n_img):
        d = make_inputs(args.n_points, (args.hw, args.hw), seed=1 + 1000 * rank)
        if i:
            g = torch.Generator().manual_seed(77 + i + 1000 * rank)
            d["query_image"] = torch.rand(1, 1, args.hw, args.hw, generator=g)
        datas.append({k: v.to(dev) for k, v in d.items()})
    bank = {k: datas[0][k] for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
    for d in datas:
        d.update(bank)          # the bank is per-object constant: one resident copy
    torch.cuda.synchronize(dev)

    def step(i, slot=0, pool=None, mods=None):
        pool = pool or datas
        d = dict(pool[i % len(pool)])
        with torch.no_grad():
            if streams[slot] is None:
                (mods or models)[slot](d)
            else:
                with torch.cuda.stream(streams[slot]):
                    (mods or models)[slot](d)
        return d

    def run_steps(n, pool=None, mods=None, keep=None):
        """EXACTLY n forwards (callers pass steps x images_per_step).  With several streams one host thread per stream keeps its forward in flight (the
        forward's single D2H sync of the match count releases the GIL); the threads draw step indices from one
        shared counter, so no stream idles while another still has a backlog.  keep (a dict): filled with forward index -> returned dict for
        the forwards of the last step (references only, no device work)."""
        first_kept = n - ips
        if n_streams == 1:
            last = None
            for i in range(n):
                last = step(i, 0, pool, mods)
                if keep is not None and i >= first_kept:
                    keep[i] = last
            return last
        out = [None] * n_streams
        nxt = [0]
        lock = threading.Lock()

        def worker(slot):
            torch.cuda.set_device(dev)
            while True:
                with lock:
                    i = nxt[0]
                    nxt[0] += 1
                if i >= n:
                    break
                out[slot] = step(i, slot, pool, mods)
                if keep is not None and i >= first_kept:
                    keep[i] = out[slot]
            streams[slot].synchronize()
        th = [threading.Thread(target=worker, args=(k,)) for k in range(n_streams)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        return next(o for o in out if o is not None)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(dev)

    # warm-up: W untimed steps on EVERY stream (packs the weights, sizes the workspaces, fills the per-object token
    # cache), then one concurrent round so that the streams, their host threads and the clocks are in steady state
    for k in range(n_streams):            # per-stream module state: packed weights, workspaces, per-object token cache
        step(0, k)
    torch.cuda.synchronize(dev)
    run_steps(max(args.warmup, 1) * ips)
    lib = _lib.load()
    prof = (not args.no_roofline) and rank == 0 and world == 1

    kept = {} if args.dump_outputs else None
    last, own_elapsed, elapsed = timed_region(lambda n: run_steps(n, keep=kept), args.steps * ips, barrier, lambda: torch.cuda.synchronize(dev))
    matches_last = int(last["mconf"].numel())
    if kept is not None:
        dump_outputs(args.dump_outputs, kept, datas[0].keys(), args.steps * ips - ips, "rank%d_" % rank if world > 1 else "")
        kept = None
    obj = model._rt.get("obj")       # (key, tokens, sources, event, transformer-prefix blob or None) as the timed region left it
    cache_on = bool(getattr(model, "cache_object_tokens", True)) and obj is not None and obj[4] is not None
    props = torch.cuda.get_device_properties(dev)
    elapsed, devs, n_ranks_seen = gather_ranks(dist, torch, dev, elapsed, {
        "rank": rank, "local_rank": local_rank, "device": torch.cuda.current_device(), "name": props.name,
        "uuid": str(getattr(props, "uuid", "")), "pid": os.getpid(),
        "images_per_s": round(args.steps * ips / own_elapsed, 2), "host_affinity": affinity})

    roof = None
    if prof:
        # a kernel's own duration: one forward in flight AND the FPN fine branch on the same stream (with opp_config.fpn_overlap
        # the coarse-level kernels share the CUs with the fine-branch convolutions and every launch of both stretches)
        for m in models:
            m.set_fpn_overlap(False).set_tile_policy("latency").to(dev)
        step(0, 0)
        torch.cuda.synchronize(dev)
        roof = roofline_leg(lib, _lib, torch, dev, step, precision, min(args.steps * ips, 20))
        if roof is not None:
            roof["tile_policy"] = ("latency (single-stream pass: every launch sized to fill the chip on its own; the timed region ran the "
                                   "%s tiles with %d forward(s) in flight)" % (policy, n_streams))
        for m in models:
            m.set_fpn_overlap(overlap).set_tile_policy(policy).to(dev)
        for k in range(n_streams):
            step(0, k)
        torch.cuda.synchronize(dev)

    legs = {}
    if rank == 0 and world == 1 and not args.no_legs:
        legs = other_legs(torch, dev, cfg, models, run_steps, step, precision, n_streams, args, lib, _lib)

    cpu = None
    if rank == 0 and world == 1 and args.cpu_seconds > 0:
        cpu = cpu_baseline(torch, cfg, make_state_dict(cfg, 0), args, make_inputs)

    if rank == 0:
        total = args.steps * ips * world
        if roof is not None and legs:      # compact copies of the secondary legs inside `roofline` (the sidecar keeps both)
            roof["legs"] = compact_legs(legs)
        # FLOPs of one image: what the reference computes per image and what THIS run executed per image -- with the
        # per-object token cache on, layer 0 on the 3D stream + its layer-1 projections / KV sums are not redone per image and are
        # NOT counted in any roofline fraction of this line
        ref_flops = flops_per_image(args.n_points, cached=False)
        flops_img = flops_per_image(args.n_points, cached=cache_on)
        peak = MFMA_PEAK[precision]
        detail = {
            "metric": "query images/sec (2D-3D match fwd) at 512x512 img x 5k pts",
            "value": round(total / elapsed, 3), "unit": "images/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "ms_per_image": round(elapsed / (args.steps * ips) * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": DTYPE[precision],
            "data": "synthetic (seeded random image, descriptor bank and weights)",
            "config": {"workload": "%s: single object, %dx%d image x %d points, %s, B=1 per forward, "
                                   "a step = %d forwards per GPU, %d forward(s) in flight per GPU on separate HIP streams, one object per GPU; image and "
                                   "descriptor banks resident in HBM; the image-independent work on the resident object (keypoint-MLP encoding of the "
                                   "bank, layer-0 self-attention of the 3D stream, its layer-1 projections and KV sums: 2.6 %% of the reference's FLOPs, "
                                   "NOT counted in executed_gflop_per_image) is cached per object -- `object_token_cache_off` is the leg without it; thr %.2f gives M = %d "
                                   "matches on these random weights (the conf matrix is still fully materialised)"
                                   % ("configs[2] / [3] shape" if args.fine else "configs[1]", args.hw, args.hw, args.n_points,
                                      "full coarse-to-fine (match-driven fine branch)" if args.fine else "coarse-match only", ips, n_streams,
                                      args.thr, matches_last),
                       "workload_short": "%s: %dx%d x %d pts, %s, B=1, %d fwd/step, %d stream(s)/GPU, banks resident, object-token cache %s"
                                         % ("configs[2]" if args.fine else "configs[1]", args.hw, args.hw, args.n_points,
                                            "coarse-to-fine" if args.fine else "coarse-match only", ips, n_streams, "on" if cache_on else "off"),
                       "images_per_step": ips, "streams_per_gpu": n_streams,
                       "per_rank_images_per_s": per_rank_summary(devs), "gemm_precision": precision, "tile_policy": policy, "fpn_overlap": bool(overlap),
                       "matches_last_step": matches_last, "object_token_cache": cache_on,
                       "n_ranks_seen": n_ranks_seen, "rank_devices": devs,
                       "reference_gflop_per_image": round(ref_flops / 1e9, 1),
                       "executed_gflop_per_image": round(flops_img / 1e9, 1),
                       "model_tflops": round(flops_img * total / elapsed / 1e12, 2),
                       "model_frac_of_mfma_peak": round(flops_img * total / elapsed / 1e12 / world / peak, 4),
                       "mfma_peak_tflops_for_this_arithmetic": round(peak, 1),
                       **legs},
            "roofline": roof, "cpu_baseline": cpu,
        }
        off = (legs.get("object_token_cache_off_leg") or {}).get("value")
        if off:           # first-class: the same workload doing exactly the reference's per-image work (cache off), fraction on ALL its FLOPs
            detail["config"]["value_cache_off"] = off
            detail["config"]["frac_cache_off"] = round(ref_flops * off / 1e12 / peak, 4)
        where = write_detail(detail)
        print(bounded_dumps(compact_line(detail, where)), flush=True)
    if dist is not None:
        dist.destroy_process_group()


LINE_LIMIT = 6000            # bytes of the ONE JSON line of rank 0 (the driver keeps the last ~8 KB of stdout); the rest is the sidecar
# per-token multiply-adds of one encoder layer: x side 532,480 + source side 139,264; QKV projections 3 x 65,536; KV sums 8,192
MACS_LAYER_TOKEN, MACS_QKV_TOKEN, MACS_KV_TOKEN = 671744, 196608, 8192


def flops_per_image(n_points, cached):
    """Algorithmic FLOPs of one coarse forward.  cached = True: minus what a resident object's token cache keeps out of
    the per-image work (opp_object_prefix: layer 0 on the 3D stream, its layer-1 QKV projections and KV / Ksum reduction)."""
    f = 2.0 * (126.726e9 + 6 * (4096 + n_points) * MACS_LAYER_TOKEN + n_points * 4096 * 256)
    if cached:
        f -= 2.0 * n_points * (MACS_LAYER_TOKEN + MACS_QKV_TOKEN + MACS_KV_TOKEN)
    return f


def write_detail(detail):
    """Everything the run measured -> bench_detail.json next to this file (and gpurun_out/ when it exists, so that it travels back
    from a GPU box).  -> the path written, relative to the repo root, or None"""
    where = None
    for d in ([os.environ["OPP_BENCH_DETAIL"]] if os.environ.get("OPP_BENCH_DETAIL") else
              [os.path.join(ROOT, "bench_detail.json"), os.path.join(ROOT, "gpurun_out", "bench_detail.json")]):
        try:
            if os.path.isdir(os.path.dirname(d) or "."):
                with open(d, "w") as f:
                    json.dump(detail, f, indent=1)
                where = where or os.path.relpath(d, ROOT)
        except OSError:
            pass
    return where


DUMP_FULL_MAX = 1 << 20      # --dump-outputs: arrays up to this many elements are written whole, larger ones as a sample
DUMP_SAMPLE = 1 << 18        # elements of that sample: fixed positions drawn from a seeded generator, the same for every run and build
DUMP_LIMIT = 64 << 20        # bytes written by --dump-outputs in all


def dump_outputs(out_dir, kept, input_keys, first, prefix=""):
    """--dump-outputs: the arrays the forwards of the last timed step returned (every tensor the forward added to its dict, not the
    inputs; empty ones -- the match lists when a forward finds no match -- are left out) -> out_dir/<prefix>fKK_<name>.npy, KK = the
    forward's position in the step.  Floating tensors as float32 (float64 stays
    float64), integer / bool tensors as float64 (exact: the indices are far below 2^53).  An array of more than DUMP_FULL_MAX elements
    (the N x L confidence matrix) is written as `<name>_sample` at the flat positions stored in <prefix>sample_index_n<numel>.npy."""
    import numpy as np
    import torch
    files, index = {}, {}
    for i in sorted(kept):
        for name, t in sorted(kept[i].items()):
            if name in input_keys or not torch.is_tensor(t) or t.numel() == 0:
                continue
            wide = t.dtype == torch.float64 or not t.is_floating_point()
            a = (t.double() if wide else t.float()).detach().cpu().reshape(-1).numpy()
            if a.size > DUMP_FULL_MAX:
                if a.size not in index:
                    pos = np.random.default_rng(0).choice(a.size, DUMP_SAMPLE, replace=False)
                    index[a.size] = np.sort(pos)
                    files["%ssample_index_n%d" % (prefix, a.size)] = index[a.size].astype(np.float64)
                a, name = a[index[a.size]], name + "_sample"
            else:
                a = a.reshape(tuple(t.shape))
            files["%sf%02d_%s" % (prefix, i - first, name)] = a
    total = sum(a.nbytes for a in files.values())
    if total > DUMP_LIMIT:
        raise SystemExit("--dump-outputs: %d bytes for %d forwards exceed the %d-byte limit (lower --images-per-step)"
                         % (total, len(kept), DUMP_LIMIT))
    os.makedirs(out_dir, exist_ok=True)
    for name, a in files.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    sys.stderr.write("--dump-outputs: %d arrays, %.1f MB -> %s\n" % (len(files), total / 2**20, out_dir))


def bounded_dumps(obj, limit=LINE_LIMIT):
    """json.dumps that refuses to print a line the driver's stdout tail would cut"""
    line = json.dumps(obj)
    if len(line) > limit:
        raise SystemExit("bench.py: JSON line of %d bytes exceeds the %d-byte bound" % (len(line), limit))
    return line


def _traffic_bytes(t):
    """PMC summary entry -> HBM bytes per launch (one launch shape), or None"""
    if isinstance(t, dict) and "hbm_bytes_per_launch" in t:
        return t["hbm_bytes_per_launch"]
    if isinstance(t, dict) and "per_launch_shape" in t:          # several shapes: launch-weighted mean
        sh = [v for v in t["per_launch_shape"].values() if "hbm_bytes_per_launch" in v]
        n = sum(v.get("launches_sampled", 1) for v in sh)
        return int(sum(v["hbm_bytes_per_launch"] * v.get("launches_sampled", 1) for v in sh) / n) if n else None
    return None


def _short_symbol(m):
    """`opp_gemm_kernel<128, 128, 4, 2, true, 0, 2, 2>` -> `gemm<128,128,4,2,conv>`; other kernels keep their name minus `_kernel`"""
    sym = m.get("symbol") or ""
    if sym and sym[0].isdigit():
        a = [x.strip() for x in sym.split(",")]
        return "gemm<%s,%s,%s,%s,%s>" % (a[0], a[1], a[2], a[3], "conv" if a[4] == "true" else "dense")
    if sym.startswith("opp_gemm_kernel<"):
        return "gemm<128,128,4,2,conv>x4K"
    return sym.replace("_kernel", "")


def compact_line(detail, detail_path=None, limit=LINE_LIMIT):
    """The ONE line rank 0 prints: the contract's keys, the dominant kernel's roofline with numbers only, a <= 8-row table of the
    other kernels, the headline figures of the secondary legs -- never more than `limit` bytes.  Prose, per-shape traffic tables and
    full legs live in the sidecar (`detail`)."""
    c = detail.get("config") or {}
    out = {k: detail.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "ms_per_image",
                                      "higher_is_better", "scaling", "vs_baseline")}
    prec = c.get("gemm_precision")
    out["dtype"] = {"bf16x3": "f32 (operands as exact bf16 triples, f32 accumulate)", "fp32": "f32"}.get(prec, str(detail.get("dtype"))[:60])
    out["data"] = "synthetic"
    cfg = {"workload": (c.get("workload_short") or c.get("workload") or "")[:200]}
    for k in ("images_per_step", "streams_per_gpu", "gemm_precision", "tile_policy", "object_token_cache", "matches_last_step",
              "n_ranks_seen", "per_rank_images_per_s", "reference_gflop_per_image", "executed_gflop_per_image", "model_tflops",
              "model_frac_of_mfma_peak", "mfma_peak_tflops_for_this_arithmetic", "value_cache_off", "frac_cache_off"):
        if c.get(k) is not None:
            cfg[k] = c[k]
    devs = c.get("rank_devices") or []
    if devs:                  # [rank, local_rank, device, images/s] per rank; names / uuids / pids / affinity: sidecar
        cfg["ranks"] = [[d.get("rank"), d.get("local_rank"), d.get("device"), d.get("images_per_s")] for d in devs]
    out["config"] = cfg
    r = detail.get("roofline")
    roof = None
    if r:
        roof = {"bound": r.get("bound"), "achieved": r.get("achieved"), "peak": r.get("peak"), "unit": r.get("unit"), "frac": r.get("frac"),
                "traffic": _traffic_bytes(r.get("traffic")), "kernel": _short_symbol(r), "avg_us": r.get("avg_launch_us"),
                "launches_per_forward": r.get("launches_per_forward"),
                **({"alg_gflop_per_launch": r["alg_gflop_per_launch"]} if "alg_gflop_per_launch" in r else
                   {"alg_mbytes_per_launch": r.get("alg_mbytes_per_launch")}),
                "frac_event_corrected": r.get("frac_event_corrected"),
                "how": "HIP events on the launch stream, 1 forward in flight"}
        top = []
        for m in (r.get("other_kernels") or []):
            top.append({"sym": _short_symbol(m), "us": m.get("us_per_forward"), "n": m.get("launches_per_forward"),
                        "frac": m.get("frac"), "of": "mfma" if m.get("bound") == "mfma" else "hbm"})
        roof["top"] = top[:8]
        ss = next((m for m in [r] + (r.get("other_kernels") or []) if (m.get("symbol") or "").startswith("gemm_ss_kernel<3>")), None)
        if ss:                # the kernel north_star names: coarse score GEMM
            roof["score_gemm"] = {"us": ss.get("avg_launch_us"), "frac": ss.get("frac"), "frac_event_corrected": ss.get("frac_event_corrected"),
                                  "traffic": _traffic_bytes(ss.get("traffic"))}
        if r.get("launches_per_coarse_forward") is not None:
            roof["launches_per_coarse_forward"] = r["launches_per_coarse_forward"]
    out["roofline"] = roof
    cb = detail.get("cpu_baseline")
    if cb:
        out["cpu_baseline"] = {"value": cb.get("value"), "unit": cb.get("unit"), "cores": cb.get("cores"), "kind": cb.get("kind"),
                               "one_thread": cb.get("one_thread_images_per_s"), "sample": (cb.get("sample_short") or cb.get("sample") or "")[:240]}
        if cb.get("reference_in_build_container") is not None:
            out["cpu_baseline"]["reference_in_build_container"] = cb["reference_in_build_container"]
    else:
        out["cpu_baseline"] = None
    legs = {}
    oa = c.get("other_arithmetics") or {}
    if (oa.get("fp32") or {}).get("value") is not None:
        legs["fp32_images_per_s"] = oa["fp32"]["value"]
    for pol in ("latency", "throughput"):
        if (c.get(pol + "_tiles_leg") or {}).get("value") is not None:
            legs[pol + "_tiles_images_per_s"] = c[pol + "_tiles_leg"]["value"]
    f = c.get("fine_leg") or {}
    if "ms_per_forward" in f:
        legs["fine"] = {k: f.get(k) for k in ("matches", "ms_per_forward", "images_per_s", "fine_stage_ms", "fine_stage_frac_of_mfma_peak")}
    for name, key in (("train", "train_leg"), ("train_n15000", "train_leg_n15000")):
        t = c.get(key) or {}
        if "step_ms" in t:
            legs[name] = {"step_ms": t["step_ms"], "forward_ms": t.get("forward_ms"), "samples_per_s": t.get("step_samples_per_s"),
                          "frac": (t.get("roofline") or {}).get("frac"),
                          "wgrad_frac": ((t.get("roofline") or {}).get("dominant_kernel") or {}).get("frac")}
            if name == "train":
                legs[name]["arith"] = "bf16x3 = f32-exact operands (reference trains f32, lightning_model:59); no bf16 autocast offered"
        elif "error" in t:
            legs[name] = {"error": str(t["error"])[:80]}
    if legs:
        out["legs"] = legs
    if detail_path:
        out["detail"] = detail_path
    # hard bound: shed optional parts until the line fits
    for shed in (lambda: out.get("legs", {}).pop("train_n15000", None), lambda: out.get("legs", {}).pop("fine", None),
                 lambda: roof and roof.__setitem__("top", roof["top"][:4]), lambda: out.pop("legs", None),
                 lambda: roof and roof.pop("top", None), lambda: cfg.pop("ranks", None)):
        if len(json.dumps(out)) <= limit:
            break
        shed()
    return out


def compact_legs(legs):
    """The numbers of the secondary legs a reader wants next to the roofline, without the prose."""
    out = {}
    oa = legs.get("other_arithmetics") or {}
    if oa:
        out["other_arithmetics_images_per_s"] = {k: v.get("value") for k, v in oa.items()}
    for pol in ("throughput", "latency"):
        t = legs.get(pol + "_tiles_leg")
        if t:
            out[pol + "_tiles_images_per_s"] = t.get("value")
    t = legs.get("coarse_only_without_unused_fine_map_leg")
    if t:
        out["coarse_only_without_unused_fine_map_images_per_s"] = t.get("value")
    t = legs.get("object_token_cache_off_leg")
    if t:
        out["object_token_cache_off_images_per_s"] = t.get("value")
    f = legs.get("fine_leg") or {}
    if "ms_per_forward" in f:
        out["fine"] = {k: f.get(k) for k in ("matches", "ms_per_forward", "images_per_s", "fine_stage_ms", "fine_stage_frac_of_mfma_peak",
                                             "fine_branch_path", "match_driven_fine_branch")}
    elif f:
        out["fine"] = f
    tr = legs.get("train_leg") or {}
    if "step_ms" in tr:
        out["train"] = {k: tr.get(k) for k in ("forward_ms", "step_ms", "backward_ms_in_opp_kernels", "backward_kernel_split", "step_samples_per_s", "roofline")}
    elif tr:
        out["train"] = tr
    t15 = legs.get("train_leg_n15000") or {}
    if t15:
        out["train_n15000"] = {k: t15.get(k) for k in ("forward_ms", "step_ms", "step_samples_per_s", "roofline", "error") if k in t15}
    return out


def traffic_of(traffic, template, kernel_name=None):
    """HBM bytes per launch of one kernel symbol from the committed PMC summary.  The summary is keyed by
    "<template args>|grid <workgroups>" (one entry per launch shape): a symbol with ONE shape returns that entry, a
    symbol that runs several shapes returns all of them rather than an average that fits none."""
    key = template if template is not None else kernel_name
    hits = {k: v for k, v in traffic.items() if k == key or k.startswith(key + "|")}
    if not hits:
        return None
    if len(hits) == 1:
        return next(iter(hits.values()))
    return {"per_launch_shape": hits}


def prof_run(lib, _lib, torch, dev, step, tile_cfg, kind, nsteps, pool=None, mods=None):
    """one single-stream pass of `nsteps` forwards with one kernel symbol armed -> (ms, work, launches)"""
    _lib.check(lib.opp_profile_start(tile_cfg, kind, nsteps * 40), "profile_start")
    for i in range(nsteps):
        step(i, 0, pool, mods)
    torch.cuda.synchronize(dev)
    ms, wk, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    _lib.check(lib.opp_profile_stop(ctypes.byref(ms), ctypes.byref(wk), ctypes.byref(n)), "profile_stop")
    return ms.value, wk.value, n.value


def roofline_leg(lib, _lib, torch, dev, step, precision, nsteps):
    """HIP events recorded by the library on the launch stream around every launch of one kernel symbol.  With
    several forwards in flight kernels of different streams share the CUs, so a kernel's own launch duration is only
    meaningful on its own: every symbol is timed in a single-stream pass of the same steps right after the timed
    region."""
    how = ("HIP events on the launch stream, single-stream pass of %d forwards after the timed region, fpn_overlap off "
           "(every kernel alone on the chip)" % nsteps)
    pid = PREC_ID[precision]
    peak = MFMA_PEAK[precision]
    tpath = os.path.join(ROOT, "profiles", "traffic_symbols_%s.json" % precision)
    traffic = {}
    if os.path.exists(tpath):     # HBM bytes per launch from the committed rocprofv3 --pmc passes
        with open(tpath) as f:
            traffic = json.load(f)
    meas = []
    ov, ek = ctypes.c_double(), ctypes.c_double()
    _lib.check(lib.opp_profile_event_overhead(200, ctypes.byref(ov), torch.cuda.current_stream(dev).cuda_stream), "profile_event_overhead")
    event_pair_us = ov.value          # what an (event, empty kernel, event) triple reads: the floor of every measurement below
    # the empty kernel's own duration, measured in this run: 400 of them back to back between ONE event pair (the launch-to-launch
    # interval of a kernel that does nothing = what the rocprofv3 kernel trace shows as its duration, 3.6 us in round 4)
    _lib.check(lib.opp_profile_empty_kernel(400, ctypes.byref(ek), torch.cuda.current_stream(dev).cuda_stream), "profile_empty_kernel")
    empty_kernel_us = ek.value if 0.5 < ek.value < 20.0 else EMPTY_KERNEL_US
    # what the event pair adds to a REAL launch: a 10-us spin kernel timed per launch between its own events and back to back between one pair
    # (an empty kernel over-corrects: its pair reading is mostly launch latency that real kernels overlap)
    cp, cb = ctypes.c_double(), ctypes.c_double()
    _lib.check(lib.opp_profile_event_calibration(200, 10.0, ctypes.byref(cp), ctypes.byref(cb), torch.cuda.current_stream(dev).cuda_stream), "event_calibration")
    event_extra_us = min(max(cp.value - cb.value, 0.0), max(event_pair_us - empty_kernel_us, 0.0))
    for cfg_id, kind, tile, what in GEMM_SYMBOLS:
        spid = 0 if (kind == 2 and precision == "fp16x2") else pid      # fp16x2: the score GEMM stays fp32
        ms, fl, n = prof_run(lib, _lib, torch, dev, step, cfg_id, kind, nsteps)
        if n <= 0 or ms <= 0:
            continue
        speak = MFMA_PEAK["fp32"] if spid == 0 else peak
        sym = "%s, 0, %d, %d" % (tile, DEPTH_OF_CFG.get(cfg_id, 2), spid)
        ach = fl / (ms * 1e-3) / 1e12
        meas.append({"bound": "mfma", "achieved": round(ach, 2), "peak": round(speak, 1), "unit": "TFLOP/s",
                     "frac": round(ach / speak, 4), "traffic": traffic_of(traffic, sym),
                     "kernel": "opp_gemm_kernel<%s> (%s, %s operands)" % (sym, what, ["fp32", "fp16x2", "bf16x3"][spid]),
                     "symbol": sym, "measured": how, "launches": n, "launches_per_forward": round(n / nsteps, 2),
                     "avg_launch_us": round(ms * 1e3 / n, 2), "us_per_forward": round(ms * 1e3 / nsteps, 1),
                     "alg_gflop_per_launch": round(fl / n / 1e9, 3)})
    for sid, kname, what in MFMA_SYMBOLS:
        ms, fl, n = prof_run(lib, _lib, torch, dev, step, sid, 0, nsteps)
        if n <= 0 or ms <= 0:
            continue
        ach = fl / (ms * 1e-3) / 1e12
        meas.append({"bound": "mfma", "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
                     "frac": round(ach / peak, 4), "traffic": traffic_of(traffic, None, kname),
                     "kernel": "%s (%s, %s operands)" % (kname, what, precision), "symbol": kname, "measured": how, "launches": n,
                     "launches_per_forward": round(n / nsteps, 2), "avg_launch_us": round(ms * 1e3 / n, 2),
                     "us_per_forward": round(ms * 1e3 / nsteps, 1), "alg_gflop_per_launch": round(fl / n / 1e9, 3)})
    for sid, kname, what in HBM_SYMBOLS:
        ms, by, n = prof_run(lib, _lib, torch, dev, step, sid, 0, nsteps)
        if n <= 0 or ms <= 0:
            continue
        ach = by / (ms * 1e-3) / 1e9
        meas.append({"bound": "hbm", "achieved": round(ach, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                     "frac": round(ach / PEAK_HBM_GBS, 4), "traffic": traffic_of(traffic, None, kname),
                     "kernel": "%s (%s)" % (kname, what), "symbol": kname, "measured": how, "launches": n,
                     "launches_per_forward": round(n / nsteps, 2), "avg_launch_us": round(ms * 1e3 / n, 2),
                     "us_per_forward": round(ms * 1e3 / nsteps, 1), "alg_mbytes_per_launch": round(by / n / 1e6, 3)})
    if not meas:
        return None
    # the event pair around a launch reads `event_pair_us` even for an EMPTY kernel (whose own duration in the rocprofv3 kernel
    # trace is EMPTY_KERNEL_US), so event_pair_us - EMPTY_KERNEL_US of every reading is not the kernel: 30 ... 60 % of a sub-15-us
    # launch, 5 ... 15 % of a 40-us one.  `frac` stays the raw reading; `frac_event_corrected` is what the kernel trace shows.
    for m in meas:
        t = max(m["avg_launch_us"] - event_extra_us, 0.25 * m["avg_launch_us"])
        m["avg_launch_us_event_corrected"] = round(t, 2)
        m["frac_event_corrected"] = round(m["frac"] * m["avg_launch_us"] / t, 4)
    # one entry per KERNEL SYMBOL (what a rocprofv3 trace lists): launch shapes of the same template instance are merged, their own
    # figures stay under `launch_shapes`, and the dominant kernel is picked by the merged time per forward
    for keep_sym, gone_sym in SAME_SYMBOL:
        a = next((m for m in meas if m["symbol"] == keep_sym), None)
        b = next((m for m in meas if m["symbol"] == gone_sym), None)
        if a is None or b is None:
            continue
        shapes = [{k: x.get(k) for k in ("kernel", "launches_per_forward", "avg_launch_us", "avg_launch_us_event_corrected", "us_per_forward",
                                        "alg_gflop_per_launch", "achieved", "frac", "frac_event_corrected", "traffic")} for x in (a, b)]
        n = a["launches"] + b["launches"]
        us_f = a["us_per_forward"] + b["us_per_forward"]
        fl = a["alg_gflop_per_launch"] * a["launches"] + b["alg_gflop_per_launch"] * b["launches"]          # GFLOP over the pass
        tot_us = a["avg_launch_us"] * a["launches"] + b["avg_launch_us"] * b["launches"]
        tot_us_c = a["avg_launch_us_event_corrected"] * a["launches"] + b["avg_launch_us_event_corrected"] * b["launches"]
        ach = fl * 1e9 / (tot_us * 1e-6) / 1e12
        a.update({"launches": n, "launches_per_forward": round(a["launches_per_forward"] + b["launches_per_forward"], 2),
                  "avg_launch_us": round(tot_us / n, 2), "avg_launch_us_event_corrected": round(tot_us_c / n, 2),
                  "us_per_forward": round(us_f, 1), "alg_gflop_per_launch": round(fl / n, 3), "achieved": round(ach, 2),
                  "frac": round(ach / a["peak"], 4), "frac_event_corrected": round(ach / a["peak"] * tot_us / tot_us_c, 4),
                  "traffic": a.get("traffic") or b.get("traffic"),      # (the PMC summary keys by template + workgroup count: both shapes have 256)
                  "launch_shapes": shapes,
                  "kernel": a["kernel"] + " -- all launch shapes of this symbol: unsplit (1/4-resolution stage) + 4 K slices (1/8-resolution stage)"})
        meas.remove(b)
    meas.sort(key=lambda m: -m["us_per_forward"])
    # the line stays short enough for log tails: strings every entry shares are kept once, on the dominant kernel's entry
    src = None
    for m in meas:
        for t in ([m["traffic"]] if isinstance(m["traffic"], dict) and "per_launch_shape" not in m["traffic"] else
                  list(m["traffic"]["per_launch_shape"].values()) if isinstance(m["traffic"], dict) else []):
            src = t.pop("source", None) or src
    for m in meas[1:]:
        m.pop("measured", None)
    roof = dict(meas[0])
    if src:
        roof["traffic_source"] = src
    roof["other_kernels"] = meas[1:]
    roof["event_pair_us"] = round(event_pair_us, 2)
    roof["empty_kernel_us"] = round(empty_kernel_us, 2)
    roof["event_extra_us"] = round(event_extra_us, 2)
    roof["event_calibration"] = {"spin_kernel_pair_us": round(cp.value, 2), "spin_kernel_back_to_back_us": round(cb.value, 2)}
    roof["event_correction"] = ("frac_event_corrected: launch time minus event_extra_us = what a 10-us spin kernel reads between its own event pair "
                                "minus its back-to-back launch interval, measured in this run (event_pair_us / empty_kernel_us: the same for an empty kernel)")
    return roof


def other_legs(torch, dev, cfg, models, run_steps, step, precision, n_streams, args, lib, _lib):
    """Secondary measurements of the same run: the other GEMM arithmetics on the same workload, and the full
    coarse-to-fine forward on a bank with ~1500 confident matches (fine stage timed with HIP events)."""
    legs = {}
    other = {}
    for p in ("fp32",):
        if p == precision:
            continue
        for m in models:
            m.set_gemm_precision(p).to(dev)
        for k in range(n_streams):
            step(0, k)
        torch.cuda.synchronize(dev)
        n = min(args.steps * max(1, args.images_per_step), 240)     # >= 0.5 s: the start-up of run_steps' host threads is a few ms each
        t1 = time.perf_counter()
        run_steps(n)
        torch.cuda.synchronize(dev)
        other[p] = {"value": round(n / (time.perf_counter() - t1), 3), "unit": "images/s", "steps": n,
                    "note": "exact fp32 MFMA GEMMs" if p == "fp32" else
                            "opt-in fast mode, operands NARROWER than fp32 (22-bit mantissa, fp16 range): not the headline"}
    for m in models:
        m.set_gemm_precision(precision).to(dev)
    legs["other_arithmetics"] = other
    policy = getattr(models[0], "tile_policy", "latency")
    if n_streams > 1:
        # the same workload with the other tile policy (bit-identical results): latency = every launch sized to fill the chip on
        # its own, throughput = least CU time per launch
        other_policy = "latency" if policy == "throughput" else "throughput"
        for m in models:
            m.set_tile_policy(other_policy).to(dev)
        for k in range(n_streams):
            step(0, k)
        torch.cuda.synchronize(dev)
        run_steps(2 * n_streams)
        n = min(args.steps * max(1, args.images_per_step), 320)
        t1 = time.perf_counter()
        run_steps(n)
        torch.cuda.synchronize(dev)
        legs["%s_tiles_leg" % other_policy] = {"value": round(n / (time.perf_counter() - t1), 3), "unit": "images/s", "steps": n,
                                               "note": "opp_config.tile_policy = %s instead of %s" % (other_policy, policy)}
        for m in models:
            m.set_tile_policy(policy).to(dev)
    if not args.fine:
        # the same coarse-only workload without the fine feature map nothing reads (model.set_skip_unused_fine_map: an opt-in
        # dead-branch elimination the reference cannot do; NOT the headline, which launches every operator of the reference)
        for m in models:
            m.set_skip_unused_fine_map(True)
        for k in range(n_streams):
            step(0, k)
        torch.cuda.synchronize(dev)
        run_steps(2 * n_streams)
        n = min(args.steps * max(1, args.images_per_step), 320)
        t1 = time.perf_counter()
        run_steps(n)
        torch.cuda.synchronize(dev)
        legs["coarse_only_without_unused_fine_map_leg"] = {
            "value": round(n / (time.perf_counter() - t1), 3), "unit": "images/s", "steps": n,
            "note": "fine_matching.enable = False and the FPN fine branch (dead: not an output, read by nothing) not launched; "
                    "match indices / confidences identical"}
        for m in models:
            m.set_skip_unused_fine_map(False)
    # the headline keeps the image-independent work on the resident object cached (keypoint MLP + bank transpose, and since round 5
    # the transformer prefix: layer 0 on the 3D stream + its layer-1 projections / KV sums); this leg redoes all of it for every
    # image, i.e. does exactly the reference's per-image work
    for m in models:
        m.cache_object_tokens = False
        m.invalidate_object_cache()
    for k in range(n_streams):
        step(0, k)
    torch.cuda.synchronize(dev)
    run_steps(2 * n_streams)
    n = min(args.steps * max(1, args.images_per_step), 320)
    t1 = time.perf_counter()
    run_steps(n)
    torch.cuda.synchronize(dev)
    legs["object_token_cache_off_leg"] = {"value": round(n / (time.perf_counter() - t1), 3), "unit": "images/s", "steps": n,
                                          "note": "cache_object_tokens = False: keypoint encoding, bank transpose and every transformer layer on both "
                                                  "streams per image like OnePosePlusModel.py:144-164"}
    for m in models:
        m.cache_object_tokens = True
    try:
        legs["fine_leg"] = fine_leg(torch, dev, precision, lib, _lib)
    except Exception as e:      # the fixture is optional for the headline
        legs["fine_leg"] = {"error": str(e)}
    try:
        legs["train_leg"] = train_leg(torch, dev, precision)
    except Exception as e:
        legs["train_leg"] = {"error": str(e)}
    try:
        torch.cuda.empty_cache()
        legs["train_leg_n15000"] = train_leg(torch, dev, precision, N=15000, light=True)
    except Exception as e:
        legs["train_leg_n15000"] = {"error": str(e)[:300]}
    torch.cuda.empty_cache()
    return legs


def train_leg(torch, dev, precision, nsteps=2, step_profiler=None, N=7000, light=False):
    """One training step at the per-GPU shape of BASELINE configs[4] (B = 4, 512x512, N = 7000 points padded as the
    reference's dataset does, train.yaml:185,194): train()-mode forward on the HIP path (BatchNorm batch statistics,
    training branch of get_coarse_match, fine level on the padded matches) built ONCE as a graph of autograd nodes whose
    forward and backward are HIP kernels (onepose_plus_plus_amd/train_autograd.py: backbone with a tape, Linear, linear
    attention, LayerNorm, coarse matcher, fine windows), `fine_supervision` + `Loss` of this package (focal loss over the
    115 M-entry confidence matrix and its gradient in HIP), backward through those nodes and an AdamW update."""
    from onepose_plus_plus_amd import OnePosePlus_model, default_config, _lib
    from onepose_plus_plus_amd.synthetic import make_state_dict, make_inputs
    B, hw = 4, (512, 512)
    cfg = default_config(thr=0.2)
    model = OnePosePlus_model(cfg).set_gemm_precision(precision).to(dev)
    model.load_state_dict(make_state_dict(cfg, 0), strict=True)
    model.train()
    parts = [make_inputs(N, hw, 30 + b) for b in range(B)]
    base = {k: torch.cat([p[k] for p in parts], 0).to(dev) for k in parts[0]}
    g = torch.Generator().manual_seed(9)
    gt = torch.zeros(B, N, 4096, dtype=torch.int16)
    for b in range(B):
        gt[b, torch.randperm(N, generator=g)[:1500], torch.randperm(4096, generator=g)[:1500]] = 1
    base["conf_matrix_gt"] = gt.to(dev)
    from onepose_plus_plus_amd.losses import Loss, fine_supervision
    loc = torch.full((B, N, 4096, 2), -50.0, device=dev)                      # fine_location_matrix_gt as the loader pads it
    pos = torch.nonzero(base["conf_matrix_gt"] == 1)
    cell = torch.stack([pos[:, 2] % 64, pos[:, 2] // 64], 1).float() * 8.0
    loc[pos[:, 0], pos[:, 1], pos[:, 2]] = cell + torch.rand(len(pos), 2, device=dev) * 4.0 - 2.0
    base["fine_location_matrix_gt"] = loc
    hparams = {"OnePosePlus": cfg, "loss": {"coarse_type": "focal", "coarse_weight": 1.0, "fine_type": "l2_with_std",
                                            "fine_weight": 0.81, "focal_alpha": 0.5, "focal_gamma": 2.0, "pos_weight": 1.0,
                                            "neg_weight": 1.0, "fine_correct_thr": 1.0}}      # train.yaml:129-144
    loss_mod = Loss(hparams["loss"]).train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-6)

    def fwd_only():
        d = dict(base)
        with torch.no_grad():
            model(d)

    def full_step():                         # PL_OnePosePlus.training_step, lightning_model:54-60, + the optimiser
        d = dict(base)
        model(d)
        fine_supervision(d, hparams)
        loss_mod(d)
        opt.zero_grad(set_to_none=True)
        d["loss"].backward()
        opt.step()
        return float(d["loss"].detach())

    def loss_only():
        d = dict(base)
        with torch.no_grad():
            model(d)
        conf = d["conf_matrix"].detach().requires_grad_(True)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        lc = loss_mod.compute_coarse_loss(conf, d["conf_matrix_gt"])
        lc.backward()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    def timed(fn):
        fn()                                  # two untimed calls: code objects, allocator pools and workspaces reach steady state
        fn()
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        for _ in range(nsteps):
            r = fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t) / nsteps * 1e3, r

    fwd_ms, _ = timed(fwd_only)
    step_ms, loss = timed(full_step)
    # roofline of the step: a training step is ~3x the forward's FLOPs (forward + input gradients + weight gradients), MFMA-bound;
    # its largest kernel is conv_wgrad_kernel (every convolution's and every Linear's weight gradient), timed with HIP events on the
    # launch stream over one more step
    lib = _lib.load()
    flops_fwd = B * 2.0 * (126.726e9 + 6 * (4096 + N) * 671744 + N * 4096 * 256)
    peak = MFMA_PEAK[precision]
    roof = {"bound": "mfma", "step_alg_tflop": round(3 * flops_fwd / 1e12, 3), "achieved": round(3 * flops_fwd / (step_ms * 1e-3) / 1e12, 2),
            "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(3 * flops_fwd / (step_ms * 1e-3) / 1e12 / peak, 4),
            "note": "step FLOPs = 3 x the forward's algorithmic FLOPs over the batch (coarse level; the fine level adds < 2 %)"}
    try:
        _lib.check(lib.opp_profile_start(1013, 0, 4096), "profile_start")
        full_step()
        torch.cuda.synchronize(dev)
        ms, wk, nl = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        _lib.check(lib.opp_profile_stop(ctypes.byref(ms), ctypes.byref(wk), ctypes.byref(nl)), "profile_stop")
        if nl.value > 0 and ms.value > 0:
            ach = wk.value / (ms.value * 1e-3) / 1e12
            roof["dominant_kernel"] = {"kernel": "conv_wgrad_kernel (weight gradient of every convolution and Linear, pixel-major operands)",
                                       "launches_per_step": nl.value, "ms_per_step": round(ms.value, 3), "alg_gflop_per_step": round(wk.value / 1e9, 1),
                                       "achieved": round(ach, 2), "frac": round(ach / peak, 4),
                                       "measured": "HIP events on the launch stream around every launch of one step"}
    except Exception as e:
        roof["dominant_kernel"] = {"error": str(e)[:120]}
    if light:
        return {"workload": "as train_leg with N = %d points per sample (BASELINE configs[4]: '15k-point clouds')" % N,
                "forward_ms": round(fwd_ms, 2), "step_ms": round(step_ms, 1), "step_samples_per_s": round(B / step_ms * 1e3, 2),
                "loss": round(loss, 5), "roofline": roof}
    if step_profiler is not None:            # tools/train_probe.py: a profiler context around warmed-up steps only
        with step_profiler:
            for _ in range(nsteps):
                full_step()
            torch.cuda.synchronize(dev)
    loss_only()
    focal_ms = min(loss_only() for _ in range(3))
    bwd = backward_kernel_split(torch, dev, model, base, hparams, loss_mod, fine_supervision)
    n_conf = B * N * 4096
    return {"workload": "BASELINE configs[4] per-GPU shape: B = 4, 512x512, %d points, train() mode, single stream; "
                        "step = model(batch), fine_supervision, Loss (focal + l2_with_std, train.yaml:129-144), backward, AdamW" % N,
            "roofline": roof,
            "forward_ms": round(fwd_ms, 2), "forward_samples_per_s": round(B / fwd_ms * 1e3, 1),
            "step_ms": round(step_ms, 1), "step_samples_per_s": round(B / step_ms * 1e3, 2), "loss": round(loss, 5),
            "focal_loss_fwd_bwd_ms": round(focal_ms, 3),
            "focal_loss_alg_gbs": round(n_conf * 16.0 / (focal_ms * 1e-3) / 1e9, 1),
            "backward_ms_in_opp_kernels": bwd.get("hand_written_ms"), "backward_kernel_split": bwd,
            "note": "forward and backward = one graph of HIP nodes (backbone conv dgrad / wgrad + BatchNorm backward, Linear, linear "
                    "attention, LayerNorm, dual softmax, focal loss); PyTorch = autograd tape, elementwise glue, AdamW"}


def library_kernel_names():
    """names of every __global__ kernel of libopp_hip.so, read from the sources next to it (csrc/*.hip travel with the library)"""
    import glob
    import re
    names = set()
    for f in glob.glob(os.path.join(ROOT, "onepose_plus_plus_amd", "csrc", "*.hip")):
        with open(f) as fh:
            src = fh.read()
        names.update(re.findall(r"__global__(?:\s+__launch_bounds__\([^)]*\))?\s+void\s+(\w+)\s*\(", src))
    return names


def classify_kernel(name, ours):
    """-> "ours" (a kernel of libopp_hip.so, matched POSITIVELY by name), "vendor" (MIOpen / rocBLAS / Tensile / rocPRIM / hipCUB /
    Thrust: somebody else's tuned library), "aten" (PyTorch's own elementwise / reduction / copy kernels) or "other" """
    import re
    low = name.lower()
    if "at::" not in name and "rocprim" not in low and any(tok in ours for tok in re.findall(r"[A-Za-z_]\w*", name)):
        return "ours"
    if any(t in low for t in ("miopen", "igemm", "cijk_", "rocblas", "tensile", "rocprim", "hipcub", "thrust", "cub::")):
        return "vendor"
    if "at::native" in name or "at::cuda" in name or "memcpy" in low or "memset" in low or "fill" in low or "copybuffer" in low:
        return "aten"
    return "other"


def backward_kernel_split(torch, dev, model, base, hparams, loss_mod, fine_supervision):
    """Device time of ONE backward pass (loss.backward() of the training step) by who wrote the kernel, from torch.profiler's
    kernel records: hand-written HIP of libopp_hip.so (matched positively against the kernel names in csrc/*.hip) vs PyTorch's own
    elementwise / reduction kernels (at::native) vs vendor libraries (MIOpen / rocBLAS / Tensile / rocPRIM behind torch indexing)
    vs anything else."""
    try:
        from torch.profiler import ProfilerActivity, profile
        d = dict(base)
        model(d)
        fine_supervision(d, hparams)
        loss_mod(d)
        for p in model.parameters():
            p.grad = None
        torch.cuda.synchronize(dev)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            d["loss"].backward()
            torch.cuda.synchronize(dev)
        lib_names = library_kernel_names()
        tsum = {"ours": 0.0, "aten": 0.0, "vendor": 0.0, "other": 0.0}
        seen = {"vendor": [], "other": []}
        for e in prof.key_averages():
            t = getattr(e, "self_device_time_total", None)
            if t is None:
                t = getattr(e, "self_cuda_time_total", 0.0)
            if not t:
                continue
            kind = classify_kernel(e.key, lib_names)
            tsum[kind] += t
            if kind in seen:
                seen[kind].append(e.key[:60])
        tot = sum(tsum.values())
        return {"hand_written_ms": round(tsum["ours"] / 1e3, 2), "aten_elementwise_ms": round(tsum["aten"] / 1e3, 2),
                "vendor_library_ms": round(tsum["vendor"] / 1e3, 2), "other_ms": round(tsum["other"] / 1e3, 2),
                "hand_written_frac": round(tsum["ours"] / tot, 3) if tot else None, "vendor_kernels": seen["vendor"][:6],
                "other_kernels": seen["other"][:6]}
    except Exception as e:                    # the split is a report, never a reason to lose the leg
        return {"error": str(e)[:200]}


def fine_leg(torch, dev, precision, lib, _lib, nsteps=10):
    """Full coarse-to-fine forward (BASELINE configs[2] shape) on the committed high-confidence bank
    (tests/golden/highconf_512x512_n3000.npz: ~1500 matches): whole-forward rate and the fine stage on its own."""
    import numpy as np
    from onepose_plus_plus_amd import OnePosePlus_model, default_config
    from onepose_plus_plus_amd.synthetic import make_state_dict, make_inputs
    from tests.golden.cases import HIGHCONF_CASES
    name = "highconf_512x512_n3000"
    hw, n, n_planted, thr, wseed, iseed = HIGHCONF_CASES[name]
    cfg = default_config(thr=thr)
    model = OnePosePlus_model(cfg).eval().set_gemm_precision(precision).to(dev)
    model.load_state_dict(make_state_dict(cfg, wseed), strict=True)
    data = make_inputs(n, hw, iseed)
    gold = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    data["keypoints3d"] = torch.from_numpy(gold["keypoints3d"])               # the fixture's own object (tests/helpers.highconf_setup):
    data["descriptors3d_coarse_db"] = torch.from_numpy(gold["bank_c_f16"]).float()   # the parity-checked input, M = 1487
    data = {k: v.to(dev) for k, v in data.items()}

    def fwd():
        d = dict(data)
        with torch.no_grad():
            model(d)
        return d
    for _ in range(3):
        d = fwd()
    torch.cuda.synchronize(dev)
    M = int(d["mconf"].numel())
    t = time.perf_counter()
    for _ in range(nsteps):
        fwd()
    torch.cuda.synchronize(dev)
    full_ms = (time.perf_counter() - t) / nsteps * 1e3

    def span(symbol):
        """HIP-event time / algorithmic bytes / launches of one profiler symbol over nsteps forwards."""
        _lib.check(lib.opp_profile_start(symbol, 0, nsteps * 40), "profile_start")
        for _ in range(nsteps):
            fwd()
        torch.cuda.synchronize(dev)
        ms, by, nl = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        _lib.check(lib.opp_profile_stop(ctypes.byref(ms), ctypes.byref(by), ctypes.byref(nl)), "profile_stop")
        return ms.value / nsteps, by.value / nsteps, nl.value / nsteps

    out = {"workload": "full coarse-to-fine forward, %dx%d x %d points, thr %.1f, bank optimised for confident matches "
                       "(tests/golden/%s.npz), single stream" % (hw[0], hw[1], n, thr, name),
           "matches": M, "ms_per_forward": round(full_ms, 3), "images_per_s": round(1e3 / full_ms, 2),
           "fine_branch_path": model._rt.get("fine_path")}
    # the match-driven fine branch (opp_fine_patches) against the dense fine map inside the fused coarse call, same matches, at the
    # fixture's own M and at a typical few-hundred-match load (threshold raised until ~300 of the fixture's matches remain)
    try:
        mc = torch.sort(d["mconf"].detach().float().cpu()).values
        cases = [("all", thr)]
        if M > 320:
            cases.append(("about_300", float(0.5 * (mc[M - 301] + mc[M - 300]))))
        md = {}
        for label, th in cases:
            cfg_t = default_config(thr=th)
            row = {"thr": round(th, 6)}
            for pname, pmax in (("dense_ms", 0), ("patch_ms", 1 << 20)):
                mt = OnePosePlus_model(cfg_t).eval().set_gemm_precision(precision).set_fine_patch_max_matches(pmax).to(dev)
                mt.fine_patch_pixels_per_match = 0                   # force the path under test at every match count
                mt.load_state_dict(make_state_dict(cfg_t, wseed), strict=True)

                def fwd_t():
                    dd = dict(data)
                    with torch.no_grad():
                        mt(dd)
                    return dd
                for _ in range(3):
                    dd = fwd_t()
                torch.cuda.synchronize(dev)
                t = time.perf_counter()
                for _ in range(nsteps):
                    fwd_t()
                torch.cuda.synchronize(dev)
                row[pname] = round((time.perf_counter() - t) / nsteps * 1e3, 3)
                row["matches"] = int(dd["mconf"].numel())
                del mt
            row["patch_speedup"] = round(row["dense_ms"] / row["patch_ms"], 3)
            if label == "about_300":
                # the same comparison the way the headline is measured: 3 forwards in flight on separate streams (the coarse level of one
                # forward fills the CUs the short patch GEMMs of another leave idle), throughput tiles, images/s
                for pname, pmax in (("dense_images_per_s_3_streams", 0), ("patch_images_per_s_3_streams", 1 << 20)):
                    row[pname] = fine_throughput(torch, dev, cfg_t, make_state_dict(cfg_t, wseed), data, precision, pmax)
                row["patch_speedup_3_streams"] = round(row["patch_images_per_s_3_streams"] / row["dense_images_per_s_3_streams"], 3)
            md[label] = row
        out["match_driven_fine_branch"] = md
    except Exception as e:
        out["match_driven_fine_branch"] = {"error": str(e)[:200]}
    fine_ms, _, nl = span(1003)
    if nl > 0 and fine_ms > 0:
        # the fine level is 17.47 MFLOP per match (window transformer, C = 128) -> MFMA-bound as a whole;
        # its gather / attention / head kernels are HBM-bound and reported against the HBM peak on their own
        gflop = M * 17.47e6 / 1e9
        out.update({"fine_stage_ms": round(fine_ms, 4), "fine_ms_per_1000_matches": round(fine_ms / max(M, 1) * 1000, 4),
                    "fine_stage_alg_gflop": round(gflop, 2), "fine_stage_tflops": round(gflop / fine_ms, 2),
                    "fine_stage_frac_of_mfma_peak": round(gflop / fine_ms / MFMA_PEAK[precision], 4), "kernels": []})
        for sym, label in ((1005, "fine_gather_kernel (5x5 windows + point descriptors, read + written once)"),
                           (1004, "linattn_small_pair_kernel (fine-level linear attention: Q, K, V read, message written)"),
                           (1006, "fine_head_kernel (windows + point tokens read once)")):
            ms, by, k = span(sym)
            if k > 0 and ms > 0:
                gbs = by / (ms * 1e-3) / 1e9
                out["kernels"].append({"kernel": label, "bound": "hbm", "launches_per_forward": round(k, 1),
                                       "avg_launch_us": round(ms / k * 1e3, 2), "alg_mbytes_per_launch": round(by / k / 1e6, 2),
                                       "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                       "frac": round(gbs / PEAK_HBM_GBS, 4)})
    return out


def fine_throughput(torch, dev, cfg, sd, data, precision, patch_max, n_streams=3, n=60):
    """images/s of the full coarse-to-fine forward with `n_streams` forwards in flight (one module + stream + host thread each)"""
    from onepose_plus_plus_amd import OnePosePlus_model
    mods = []
    for _ in range(n_streams):
        m = OnePosePlus_model(cfg).eval().set_gemm_precision(precision).set_tile_policy("throughput").set_fpn_overlap(False)
        m.set_fine_patch_max_matches(patch_max).to(dev)
        m.fine_patch_pixels_per_match = 0
        m.load_state_dict(sd, strict=True)
        mods.append(m)
    streams = [torch.cuda.Stream(device=dev) for _ in range(n_streams)]

    def run(total):
        nxt, lock = [0], threading.Lock()

        def worker(k):
            torch.cuda.set_device(dev)
            while True:
                with lock:
                    i = nxt[0]
                    nxt[0] += 1
                if i >= total:
                    break
                with torch.no_grad(), torch.cuda.stream(streams[k]):
                    mods[k](dict(data))
            streams[k].synchronize()
        th = [threading.Thread(target=worker, args=(k,)) for k in range(n_streams)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    run(3 * n_streams)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    run(n)
    torch.cuda.synchronize(dev)
    return round(n / (time.perf_counter() - t0), 2)


def cpu_baseline(torch, cfg, sd, args, make_inputs):
    """Oracle (port of the reference PyTorch CPU path) timed on the host cores over a bounded
    sample: forwards of the SAME workload for ~cpu_seconds.  The thread count is picked by a
    short calibration (a 256-thread pool on this class of box is slower than a small one), and
    the count actually used is reported as `cores`."""
    from oracle import onepose_oracle as O
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    data = make_inputs(args.n_points, (args.hw, args.hw), seed=1)
    # thread count calibrated on the FULL-SIZE workload (round-4 review: a 128x128 x 500-point toy picked 16 threads, the real
    # forward may prefer more): one warm-up + one timed forward per candidate, ~1 s each
    best, calib = None, {}
    for th in sorted({min(avail, c) for c in (8, 16, 32, 64, 128)}):
        torch.set_num_threads(th)
        O.forward(sd, dict(data), cfg)
        t = time.perf_counter()
        O.forward(sd, dict(data), cfg)
        dt = time.perf_counter() - t
        calib[th] = round(dt, 3)
        if best is None or dt < best[1]:
            best = (th, dt)
    torch.set_num_threads(best[0])
    times = []
    t_end = time.perf_counter() + args.cpu_seconds
    while len(times) < 2 or (time.perf_counter() < t_end and len(times) < 50):
        d = dict(data)
        t = time.perf_counter()
        O.forward(sd, d, cfg)
        times.append(time.perf_counter() - t)
    med = sorted(times)[len(times) // 2]
    used = torch.get_num_threads()
    torch.set_num_threads(1)                  # one forward on ONE thread, for per-core normalisation
    d = dict(data)
    t = time.perf_counter()
    O.forward(sd, d, cfg)
    one = time.perf_counter() - t
    torch.set_num_threads(used)
    return {"value": round(1.0 / med, 4), "unit": "images/s", "cores": used, "kind": "port", "one_thread_images_per_s": round(1.0 / one, 4),
            "thread_calibration_s_per_forward": calib,
            # the reference module itself cannot travel to the GPU box; its figure where it can run (build container, 8 cores)
            "reference_in_build_container": {"value": 0.90, "unit": "images/s", "cores": 8, "source": "BASELINE.md: stubbed reference module, N=5000"},
            "sample_short": "%d forwards of this workload through oracle/onepose_oracle.py = PORT OF the reference fp32 PyTorch CPU path (pinned "
                            "bit-level to it by tests/test_oracle_golden.py), %d of %d threads (fastest of 8..128), median; min %.3f s"
                            % (len(times), best[0], avail, min(times)),
            "sample": "%d forwards of the same %dx%d x %d-pt workload through oracle/onepose_oracle.py "
                      "(fp32 PyTorch CPU, %d of %d available threads: the fastest of {8, 16, 32, 64, 128} on this full-size workload), median; min %.3f s"
                      % (len(times), args.hw, args.hw, args.n_points, best[0], avail, min(times))}


if __name__ == "__main__":
    main()
