"""Full-attention kernels (csrc/full_attention.hip) and the forward with full attention, measured with device events after warm-up:
    python tools/fullattn_bench.py [--iters 20] [--skip-forward] [--train]
  * opp_full_attention at the coarse shapes (4096 self, 5000 self, the 4096 <-> 5000 cross pair, 15000 self), both arithmetics:
    us per call, algorithmic TFLOP/s (4 Lq Lk C per direction) and the share of the arithmetic's peak (bf16x3 2500 / 6 = 416.7 TF/s,
    fp32 MFMA 157.3 TF/s);
  * torch.nn.functional.scaled_dot_product_attention (fp32) on the same shapes, for comparison;
  * the whole forward at 512 x 512 x 5000 points, coarse level only, with linear and with full attention (images/s).
  * --train (instead of the above): opp_full_attention_train_forward (forward that keeps the log-sum-exp) and
    opp_full_attention_train_backward (delta pre-pass + dK/dV kernel + dQ kernel) of csrc/full_attention_train.hip at B = 1, 8 heads,
    D = 32, queries x keys = 4096 x 5000 and 4096 x 7000 (cross) and 4096 x 4096, 5000 x 5000, 7000 x 7000 (self), both arithmetics: us per call and the
    backward / forward ratio, to be read against the MFMA products per tile pair: 3 + 4 = 7 in the two backward kernels, 2 in the forward.
One JSON line per measurement.  Kernel times of record come from a separate `rocprofv3 --kernel-trace --stats` run of this tool
(kernel names full_attn_flash_kernel / full_attn_small_kernel)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from onepose_plus_plus_amd import _lib, OnePosePlus_model  # noqa: E402
from onepose_plus_plus_amd.config import default_config  # noqa: E402
from onepose_plus_plus_amd.synthetic import make_state_dict, make_inputs  # noqa: E402

PEAK = {"bf16x3": 2500.0 / 6, "fp32": 157.3}
PREC = {"bf16x3": 3, "fp32": 0}
# (label, len0, len1, cross): Lq x Lk per direction
SHAPES = [("self_4096", 4096, 4096, 0), ("self_5000", 5000, 5000, 0), ("cross_4096x5000", 4096, 5000, 1), ("self_15000", 15000, 15000, 0)]


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters   # us


def bench_kernels(iters):
    lib = _lib.load()
    C, nhead = 256, 8
    for label, l0, l1, cross in SHAPES:
        # self shapes: one stream of l0 rows attending to itself (the second stream is a single row); cross: both directions
        if cross:
            n0, n1 = l0, l1
            flop = 4.0 * l0 * l1 * C * 2
        else:
            n0, n1 = l0, 1
            flop = 4.0 * l0 * l0 * C + 4.0 * C
        qkv = torch.randn(n0 + n1, 3 * C, device="cuda")
        msg = torch.empty(n0 + n1, C, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        for prec in ("bf16x3", "fp32"):
            def run():
                _lib.check(lib.opp_full_attention(qkv.data_ptr(), 1, n0, n1, C, nhead, cross, PREC[prec], msg.data_ptr(), None, 0, s),
                           "opp_full_attention")
            us = timed(run, iters)
            tf = flop / us * 1e-6
            print(json.dumps({"what": "opp_full_attention", "shape": label, "precision": prec, "us": round(us, 1), "tflops": round(tf, 1),
                              "share_of_peak": round(tf / PEAK[prec], 3)}), flush=True)
        q = qkv[:, :C].view(1, -1, nhead, 32).transpose(1, 2)
        k = qkv[:, C:2 * C].view(1, -1, nhead, 32).transpose(1, 2)
        v = qkv[:, 2 * C:].view(1, -1, nhead, 32).transpose(1, 2)
        if cross:
            def sdpa():
                torch.nn.functional.scaled_dot_product_attention(q[:, :, :n0], k[:, :, n0:], v[:, :, n0:])
                torch.nn.functional.scaled_dot_product_attention(q[:, :, n0:], k[:, :, :n0], v[:, :, :n0])
        else:
            def sdpa():
                torch.nn.functional.scaled_dot_product_attention(q[:, :, :n0], k[:, :, :n0], v[:, :, :n0])
        us = timed(sdpa, iters)
        print(json.dumps({"what": "torch_sdpa_fp32", "shape": label, "us": round(us, 1), "tflops": round(flop / us * 1e-6, 1)}), flush=True)


def bench_forward(iters):
    for attention in ("linear", "full"):
        cfg = default_config(thr=0.1, fine=False)
        cfg["loftr_coarse"]["attention"] = attention
        cfg["loftr_fine"]["attention"] = attention
        m = OnePosePlus_model(cfg).eval()
        m.load_state_dict(make_state_dict(cfg, 0), strict=True)
        m = m.cuda()
        d0 = {k: v.cuda() for k, v in make_inputs(5000, (512, 512), 1).items()}

        def fwd():
            with torch.no_grad():
                m(dict(d0))
        us = timed(fwd, iters)
        print(json.dumps({"what": "forward_512x512_n5000_coarse", "attention": attention, "ms": round(us / 1e3, 3),
                          "images_per_s": round(1e6 / us, 1)}), flush=True)


TRAIN_SHAPES = [("cross_4096x5000", 4096, 5000), ("cross_4096x7000", 4096, 7000), ("self_4096", 4096, 4096), ("self_5000", 5000, 5000), ("self_7000", 7000, 7000)]


def bench_train(iters):
    lib = _lib.load()
    B, H, D = 1, 8, 32
    s = torch.cuda.current_stream().cuda_stream
    for label, L, S in TRAIN_SHAPES:
        q = torch.randn(B, L, H, D, device="cuda")
        k, v = torch.randn(B, S, H, D, device="cuda"), torch.randn(B, S, H, D, device="cuda")
        go = torch.randn(B, L, H, D, device="cuda")
        out, lse = torch.empty_like(q), torch.empty(B, H, L, device="cuda")
        gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        nb = lib.opp_full_attention_train_workspace_bytes(B, L, S, H, D)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        for prec in ("bf16x3", "fp32"):
            def fwd():
                _lib.check(lib.opp_full_attention_train_forward(q.data_ptr(), k.data_ptr(), v.data_ptr(), B, L, S, H, D, PREC[prec], out.data_ptr(),
                                                                lse.data_ptr(), ws.data_ptr(), nb, s), "opp_full_attention_train_forward")

            def bwd():
                _lib.check(lib.opp_full_attention_train_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(),
                                                                 go.data_ptr(), B, L, S, H, D, PREC[prec], gq.data_ptr(), gk.data_ptr(),
                                                                 gv.data_ptr(), ws.data_ptr(), nb, s), "opp_full_attention_train_backward")
            us_f, us_b = timed(fwd, iters), timed(bwd, iters)
            flop = 2.0 * L * S * H * D          # one L x S x D product over all heads
            print(json.dumps({"what": "opp_full_attention_train", "shape": label, "precision": prec, "forward_us": round(us_f, 1),
                              "backward_us": round(us_b, 1), "backward_over_forward": round(us_b / us_f, 2), "mfma_products": "7 : 2",
                              "forward_tflops": round(2 * flop / us_f * 1e-6, 1), "backward_tflops": round(7 * flop / us_b * 1e-6, 1)}),
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip-forward", action="store_true")
    ap.add_argument("--train", action="store_true")
    a = ap.parse_args()
    if a.train:
        bench_train(a.iters)
        return
    bench_kernels(a.iters)
    if not a.skip_forward:
        bench_forward(a.iters)


if __name__ == "__main__":
    main()
