"""What one image pair costs through `LoFTRMatcher` (onepose_plus_plus_amd/loftr.py) on the device: milliseconds per pair at 512 x 512
and 480 x 640, coarse-only (SfM's `enable_fine_matching=False`) and with the fine level at W = 9, in both arithmetics, with the number
of matches M; beside them the 2D-3D forward of `OnePosePlus_model` at N = 4096 points on the same build -- the same token counts at
512 x 512 (4096 + 4096), six encoder layers in its fused default path against the matcher's eight unfused ones.

Inputs: two crops, (16, 24) pixels apart, of the texture of tests/golden/loftr_cases.py generated at the size they need; weights:
`content_state_dict` of the same file, under which coarse matching follows the image content, so that the fine level has a realistic
number of matches to work on at the shipped threshold 0.2 (plain random weights match almost nothing).  Each figure is the median
of `--reps` forwards between one pair of device events each, after `--warmup` forwards of the same shape; a forward contains its
one device-to-host copy (the match count).  No pass / fail threshold: the file is the record.  A per-kernel trace belongs in a run of its own:

    python tools/loftr_bench.py [--reps 20] [--warmup 5] > profiles/loftr_bench.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/loftr_bench.py --trace-one 512x512
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHIFT = (16, 24)
THR = 0.2


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def pair(hw):
    """two crops, SHIFT apart, of one texture generated at the size they need"""
    from tests.golden.loftr_cases import texture
    tex = texture(hw=(hw[0] + SHIFT[0], hw[1] + SHIFT[1]))
    a = tex[:hw[0], :hw[1]]
    b = tex[SHIFT[0]:SHIFT[0] + hw[0], SHIFT[1]:SHIFT[1] + hw[1]]
    return a[None, None].contiguous().cuda(), b[None, None].contiguous().cuda()


def time_forward(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return median(ms), min(ms), max(ms)


def matcher(precision, fine):
    from onepose_plus_plus_amd.loftr import LoFTRMatcher
    from tests.golden.loftr_cases import content_state_dict, loftr_cfg
    m = LoFTRMatcher(loftr_cfg(THR, 9), enable_fine_matching=fine).eval()
    m.load_state_dict(content_state_dict(), strict=True)
    m.set_gemm_precision(precision)
    return m.cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace-one", default=None, help="HxW: three forwards with the fine level in bf16x3 and nothing else (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loftr_bench: no GPU (timings are taken on the device only)")
    if args.trace_one:
        hw = tuple(int(v) for v in args.trace_one.split("x"))
        a, b = pair(hw)
        m = matcher("bf16x3", True)
        with torch.no_grad():
            for _ in range(3):
                d = m({"image0": a, "image1": b})
        torch.cuda.synchronize()
        print("traced 3 forwards at %dx%d, M = %d" % (hw + (len(d["i_ids"]),)))
        return
    print("device: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    print("LoFTRMatcher, ms per image pair: median of %d forwards (min, max) after %d warm-up forwards; thr %g, W = 9, shift %s" %
          (args.reps, args.warmup, THR, SHIFT))
    for hw in ((512, 512), (480, 640)):
        a, b = pair(hw)
        for precision in ("bf16x3", "fp32"):
            for fine in (False, True):
                m = matcher(precision, fine)
                out = {}

                def fn():
                    with torch.no_grad():
                        out["d"] = m({"image0": a, "image1": b})
                t = time_forward(fn, args.reps, args.warmup)
                print("  %dx%d %-6s %-22s %9.3f ms   (min %.3f, max %.3f)   M = %d" %
                      (hw + (precision, "with fine level W = 9" if fine else "coarse only", t[0], t[1], t[2], len(out["d"]["i_ids"]))))
                del m
    # the 2D-3D forward on the same build: 4096 image tokens + 4096 points, six layers, default (fused) path
    from onepose_plus_plus_amd import OnePosePlus_model, default_config
    from onepose_plus_plus_amd.synthetic import make_inputs, make_state_dict
    cfg = default_config(thr=0.0)
    sd = make_state_dict(cfg, 0)
    data = {k: v.cuda() for k, v in make_inputs(4096, (512, 512), 1).items()}
    for precision in ("bf16x3", "fp32"):
        model = OnePosePlus_model(cfg).eval()
        model.load_state_dict(sd, strict=True)
        model.set_gemm_precision(precision)
        model.cuda()
        out = {}

        def fn():
            d = dict(data)
            with torch.no_grad():
                model(d)
            out["d"] = d
        t = time_forward(fn, args.reps, args.warmup)
        print("  2D-3D OnePosePlus_model 512x512, N = 4096, %-6s %9.3f ms   (min %.3f, max %.3f)   M = %d" %
              (precision, t[0], t[1], t[2], len(out["d"]["i_ids"])))
        del model


if __name__ == "__main__":
    main()
