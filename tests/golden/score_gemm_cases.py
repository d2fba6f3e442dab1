"""Cases shared by tests/test_score_gemm_gpu.py and tests/golden/gen_score_gemm_digest.py: the coarse matcher on every kernel of
csrc/gemm_ss.hip, at the smallest shapes that reach each branch of its tile setup, K loop and epilogues.  Inputs as in
test_stages_gpu.py::test_two_sweep_matcher_equals_the_materialised_path (tokens of magnitude 4, C = 256, planted matches at noise 0.4,
thr 0.1, bf16x3).

    python -m tests.golden.score_gemm_cases LEG      prints the digests of one leg as JSON (the `persist` leg needs a process of its own:
                                                     OPP_SS_PERSIST is read once)"""
import hashlib
import json
import os
import subprocess
import sys

import torch

PARENT_DIGEST = "score_gemm_parent_digest"        # sha256 of the outputs of the build that precedes the shared pieces of gemm_ss.hip
KEYS = ("conf_matrix", "i_ids", "j_ids", "mconf", "mkpts_query_c")
TILE = 128
PERSIST_WALK_TILES = 544                          # 32 x 17 tiles of the largest case: more than 2 x 256 CUs
# leg -> (set_score_two_sweep, environment): the launcher's rules (opp_gemm_ss) then give
#   res3     gemm_ss_res3_kernel (gemm_ss_kernel<STATS_STORE> where the output rows are not 16-byte multiples)
#   res2     gemm_ss_kernel<STATS_STORE>
#   two      gemm_ss_kernel<STATS>, then <CONF>
#   persist  gemm_ss_persist_kernel above 8 tiles with 16-byte output rows, else gemm_ss_kernel<STATS_STORE>
LEGS = {"res3": (2, {}), "res2": (2, {"OPP_SS_RES3": "0"}), "two": (1, {}), "persist": (2, {"OPP_SS_PERSIST": "1"})}
# name -> (hw_c, N, planted, mask kind of tests/mask_cases.py, legs)
ALL = tuple(LEGS)
CASES = {
    "one_ragged_tile": ((12, 8), 77, 40, None, ALL),          # FULL false everywhere
    "3x3_tiles": ((16, 24), 300, 200, None, ALL),             # six FULL tiles beside a ragged column panel (44 columns)
    "3x3_tiles_masked": ((16, 24), 300, 200, "b", ALL),       # zeros in the second and third row tile (and the first): the row_mask add
    "odd_row_stride": ((11, 7), 130, 40, None, ALL),          # ldc % 4 != 0: the scalar store loops; res3 / persist fall through
    "second_strip": ((36, 32), 300, 200, None, ALL),          # 9 row panels: a one-panel second strip; 27 tiles, persistent kernel
    "persist_walks": ((64, 64), 2100, 1000, None, ("persist",)),   # 544 tiles: a workgroup of the persistent kernel takes a second one
}


def pairs():
    return [(c, leg) for c, v in CASES.items() for leg in v[4]]


def inputs(name):
    hw_c, n, planted, kind, _ = CASES[name]
    g = torch.Generator().manual_seed(5 + n)
    L = hw_c[0] * hw_c[1]
    f2d = torch.randn(L, 256, generator=g) * 4
    f3d = torch.randn(n, 256, generator=g) * 4
    m = min(planted, L, n)
    cells = torch.randperm(L, generator=g)[:m]
    f3d[:m] = f2d[cells] + 0.4 * torch.randn(m, 256, generator=g)
    kpts = torch.rand(n, 3, generator=g) - 0.5
    mask = None
    if kind is not None:
        from tests import mask_cases as MC
        mask = MC.mask((hw_c[0], hw_c[1], n), kind)
        assert (mask[TILE:2 * TILE] == 0).any() and (mask[2 * TILE:] == 0).any()
    return f3d, f2d, hw_c, kpts, mask, m


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def run_leg(leg):
    """-> {"case.leg.key": sha256} of every case of the leg, or {"case.leg.skip": reason}.  Needs a GPU; `persist` needs OPP_SS_PERSIST=1
    from the start of the process."""
    from onepose_plus_plus_amd import default_config
    from onepose_plus_plus_amd.synthetic import make_state_dict
    from tests import hip_ops as ops
    mode, env = LEGS[leg]
    if leg == "persist":
        assert os.environ.get("OPP_SS_PERSIST") == "1"
    cfg = default_config(thr=0.1)
    model = ops.make_model(cfg, make_state_dict(cfg, 0), "bf16x3").set_score_two_sweep(mode).cuda()
    out = {}
    for name, case in CASES.items():
        if leg not in case[4]:
            continue
        if name == "persist_walks":
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            if 2 * cus >= PERSIST_WALK_TILES:
                out["%s.%s.skip" % (name, leg)] = "%d CUs: no workgroup of the persistent kernel walks to a second tile" % cus
                continue
        f3d, f2d, hw_c, kpts, mask, m = inputs(name)
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            got = ops.coarse_match(model, f3d, f2d, hw_c, kpts, 8.0, None, mask=mask)
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        # what keeps the digests from being vacuous: matches are found, and the NaN prefill of conf_matrix is overwritten everywhere
        assert len(got["i_ids"]) > m // 4, (name, leg, len(got["i_ids"]), m)
        assert torch.isfinite(got["conf_matrix"]).all(), (name, leg)
        for k in KEYS:
            out["%s.%s.%s" % (name, leg, k)] = sha(got[k])
    return out


def run_leg_in_child(leg):
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r = subprocess.run([sys.executable, "-m", "tests.golden.score_gemm_cases", leg], env=dict(os.environ, **LEGS[leg][1]),
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def all_digests():
    out = {}
    for leg in LEGS:
        out.update(run_leg_in_child(leg) if leg == "persist" else run_leg(leg))
    # OPP_SS_RES3 acted: the two kernels merge the row statistics differently, so somewhere their confidences differ in the last bit
    assert any(out["%s.res3.conf_matrix" % c] != out["%s.res2.conf_matrix" % c] for c, v in CASES.items() if "res3" in v[4])
    return out


if __name__ == "__main__":
    print(json.dumps(run_leg(sys.argv[1])))
