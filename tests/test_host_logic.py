"""CPU: host-side mirror of the reference module API (construction, state-dict contract,
pickling, error behaviour) -- no device work."""
import pickle

import pytest
import torch

from onepose_plus_plus_amd import OnePosePlus_model, default_config
from onepose_plus_plus_amd.synthetic import make_state_dict
from tests import helpers as H


def test_state_dict_contract():
    cfg = default_config()
    m = OnePosePlus_model(cfg)
    sd = m.state_dict()
    assert len(sd) == 195
    assert sum(v.numel() for k, v in sd.items() if "num_batches_tracked" not in k) == 10233184 - 0
    assert "dense_pos_encoding.pe" not in sd               # non-persistent buffer
    assert m.dense_pos_encoding.pe.shape == (1, 256, 256, 256)
    gold = make_state_dict(cfg, 0)
    assert list(sd.keys()) == list(gold.keys())
    for k in sd:
        assert tuple(sd[k].shape) == tuple(gold[k].shape), k
    m.load_state_dict(gold, strict=True)
    # checkpoint convention of the caller: strip 'matcher.' (inference_OnePosePlus.py:32-36)
    ckpt = {"matcher." + k: v for k, v in gold.items()}
    stripped = {k.replace("matcher.", ""): v for k, v in ckpt.items()}
    OnePosePlus_model(cfg).load_state_dict(stripped, strict=True)
    with pytest.raises(RuntimeError):
        OnePosePlus_model(cfg).load_state_dict({k: v for k, v in list(gold.items())[:-1]}, strict=True)


def test_state_dict_matches_reference_fixture():
    """The reference module's state-dict contract and positional table, stored from the reference by tests/golden/gen_golden.py
    (module_contract): same keys in the same order, same shapes and dtypes, a state dict of that layout strict-loads, and the
    dense positional table is bit-identical."""
    cfg = default_config()
    ours = OnePosePlus_model(cfg)
    gold = H.load_golden("reference_module_contract")
    os_ = ours.state_dict()
    assert list(os_.keys()) == gold["keys"].tolist()
    for k, shape, dtype in zip(gold["keys"].tolist(), gold["shapes"].tolist(), gold["dtypes"].tolist()):
        shape = tuple(s for s in shape if s >= 0)
        assert tuple(os_[k].shape) == shape and str(os_[k].dtype) == dtype, k
    rs = {k: torch.zeros(tuple(s for s in shape if s >= 0), dtype=getattr(torch, dtype.split(".")[1]))
          for k, shape, dtype in zip(gold["keys"].tolist(), gold["shapes"].tolist(), gold["dtypes"].tolist())}
    ours.load_state_dict(rs, strict=True)
    row, col, along_x = (torch.from_numpy(gold[k]) for k in ("pe_row", "pe_col", "pe_along_x"))
    pe = torch.where(along_x[:, None, None], row[:, None, :], col[:, :, None])[None]
    assert tuple(pe.shape) == tuple(gold["pe_shape"].tolist())
    assert torch.equal(ours.dense_pos_encoding.pe, pe)


def test_pickle_roundtrip():
    """Ray pickles the module into its workers (inference_OnePosePlus.py:85-95)."""
    cfg = default_config()
    m = OnePosePlus_model(cfg).eval()
    m.load_state_dict(make_state_dict(cfg, 0))
    m2 = pickle.loads(pickle.dumps(m))
    assert not m2.training
    for (k1, v1), (k2, v2) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)
    assert m2._rt["ctx"] is None and m2._rt["dirty"]


def test_pretrained_backbone_loading(tmp_path):
    """OnePosePlusModel.py:78-94: keys containing 'backbone' are stripped and strict-loaded."""
    cfg = default_config()
    gold = make_state_dict(cfg, 5)
    ck = {"matcher.backbone." + k[len("backbone."):]: v for k, v in gold.items() if k.startswith("backbone.")}
    ck["matcher.loftr_coarse.layers.0.q_proj.weight"] = torch.zeros(1)    # must be ignored
    path = tmp_path / "loftr.ckpt"
    torch.save({"state_dict": ck}, path)
    cfg["loftr_backbone"]["pretrained"] = str(path)
    cfg["loftr_backbone"]["pretrained_fix"] = True
    m = OnePosePlus_model(cfg)
    assert torch.equal(m.backbone.conv1.weight, gold["backbone.conv1.weight"])
    assert not any(p.requires_grad for p in m.backbone.parameters())
    assert all(p.requires_grad for p in m.loftr_coarse.parameters())


def test_unsupported_config_values_raise_like_reference():
    cfg = default_config()
    cfg["loftr_backbone"]["resolution"] = [16, 4]
    with pytest.raises(NotImplementedError):          # backbone/__init__.py:9-12
        OnePosePlus_model(cfg)
    cfg = default_config()
    cfg["loftr_backbone"]["type"] = "VGG"
    with pytest.raises(ValueError):                   # backbone/__init__.py:13-14
        OnePosePlus_model(cfg)
    cfg = default_config()
    cfg["keypoints_encoding"]["type"] = "mlp_conv"
    with pytest.raises(NotImplementedError):          # OnePosePlusModel.py:47-50
        OnePosePlus_model(cfg)
    cfg = default_config()
    cfg["coarse_matching"]["type"] = "sinkhorn"
    with pytest.raises(NotImplementedError):          # coarse_matching.py:63-66
        OnePosePlus_model(cfg)
    cfg = default_config()
    cfg["loftr_coarse"]["layer_names"] = ["self", "foo"]
    with pytest.raises(NotImplementedError):          # transformer.py:117-120
        OnePosePlus_model(cfg)


def test_inference_only_and_no_cpu_fallback():
    m = OnePosePlus_model(default_config())
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # train() mode included
        m({"query_image": torch.zeros(1, 1, 64, 64)})
    m.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m({"query_image": torch.zeros(1, 1, 64, 64)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # masks / batches are supported, CPU tensors are not
        m({"query_image": torch.zeros(2, 1, 64, 64), "query_image_mask": torch.ones(2, 8, 8)})



def test_product_never_imports_oracle():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "onepose_plus_plus_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dp, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f


def test_gemm_precision_selector(monkeypatch):
    """Host side of `opp_config.gemm_precision`: names, default, env override, pickling, bad values."""
    import pickle
    from onepose_plus_plus_amd import model as M
    m = OnePosePlus_model(default_config())
    assert m.gemm_precision == M.DEFAULT_GEMM_PRECISION == "bf16x3"        # the default is not narrower than fp32
    assert [m.set_gemm_precision(p)._c_config().gemm_precision for p in ("fp32", "bf16x3")] == [0, 3]
    for narrower in ("fp16x2", "fp16x2_all", "bf16"):                      # nothing narrower than fp32 is offered
        with pytest.raises(ValueError):
            m.set_gemm_precision(narrower)
    assert pickle.loads(pickle.dumps(m)).gemm_precision == "bf16x3"              # travels to Ray-style workers
    with pytest.raises(ValueError):
        m.set_gemm_precision("bf16")
    monkeypatch.setenv("OPP_GEMM_PRECISION", "fp32")
    assert OnePosePlus_model(default_config()).gemm_precision == "fp32"
    monkeypatch.setenv("OPP_GEMM_PRECISION", "tf32")
    with pytest.raises(ValueError):
        OnePosePlus_model(default_config())._c_config()


def test_scheduling_switches(monkeypatch):
    """Host side of the scheduling switches (results are bit-identical for every value; GPU tests check that): defaults, setters,
    `opp_config` fields, env overrides, pickling, bad values."""
    import pickle
    for k in ("OPP_ENCODER_FUSION", "OPP_SCORE_PATH", "OPP_FPN_OVERLAP", "OPP_SKIP_UNUSED_FINE_MAP"):
        monkeypatch.delenv(k, raising=False)
    m = OnePosePlus_model(default_config())
    c = m._c_config()
    assert (c.encoder_fusion, c.score_two_sweep, c.fpn_overlap, c.tile_policy) == (2, 2, 1, 0)
    assert m.skip_unused_fine_map is False                       # the default launches every operator of the reference
    m.set_encoder_fusion(1).set_score_two_sweep(0).set_fpn_overlap(False).set_tile_policy("throughput").set_skip_unused_fine_map(True)
    c = m._c_config()
    assert (c.encoder_fusion, c.score_two_sweep, c.fpn_overlap, c.tile_policy) == (1, 0, 0, 1)
    m2 = pickle.loads(pickle.dumps(m))                           # the switches travel with the module
    c2 = m2._c_config()
    assert (c2.encoder_fusion, c2.score_two_sweep, c2.fpn_overlap, c2.tile_policy, m2.skip_unused_fine_map) == (1, 0, 0, 1, True)
    for bad in (lambda: m.set_encoder_fusion(3), lambda: m.set_score_two_sweep(5), lambda: m.set_tile_policy("fastest")):
        with pytest.raises(ValueError):
            bad()
    monkeypatch.setenv("OPP_ENCODER_FUSION", "0")
    monkeypatch.setenv("OPP_SCORE_PATH", "1")
    monkeypatch.setenv("OPP_FPN_OVERLAP", "0")
    monkeypatch.setenv("OPP_SKIP_UNUSED_FINE_MAP", "1")
    e = OnePosePlus_model(default_config())
    c = e._c_config()
    assert (c.encoder_fusion, c.score_two_sweep, c.fpn_overlap, e.skip_unused_fine_map) == (0, 1, 0, True)



def test_smi_trace_summary_reads_amd_smi_samples():
    """tools/smi_trace.py (clock / power evidence beside a bench run): the amd-smi JSON samples are reduced to activity, socket
    power and per-XCD gfx clocks over the busy part of the run; malformed samples are skipped."""
    import importlib.util
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("smi_trace", os.path.join(root, "tools", "smi_trace.py"))
    smi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(smi)

    def sample(t, act, watts, clocks):
        gpu = {"gpu": 0, "usage": {"gfx_activity": {"value": act, "unit": "%"}}, "power": {"socket_power": {"value": watts, "unit": "W"}},
               "clock": {"gfx_%d" % i: {"clk": {"value": c, "unit": "MHz"}, "max_clk": {"value": 2400, "unit": "MHz"}} for i, c in enumerate(clocks)}}
        gpu["clock"]["mem_0"] = {"clk": {"value": 2000, "unit": "MHz"}}
        return json.dumps({"t": t, "tool": "amd-smi", "out": json.dumps({"gpu_data": [gpu]})})

    lines = [sample(0.1, 0, 250, [150] * 8), sample(1.0, 100, 1380, [2000, 2100] * 4), sample(2.0, 98, 1360, [2050] * 8), "not json",
             json.dumps({"t": 3.0, "tool": "amd-smi", "out": "{}"})]
    rows = smi.smi_rows(lines)
    assert len(rows) == 3 and rows[1]["xcds"] == 8 and rows[1]["gfx_clk_mhz_mean"] == 2050.0 and rows[1]["gfx_clk_mhz_limit"] == 2400.0
    s = smi.smi_summary(rows)
    assert s["samples"] == 3 and s["busy_samples (gfx_activity >= 50 %)"] == 2
    assert s["socket_power_w"] == {"min": 1360.0, "mean": 1370.0, "max": 1380.0}
    assert s["gfx_clk_mhz_mean"]["mean"] == 2050.0 and s["gfx_clk_mhz_min"]["min"] == 2000.0


def _k3(cin):
    """packed K of a 3x3 convolution (opp_conv_packed_k): 32 n + (1..4) channels pack their last channels 8 taps to a chunk"""
    g, t = divmod(cin, 32)
    return (g * 9 + 2) * 32 if 1 <= t <= 4 else ((cin + 31) // 32) * 32 * 9


# layer, M = output pixels, real / stored output channels, K, conv -> (latency policy, throughput policy) tile of the default arithmetic; + 1000 = four K slices.
# Cross-checked against the kernel traces of both conditions (profiles/r05_kernel_stats_bench_streams1.csv: 5 launches of 256x128, 2 of 128x224, 6 + 4 of
# 128x128, 2 of 64x128, 2 of 64x64 per forward; ..._default_streams4.csv: 10 of 128x256, 5 of 256x128, 4 K-sliced).
TILE_POLICY_CASES = [
    ("layer1 3x3 128->128 @256^2", 65536, 128, 128, 1152, 1, 20, 20),
    ("layer1_outconv2.1 3x3 196->128 @256^2", 65536, 128, 128, _k3(196), 1, 20, 20),
    ("layer1_outconv2.0 3x3 196->196 @256^2", 65536, 196, 224, _k3(196), 1, 27, 22),      # the 224-column ring tile: latency policy, full rounds only
    ("layer1_outconv 1x1 128->196 @256^2", 65536, 196, 224, 128, 1, 27, 22),
    ("layer2 3x3 196->196 @128^2", 16384, 196, 224, _k3(196), 1, 25, 22),                 # half a round: never the ring tile
    ("layer2_outconv2.0 3x3 256->256 @128^2", 16384, 256, 256, 2304, 1, 25, 22),
    ("layer2_outconv 1x1 196->256 @128^2", 16384, 256, 256, 224, 1, 26, 22),
    ("layer3 3x3 256->256 @64^2", 4096, 256, 256, 2304, 1, 1025, 1025),                    # split-K is a shape decision, the same under both policies
    ("layer3_outconv 1x1 256->256 @64^2", 4096, 256, 256, 256, 1, 2, 26),
    ("batch of 4: layer2 3x3 196->196", 65536, 196, 224, _k3(196), 1, 27, 22),
]


@pytest.mark.parametrize("case", TILE_POLICY_CASES, ids=[c[0] for c in TILE_POLICY_CASES])
def test_tile_policy_of_the_launcher(case):
    """The launcher's own tile choice is a pure host function (opp_gemm_tile_for): pinned here per backbone layer shape and tile policy.
    The 128 x 224 ring tile only where it measured faster: latency policy, 224 stored / <= 208 real columns, a grid of >= 256 tiles."""
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    _, M, n_real, n_store, K, conv, lat, thr = case
    assert lib.opp_gemm_tile_for(M, n_real, n_store, K, conv, 2, 0) == lat
    assert lib.opp_gemm_tile_for(M, n_real, n_store, K, conv, 2, 1) == thr


def test_tile_policy_guards():
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    # unknown or too many real columns: the ring tile's "rows >= 208 are zero padding" premise does not hold -> 128 x 256
    assert lib.opp_gemm_tile_for(65536, 0, 224, _k3(196), 1, 2, 0) == 22
    assert lib.opp_gemm_tile_for(65536, 224, 224, _k3(196), 1, 2, 0) == 22
    assert lib.opp_gemm_tile_for(65536, 196, 224, _k3(196), 1, 0, 0) != 27       # exact-fp32 arithmetic has no such tile
    assert lib.opp_gemm_tile_for(65536, 196, 224, _k3(196), 1, 1, 0) != 27       # nor fp16x2
    for bad in [(0, 1, 128, 128, 1, 2, 0), (128, 1, 128, 100, 1, 2, 0), (128, 1, 128, 128, 1, 5, 0), (128, 1, 128, 128, 1, 2, 7)]:
        assert lib.opp_gemm_tile_for(*bad) < 0


# (B, H, W) -> opp_backbone_tape_bytes, opp_backbone_train_tape_workspace_bytes of the default configuration, recorded from the build of
# commit 9537b0a.  tests/test_train_bwd_gpu.py builds views on this layout.
TAPE_BYTES = {(1, 128, 128): (46696704, 2164992), (4, 512, 512): (2986379520, 138414336)}


@pytest.mark.parametrize("shape", sorted(TAPE_BYTES), ids=lambda s: "B%d_%dx%d" % s)
def test_tape_layout_sizes_are_pinned(shape):
    """The tape of the training step is a contract between opp_backbone_train_tape, opp_backbone_backward and the callers that
    slice it: its size and that of the forward's workspace are host arithmetic (no device needed) and must not move."""
    import ctypes
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    ccfg = OnePosePlus_model(default_config())._c_config()
    _lib.check(lib.opp_create(ctypes.byref(ccfg), ctypes.byref(ctx)), "opp_create")
    try:
        assert (lib.opp_backbone_tape_bytes(ctx, *shape), lib.opp_backbone_train_tape_workspace_bytes(ctx, *shape)) == TAPE_BYTES[shape]
    finally:
        lib.opp_destroy(ctx)


# (which, n_seg, len0, len1) -> opp_transformer_workspace_bytes, kv_offset, ks_offset (opp_transformer_kv_offsets) of the default
# configuration, recorded from the build of commit 4c7012e.  tests/test_kv_fold_gpu.py reads KV / Ksum at these offsets.
TRANSFORMER_WS = {(0, 1, 4096, 5000): (70100224, 65200128, 65265664), (0, 1, 96, 77): (1443072, 1240064, 1305600),
                  (0, 2, 96, 77): (2750720, 2480128, 2611200), (0, 1, 0, 300): (2387200, 2150400, 2215936),
                  (1, 500, 25, 1): (59648256, 46592000, 54784000), (1, 1, 25, 1): (119552, 93184, 109568)}
# opp_object_prefix_bytes, opp_object_prefix_workspace_bytes at 5000 points, same build (no weights packed: no prefix, 0 bytes)
PREFIX_BYTES_N5000 = (0, 38577408)


def test_transformer_workspace_layout_is_pinned():
    """The workspace plan of the encoder walk is host arithmetic shared by opp_transformer, its callers and the tests that read
    KV / Ksum out of the workspace: sizes and offsets of both levels must not move (one and many segments, an empty stream)."""
    import ctypes
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    ccfg = OnePosePlus_model(default_config())._c_config()
    _lib.check(lib.opp_create(ctypes.byref(ccfg), ctypes.byref(ctx)), "opp_create")
    try:
        for case, pinned in TRANSFORMER_WS.items():
            kv, ks = ctypes.c_size_t(), ctypes.c_size_t()
            _lib.check(lib.opp_transformer_kv_offsets(ctx, *case, ctypes.byref(kv), ctypes.byref(ks)), "opp_transformer_kv_offsets")
            assert (lib.opp_transformer_workspace_bytes(ctx, *case), kv.value, ks.value) == pinned, case
        assert (lib.opp_object_prefix_bytes(ctx, 5000), lib.opp_object_prefix_workspace_bytes(ctx, 5000)) == PREFIX_BYTES_N5000
    finally:
        lib.opp_destroy(ctx)


# (H, W) -> opp_backbone_workspace_bytes, opp_forward_coarse_workspace_bytes at n = 150 / 5000 as (fpn_overlap 0, fpn_overlap 1) each,
# opp_backbone_fine_branch_workspace_bytes, opp_fine_patch_buffer_floats (which = 0, 1) of the default configuration, recorded from
# the build of commit 88bd034 (one backbone_impl behind a phase number; the fine-branch size a formula beside its buffers)
BACKBONE_WS = {(64, 96): (42746112, ((43097344, 45098496), (48063744, 87397888)), 19530752, (196608, 86016)),
               (136, 104): (54714112, ((55321344, 58286080), (60287744, 100585472)), 23114752, (452608, 198016)),
               (512, 512): (425722112, ((434265344, 467033600), (439231744, 509332992)), 134218752, (8388608, 3670016))}
# the first two once more with OPP_ASP=1 in the environment (the plan adds the pre-split twins), same build
BACKBONE_WS_ASP = {(64, 96): (49602816, ((49954048, 51955200), (54920448, 94254592))),
                   (136, 104): (70498816, ((71106048, 74070784), (76072448, 116370176))),
                   (512, 512): (718274816, ((726818048, 759586304), (731784448, 801885696)))}
BACKBONE_WS_N = (150, 5000)


def _backbone_ws_sizes():
    """{(H, W): sizes in the layout of BACKBONE_WS} from the library as the environment of THIS process configures it"""
    import ctypes
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    ctxs = []
    try:
        for overlap in (False, True):
            ccfg = OnePosePlus_model(default_config()).set_fpn_overlap(overlap)._c_config()
            assert ccfg.fpn_overlap == int(overlap)
            ctxs.append(ctypes.c_void_p())
            _lib.check(lib.opp_create(ctypes.byref(ccfg), ctypes.byref(ctxs[-1])), "opp_create")
        c0, c1 = ctxs
        return {hw: (lib.opp_backbone_workspace_bytes(c1, *hw),
                     tuple((lib.opp_forward_coarse_workspace_bytes(c0, *hw, n), lib.opp_forward_coarse_workspace_bytes(c1, *hw, n))
                           for n in BACKBONE_WS_N),
                     lib.opp_backbone_fine_branch_workspace_bytes(c1, *hw),
                     (lib.opp_fine_patch_buffer_floats(c1, *hw, 0), lib.opp_fine_patch_buffer_floats(c1, *hw, 1)))
                for hw in BACKBONE_WS}
    finally:
        for ctx in ctxs:
            lib.opp_destroy(ctx)


def test_backbone_workspace_sizes_are_pinned():
    """The workspace of the eval-mode backbone, of the fused coarse call (with and without the fine branch beside the coarse level), of
    the fine branch completed afterwards and the caller's x1 / x2_out buffers are host arithmetic over one plan per entry: none of
    them may move (the callers allocate by these numbers and the stages carve the same buffers out of them)."""
    assert _backbone_ws_sizes() == BACKBONE_WS


def test_backbone_workspace_sizes_are_pinned_with_presplit_twins():
    """OPP_ASP=1 is read by the plan, per call, from the environment: a child process started with it reports the sizes with the
    pre-split twins (backbone and fused coarse call; the other entries plan no twins and stay as above)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import json, sys; sys.path.insert(0, %r); from tests import test_host_logic as T; "
            "print(json.dumps([[list(k), v] for k, v in T._backbone_ws_sizes().items()]))" % root)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OPP_ASP="1"), cwd=root, capture_output=True, text=True, check=True)
    got = {tuple(k): v for k, v in json.loads(out.stdout.strip().splitlines()[-1])}
    for hw, (backbone, coarse) in BACKBONE_WS_ASP.items():
        assert (got[hw][0], tuple(tuple(c) for c in got[hw][1])) == (backbone, coarse), hw
        assert (got[hw][2], tuple(got[hw][3])) == BACKBONE_WS[hw][2:], hw


# Every other size query of csrc/api.hip, at the shapes of tests/test_memory_contract_gpu.py (IMAGES, POINTS, TOKENS, MATCHER, M = 1 / 33 /
# 300 matches, B = 1 / 3) and at the flagship shape (512 x 512, n = 5000, M = 500), recorded from the build of commit 6d0f003 (the size
# of a call stated by a formula or a sum of nested queries beside the plans that carve it)
WS_IMAGES = [(40, 72), (64, 96), (128, 192), (512, 512)]
WS_POINTS = [77, 129, 257, 333, 5000]
WS_MATCHES = [1, 33, 300, 500]
WS_TOKENS = [(31, 1), (45, 77), (65, 129), (96, 200), (4096, 5000)]
WS_FINE_TOKENS = [(3, 25, 1), (3, 49, 1), (3, 64, 3), (500, 25, 1)]                     # (n_seg, len0, len1) at C = 128
WS_MATCHER = [(8, 12, 77), (16, 24, 300), (16, 32, 333), (64, 64, 5000)]              # (hc, wc, N)
WS_BATCH = (1, 3)
# (cin, cout, ks, stride, (H, W)): the cases of the conv2d_backward stage of the contract file
WS_CONV_BWD = [(196, 196, 3, 1, (5, 9)), (128, 196, 3, 2, (10, 18)), (196, 256, 1, 2, (10, 18)), (64, 64, 3, 1, (24, 32)), (256, 196, 1, 1, (3, 11)),
               (128, 196, 1, 1, (15, 20))]
WS_SCORE_CTX = {"bf16x3-dense": ("bf16x3", 0), "bf16x3-two_sweep": ("bf16x3", 1), "bf16x3-single": ("bf16x3", 2), "fp32": ("fp32", 2)}


_entry_ws_cache = {}


def _entry_ws_sizes():
    """{query name: [sizes in the order of the WS_* lists]} from the library (asked once per process)"""
    if not _entry_ws_cache:
        _entry_ws_cache.update(_ask_entry_ws_sizes())
    return _entry_ws_cache


def _ask_entry_ws_sizes():
    import ctypes
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    ctxs = {}

    def ctx_of(precision="bf16x3", score=2, window=5):
        key = (precision, score, window)
        if key not in ctxs:
            cfg = default_config()
            cfg["loftr_fine"]["window_size"] = window
            ccfg = OnePosePlus_model(cfg).set_gemm_precision(precision).set_score_two_sweep(score)._c_config()
            ctxs[key] = ctypes.c_void_p()
            _lib.check(lib.opp_create(ctypes.byref(ccfg), ctypes.byref(ctxs[key])), "opp_create")
        return ctxs[key]

    try:
        out = {}
        for window in (5, 7):
            out["fine-w%d" % window] = [lib.opp_fine_workspace_bytes(ctx_of(window=window), M) for M in WS_MATCHES]
            out["fine_patches-w%d" % window] = [lib.opp_fine_patches_workspace_bytes(ctx_of(window=window), M) for M in WS_MATCHES]
        for name, (precision, score) in WS_SCORE_CTX.items():
            out["coarse_match-" + name] = [lib.opp_coarse_match_workspace_bytes(ctx_of(precision, score), n, hc * wc) for hc, wc, n in WS_MATCHER]
            out["forward_coarse-" + name] = [lib.opp_forward_coarse_workspace_bytes(ctx_of(precision, score), *hw, n)
                                             for hw, n in zip(WS_IMAGES, (77, 129, 333, 5000))]
        out["coarse_match-null"] = [lib.opp_coarse_match_workspace_bytes(None, n, hc * wc) for hc, wc, n in WS_MATCHER]
        out["linear_attention"] = ([lib.opp_linear_attention_workspace_bytes(1, l0, l1, 256, 8) for l0, l1 in WS_TOKENS] +
                                   [lib.opp_linear_attention_workspace_bytes(n_seg, l0, l1, 128, 8) for n_seg, l0, l1 in WS_FINE_TOKENS])
        out["object_prefix"] = [lib.opp_object_prefix_workspace_bytes(ctx_of(), n) for n in WS_POINTS]
        for precision in ("bf16x3", "fp32"):
            c = ctx_of(precision)
            for q in ("backbone_train", "backbone_train_tape", "backbone_backward"):
                fn = getattr(lib, "opp_%s_workspace_bytes" % q)
                out["%s-%s" % (q, precision)] = [fn(c, B, *hw) for B in WS_BATCH for hw in WS_IMAGES]
        for prec_name, prec in (("bf16x3", 2), ("fp32", 0)):
            out["conv2d_backward-" + prec_name] = [lib.opp_conv2d_backward_workspace_bytes(B, *hw, cin, cout, ks, stride, prec)
                                                   for cin, cout, ks, stride, hw in WS_CONV_BWD for B in WS_BATCH]
        return out
    finally:
        for ctx in ctxs.values():
            lib.opp_destroy(ctx)


ENTRY_WS = {
    "fine-w5": [133888, 4377344, 39783680, 66305280],
    "fine_patches-w5": [468736, 15386368, 139855104, 233090304],
    "fine-w7": [232192, 7621376, 69274880, 115457280],
    "fine_patches-w7": [766720, 25219840, 229250304, 382082304],
    "coarse_match-bf16x3-dense": [154880, 652032, 873472, 14816768],
    "forward_coarse-bf16x3-dense": [39079936, 44926464, 77062656, 509332992],
    "coarse_match-bf16x3-two_sweep": [273152, 1112832, 1384960, 22496768],
    "forward_coarse-bf16x3-two_sweep": [39079936, 44926464, 77062656, 509332992],
    "coarse_match-bf16x3-single": [273152, 1112832, 1384960, 22496768],
    "forward_coarse-bf16x3-single": [39079936, 44926464, 77062656, 509332992],
    "coarse_match-fp32": [7424, 62208, 87040, 8525312],
    "forward_coarse-fp32": [39079936, 44926464, 77062656, 509332992],
    "coarse_match-null": [273920, 1113600, 1385728, 22497536],
    "linear_attention": [135424, 169216, 236800, 270592, 4900096, 78592, 78592, 78592, 13056256],
    "object_prefix": [687360, 1093888, 2078976, 2657536, 38577408],
    "backbone_train-bf16x3": [4968192, 10594560, 42371328, 451938560, 14899968, 31779072, 127109376, 1355811072],
    "backbone_train_tape-bf16x3": [383232, 813312, 3246336, 34605312, 1145088, 2435328, 9734400, 103811328],
    "backbone_backward-bf16x3": [20910592, 33943808, 73130240, 372678912, 31978240, 47485184, 146170112, 1025941760],
    "backbone_train-fp32": [4968192, 10594560, 42371328, 451938560, 14899968, 31779072, 127109376, 1355811072],
    "backbone_train_tape-fp32": [383232, 813312, 3246336, 34605312, 1145088, 2435328, 9734400, 103811328],
    "backbone_backward-fp32": [19730944, 32764160, 71950592, 371499264, 30798592, 46305536, 144990464, 1024762112],
    "conv2d_backward-bf16x3": [7790592, 7791360, 4571904, 4895232, 1226496, 1595904, 2892032, 7622912, 1040128, 1040128, 653056, 1046272],
    "conv2d_backward-fp32": [6987776, 6988544, 4113152, 4436480, 1111808, 1481216, 2818304, 7549184, 925440, 925440, 595712, 988928],
}


@pytest.mark.parametrize("query", sorted(ENTRY_WS))
def test_entry_workspace_sizes_are_pinned(query):
    """Python allocates every call's workspace by its size query, and the entry carves the same plan out of it: the number a query reports
    for a shape is part of the interface and must not move, whichever way the plan behind it is written."""
    assert _entry_ws_sizes()[query] == ENTRY_WS[query]
