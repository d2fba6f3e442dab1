"""The cases of tests/train_graph_cases.py, judged from their references alone (no GPU): every seed keeps the ReLU pre-activations clear of
their kinks, the float32 evaluation of each reference -- the yardstick the bars of tests/test_train_graph_nodes_gpu.py are made of -- sits
where it was measured, the masks and shapes reach the branches they are there for, and the factored fine-level reference is the fine half
of `differentiable_forward`."""
import pytest
import torch

from tests import train_graph_cases as TC

WITH_RELUS = [n for n in TC.names() if TC.CASES[n]["kind"] in ("layer", "transformer", "kpt") or n == "fine_transformer_on"]


@pytest.mark.parametrize("name", WITH_RELUS)
def test_relu_pre_activations_are_clear_of_the_kink_at_the_chosen_seed(name):
    """min|z64| >= 8 max|z32 - z64| over all ReLUs of the case and no sign change between the two runs -- at seed CASES[name]["seed"] of
    the inputs and WEIGHT_SEED of synthetic.make_state_dict.  A change of the synthetic weights that breaks it fails here, by name"""
    ok, (n, zmin, dz, flips) = TC.kinks_are_clear(name)
    seed = TC.CASES[name]["seed"]
    print("%s seed %d: %d pre-activations, min|z64| %.2e, max|z32 - z64| %.2e, %d sign changes" % (name, seed, n, zmin, dz, flips))
    assert n > 0 and flips == 0, (name, seed, flips)
    if TC.CASES[name].get("kinks") == "device_sides":
        # (module docstring of train_graph_cases) half a million pre-activations: the margin is out of reach, the GPU test takes the device's sides
        assert n > 400000 and zmin > 0.0, (name, seed, n, zmin)
    else:
        assert ok, "seed %d of %s no longer qualifies: min|z64| %.2e < %g x %.2e; choose the next seed that does" % (seed, name, zmin, TC.KINK_MARGIN, dz)


def test_cases_without_relus_have_none():
    for name in set(TC.names()) - set(WITH_RELUS):
        assert not TC.reference(name)[0].relus, name


@pytest.mark.parametrize("name", TC.names())
def test_float32_distance_of_the_reference_is_where_it_was_measured(name):
    """d32 -- torch's own float32 evaluation against float64, in the error measure of the GPU test -- per case: the largest one among the
    outputs and among the gradients stays within D32_RANGE x beyond the quoted (smallest, largest) both ways, every bar is positive wherever float32 rounds
    at all, and no bar needs the cap to hide a reference gone wrong"""
    r64, r32 = TC.reference(name)
    for res, dtype in ((r64, torch.float64), (r32, torch.float32)):
        for group in (res.outs, res.grads):
            assert group and all(v is not None and v.dtype == dtype and torch.isfinite(v).all() for v in group.values()), name
    d = TC.d32(name)
    out, grad = TC.d32_summary(d)
    print("%s: d32 outputs %.2e gradients %.2e (%d tensors, smallest %.2e)" % (name, out, grad, len(d), min(d.values())))
    for got, (lo, hi) in zip((out, grad), TC.D32[name]):
        assert lo / TC.D32_RANGE <= got <= hi * TC.D32_RANGE, (name, got, lo, hi)
    assert all(0.0 <= b <= TC.BAR_CAP for b in TC.bars(name).values())
    # the gradients are not trivially small against the floor: every case has tensors far above it
    assert max(float(v.abs().max()) for v in r64.grads.values()) > 1e-3


def test_every_parameter_of_a_case_takes_a_gradient():
    for name in TC.names():
        r64 = TC.reference(name)[0]
        case = TC.CASES[name]
        n_params = len(TC.inputs(name).params)
        assert len(r64.grads) == n_params + len(TC.inputs(name).leaves)
        if case["kind"] == "layer":
            rezero = "rezero" in case["settings"]
            assert n_params == (7 if rezero else 10), (name, n_params)         # 6 matrices + res_weight, or + 4 norm tensors
            assert any(k.endswith(".res_weight") for k in r64.grads) == rezero
            assert any(".norm" in k for k in r64.grads) == (not rezero)
        if case["kind"] == "transformer":
            assert n_params == 20
        if case["kind"] == "kpt":
            assert n_params == (14 if "kptln" in case["settings"] else 8)
        if case["kind"] == "fine":
            assert n_params == (20 if case["enable"] else 0)


def test_masks_leave_cells_and_reach_the_branches():
    unmasked_sample = masked_odd = False
    for name in TC.names():
        m = TC.inputs(name).consts.get("mask")
        if m is None:
            continue
        assert ((m == 0) | (m == 1)).all() and (m.sum(1) >= 1).all() and (m == 0).any(), name      # at least one cell left per sample
        if TC.CASES[name]["kind"] == "matcher":
            B, L = m.shape
            assert (m[0, -3:] == 0).all() and m[0].sum() == L - 3 and (m[-1, 2:7] == 0).all() and m[-1].sum() == L - 5
            unmasked_sample |= bool((m.sum(1) == L).any())
            masked_odd |= L % 32 != 0 and L % 4 != 0
    assert unmasked_sample and masked_odd
    shapes = sorted(TC.CASES[n]["shape"][2] * TC.CASES[n]["shape"][3] for n in TC.names("matcher"))
    assert shapes == [32, 36, 65]                                          # no padding; padding; padding with L % 4 != 0


@pytest.mark.parametrize("name", TC.names("matcher"))
def test_matcher_reference_is_peaked(name):
    """the softmaxes are not flat: the largest confidence is at least 0.5 and at least 90 % of the entries are below 1e-2; masked columns
    are exact zeros in the reference too; the gradient that arrives looks like a focal loss's"""
    r64 = TC.reference(name)[0]
    conf = r64.outs["conf"]
    print("%s: largest confidence %.3f, %.1f %% below 1e-2" % (name, float(conf.max()), 100 * float((conf < 1e-2).double().mean())))
    assert float(conf.max()) >= 0.5 and float((conf < 1e-2).double().mean()) >= 0.9
    inp = TC.inputs(name)
    assert int((inp.grad_out["conf"] < 0).sum()) == TC.N_FOCAL
    m = inp.consts["mask"]
    if m is not None:
        dead = (m == 0)
        assert (conf.transpose(1, 2)[dead] == 0).all() and (r64.grads["f2"][dead] == 0).all()
        assert (r64.grads["f2"][~dead].abs().amax(-1) > 0).all()


def test_matcher_scale_is_restated_from_the_config():
    assert TC.matcher_scale(TC.config("match_b1_n33_4x8")) == pytest.approx(1.0 / 256 / 0.0801, rel=1e-12)
    assert TC.matcher_scale(TC.config("match_b3_n130_6x6_masked_featnone")) == pytest.approx(1.0 / 0.0801, rel=1e-12)


def test_transformer_reference_routes_masks_and_pre_update_tensors_as_restated_here():
    """The reference of the transformer case is the product's own `_transformer`, so a wrong routing INSIDE it would be on both sides of
    the GPU comparison.  Restated here layer call by layer call (loftr_module/transformer.py:160-169): the self layer masks the image
    stream on both sides and the point stream not at all; the cross layer updates the image stream from the points under x_mask, and the
    points from the image stream AS IT WAS BEFORE that update (quirk q6) under source_mask.  Bit for bit, and a swapped mask is far away"""
    from onepose_plus_plus_amd import train_autograd as TA
    name = "transformer_self_cross_masked"
    t = TC.tensors(name, torch.float64)
    tcfg = TC.transformer_config(name)
    with torch.no_grad():
        f3, f2, mask, p, nh = t.leaves["f3"], t.leaves["f2"], t.consts["mask"], t.params, tcfg["nhead"]
        a2 = TA._encoder_layer(p, "loftr_coarse.layers.0", nh, f2, f2, mask, mask)
        a3 = TA._encoder_layer(p, "loftr_coarse.layers.0", nh, f3, f3, None, None)
        b2 = TA._encoder_layer(p, "loftr_coarse.layers.1", nh, a2, a3, mask, None)
        b3 = TA._encoder_layer(p, "loftr_coarse.layers.1", nh, a3, a2, None, mask)
        got = TC.forward(name, t)
        assert torch.equal(got["f3"], b3) and torch.equal(got["f2"], b2)
        wrong3 = TA._encoder_layer(p, "loftr_coarse.layers.1", nh, a3, b2, None, mask)          # the updated image stream
        wrong3m = TA._encoder_layer(p, "loftr_coarse.layers.1", nh, a3, a2, None, None)         # image cells not masked as sources
        for w in (wrong3, wrong3m):
            assert float((w - b3).abs().max()) / float(b3.abs().max()) > 100 * TC.BAR_CAP


@pytest.mark.parametrize("name", TC.names("fine"))
def test_fine_cases_cover_corners_and_a_duplicate(name):
    """the coverage of test_fine_window_gather_node_vs_unfold, and no heatmap on the clamp of the std column (so no gradient row is left out)"""
    s = TC.FINE_SHAPE
    c = TC.inputs(name).consts
    L = s["hc"] * s["wc"]
    assert set(c["j_ids"][:4].tolist()) == {0, s["wc"] - 1, L - 1, (s["hc"] - 1) * s["wc"]}
    a, b = TC.FINE_DUPLICATE_ROWS
    assert c["j_ids"][a] == c["j_ids"][b] and c["b_ids"][a] == c["b_ids"][b]
    assert len(c["b_ids"]) == s["M"] == 37 and set(c["b_ids"].tolist()) == {0, 1}
    var = TC.reference(name)[0].var
    assert var.shape == (s["M"], 2) and float(var.min()) > TC.VAR_MIN, float(var.min())


def test_fine_level_ref_is_the_fine_half_of_differentiable_forward():
    """the factored function on the backbone's fine map gives `differentiable_forward`'s expec_f and gradients bit for bit"""
    from onepose_plus_plus_amd.config import default_config
    from onepose_plus_plus_amd.synthetic import make_inputs, make_state_dict
    from tests import torch_graph_ref as GR
    cfg = default_config(thr=0.0)
    sd = make_state_dict(cfg, 7)
    data = make_inputs(30, (32, 48), 5)
    g = torch.Generator().manual_seed(9)
    M = 12
    ids = (torch.zeros(M, dtype=torch.long), torch.randint(0, 30, (M,), generator=g), torch.randint(0, 4 * 6, (M,), generator=g))
    we = torch.randn(M, 3, generator=g).double()
    inputs = {k: data[k].double() for k in ("query_image", "keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
    inputs["query_image_mask"] = None

    def params():
        return {k: v.double().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k}
    p = params()
    _, expec = GR.differentiable_forward(p, cfg, inputs, ids, None)
    (expec * we).sum().backward()
    q = params()
    feat_c, feat_f = GR._backbone(q, inputs["query_image"])
    mine = GR.fine_level_ref(q, cfg, feat_f, inputs["descriptors3d_db"], *ids, feat_f.shape[2] // feat_c.shape[2])
    (mine * we).sum().backward()
    assert expec.shape == (M, 3) and torch.equal(expec.detach(), mine.detach())
    n = 0
    for k in p:
        assert (p[k].grad is None) == (q[k].grad is None), k
        if p[k].grad is not None:
            assert torch.equal(p[k].grad, q[k].grad), k
            n += float(p[k].grad.abs().max()) > 0
    assert n > 40            # loftr_fine and the backbone's fine branch
