"""The cases of tests/mask_cases.py, judged from their float64 references alone (no GPU): a kernel that drops, shifts or ignores the query
mask, or the batch-0 keypoint extent, lands far outside the bars of tests/test_query_mask_gpu.py, and the references themselves are
exact enough to carry those bars."""
import pytest
import torch

from tests import mask_cases as MC

SHAPES = MC.SHAPES


@pytest.mark.parametrize("kind", ["a", "b", "d"])
@pytest.mark.parametrize("shape", SHAPES)
def test_transformer_reference_moves_with_the_mask(shape, kind):
    """masked against unmasked reference: at least 1e-2 of the largest reference entry on the unmasked image rows and on the point rows,
    200 times the 5e-5 bar"""
    L = shape[0] * shape[1]
    m = MC.mask(shape, kind).bool()
    ref, ref0 = MC.transformer_ref(shape, kind), MC.transformer_ref(shape, None)
    assert ref.dtype == torch.float64 and torch.isfinite(ref).all()
    scale = ref.abs().max().item()
    d = (ref - ref0).abs()
    img, pts = d[:L][m].max().item() / scale, d[L:].max().item() / scale
    assert img >= 1e-2 and pts >= 1e-2, (shape, kind, img, pts)
    if kind == "b":
        assert int((~m).sum()) == 6 * MC.SINGLE_RUN and not m[0] and not m[63] and not m[64] and not m[127] and not m[128] and not m[L - 1]


@pytest.mark.parametrize("shape", SHAPES)
def test_masked_image_rows_of_the_reference_carry_a_zero_message(shape):
    """the stage returns the masked image rows too: with phi(Q) = 0 their message is zero, so each layer adds norm2(mlp([x, norm1.bias]))
    -- a row-local function, the same whichever other cells are masked"""
    L = shape[0] * shape[1]
    both = ~MC.mask(shape, "a").bool() & ~MC.mask(shape, "d").bool()
    assert both.sum() > 0
    a, d = MC.transformer_ref(shape, "a")[:L][both], MC.transformer_ref(shape, "d")[:L][both]
    assert (a - d).abs().max().item() < 1e-12
    assert (a - MC.transformer_tokens(shape)[:L][both].double()).abs().max().item() > 1e-2


@pytest.mark.parametrize("shape", SHAPES)
def test_mask_c_is_no_mask_in_the_reference(shape):
    assert torch.equal(MC.transformer_ref(shape, "c"), MC.transformer_ref(shape, None))
    assert torch.equal(MC.matcher_conf(shape, "c"), MC.matcher_conf(shape, None))


@pytest.mark.parametrize("shape", SHAPES)
def test_matcher_reference_moves_with_the_padding_mask(shape):
    m = MC.mask(shape, "a").bool()
    ref, ref0 = MC.matcher_ref(shape, "a"), MC.matcher_ref(shape, None)
    conf, conf0 = ref["conf"], ref0["conf"]
    assert (conf[:, ~m] == 0.0).all()                                   # exactly zero, not merely small
    assert (conf[:, m] - conf0[:, m]).abs().max().item() > 0.5
    n, n0 = len(ref["matches"]), len(ref0["matches"])
    assert n0 > 0 and abs(n - n0) >= 0.1 * n0, (n0, n)
    # part of the planted cells lie under the mask, and no reference match does
    assert any(not m[j] for _, j in ref0["matches"]) and all(m[j] for _, j in ref["matches"])


@pytest.mark.parametrize("kind", ["a", "b"])
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_matches_are_decisive(shape, kind):
    """at most 1 % of a case's reference matches are within 1e-3 of thr or of the runner-up of their row or column (those are the ones a
    correct kernel may report differently); every match is a candidate"""
    ref = MC.matcher_ref(shape, kind)
    n, nd = len(ref["matches"]), len(ref["decisive"])
    assert n >= 20 and n - nd <= 0.01 * n, (shape, kind, n, nd)
    assert all(ref["candidates"][i, j] for i, j in ref["matches"])
    assert int(ref["candidates"].sum()) - n <= 0.01 * n
    # the single cells of mask (b) include unmasked neighbours that do match: a shifted mask would remove them
    if kind == "b":
        cols = {j for _, j in ref["matches"]}
        assert len(cols) > 20


@pytest.mark.parametrize("shape", SHAPES)
def test_rounding_floor_of_the_reference(shape):
    """the float32 oracle's own distance from float64 is below a tenth of the bars the HIP stages are held to"""
    for kind in ("a", "b", "d"):
        e = MC.rel_err(MC.transformer_ref(shape, kind, torch.float32), MC.transformer_ref(shape, kind))
        assert e < 0.1 * MC.BAR_TRANSFORMER, (shape, kind, e)
    for kind in ("a", "b"):
        e = (MC.matcher_conf(shape, kind, torch.float32).double() - MC.matcher_conf(shape, kind)).abs().max().item()
        assert e < 0.1 * MC.BAR_CONF, (shape, kind, e)
    for n in MC.KPT_SIZES:
        kpts, bank = MC.kpt_inputs(n)
        e = MC.rel_err(MC.kpt_ref(kpts, bank, dtype=torch.float32), MC.kpt_ref(kpts, bank))
        assert e < 0.1 * MC.BAR_KPT, (n, e)


def test_keypoint_reference_moves_with_the_extent_of_batch_element_0():
    kpts, bank = MC.kpt_inputs(MC.KPT_EXTENT_N)
    e = MC.kpt_extent_cloud()
    own, other = MC.kpt_ref(kpts, bank), MC.kpt_ref(kpts, bank, e)
    assert (own - other).abs().max().item() > 1e-2
    # repeating the points of batch element 0 up to the batch's length leaves the scaling as the 50-point cloud gives it
    ext = (e.max(0).values - e.min(0).values).max().double() * 0.6
    centred = kpts[0].double() - kpts[0].double().mean(0, keepdim=True)
    import oracle.onepose_oracle as O
    direct = O.keypoint_encoding(MC.state_dict(torch.float64), (centred / ext)[None], bank.double())[0].t()
    assert (direct - other).abs().max().item() < 1e-12
    assert 1.7 < (ext / ((kpts[0].max(0).values - kpts[0].min(0).values).max().double() * 0.6)).item() < 2.3
