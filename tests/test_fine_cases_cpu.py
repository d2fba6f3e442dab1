"""The cases of tests/fine_cases.py, judged from their float64 references alone (no GPU): the references are exact enough to carry the
bars of tests/test_fine_level_gpu.py, a kernel that shifts the window, picks other points, flattens the window the other way round or
swaps the image scales lands at least 100 bars away, and the shapes reach both attention paths and the clamp of the variance."""
import pytest
import torch

from tests import fine_cases as FC

F32, F64 = torch.float32, torch.float64
M_STATS = 41


def _floor(W, M, amp, run_transformer):
    """float32 oracle against float64 -> offsets, std on the compared rows, pixels"""
    e64, m64, _ = FC.fine_ref(W, M, amp, True, run_transformer, F64)
    e32, m32, _ = FC.fine_ref(W, M, amp, True, run_transformer, F32)
    assert e64.dtype == F64 and e32.dtype == F32 and torch.isfinite(e64).all() and torch.isfinite(m64).all()
    d = (e32.double() - e64).abs()
    rows = FC.std_rows(W, M, amp, run_transformer)
    return d[:, :2].max().item(), (d[:, 2][rows].max().item() if rows.any() else 0.0), (m32.double() - m64).abs().max().item()


@pytest.mark.parametrize("amp", FC.AMPS)
@pytest.mark.parametrize("W", FC.WINDOWS)
def test_rounding_floor_of_the_reference(W, amp):
    """the float32 oracle's own distance from float64 is below a tenth of every bar the HIP stages are held to, in the soft and in the
    sharp cases (there: the std column on the rows above VAR_MIN)"""
    for M in FC.M_HEAD:
        for rt in (False, True):
            off, std, px = _floor(W, M, amp, rt)
            print("floor W %d M %d amp %.1f transformer %d: offsets %.2e std %.2e pixels %.2e" % (W, M, amp, rt, off, std, px))
            assert off < 0.1 * FC.BAR_OFFSET and std < 0.1 * FC.BAR_STD and px < 0.1 * FC.BAR_PIXEL, (W, M, amp, rt, off, std, px)
            if not rt:      # gather + head alone is the only outside view of the gather: its floor is far lower
                assert off < 0.02 * FC.BAR_OFFSET, (W, M, amp, off)


@pytest.mark.parametrize("W", FC.WINDOWS)
def test_rounding_floor_of_the_transformer_reference(W):
    for M in FC.M_TRANSFORMER + ((FC.M_LARGE,) if W == FC.W_LARGE else ()):
        ref = FC.transformer_ref(W, M, FC.AMP_SOFT, F64)
        assert ref.shape == (M * W * W + M, FC.C) and ref.dtype == F64 and torch.isfinite(ref).all()
        e = FC.rel_err(FC.transformer_ref(W, M, FC.AMP_SOFT, F32), ref)
        print("floor transformer W %d M %d: %.2e of %.2f" % (W, M, e, ref.abs().max().item()))
        assert e < 0.1 * FC.BAR_TRANSFORMER, (W, M, e)
        assert (ref - FC.transformer_tokens(W, M).double()).abs().max().item() > 1.0          # the stage does something


@pytest.mark.parametrize("run_transformer", [False, True])
@pytest.mark.parametrize("W", FC.WINDOWS)
def test_sharp_cases_reach_the_clamp_and_keep_half_of_the_std_column(W, run_transformer):
    """at most half of a sharp case's matches are left out of the std comparison, at least a quarter have a clamped variance in float64;
    the rows left out are finite and non-negative in the reference too"""
    for M in (3, 4, M_STATS):
        expec, _, var = FC.fine_ref(W, M, FC.AMP_SHARP, True, run_transformer, F64)
        rows = FC.std_rows(W, M, FC.AMP_SHARP, run_transformer)
        out, clamped = int((~rows).sum()), int((var < FC.VAR_CLAMP).any(1).sum())
        print("sharp W %d M %d transformer %d: %d left out, %d clamped, smallest std %.1e" % (W, M, run_transformer, out, clamped, expec[:, 2].min().item()))
        assert 2 * out <= M, (W, M, out)
        assert 4 * clamped >= M, (W, M, clamped)
        assert (expec[:, 2][~rows] >= 0).all()
    # the planted rows are the clamped ones: one-hot on the planted cell, off the window centre
    expec, _, var = FC.fine_ref(W, M_STATS, FC.AMP_SHARP, True, False, F64)
    i_ids, j_ids = FC.match_ids(M_STATS)
    for r in range(FC.PLANT_EVERY - 1, M_STATS, FC.PLANT_EVERY):
        y, x = FC.planted_pixel(r, int(j_ids[r]))
        want = torch.tensor([x - (int(j_ids[r]) % FC.HW_C[1]) * FC.STRIDE, y - (int(j_ids[r]) // FC.HW_C[1]) * FC.STRIDE], dtype=F64) / (W // 2)
        assert (expec[r, :2] - want).abs().max().item() < 1e-6 and (var[r] < FC.VAR_CLAMP).all(), (W, r, expec[r], want)
    # the soft cases compare every row and clamp none
    assert FC.std_rows(W, M_STATS, FC.AMP_SOFT, run_transformer).all()
    assert (FC.fine_ref(W, M_STATS, FC.AMP_SOFT, True, run_transformer, F64)[2] > FC.VAR_MIN).all()


@pytest.mark.parametrize("run_transformer", [False, True])
@pytest.mark.parametrize("W", FC.WINDOWS)
def test_references_move_with_what_a_kernel_could_get_wrong(W, run_transformer):
    """each wrong reading moves the outputs by at least 100 times the bar concerned: a fine map rolled by one pixel (a window origin
    off by one), other points' descriptors, a column-major window, query_image_scale in [0, 1] order, W / 2 for W // 2 in the pixels"""
    ref_e, ref_m, _ = FC.fine_ref(W, M_STATS, FC.AMP_SOFT, True, run_transformer, F64)
    for variant, column, bar in (("roll_x", 0, FC.BAR_OFFSET), ("roll_y", 0, FC.BAR_OFFSET), ("other_points", 0, FC.BAR_OFFSET),
                                 ("column_major", 0, FC.BAR_OFFSET), ("scale_order", 1, FC.BAR_PIXEL), ("half_window", 1, FC.BAR_PIXEL)):
        got = FC.fine_ref(W, M_STATS, FC.AMP_SOFT, True, run_transformer, F64, variant)
        d = ((got[0][:, :2] - ref_e[:, :2]) if column == 0 else (got[1] - ref_m)).abs().max(1).values
        moved = int((d > 10 * bar).sum())
        print("W %d transformer %d %s: max %.3f, %d of %d rows beyond 10 bars" % (W, run_transformer, variant, d.max().item(), moved, M_STATS))
        assert d.max().item() >= 100 * bar, (W, run_transformer, variant, d.max().item())
        assert 2 * moved >= M_STATS, (W, run_transformer, variant, moved)
        if column == 1:         # the pixel conversion alone is wrong: the offsets are the reference's
            assert torch.equal(got[0], ref_e)
    # the x and the y side of the pixel conversion are told apart by the scales and by the non-square map
    assert FC.QUERY_SCALE[0] != FC.QUERY_SCALE[1] and FC.HW_F[0] != FC.HW_F[1] and FC.HW_C[0] != FC.HW_C[1]
    unscaled = FC.fine_ref(W, M_STATS, FC.AMP_SOFT, False, run_transformer, F64)
    assert torch.equal(unscaled[0], ref_e) and (unscaled[1] - ref_m).abs().max().item() >= 100 * FC.BAR_PIXEL


@pytest.mark.parametrize("W", FC.WINDOWS)
def test_windows_of_the_reference_are_zero_exactly_outside_the_map(W):
    """windows_ref against the geometry: cell (ky, kx) of match m is pixel (4 jy + ky - W // 2, 4 jx + kx - W // 2) of the map, exact
    zeros in exactly the cells outside it; the point tokens are the bank's columns"""
    win, f3 = FC.windows_ref(W, M_STATS, FC.AMP_SOFT, F64)
    feat, bank = FC.features(FC.AMP_SOFT, M_STATS)
    i_ids, j_ids = FC.match_ids(M_STATS)
    assert win.shape == (M_STATS, W * W, FC.C) and f3.shape == (M_STATS, FC.C)
    h = W // 2
    n_out = []
    for m, j in enumerate(j_ids.tolist()):
        out = FC.outside_cells(W, j)
        n_out.append(int(out.sum()))
        assert (win[m][out] == 0).all() and (win[m][~out] != 0).all(), (W, m, j)
        jy, jx = j // FC.HW_C[1], j % FC.HW_C[1]
        for r in torch.nonzero(~out)[:, 0].tolist():
            assert torch.equal(win[m, r], feat[0, :, jy * FC.STRIDE + r // W - h, jx * FC.STRIDE + r % W - h].double()), (W, m, r)
        assert torch.equal(f3[m], bank[0, :, i_ids[m]].double())
    # rows 0 .. 7: the corners (top-left, top-right, bottom-right, bottom-left), then the top, bottom, left and right edge
    assert n_out[:8] == [W * W - (W - h) ** 2, h * W, 0, h * W, h * W, 0, h * W, 0], n_out[:8]
    assert sum(1 for n in n_out if n == 0) >= M_STATS // 2


def test_match_lists_hold_what_the_kernels_branch_on():
    hc, wc = FC.HW_C
    L = hc * wc
    for M in FC.M_HEAD + (FC.M_LARGE,):
        i_ids, j_ids = FC.match_ids(M)
        assert i_ids.shape == j_ids.shape == (M,) and i_ids.dtype == j_ids.dtype == torch.int64
        assert 0 <= int(i_ids.min()) and int(i_ids.max()) < FC.N_POINTS and 0 <= int(j_ids.min()) and int(j_ids.max()) < L
        if M >= 4:
            assert j_ids[:4].tolist() == [0, wc - 1, L - 1, (hc - 1) * wc]
    assert sorted(M % 4 for M in FC.M_HEAD) == [0, 1, 1, 3] and 0 not in FC.M_HEAD
    i_ids, j_ids = FC.match_ids(M_STATS)
    corners = {0, wc - 1, L - 1, (hc - 1) * wc}
    jy, jx = j_ids // wc, j_ids % wc
    edge = [int(j_ids[r]) for r in FC.EDGE_ROWS]
    assert not corners & set(edge)
    assert [(int(jy[r]) == 0, int(jy[r]) == hc - 1, int(jx[r]) == 0, int(jx[r]) == wc - 1) for r in FC.EDGE_ROWS] == \
        [(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True)]
    a, b = FC.SAME_J_ROWS
    assert j_ids[a] == j_ids[b] and i_ids[a] != i_ids[b]
    a, b = FC.SAME_I_ROWS
    assert i_ids[a] == i_ids[b] and j_ids[a] != j_ids[b]
    for a, b in FC.DUPLICATE_ROWS:
        assert i_ids[a] == i_ids[b] and j_ids[a] == j_ids[b]
    assert torch.equal((FC.coarse_points(M_STATS, True) != 0).any(1), j_ids != 0) and int((j_ids != 0).sum()) > M_STATS // 2


def test_window_sizes_reach_both_attention_paths():
    """W = 3 and 5 fit the 32 tokens of the one-workgroup attention kernel, W = 7 does not; the large case has more than 128 segments"""
    assert [W * W + 1 > 32 for W in FC.WINDOWS] == [False, False, True]
    assert all(W * W <= 64 for W in FC.WINDOWS)                      # one lane of the head per window cell
    assert FC.W_LARGE * FC.W_LARGE + 1 > 32 and FC.M_LARGE > 128 and FC.M_LARGE * (FC.W_LARGE ** 2 + 1) == 6500
    assert {W * W + 1 for W in FC.WINDOWS} == {10, 26, 50}           # none a divisor of the 32-token tile of the fused encoder tail
    for W in FC.WINDOWS:
        assert FC.transformer_tokens(W, 3).shape == (3 * W * W + 3, FC.C) and FC.config(W)["loftr_fine"]["window_size"] == W


def test_bars_are_the_project_constants():
    from tests import helpers as H
    from tests import mask_cases as MC
    assert FC.BAR_TRANSFORMER == MC.BAR_TRANSFORMER and FC.BAR_OFFSET == H.TOL_OFFSET and FC.BAR_STD == H.STD_TOL_FACTOR * H.TOL_OFFSET
    assert FC.BAR_PIXEL == H.TOL_PIXEL


def test_empty_match_list_in_the_reference():
    for W in FC.WINDOWS:
        for rt in (False, True):
            expec, mk, var = FC.fine_ref(W, 0, FC.AMP_SOFT, True, rt, F64)
            assert expec.shape == (0, 3) and mk.shape == (0, 2) and var.shape == (0, 2)


@pytest.mark.parametrize("window", FC.MODULE_WINDOWS)
def test_module_case_is_carried_by_the_float32_oracle(window):
    """the float32 oracle that the module is compared with is within a tenth of each bar of its own float64 evaluation, reports the same
    matches, and some of them lie on the border of the coarse grid"""
    r32, r64 = FC.module_ref(window, F32), FC.module_ref(window, F64)
    assert r32["W"] == window and r32["expec_f"].dtype == F32 and r64["expec_f"].dtype == F64
    assert torch.equal(r32["i_ids"], r64["i_ids"]) and torch.equal(r32["j_ids"], r64["j_ids"]) and len(r32["mconf"]) > 4
    assert FC.border_matches(r32["j_ids"]) > 0
    for k, bar in FC.MODULE_BARS.items():
        e = (r32[k].double() - r64[k]).abs().max().item()
        print("module case W %d %s: float32 oracle %.2e from float64" % (window, k, e))
        assert e < 0.1 * bar, (window, k, e)
