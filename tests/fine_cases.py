"""Seeded cases of the fine level -- window gather (loftr_module/fine_preprocess.py:32-55), loftr_fine on M x (W^2 + 1) tokens
(loftr_module/transformer.py:133-171) and the expectation head (utils/fine_matching.py:28-110) -- at window sizes 3, 5 and 7, with
references evaluated on the CPU by oracle/onepose_oracle.py in float64.  Shared by tests/test_fine_cases_cpu.py (which shows from the
references alone that a wrong kernel cannot pass) and tests/test_fine_level_gpu.py (which holds the HIP stages to them).  Nothing here
touches a GPU.

The window size decides which kernels run: W^2 + 1 = 10 and 26 tokens per match take the one-workgroup attention kernel
(opp_linattn_small_ok: at most 32 tokens), 50 tokens take the generic KV / apply pair with one segment per match; the 32-token tiles of
the fused encoder tail straddle matches differently at 10, 26 and 50 rows; the head uses 9, 25 or 49 of its 64 lanes and redoes the last
match in its spare waves when M % 4 != 0; the gather's zero padding reaches 1, 2 or 3 pixels outside the map.

Shape: fine map 24 x 36 (coarse grid 6 x 9, stride 4; image 48 x 72), not square so that a swap of rows and columns shows.  With
stride 4 and W <= 7 only the first row and the first column of coarse cells have window cells outside the map (the last centre is at
pixel 20 of 24 and 32 of 36), which is what the reference does at every image size.
"""
import functools

import torch

from onepose_plus_plus_amd.config import default_config
from onepose_plus_plus_amd.synthetic import make_state_dict
from oracle import onepose_oracle as O

WINDOWS = (3, 5, 7)
HW_I, HW_C, HW_F = (48, 72), (6, 9), (24, 36)
STRIDE = HW_F[0] // HW_C[0]
C = 128
N_POINTS = 50
SEED = 7
WEIGHT_SEED = 3
M_HEAD = (1, 3, 4, 41)              # gather + head and whole stage (M = 0 has a test of its own); 3 and 41 are no multiples of 4
M_TRANSFORMER = (1, 3, 41)          # transformer stage ...
M_LARGE, W_LARGE = 130, 7           # ... plus 130 x 50 = 6500 rows: the generic attention path with more than 128 segments
AMP_SOFT = 1.0
# Sharp heatmaps.  Plain `randn * 4.0` cannot meet both shares tests/test_fine_cases_cpu.py asserts: measured on the CPU at M = 41, W = 3 /
# 5 / 7, transformer off and on, it leaves 17 .. 25 of 41 matches below VAR_MIN (more than half at W = 3) while only 1 .. 4 of 41 have a
# clamped variance (a quarter is asked), and any single amplitude that clamps more leaves out more.  So the amplitude is lowered to 2.0
# (0 .. 2 of 41 below VAR_MIN, none clamped) and the clamp branch is reached the way real matches reach it: the point of every third
# row of the match list (rows 2, 5, 8, ...) carries the feature of a fine-map pixel inside its window (`planted_pixel`), so its heatmap
# is one-hot on an off-centre cell: logits of 45 against +-10, both variances below 1e-10.  Measured: 14 of 41 clamped, 14 .. 15 of 41
# below VAR_MIN; 1 of 3 and 1 of 4 at M = 3 and 4; the single match of M = 1 is not planted.
AMP_SHARP = 2.0
PLANT_EVERY = 3
AMPS = (AMP_SOFT, AMP_SHARP)
QUERY_SCALE = (1.25, 0.75)          # query_image_scale [[sy, sx]]; the cases run with it and without (None)
BASE_SCALE = HW_I[0] / HW_F[0]      # fine_matching.py:41

# what the match list of M = 41 holds beyond the four corners (rows of the list)
EDGE_ROWS = {4: 4, 5: 5 * 9 + 3, 6: 2 * 9, 7: 3 * 9 + 8}      # row -> cell: top, bottom, left, right edge, none a corner
SAME_J_ROWS = (8, 9)                # equal j_ids, different i_ids
SAME_I_ROWS = (10, 11)              # equal i_ids, different j_ids
DUPLICATE_ROWS = ((12, 13), (0, 14))    # equal (i, j): an interior cell and the top-left corner

# bars, the project's existing ones
BAR_TRANSFORMER = 5e-5              # of max(1, |ref|max): tests/mask_cases.py BAR_TRANSFORMER
BAR_OFFSET = 1e-4                   # expec_f[:, :2]: tests/helpers.py TOL_OFFSET
BAR_STD = 5.0 * BAR_OFFSET          # expec_f[:, 2]: tests/helpers.py STD_TOL_FACTOR
BAR_PIXEL = 1e-3                    # mkpts_query_f: tests/helpers.py TOL_PIXEL

# The std column is sum_xy sqrt(clamp(var, 1e-10)) with var = E[g^2] - E[g]^2 (fine_matching.py:92-94).  In float32 the two terms are
# O(1) and carry an absolute error of a few ulp, e ~ 3e-7, which the square root turns into e / (2 sqrt(var)).  A tenth of the std bar,
# 5e-5 for both axes together, therefore needs sqrt(var) >= 3e-7 / 5e-5 = 6e-3, var >= 3.6e-5; the threshold is rounded up to 1e-4.
# Matches whose float64 var_x or var_y is below it are held to the offset and pixel bars only (std: finite and non-negative).
# Float32 oracle against float64 on the CPU, maxima over W = 3 / 5 / 7, M = 1 / 3 / 4 / 41, transformer off and on
# (tests/test_fine_cases_cpu.py re-establishes them):
#                       offsets [1e-4]   std, compared rows [5e-4]   pixels [1e-3]   transformer tokens [5e-5 of scale]
#   AMP_SOFT            3.7e-6           2.8e-6                      1.4e-5          5.1e-7 (M = 130: 4.6e-7)
#   AMP_SHARP           4.0e-6           5.9e-6                      1.4e-5
#   transformer off     2.3e-7 soft, 1.6e-6 sharp
# At `randn * 4.0` the std column of the float32 oracle is 1.5e-4 .. 4.1e-4 from float64 over all rows and 2.1e-6 .. 9.8e-6 on the rows
# above VAR_MIN.
VAR_MIN = 1e-4
VAR_CLAMP = 1e-10                   # fine_matching.py:93


def config(W):
    cfg = default_config()
    cfg["loftr_fine"]["window_size"] = W
    return cfg


@functools.lru_cache(maxsize=None)
def state_dict(dtype=torch.float32):
    """the weights do not depend on the window size (loftr_fine has no window-shaped parameter)"""
    sd = make_state_dict(config(5), WEIGHT_SEED)
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _randn():
    g = torch.Generator().manual_seed(SEED)
    return torch.randn(1, C, HW_F[0], HW_F[1], generator=g), torch.randn(1, C, N_POINTS, generator=g)


def planted_pixel(r, j):
    """the fine-map pixel (y, x) whose feature the point of row r of a sharp case's match list carries: one of the 3 x 3 pixels around the
    centre of cell j (inside every window size), moved into the map at the first row and column"""
    y = max(0, (j // HW_C[1]) * STRIDE + r % 3 - 1)
    x = max(0, (j % HW_C[1]) * STRIDE + (r // 3) % 3 - 1)
    return y, x


@functools.lru_cache(maxsize=None)
def features(amp, M):
    """-> feat_f [1, 128, 24, 36], bank_f [1, 128, 50] (float32), both randn * amp.  In the sharp cases the point of every PLANT_EVERY-th
    match carries the feature of `planted_pixel` instead (see AMP_SHARP).  Read-only: shared between tests."""
    feat, bank = _randn()
    feat, bank = feat * amp, bank * amp
    if amp != AMP_SOFT:
        i_ids, j_ids = match_ids(M)
        for r in range(PLANT_EVERY - 1, M, PLANT_EVERY):
            y, x = planted_pixel(r, int(j_ids[r]))
            bank[0, :, i_ids[r]] = feat[0, :, y, x]
    return feat, bank


@functools.lru_cache(maxsize=None)
def match_ids(M):
    """-> i_ids [M], j_ids [M] int64.  M >= 4: the first four cells are the corners, as synthetic.make_fine_ids places them; M >= 15:
    the rows named by EDGE_ROWS, SAME_J_ROWS, SAME_I_ROWS and DUPLICATE_ROWS."""
    hc, wc = HW_C
    L = hc * wc
    g = torch.Generator().manual_seed(SEED + M)
    if M <= N_POINTS:
        i_ids = torch.sort(torch.randperm(N_POINTS, generator=g)[:M]).values
    else:
        i_ids = torch.randint(0, N_POINTS, (M,), generator=g)
    j_ids = torch.randint(0, L, (M,), generator=g)
    if M >= 4:
        j_ids[0], j_ids[1], j_ids[2], j_ids[3] = 0, wc - 1, L - 1, (hc - 1) * wc
    if M >= 15:
        for r, cell in EDGE_ROWS.items():
            j_ids[r] = cell
        a, b = SAME_J_ROWS
        j_ids[a] = j_ids[b] = 2 * wc + 4
        a, b = SAME_I_ROWS
        i_ids[b] = i_ids[a]
        j_ids[a], j_ids[b] = 2 * wc + 2, 3 * wc + 4
        for a, b in DUPLICATE_ROWS:
            i_ids[b], j_ids[b] = i_ids[a], j_ids[a]
    return i_ids.long(), j_ids.long()


def query_scale(scaled):
    return torch.tensor([list(QUERY_SCALE)]) if scaled else None


def coarse_points(M, scaled):
    """mkpts_query_c as tests/helpers.py::fine_setup builds it: cell (x, y) * 8 * query_image_scale[[1, 0]]"""
    _, j_ids = match_ids(M)
    xy = torch.stack([j_ids % HW_C[1], j_ids // HW_C[1]], 1) * (HW_I[0] / HW_C[0])
    if scaled:
        xy = xy * query_scale(True)[0][[1, 0]]
    return xy.float()


def _data(M, scaled, dtype):
    i_ids, j_ids = match_ids(M)
    data = {"q_hw_i": torch.Size(HW_I), "q_hw_c": torch.Size(HW_C), "q_hw_f": torch.Size(HW_F), "b_ids": torch.zeros(M, dtype=torch.long),
            "i_ids": i_ids, "j_ids": j_ids, "mkpts_query_c": coarse_points(M, scaled).to(dtype)}
    if scaled:
        data["query_image_scale"] = query_scale(True).to(dtype)
    return data


# ---- what a wrong kernel could do, restated on the reference (tests/test_fine_cases_cpu.py) ----------------------------------------
VARIANTS = (None, "roll_x", "roll_y", "other_points", "column_major", "scale_order", "half_window")


def _windows(W, M, amp, dtype, variant=None):
    feat, bank = features(amp, M)
    if variant == "roll_x":
        feat = torch.roll(feat, 1, 3)
    if variant == "roll_y":
        feat = torch.roll(feat, 1, 2)
    data = _data(M, False, dtype)
    if variant == "other_points":
        data["i_ids"] = (data["i_ids"] + 1) % N_POINTS
    g3, win = O.fine_preprocess(data, bank.to(dtype), feat.to(dtype), config(W)["loftr_fine"])
    if variant == "column_major" and M:
        win = win.reshape(M, W, W, C).transpose(1, 2).reshape(M, W * W, C)
    return g3, win


@functools.lru_cache(maxsize=None)
def windows_ref(W, M, amp=AMP_SOFT, dtype=torch.float64):
    """-> win [M, W * W, 128] (cells (ky, kx) row-major, zero outside the map), f3 [M, 128]: the tokens before the transformer"""
    g3, win = _windows(W, M, amp, dtype)
    return win.contiguous(), g3[:, :, 0].contiguous()


def transformer_tokens(W, M, amp=AMP_SOFT):
    """-> [M * W * W + M, 128] float32, all window rows first, then the point rows: what opp_transformer(which = 1) takes"""
    win, f3 = windows_ref(W, M, amp, torch.float32)
    return torch.cat([win.reshape(-1, C), f3], 0).contiguous()


@functools.lru_cache(maxsize=None)
def transformer_ref(W, M, amp=AMP_SOFT, dtype=torch.float64):
    """-> [M * W * W + M, 128] in `dtype`, rows as in `transformer_tokens`: the oracle's loftr_fine on the gathered tokens"""
    g3, win = _windows(W, M, amp, dtype)
    with torch.no_grad():
        o3, o2 = O.local_feature_transformer(state_dict(dtype), "loftr_fine", config(W)["loftr_fine"], g3, win)
    return torch.cat([o2.reshape(-1, C), o3.reshape(-1, C)], 0)


@functools.lru_cache(maxsize=None)
def fine_ref(W, M, amp=AMP_SOFT, scaled=True, run_transformer=True, dtype=torch.float64, variant=None):
    """-> expec_f [M, 3], mkpts_query_f [M, 2], var [M, 2] (the unclamped variances of the heatmap along x and y) in `dtype`"""
    data = _data(M, scaled, dtype)
    g3, win = _windows(W, M, amp, dtype, variant)
    with torch.no_grad():
        if run_transformer and M:
            g3, win = O.local_feature_transformer(state_dict(dtype), "loftr_fine", config(W)["loftr_fine"], g3, win)
        else:
            g3 = g3.transpose(1, 2)
        if variant == "scale_order":
            data["query_image_scale"] = data["query_image_scale"][:, [1, 0]]
        O.fine_matching(g3, win, data)
        expec, mk = data["expec_f"], data["mkpts_query_f"]
        if variant == "half_window":                        # W / 2 instead of W // 2 in fine_matching.py:104
            mk = data["mkpts_query_c"] + (mk - data["mkpts_query_c"]) * ((W / 2) / (W // 2))
        if M == 0:
            return expec, mk, torch.empty(0, 2, dtype=dtype)
        # the variances the std column takes the root of, from the same heatmap (fine_matching.py:82-93)
        heat = torch.softmax(torch.einsum("mc,mrc->mr", g3[:, 0], win) / C ** 0.5, 1)
        lin = ((torch.linspace(0, W - 1, W) / (W - 1) - 0.5) * 2).to(dtype)      # the oracle's own grid: float32 values, inexact at W = 7
        grid = torch.stack([lin.view(1, W).expand(W, W).reshape(-1), lin.view(W, 1).expand(W, W).reshape(-1)], -1)
        var = (grid[None] ** 2 * heat[:, :, None]).sum(1) - expec[:, :2] ** 2
    return expec, mk, var


def std_rows(W, M, amp, run_transformer=True):
    """-> [M] bool: the matches whose std column is compared (both float64 variances above VAR_MIN).  All of them in the soft cases."""
    var = fine_ref(W, M, amp, True, run_transformer)[2]
    if amp == AMP_SOFT:
        return torch.ones(M, dtype=torch.bool)
    return (var > VAR_MIN).all(1)


def outside_cells(W, j):
    """-> [W * W] bool: the window cells of coarse cell j that lie outside the fine map, from the geometry alone"""
    jy, jx = j // HW_C[1], j % HW_C[1]
    k = torch.arange(W) - W // 2
    y, x = (jy * STRIDE + k).view(W, 1).expand(W, W), (jx * STRIDE + k).view(1, W).expand(W, W)
    return ((y < 0) | (y >= HW_F[0]) | (x < 0) | (x >= HW_F[1])).reshape(-1)


def rel_err(got, ref):
    """max |got - ref| over max(1, |ref|max), in float64"""
    ref = ref.double()
    return (got.double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())


# ---- through the module ------------------------------------------------------------------------------------------------------------
# One forward at 64 x 96 with 136 points, thr = 0 and border_rm = 0, windows 3 and 7, against the float32 oracle at the bars of
# test_stages_gpu.py::test_tiny_shapes_vs_oracle (1e-4 on conf_matrix and on all three columns of expec_f, 1e-3 on the pixels).  The
# input seed is the first of 21 .. 26 at which the float32 oracle is within a tenth of those bars of its own float64 evaluation at both
# windows (12 matches, 9 on the border; expec_f 3.2e-6, pixels 1.9e-5, conf_matrix 3.3e-6).  At seed 21 the oracle's std column is
# 1.2e-4 from float64 at window 3: a reference that far out cannot carry a 1e-4 bar.
MODULE_WINDOWS = (3, 7)
MODULE_HW, MODULE_N, MODULE_WEIGHT_SEED, MODULE_INPUT_SEED = (64, 96), 136, 3, 25
MODULE_BARS = {"conf_matrix": 1e-4, "expec_f": 1e-4, "mkpts_query_f": 1e-3}


def module_case(window):
    """-> cfg, state dict, data (float32)"""
    from onepose_plus_plus_amd.synthetic import make_inputs
    cfg = default_config(thr=0.0)
    cfg["coarse_matching"]["border_rm"] = 0
    cfg["loftr_fine"]["window_size"] = window
    return cfg, make_state_dict(cfg, MODULE_WEIGHT_SEED), make_inputs(MODULE_N, MODULE_HW, MODULE_INPUT_SEED)


@functools.lru_cache(maxsize=None)
def module_ref(window, dtype=torch.float32):
    """-> the oracle's data dict after O.forward in `dtype`.  Read-only: shared between tests."""
    cfg, sd, data = module_case(window)
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    ref = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in data.items()}
    O.forward(sd, ref, cfg)
    return ref


def border_matches(j_ids):
    hc, wc = MODULE_HW[0] // 8, MODULE_HW[1] // 8
    jy, jx = j_ids // wc, j_ids % wc
    return int(((jy == 0) | (jx == 0) | (jy == hc - 1) | (jx == wc - 1)).sum())
