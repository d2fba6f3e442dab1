"""Seeded cases of the per-sample state of the coarse level -- `query_image_mask` (OnePosePlusModel.py:158, linear_attention.py:49-53,
coarse_matching.py:108-114) and the B > 1 keypoint extent (utils/normalize.py:20-21, quirk q4) -- with references evaluated on the CPU
by oracle/onepose_oracle.py in float64.  Shared by tests/test_mask_cases_cpu.py (which shows from the references alone that a wrong
mask cannot pass) and tests/test_query_mask_gpu.py (which holds the HIP stages to them).  Nothing here touches a GPU.

Shapes (hc, wc, N): the smallest that put masked cells into a second and a third tile of every kernel that reads the mask -- the
64-token tile of the fused encoder layer, the 128-row tile of the QKV GEMM, the 128-cell tile of the score kernels and the 64-column
halves of their row statistics -- and end inside a tile: L = 192, 260, 768.
"""
import functools

import torch

from onepose_plus_plus_amd.config import default_config
from onepose_plus_plus_amd.synthetic import make_state_dict
from oracle import onepose_oracle as O

SHAPES = [(12, 16, 77), (20, 13, 261), (24, 32, 1000)]
VALID = {(12, 16, 77): (9, 13), (20, 13, 261): (20, 9), (24, 32, 1000): (17, 32)}     # mask (a): ones on [:hv, :wv]
SINGLE_CELLS = (0, 63, 64, 127, 128, -1)     # mask (b): flat indices (-1 = L - 1) on either side of the tile boundaries
# mask (b) zeroes ONE cell at each index: six cells move the float64 transformer reference by 4.2e-2 .. 9.4e-2 of its largest entry on
# the unmasked image rows and by 2.1e-2 .. 4.5e-2 on the point rows (the smaller figures at L = 768), above the 1e-2 that
# tests/test_mask_cases_cpu.py asks for, so a run of 8 cells per index is not needed
SINGLE_RUN = 1
LONE_CELL = 70                               # mask (d): the only unmasked cell
WEIGHT_SEED = 3
THR = 0.1
C = 256

# bars of the stages, the project's existing ones
BAR_TRANSFORMER = 5e-5     # of max(1, |ref|max): test_stages_gpu.py::test_tokens_and_transformer
BAR_CONF = 1e-4            # absolute, conf_matrix and mconf: tests/helpers.py TOL_CONF
BAR_KPT = 3e-5             # of max(1, |ref|max): test_stages_gpu.py::test_tokens_and_transformer (point rows)
DECISIVE = 1e-3            # margin of a decisive reference match to thr and to the runner-up of its row and column

KPT_SIZES = (2, 31, 32, 33, 1023, 1025, 2100)    # around the 32 points of a block and the 1024 threads of the statistics kernel
KPT_EXTENT_N, KPT_EXTENT_N0 = 333, 50
KPT_DISABLED_SIZES = (33, 1000)
KPT_OFFCENTRE = (300, (5.0, -3.0, 2.0), 0.3)     # N, centre, extent


def config(kpt_enc=True):
    cfg = default_config(thr=THR)
    cfg["keypoints_encoding"]["enable"] = bool(kpt_enc)
    return cfg


@functools.lru_cache(maxsize=None)
def state_dict(dtype=torch.float32, kpt_enc=True):
    sd = make_state_dict(config(kpt_enc), WEIGHT_SEED)
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def mask(shape, kind):
    """-> [L] floats (1 = valid cell), or None for kind None"""
    hc, wc, _ = shape
    L = hc * wc
    if kind is None:
        return None
    if kind == "a":
        hv, wv = VALID[shape]
        m = torch.zeros(hc, wc)
        m[:hv, :wv] = 1.0
        return m.reshape(L)
    if kind == "b":
        m = torch.ones(L)
        for c in SINGLE_CELLS:
            c = c % L
            m[c:min(L, c + SINGLE_RUN)] = 0.0
        return m
    if kind == "c":
        return torch.ones(L)
    if kind == "d":
        m = torch.zeros(L)
        m[LONE_CELL] = 1.0
        return m
    raise ValueError(kind)


# ---- coarse transformer --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def transformer_inputs(shape):
    """-> f2 [1, L, 256] image tokens, f3 [1, 256, N] point tokens (the layout LocalFeatureTransformer.forward takes)"""
    hc, wc, n = shape
    L = hc * wc
    g = torch.Generator().manual_seed(L + n)
    return torch.randn(1, L, C, generator=g), torch.randn(1, C, n, generator=g)


def transformer_tokens(shape):
    """-> [L + N, 256], image tokens first: what opp_transformer takes"""
    f2, f3 = transformer_inputs(shape)
    return torch.cat([f2[0], f3[0].t()], 0).contiguous()


@functools.lru_cache(maxsize=None)
def transformer_ref(shape, kind, dtype=torch.float64):
    """-> [L + N, 256] in `dtype`: the oracle's loftr_coarse on the case's tokens under mask `kind`.  Read-only: shared between tests."""
    f2, f3 = transformer_inputs(shape)
    m = mask(shape, kind)
    with torch.no_grad():
        o3, o2 = O.local_feature_transformer(state_dict(dtype), "loftr_coarse", config()["loftr_coarse"], f3.to(dtype), f2.to(dtype),
                                             m[None].to(dtype) if m is not None else None)
    return torch.cat([o2[0], o3[0]], 0)


def rel_err(got, ref):
    """max |got - ref| over max(1, |ref|max), in float64"""
    ref = ref.double()
    return (got.double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())


# ---- coarse matcher ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matcher_inputs(shape):
    """As test_two_sweep_matcher_equals_the_materialised_path: features of magnitude 4, min(N, L) // 2 points planted on randomly
    chosen cells with 0.4 noise (so part of the planted cells lie under mask (a)).  -> f3d [N, 256], f2d [L, 256], kpts [N, 3]"""
    hc, wc, n = shape
    L = hc * wc
    g = torch.Generator().manual_seed(5 + n)
    f2d = torch.randn(L, C, generator=g) * 4
    f3d = torch.randn(n, C, generator=g) * 4
    m = min(n, L) // 2
    cells = torch.randperm(L, generator=g)[:m]
    f3d[:m] = f2d[cells] + 0.4 * torch.randn(m, C, generator=g)
    kpts = torch.rand(n, 3, generator=g) - 0.5
    return f3d, f2d, kpts


@functools.lru_cache(maxsize=None)
def matcher_conf(shape, kind, dtype=torch.float64):
    """-> conf_matrix [N, L] in `dtype` (dual softmax with -1e9 on the masked columns)"""
    f3d, f2d, _ = matcher_inputs(shape)
    m = mask(shape, kind)
    t = config()["coarse_matching"]["dual_softmax"]["temperature"]
    with torch.no_grad():
        return O.dual_softmax_conf(f3d[None].to(dtype), f2d[None].to(dtype), t, m[None].to(dtype) if m is not None else None)[0]


def _border_ok(shape):
    hc, wc, _ = shape
    b = config()["coarse_matching"]["border_rm"]
    ok = torch.ones(hc, wc, dtype=torch.bool)
    if b > 0:               # quirk q1: only the first `border_rm` rows / columns of the grid are cleared
        ok[:b] = False
        ok[:, :b] = False
    return ok.reshape(-1)


@functools.lru_cache(maxsize=None)
def matcher_ref(shape, kind):
    """Float64 reference of the match list.  -> dict:
      conf       [N, L] float64
      matches    {(i, j): confidence}: the reference's matches (coarse_matching.py:145-172)
      decisive   the matches more than DECISIVE away from thr and ahead of the runner-up of their row and of their column by more than DECISIVE
      candidates [N, L] bool: every pair an implementation within DECISIVE of the reference could report -- within DECISIVE of thr, of
                 its row maximum and of its column maximum, outside the removed border.  Matches are a subset."""
    conf = matcher_conf(shape, kind)
    hc, wc, _ = shape
    cm = config()["coarse_matching"]
    _, i_ids, j_ids, mconf = O.coarse_match_select(conf[None], (hc, wc), cm["thr"], cm["border_rm"])
    matches = {(int(i), int(j)): float(c) for i, j, c in zip(i_ids, j_ids, mconf)}
    row2 = conf.topk(2, dim=1).values[:, 1]
    col2 = conf.topk(2, dim=0).values[1]
    decisive = {ij for ij, c in matches.items()
                if abs(c - cm["thr"]) > DECISIVE and c - float(row2[ij[0]]) > DECISIVE and c - float(col2[ij[1]]) > DECISIVE}
    cand = (conf > cm["thr"] - DECISIVE) & (conf >= conf.max(1, keepdim=True).values - DECISIVE) & \
        (conf >= conf.max(0, keepdim=True).values - DECISIVE) & _border_ok(shape)[None]
    return {"conf": conf, "matches": matches, "decisive": decisive, "candidates": cand}


# ---- keypoint tokens -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kpt_inputs(n, centre=(0.0, 0.0, 0.0), extent=1.0):
    """-> kpts [1, n, 3] uniform in a cube of edge `extent` around `centre`, coarse bank [1, 256, n]"""
    g = torch.Generator().manual_seed(100 + n)
    kpts = (torch.rand(1, n, 3, generator=g) - 0.5) * extent + torch.tensor(centre)
    return kpts, torch.randn(1, C, n, generator=g)


def kpt_extent_cloud():
    """the cloud of batch element 0 of the extent case: KPT_EXTENT_N0 points, twice the extent of the encoded cloud"""
    g = torch.Generator().manual_seed(7)
    return (torch.rand(KPT_EXTENT_N0, 3, generator=g) - 0.5) * 2.0


def kpt_ref(kpts, bank, extent_ref=None, dtype=torch.float64):
    """-> point tokens [n, 256] in `dtype`.  extent_ref [n0, 3]: the keypoints of batch element 0.  The oracle takes a [B, n, 3] batch,
    so the reference cloud is brought to n rows by repeating its own points, which leaves its bounding box -- the only thing
    normalize_3d_keypoints reads of batch element 0 for the other elements -- unchanged; the tokens of element 1 are returned."""
    k = kpts.to(dtype)
    if extent_ref is not None:
        n = k.shape[1]
        e = extent_ref.to(dtype)
        assert e.shape[0] <= n
        e = e.repeat((n + e.shape[0] - 1) // e.shape[0], 1)[:n]
        k = torch.cat([e[None], k], 0)
    with torch.no_grad():
        norm = O.normalize_3d_keypoints(k)[-1:]
        return O.keypoint_encoding(state_dict(dtype), norm, bank.to(dtype))[0].t().contiguous()


# ---- B = 2 through the module ----------------------------------------------------------------------
BATCH_HW, BATCH_N, BATCH_VALID = (160, 208), 333, (17, 21)      # coarse grid 20 x 26, L = 520; sample 0 is valid on [:17, :21]


def batch_case():
    """-> cfg, state dict, data of a B = 2 batch built like tests/helpers.py::batch_setup (per-sample clouds of different extent, per-sample
    image scales): sample 0 carries a padding mask, sample 1's mask is all ones"""
    from onepose_plus_plus_amd.synthetic import make_inputs
    cfg = default_config(thr=0.0)
    sd = make_state_dict(cfg, 0)
    parts = [make_inputs(BATCH_N, BATCH_HW, s) for s in (11, 12)]
    data = {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}
    data["query_image_scale"] = torch.tensor([[1.0, 1.0], [1.25, 0.875]])
    data["keypoints3d"] = data["keypoints3d"] * torch.tensor([1.0, 1.5]).view(2, 1, 1)
    hc, wc = BATCH_HW[0] // 8, BATCH_HW[1] // 8
    m = torch.ones(2, hc, wc)
    m[0, BATCH_VALID[0]:] = 0.0
    m[0, :, BATCH_VALID[1]:] = 0.0
    data["query_image_mask"] = m
    return cfg, sd, data
