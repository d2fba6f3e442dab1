"""The KV / Ksum chunk partials of the coarse linear attention formed inside the fused encoder layer kernel (enc_layer64.hip, step 8:
layer i's kernel reduces phi(K)^T V and sum phi(K) of its 64-token tile for layer i + 1; linear_attention.py:57-58) against the
stand-alone gather (linattn_kv_mfma_kernel, selected by OPP_KV_FOLD=0): the same MFMA chain on the same operands and the same fixed
summation order, so every layer's reduced KV and Ksum and the final tokens must agree bit for bit."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

# (len0 image tokens, len1 point tokens, masked image tokens [begin, end) or None)
CASES = [
    (64, 8, None),            # one chunk per stream, the second one ragged
    (192, 77, None),          # an incomplete four-chunk group in both streams
    (320, 261, None),         # a second group; the last chunk of stream 1 has 5 tokens
    (256, 256, (50, 140)),    # query_image_mask zeroes a run of image tokens that crosses the tile boundaries at 64 and 128
]
C = 256


@pytest.fixture(scope="module")
def models():
    """k -> coarse transformer of the first k default layers (its workspace ends with the KV / Ksum layer k - 1 applied)"""
    from tests import hip_ops as ops
    from onepose_plus_plus_amd import default_config
    from onepose_plus_plus_amd.synthetic import make_state_dict
    t = default_config()["loftr_coarse"]
    names = list(t["layer_names"]) * t["layer_iter_n"]      # self, cross, self, cross, self, cross
    out = {}
    for k in range(1, len(names) + 1):
        cfg = default_config()
        cfg["loftr_coarse"]["layer_names"] = names[:k]
        cfg["loftr_coarse"]["layer_iter_n"] = 1
        out[k] = ops.make_model(cfg, make_state_dict(cfg, 3), "bf16x3")
    return out


def _run(model, tokens, len0, len1, mask, fold):
    """-> (tokens after the transformer, KV [2, 8192], Ksum [2, 256] of its last layer, the K | V columns left in the workspace), on the CPU"""
    from tests import hip_ops as ops
    from onepose_plus_plus_amd import _lib
    lib, ctx = ops.ctx_of(model)
    stream = torch.cuda.current_stream().cuda_stream
    x = tokens.cuda().contiguous().clone()
    n = lib.opp_transformer_workspace_bytes(ctx, 0, 1, len0, len1)
    ws = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")      # NaN patterns: nothing is read before it is written
    kv_off, ks_off = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.check(lib.opp_transformer_kv_offsets(ctx, 0, 1, len0, len1, ctypes.byref(kv_off), ctypes.byref(ks_off)), "kv_offsets")
    m = mask.cuda().contiguous() if mask is not None else None
    before = os.environ.get("OPP_KV_FOLD")
    if fold:
        os.environ.pop("OPP_KV_FOLD", None)
    else:
        os.environ["OPP_KV_FOLD"] = "0"
    try:
        _lib.check(lib.opp_set_query_mask(ctx, m.data_ptr() if m is not None else None), "query_mask")
        _lib.check(lib.opp_transformer(ctx, 0, x.data_ptr(), 1, len0, len1, ws.data_ptr(), n, stream), "transformer")
        torch.cuda.synchronize()
    finally:
        lib.opp_set_query_mask(ctx, None)
        if before is None:
            os.environ.pop("OPP_KV_FOLD", None)
        else:
            os.environ["OPP_KV_FOLD"] = before
    kv = ws[kv_off.value:kv_off.value + 2 * C * 32 * 4].view(torch.float32).view(2, C * 32)
    ks = ws[ks_off.value:ks_off.value + 2 * C * 4].view(torch.float32).view(2, C)
    # the projection rows phi(Q) | phi(K) | V / S open the workspace (plan_transformer, csrc/api.hip)
    kcols = ws[:(len0 + len1) * 3 * C * 4].view(torch.float32).view(-1, 3 * C)[:, C:]
    return x.cpu(), kv.cpu(), ks.cpu(), kcols.cpu()


@pytest.mark.parametrize("len0,len1,masked", CASES)
def test_kv_partials_of_the_layer_kernel_match_the_gather_bit_for_bit(models, len0, len1, masked):
    g = torch.Generator().manual_seed(29 + len0 + 3 * len1)
    tokens = torch.randn(len0 + len1, C, generator=g)
    mask = None
    if masked is not None:
        mask = torch.ones(len0)
        mask[masked[0]:masked[1]] = 0.0
    for k, model in models.items():
        a = _run(model, tokens, len0, len1, mask, fold=True)
        b = _run(model, tokens, len0, len1, mask, fold=False)
        for what, u, v in zip(("tokens", "kv", "ks"), a, b):
            assert torch.isfinite(u).all(), "layer %d: %s not finite" % (k - 1, what)
            assert torch.equal(u, v), "layer %d: max |fold - gather| of %s = %.3e" % (k - 1, what, (u - v).abs().max().item())
        assert not torch.equal(a[0], tokens)
        # the fold really ran: from layer 1 on it leaves the K | V columns of the projection buffer as layer 0 wrote them
        assert torch.equal(a[3], b[3]) == (k == 1), "layer %d: the two modes ran the same launches" % (k - 1)
        assert a[1].abs().max().item() > 0 and a[2].abs().max().item() > 0
        if mask is not None and k == 1:      # the mask reaches the sums: Ksum of the image stream differs from the unmasked run
            assert not torch.equal(_run(model, tokens, len0, len1, None, fold=True)[2][0], a[2][0])
