"""GPU-side test wrappers around the C ABI (include/opp_hip.h).  Test infrastructure only."""
import ctypes

import torch

from onepose_plus_plus_amd import _lib, OnePosePlus_model


def _s():
    return torch.cuda.current_stream().cuda_stream


def pad32(c):
    return (c + 31) // 32 * 32


def pack_h2(w, scaled=True):
    """-> (pre-split weights, device {scale, 1/scale} or None)"""
    lib = _lib.load()
    out = torch.empty_like(w)
    sc = torch.zeros(2, device="cuda") if scaled else None
    _lib.check(lib.opp_pack_h2(w.data_ptr(), out.data_ptr(), w.numel(), sc.data_ptr() if scaled else None, _s()),
               "opp_pack_h2")
    return out, sc


def pack_b3(w):
    """-> bf16x3 pre-split weights (1.5x the floats)"""
    lib = _lib.load()
    out = torch.empty(w.numel() // 2 * 3, device="cuda")
    _lib.check(lib.opp_pack_b3(w.data_ptr(), out.data_ptr(), w.numel(), _s()), "opp_pack_b3")
    return out


def _prec(h2):
    """test-side selector -> C ABI `prec`: 0 fp32, 1 fp16x2 (scaled split), 2 fp16x2 (unscaled split), 3 bf16x3"""
    return {0: 0, 1: 1, 2: 1, 3: 2}[h2]


def _split(W, h2):
    if h2 == 3:
        return pack_b3(W), None
    if h2:
        return pack_h2(W, scaled=(h2 == 1))
    return W, None


def linear(A, W, act=0, cfg=-1, h2=0):
    lib = _lib.load()
    A = A.cuda().contiguous()
    W = W.cuda().contiguous()
    M, K = A.shape
    N = W.shape[0]
    W, sc = _split(W, h2)
    C = torch.full((M, N), float("nan"), device="cuda")
    _lib.check(lib.opp_linear(A.data_ptr(), M, K, W.data_ptr(), N, act, C.data_ptr(), cfg, _prec(h2),
                              sc.data_ptr() if sc is not None else None, _s()), "opp_linear")
    torch.cuda.synchronize()
    return C.cpu()


def linear_layernorm(A, W, gamma, beta, residual=None, h2=0, in_place=False):
    lib = _lib.load()
    A = A.cuda().contiguous()
    W = W.cuda().contiguous()
    M, K = A.shape
    N = W.shape[0]
    W, sc = _split(W, h2)
    g, b = gamma.cuda().contiguous(), beta.cuda().contiguous()
    r = residual.cuda().contiguous() if residual is not None else None
    C = r if (in_place and r is not None) else torch.full((M, N), float("nan"), device="cuda")
    _lib.check(lib.opp_linear_layernorm(A.data_ptr(), M, K, W.data_ptr(), N, g.data_ptr(), b.data_ptr(),
                                        r.data_ptr() if r is not None else None, C.data_ptr(), _prec(h2),
                                        sc.data_ptr() if sc is not None else None, _s()), "opp_linear_layernorm")
    torch.cuda.synchronize()
    return C.cpu()


def to_nhwc_padded(x_nchw, c_pad):
    b, c, h, w = x_nchw.shape
    assert b == 1
    out = torch.zeros(h, w, c_pad)
    out[:, :, :c] = x_nchw[0].permute(1, 2, 0)
    return out.cuda().contiguous()


def from_nhwc(y, c):
    return y[:, :, :c].permute(2, 0, 1).unsqueeze(0).cpu()


def conv2d(x_nchw, w, scale=None, bias=None, stride=1, residual=None, res_mode=0, act=0, cfg=-1, h2=0):
    """x [1,Cin,H,W]; w [Cout,Cin,k,k]; y = act(conv(x, w*scale) + bias + residual)."""
    lib = _lib.load()
    cout, cin, ks, _ = w.shape
    cin_p, cout_p = pad32(cin), pad32(cout)
    x = to_nhwc_padded(x_nchw, cin_p)
    H, W = x_nchw.shape[2:]
    pad = ks // 2
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    wp = torch.empty(cout_p * lib.opp_conv_packed_k(cin, ks), device="cuda")
    wd = w.cuda().contiguous()
    sd = None
    if scale is not None:
        sd = torch.zeros(cout_p, device="cuda")
        sd[:cout] = scale.cuda()
    _lib.check(lib.opp_pack_conv_weight(wd.data_ptr(), sd.data_ptr() if sd is not None else None, cout, cin, ks,
                                        cout_p, cin_p, wp.data_ptr(), _s()), "pack")
    wp, sc = _split(wp, h2)
    bd = None
    if bias is not None:
        bd = torch.zeros(cout_p, device="cuda")
        bd[:cout] = bias.cuda()
    rd = None
    if residual is not None:
        rd = to_nhwc_padded(residual, cout_p)
    y = torch.full((Ho, Wo, cout_p), float("nan"), device="cuda")
    _lib.check(lib.opp_conv2d_nhwc(x.data_ptr(), H, W, cin, wp.data_ptr(), bd.data_ptr() if bd is not None else None,
                                   cout_p, ks, stride, rd.data_ptr() if rd is not None else None, res_mode, act,
                                   y.data_ptr(), cfg, _prec(h2), sc.data_ptr() if sc is not None else None, _s()),
               "conv2d")
    torch.cuda.synchronize()
    pad_part = y[:, :, cout:]
    return from_nhwc(y, cout), (pad_part.abs().max().item() if pad_part.numel() else 0.0)


def conv2d_split(x_nchw, w, scale=None, bias=None, stride=1, residual=None, res_mode=0, act=0, cfg=-1, give_fp32=True, give_split=True,
                 want_fp32=True, want_split=True):
    """The bf16x3 convolution through opp_conv2d_nhwc_split: input as fp32 rows and / or pre-split rows (opp_pack_b3 of the fp32 rows), output
    as fp32 rows and / or pre-split rows.  -> (y fp32 NHWC padded or None, y_split raw floats or None, the plain opp_conv2d_nhwc(prec=2) result,
    opp_pack_b3 of that result)"""
    lib = _lib.load()
    cout, cin, ks, _ = w.shape
    cin_p, cout_p = pad32(cin), pad32(cout)
    x = to_nhwc_padded(x_nchw, cin_p)
    H, W = x_nchw.shape[2:]
    pad = ks // 2
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    wp = torch.empty(cout_p * lib.opp_conv_packed_k(cin, ks), device="cuda")
    wd = w.cuda().contiguous()
    sd = None
    if scale is not None:
        sd = torch.zeros(cout_p, device="cuda")
        sd[:cout] = scale.cuda()
    _lib.check(lib.opp_pack_conv_weight(wd.data_ptr(), sd.data_ptr() if sd is not None else None, cout, cin, ks,
                                        cout_p, cin_p, wp.data_ptr(), _s()), "pack")
    wp = pack_b3(wp)
    bd = None
    if bias is not None:
        bd = torch.zeros(cout_p, device="cuda")
        bd[:cout] = bias.cuda()
    rd = to_nhwc_padded(residual, cout_p) if residual is not None else None
    ref = torch.full((Ho, Wo, cout_p), float("nan"), device="cuda")
    _lib.check(lib.opp_conv2d_nhwc(x.data_ptr(), H, W, cin, wp.data_ptr(), bd.data_ptr() if bd is not None else None,
                                   cout_p, ks, stride, rd.data_ptr() if rd is not None else None, res_mode, act,
                                   ref.data_ptr(), cfg, 2, None, _s()), "conv2d")
    xs = pack_b3(x)
    y = torch.full((Ho, Wo, cout_p), float("nan"), device="cuda") if want_fp32 else None
    ys = torch.full((Ho * Wo * cout_p // 2 * 3,), float("nan"), device="cuda") if want_split else None
    _lib.check(lib.opp_conv2d_nhwc_split(x.data_ptr() if give_fp32 else None, xs.data_ptr() if give_split else None, H, W, cin, wp.data_ptr(),
                                         bd.data_ptr() if bd is not None else None, cout_p, ks, stride,
                                         rd.data_ptr() if rd is not None else None, res_mode, act,
                                         y.data_ptr() if y is not None else None, ys.data_ptr() if ys is not None else None, cfg, _s()),
               "conv2d_split")
    torch.cuda.synchronize()
    return y, ys, ref, pack_b3(ref)


def layer_norm(x, g, b, res=None):
    lib = _lib.load()
    x = x.cuda().contiguous()
    out = torch.empty_like(x)
    r = res.cuda().contiguous() if res is not None else None
    g, b = g.cuda().contiguous(), b.cuda().contiguous()
    _lib.check(lib.opp_layer_norm(x.data_ptr(), g.data_ptr(), b.data_ptr(), r.data_ptr() if r is not None else None,
                                  out.data_ptr(), x.shape[0], x.shape[1], _s()), "layer_norm")
    torch.cuda.synchronize()
    return out.cpu()


PRECISIONS = ("bf16x3", "fp32")        # the product's arithmetics (both not narrower than the reference's fp32)


def has_fp16x2():
    """fp16x2 kernels exist in the tuning library only (OPP_HIP_LIB=.../libopp_hip_tuning.so): kernel-level tests of that arithmetic skip otherwise"""
    return bool(_lib.load().opp_supports_precision(1))


# ---- where the stage helpers below get their memory ("The workspace contract") -------------------------------------
GUARD_BYTES = 4096           # canary band in front of and behind every guarded buffer
GUARD_ALIGN = 256            # alignment of a guarded view: the alignment of the library's own bump allocator
CANARY = 0xA5
NAN_WORD = 0x7FC00000        # the float poison of the `nan` fill
WS_FILLS = ("zero", "nan", "leftover")


class Buffers:
    """The memory of one helper call: the workspace, the outputs and the device copies of the inputs.  This default allocates each
    buffer on its own, exactly sized, as the helpers always did (outputs NaN-filled where they were); `GuardedBuffers` is the
    variant that checks the memory contract of a call."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)

    def workspace(self, nbytes, name="ws"):
        return torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)

    def ws_bytes(self, ws):
        """the size the C call is told its workspace has"""
        return ws.numel()

    def output(self, shape, dtype=torch.float32, fill=float("nan"), name="out"):
        """fill None = uninitialised (the helper reads only what the call reports as written)"""
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        if fill is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        return torch.full(shape, fill, dtype=dtype, device=self.device)

    def input(self, t, name="in"):
        """device copy of a tensor the call may only read"""
        return t.to(self.device).contiguous()

    def inout(self, t, name="inout"):
        """device copy of a tensor the call updates in place"""
        return t.to(self.device).contiguous().clone()

    def call(self, rc, what):
        _lib.check(rc, what)

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()

    def check(self):
        return []


DEFAULT_BUFFERS = Buffers()


class GuardedBuffers(Buffers):
    """Every buffer is a view, `GUARD_ALIGN`-aligned, into a larger allocation of its own with `GUARD_BYTES` (at least) of `CANARY` bytes
    in front of it and behind it.  The workspace view is exactly as long as requested and prefilled:
      zero      zeros
      nan       the float pattern 0x7FC00000 in every word
      leftover  nothing: the view is a prefix of the allocation the previous call of this object used (`new_call()` between the
                two), as a grow-only cached workspace hands a small call the bytes of a larger one; a workspace that is new is zeros
    `check()` -> the buffers whose guard bands changed and the inputs whose bytes changed; `touched()` -> the outputs and workspaces
    whose bytes differ from what they held before the call (for a call that must refuse).  `ws_given` maps the true workspace size to
    the size the call is told (a refusal test passes n // 2 or 0; the view keeps its full length)."""

    def __init__(self, fill="zero", device="cuda", ws_given=None):
        super().__init__(device)
        assert fill in WS_FILLS, fill
        self.fill = fill
        self.ws_given = ws_given
        self.rcs = []                    # return codes of the C calls made through `call`
        self._arenas = {}                # workspace name -> (raw allocation, view offset, capacity)
        self._records = []               # of the current call: [name, kind, raw, offset, nbytes, view, snapshot]

    def call(self, rc, what):
        self.rcs.append(rc)
        _lib.check(rc, what)

    def new_call(self):
        """forget the outputs and inputs of the call before; the workspace allocations stay (fill `leftover`)"""
        self._records = []

    def _alloc(self, nbytes):
        raw = torch.empty(nbytes + 2 * GUARD_BYTES + GUARD_ALIGN, dtype=torch.uint8, device=self.device)
        raw.fill_(CANARY)
        off = GUARD_BYTES + (-(raw.data_ptr() + GUARD_BYTES)) % GUARD_ALIGN
        return raw, off

    def _record(self, name, kind, raw, off, nbytes, view):
        self._records.append([name, kind, raw, off, nbytes, view, view.clone()])
        return view

    def workspace(self, nbytes, name="ws"):
        nbytes = int(nbytes)
        if name in self._arenas and self.fill == "leftover":
            raw, off, cap = self._arenas[name]
            assert nbytes <= cap, "leftover: the call before must be the larger one (%d > %d bytes)" % (nbytes, cap)
            raw[off + nbytes:off + nbytes + GUARD_BYTES] = CANARY          # the band behind the shorter view
        else:
            raw, off = self._alloc(nbytes)
            self._arenas[name] = (raw, off, nbytes)
            view = raw[off:off + nbytes]
            if self.fill == "nan":
                view[:nbytes // 4 * 4].view(torch.int32).fill_(NAN_WORD)
                view[nbytes // 4 * 4:] = 0x7F
            else:
                view.zero_()
        return self._record(name, "ws", raw, off, nbytes, raw[off:off + nbytes])

    def ws_bytes(self, ws):
        return ws.numel() if self.ws_given is None else int(self.ws_given(ws.numel()))

    def _typed(self, shape, dtype, name, kind, src=None, fill=None):
        shape = tuple(shape) if not isinstance(shape, int) else (shape,)
        n = 1
        for d in shape:
            n *= d
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        raw, off = self._alloc(nbytes)
        view = raw[off:off + nbytes].view(dtype).view(shape)
        if src is not None:
            view.copy_(src)
        elif fill is not None:
            view.fill_(fill)
        return self._record(name, kind, raw, off, nbytes, view)

    def output(self, shape, dtype=torch.float32, fill=float("nan"), name="out"):
        return self._typed(shape, dtype, name, "out", fill=fill)

    def input(self, t, name="in"):
        return self._typed(t.shape, t.dtype, name, "in", src=t)

    def inout(self, t, name="inout"):
        return self._typed(t.shape, t.dtype, name, "out", src=t)

    @staticmethod
    def _same(view, snap):
        a, b = view.contiguous().view(-1).view(torch.uint8), snap.contiguous().view(-1).view(torch.uint8)
        return bool(torch.equal(a, b))

    def check(self):
        bad = []
        for name, kind, raw, off, nbytes, view, snap in self._records:
            front, back = raw[:off], raw[off + nbytes:off + nbytes + GUARD_BYTES]
            if bool((front != CANARY).any()):
                bad.append("%s: written in front of the buffer" % name)
            if bool((back != CANARY).any()):
                bad.append("%s: written behind the buffer" % name)
            if kind == "in" and not self._same(view, snap):
                bad.append("%s: read-only input changed" % name)
        return bad

    def touched(self):
        return [name for name, kind, raw, off, nbytes, view, snap in self._records if kind != "in" and not self._same(view, snap)]


def linear_attention(qkv, n_seg, len0, len1, C, nhead, cross, bufs=None):
    """qkv [n_seg*(len0+len1), 3C] (phi(Q) | phi(K) | V/S) -> message [same rows, C] (opp_linear_attention)."""
    lib = _lib.load()
    bufs = bufs or DEFAULT_BUFFERS
    q = bufs.input(qkv, "qkv")
    msg = bufs.output((q.shape[0], C), name="msg")
    ws = bufs.workspace(lib.opp_linear_attention_workspace_bytes(n_seg, len0, len1, C, nhead))
    bufs.call(lib.opp_linear_attention(q.data_ptr(), n_seg, len0, len1, C, nhead, cross, msg.data_ptr(), ws.data_ptr(),
                                       bufs.ws_bytes(ws), _s()), "linear_attention")
    torch.cuda.synchronize()
    return msg.cpu()


def make_model(cfg, sd, precision=None):
    m = OnePosePlus_model(cfg).eval()
    m.load_state_dict(sd, strict=True)
    if precision is not None:
        m.set_gemm_precision(precision)
    return m.cuda()


def ctx_of(model):
    return model._ensure_ready(torch.device("cuda", torch.cuda.current_device()))


def backbone(model, img, bufs=None):
    """img [1,1,H,W] (cpu) -> feat_c NCHW [1,256,H/8,W/8], feat_f NCHW [1,128,H/2,W/2] (cpu)."""
    lib, ctx = ctx_of(model)
    bufs = bufs or DEFAULT_BUFFERS
    H, W = img.shape[2:]
    x = bufs.input(img, "image")
    fc = bufs.output((H // 8, W // 8, 256), name="feat_c")
    ff = bufs.output((H // 2, W // 2, 128), name="feat_f")
    ws = bufs.workspace(lib.opp_backbone_workspace_bytes(ctx, H, W))
    bufs.call(lib.opp_backbone(ctx, x.data_ptr(), H, W, fc.data_ptr(), ff.data_ptr(), ws.data_ptr(), bufs.ws_bytes(ws), _s()), "backbone")
    torch.cuda.synchronize()
    return from_nhwc(fc, 256), from_nhwc(ff, 128)


def _set_state(lib, ctx, mask=None, extent_ref=None, bufs=None):
    """Per-sample state of the context (include/opp_hip.h: opp_set_query_mask, opp_set_keypoint_extent_ref) from CPU tensors.
    -> the device tensors, to be kept alive until the call has run; `_clear_state` belongs in the caller's `finally`."""
    bufs = bufs or DEFAULT_BUFFERS
    m = bufs.input(mask.float(), "query_mask") if mask is not None else None
    e = bufs.input(extent_ref.float(), "extent_ref") if extent_ref is not None else None
    _lib.check(lib.opp_set_query_mask(ctx, m.data_ptr() if m is not None else None), "query_mask")
    _lib.check(lib.opp_set_keypoint_extent_ref(ctx, e.data_ptr() if e is not None else None, e.shape[0] if e is not None else 0),
               "extent_ref")
    return m, e


def _clear_state(lib, ctx):
    lib.opp_set_query_mask(ctx, None)
    lib.opp_set_keypoint_extent_ref(ctx, None, 0)


# opp_encode_points / opp_coarse_tokens have no size query: two 8-float statistics blocks at 256-byte offsets = 288 bytes, rounded up
POINT_ENCODER_WS_BYTES = 512


def coarse_tokens(model, feat_c_nchw, pe_tokens, kpts, bank_c, extent_ref=None, bufs=None):
    """extent_ref: optional keypoints [n0, 3] of batch element 0 (B > 1: their bounding box scales this cloud, quirk q4)"""
    lib, ctx = ctx_of(model)
    hc, wc = feat_c_nchw.shape[2:]
    L = hc * wc
    N = kpts.shape[1]
    bufs = bufs or DEFAULT_BUFFERS
    fc = bufs.input(to_nhwc_padded(feat_c_nchw, 256).reshape(L, 256), "feat_c")
    tok = bufs.output((L + N, 256), name="tokens")
    ws = bufs.workspace(POINT_ENCODER_WS_BYTES)
    pe = bufs.input(pe_tokens, "pe") if pe_tokens is not None else None
    k = bufs.input(kpts, "kpts")
    b = bufs.input(bank_c, "bank_c")
    try:
        keep = _set_state(lib, ctx, None, extent_ref, bufs)
        bufs.call(lib.opp_coarse_tokens(ctx, fc.data_ptr(), pe.data_ptr() if pe is not None else None, L, k.data_ptr(),
                                        b.data_ptr(), N, tok.data_ptr(), ws.data_ptr(), bufs.ws_bytes(ws), _s()), "coarse_tokens")
        torch.cuda.synchronize()
    finally:
        _clear_state(lib, ctx)
    del keep
    return tok.cpu()


def encode_points(model, kpts, bank_c, extent_ref=None, bufs=None):
    """kpts [1, N, 3], bank_c [1, C, N] (cpu) -> the 3D-point tokens [N, C] (opp_encode_points); extent_ref as in coarse_tokens."""
    lib, ctx = ctx_of(model)
    bufs = bufs or DEFAULT_BUFFERS
    N = kpts.shape[1]
    tok = bufs.output((N, bank_c.shape[1]), name="tokens3d")
    ws = bufs.workspace(POINT_ENCODER_WS_BYTES)
    k = bufs.input(kpts, "kpts")
    b = bufs.input(bank_c, "bank_c")
    try:
        keep = _set_state(lib, ctx, None, extent_ref, bufs)
        bufs.call(lib.opp_encode_points(ctx, k.data_ptr(), b.data_ptr(), N, tok.data_ptr(), ws.data_ptr(), bufs.ws_bytes(ws), _s()),
                  "encode_points")
        torch.cuda.synchronize()
    finally:
        _clear_state(lib, ctx)
    del keep
    return tok.cpu()


def transformer(model, which, tokens, n_seg, len0, len1, mask=None, bufs=None):
    """mask: optional CPU floats [len0] (1 = valid image cell, 0 = padding): query_image_mask of the sample (which = 0, n_seg = 1)"""
    lib, ctx = ctx_of(model)
    bufs = bufs or DEFAULT_BUFFERS
    x = bufs.inout(tokens, "tokens")
    ws = bufs.workspace(lib.opp_transformer_workspace_bytes(ctx, which, n_seg, len0, len1))
    try:
        keep = _set_state(lib, ctx, mask, None, bufs)
        bufs.call(lib.opp_transformer(ctx, which, x.data_ptr(), n_seg, len0, len1, ws.data_ptr(), bufs.ws_bytes(ws), _s()), "transformer")
        torch.cuda.synchronize()
    finally:
        _clear_state(lib, ctx)
    del keep
    return x.cpu()


def coarse_match(model, f3d, f2d, hw_c, kpts, base_scale, qscale, mask=None, bufs=None):
    """f3d [N,C], f2d [L,C] -> dict like the reference data updates.  mask: optional CPU floats [L], as in `transformer`."""
    lib, ctx = ctx_of(model)
    N, L = f3d.shape[0], f2d.shape[0]
    bufs = bufs or DEFAULT_BUFFERS
    a, b, k = bufs.input(f3d, "feat3d"), bufs.input(f2d, "feat2d"), bufs.input(kpts, "kpts")
    q = bufs.input(qscale, "query_scale") if qscale is not None else None
    conf = bufs.output((1, N, L), name="conf")
    i_ids = bufs.output(N, torch.int64, None, "i_ids")
    j_ids = bufs.output(N, torch.int64, None, "j_ids")
    mconf = bufs.output(N, fill=None, name="mconf")
    mkc = bufs.output((N, 2), fill=None, name="mkpts_c")
    mk3 = bufs.output((N, 3), fill=None, name="mkpts_3d")
    cnt = bufs.output(1, torch.int32, 0, "count")
    ws = bufs.workspace(lib.opp_coarse_match_workspace_bytes(ctx, N, L))
    try:
        keep = _set_state(lib, ctx, mask, None, bufs)
        bufs.call(lib.opp_coarse_match(ctx, a.data_ptr(), b.data_ptr(), N, hw_c[0], hw_c[1], k.data_ptr(), base_scale,
                                       q.data_ptr() if q is not None else None, conf.data_ptr(), i_ids.data_ptr(),
                                       j_ids.data_ptr(), mconf.data_ptr(), mkc.data_ptr(), mk3.data_ptr(), cnt.data_ptr(),
                                       ws.data_ptr(), bufs.ws_bytes(ws), _s()), "coarse_match")
        torch.cuda.synchronize()
    finally:
        _clear_state(lib, ctx)
    del keep
    M = int(cnt.item())
    bz = torch.zeros(M, dtype=torch.int64)
    return {"conf_matrix": conf.cpu(), "b_ids": bz, "i_ids": i_ids[:M].cpu(), "j_ids": j_ids[:M].cpu(),
            "mconf": mconf[:M].cpu(), "mkpts_query_c": mkc[:M].cpu(), "mkpts_3d_db": mk3[:M].cpu(),
            "m_bids": bz, "gt_mask": torch.zeros(M, dtype=torch.bool)}


def fine(model, feat_f_nchw, bank_f, i_ids, j_ids, hw_c, mkpts_c, base_scale, qscale, run_transformer=1, spare_rows=0, bufs=None):
    """-> expec_f [M + spare_rows, 3], mkpts_query_f [M + spare_rows, 2], prefilled with NaN: the call may write the first M rows only
    (M = 0: an empty match list passes through, nothing is written)"""
    lib, ctx = ctx_of(model)
    hf, wf = feat_f_nchw.shape[2:]
    M = i_ids.numel()
    N = bank_f.shape[2]
    bufs = bufs or DEFAULT_BUFFERS
    ff = bufs.input(to_nhwc_padded(feat_f_nchw, 128), "feat_f")
    bk = bufs.input(bank_f, "bank_f")
    ii, jj = bufs.input(i_ids.long(), "i_ids"), bufs.input(j_ids.long(), "j_ids")
    mk = bufs.input(mkpts_c.float().reshape(M, 2), "mkpts_c")
    q = bufs.input(qscale, "query_scale") if qscale is not None else None
    ex = bufs.output((M + spare_rows, 3), name="expec_f")
    mf = bufs.output((M + spare_rows, 2), name="mkpts_f")
    ws = bufs.workspace(lib.opp_fine_workspace_bytes(ctx, M))
    bufs.call(lib.opp_fine(ctx, ff.data_ptr(), hf, wf, bk.data_ptr(), N, ii.data_ptr(), jj.data_ptr(), M, hw_c[0],
                           hw_c[1], mk.data_ptr(), base_scale, q.data_ptr() if q is not None else None,
                           run_transformer, ex.data_ptr(), mf.data_ptr(), ws.data_ptr(), bufs.ws_bytes(ws), _s()), "fine")
    torch.cuda.synchronize()
    return ex.cpu(), mf.cpu()


def run_model(model, data_cpu):
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in data_cpu.items()}
    with torch.no_grad():
        model(d)
    torch.cuda.synchronize()
    return d


# ---- training-step entry points (include/opp_hip.h, "training step"): device tensors in, device tensors out ------------------
def _ptr(t):
    return t.data_ptr() if t is not None else None


def conv2d_backward(xn, w, gyn, cin, cout, ks, stride, prec, want_dx=True, want_dw=True, add=None, bufs=None):
    """opp_conv2d_backward_nhwc.  xn [B,H,W,pad32(cin)], gyn [B,Ho,Wo,pad32(cout)] NHWC with zero pad channels, w [cout,cin,ks,ks].
    -> (grad_x [B,H,W,pad32(cin)] or None, grad_w [cout,cin,ks,ks] or None), NaN-prefilled.  add: a gradient already in the buffer that
    receives grad_x (grad_x_add aliased with grad_x, as the residual blocks use it)."""
    lib = _lib.load()
    bufs = bufs or DEFAULT_BUFFERS
    B, H, W, cin_p = xn.shape
    x, gy, wd = bufs.input(xn, "x"), bufs.input(gyn, "grad_y"), bufs.input(w, "w")
    gx = None
    if want_dx:
        gx = bufs.inout(add, "grad_x") if add is not None else bufs.output((B, H, W, cin_p), name="grad_x")
    gw = bufs.output((cout, cin, ks, ks), name="grad_w") if want_dw else None
    ws = bufs.workspace(lib.opp_conv2d_backward_workspace_bytes(B, H, W, cin, cout, ks, stride, prec))
    bufs.call(lib.opp_conv2d_backward_nhwc(x.data_ptr(), B, H, W, cin, wd.data_ptr(), cout, ks, stride, gy.data_ptr(), _ptr(gx),
                                           gx.data_ptr() if add is not None else None, _ptr(gw), prec, ws.data_ptr(), bufs.ws_bytes(ws), _s()),
              "opp_conv2d_backward_nhwc")
    torch.cuda.synchronize()
    return gx, gw


def batchnorm_backward(gyn, yn, rawn, C, act, gamma, mean, invstd, bufs=None):
    """opp_batchnorm_backward_nhwc over [rows, ld] tensors -> (grad_raw, grad_res [rows, ld], grad_gamma, grad_beta [C])"""
    lib = _lib.load()
    bufs = bufs or DEFAULT_BUFFERS
    rows, ld = rawn.shape
    gy, y, raw = bufs.input(gyn, "grad_y"), bufs.input(yn, "y"), bufs.input(rawn, "raw")
    g, m, i = bufs.input(gamma, "gamma"), bufs.input(mean, "mean"), bufs.input(invstd, "invstd")
    d_raw, d_res = bufs.output((rows, ld), name="grad_raw"), bufs.output((rows, ld), name="grad_res")
    dg, db = bufs.output(C, name="grad_gamma"), bufs.output(C, name="grad_beta")
    ws = bufs.workspace(lib.opp_batchnorm_backward_workspace_bytes(rows, ld))
    bufs.call(lib.opp_batchnorm_backward_nhwc(gy.data_ptr(), y.data_ptr(), raw.data_ptr(), rows, ld, C, act, g.data_ptr(), m.data_ptr(),
                                              i.data_ptr(), d_raw.data_ptr(), d_res.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                              bufs.ws_bytes(ws), _s()), "opp_batchnorm_backward_nhwc")
    torch.cuda.synchronize()
    return d_raw, d_res, dg, db


def linear_backward(gy, x, w, prec, want_dx=True, dw_into=None, bufs=None):
    """opp_linear_backward of Y [M,N] = X [M,K] W [N,K]^T -> (grad_x [M,K] or None, grad_w [N,K]).  dw_into: a tensor the weight gradient is
    ADDED to (accumulate_grad_w = 1; the result is a copy, dw_into itself is not changed)."""
    lib = _lib.load()
    bufs = bufs or DEFAULT_BUFFERS
    M, N = gy.shape
    K = x.shape[1]
    g, xd, wd = bufs.input(gy, "grad_out"), bufs.input(x, "x"), bufs.input(w, "w")
    dx = bufs.output((M, K), name="grad_x") if want_dx else None
    dw = bufs.inout(dw_into, "grad_w") if dw_into is not None else bufs.output((N, K), name="grad_w")
    ws = bufs.workspace(lib.opp_linear_backward_workspace_bytes(M, N, K, prec))
    bufs.call(lib.opp_linear_backward(g.data_ptr(), xd.data_ptr(), wd.data_ptr(), M, N, K, _ptr(dx), dw.data_ptr(), 1 if dw_into is not None else 0,
                                      prec, ws.data_ptr(), bufs.ws_bytes(ws), _s()), "opp_linear_backward")
    torch.cuda.synchronize()
    return dx, dw


def dual_softmax_forward(S, with_conf=True, bufs=None):
    """opp_dual_softmax_forward of sim [B,N,L] -> (lse_row [B,N], lse_col [B,L], conf [B,N,L] or None)"""
    lib = _lib.load()
    bufs = bufs or DEFAULT_BUFFERS
    B, N, L = S.shape
    Sc = bufs.input(S, "sim")
    lr, lc = bufs.output((B, N), name="lse_row"), bufs.output((B, L), name="lse_col")
    conf = bufs.output((B, N, L), name="conf") if with_conf else None
    ws = bufs.workspace(lib.opp_dual_softmax_forward_workspace_bytes(B, N, L), "ws_forward")
    bufs.call(lib.opp_dual_softmax_forward(Sc.data_ptr(), B, N, L, lr.data_ptr(), lc.data_ptr(), _ptr(conf), ws.data_ptr(), bufs.ws_bytes(ws), _s()),
              "opp_dual_softmax_forward")
    torch.cuda.synchronize()
    return lr, lc, conf


def dual_softmax_backward(g, S, lse_row, lse_col, bufs=None):
    """opp_dual_softmax_backward -> grad_sim [B,N,L]"""
    lib = _lib.load()
    bufs = bufs or DEFAULT_BUFFERS
    B, N, L = S.shape
    gd, Sc, lr, lc = bufs.input(g, "grad_conf"), bufs.input(S, "sim"), bufs.input(lse_row, "lse_row"), bufs.input(lse_col, "lse_col")
    ds = bufs.output((B, N, L), name="grad_sim")
    ws = bufs.workspace(lib.opp_dual_softmax_backward_workspace_bytes(B, N, L), "ws_backward")
    bufs.call(lib.opp_dual_softmax_backward(gd.data_ptr(), Sc.data_ptr(), lr.data_ptr(), lc.data_ptr(), B, N, L, ds.data_ptr(), ws.data_ptr(),
                                            bufs.ws_bytes(ws), _s()), "opp_dual_softmax_backward")
    torch.cuda.synchronize()
    return ds


def focal_loss(conf, gt, mask0, mask1, alpha, gamma, scales, bufs=None):
    """opp_focal_loss_forward_ex + opp_focal_loss_backward_ex on conf [B,N,L], fp32 ground truth and the two mask factors [B,N], [B,L]
    -> (sums [4] fp64, grad_conf [B,N,L] for `scales` [2])"""
    lib = _lib.load()
    bufs = bufs or DEFAULT_BUFFERS
    B, N, L = conf.shape
    c, t = bufs.input(conf, "conf"), bufs.input(gt.float(), "conf_gt")
    m0, m1, sc = bufs.input(mask0, "mask0"), bufs.input(mask1, "mask1"), bufs.input(scales, "scales")
    sums = bufs.output(4, torch.float64, name="sums")
    grad = bufs.output((B, N, L), name="grad_conf")
    ws = bufs.workspace(lib.opp_focal_loss_workspace_bytes(c.numel()))
    bufs.call(lib.opp_focal_loss_forward_ex(c.data_ptr(), t.data_ptr(), 1, None, m0.data_ptr(), m1.data_ptr(), N, L, c.numel(), alpha, gamma,
                                            sums.data_ptr(), ws.data_ptr(), bufs.ws_bytes(ws), _s()), "opp_focal_loss_forward_ex")
    bufs.call(lib.opp_focal_loss_backward_ex(c.data_ptr(), t.data_ptr(), 1, None, m0.data_ptr(), m1.data_ptr(), N, L, c.numel(), alpha, gamma,
                                             sc.data_ptr(), grad.data_ptr(), _s()), "opp_focal_loss_backward_ex")
    torch.cuda.synchronize()
    return sums, grad


def layer_norm_train(x, gamma, beta, grad_y, bufs=None):
    """opp_layer_norm_train_forward, then opp_layer_norm_train_backward on its statistics -> (y, grad_x [rows,C], grad_gamma, grad_beta [C])"""
    lib = _lib.load()
    bufs = bufs or DEFAULT_BUFFERS
    rows, C = x.shape
    xd, g, b, gy = bufs.input(x, "x"), bufs.input(gamma, "gamma"), bufs.input(beta, "beta"), bufs.input(grad_y, "grad_y")
    y, mean, rstd = bufs.output((rows, C), name="y"), bufs.output(rows, name="mean"), bufs.output(rows, name="rstd")
    dx, dg, db = bufs.output((rows, C), name="grad_x"), bufs.output(C, name="grad_gamma"), bufs.output(C, name="grad_beta")
    ws = bufs.workspace(lib.opp_layer_norm_train_backward_workspace_bytes(rows, C))
    bufs.call(lib.opp_layer_norm_train_forward(xd.data_ptr(), g.data_ptr(), b.data_ptr(), None, rows, C, y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                               _s()), "opp_layer_norm_train_forward")
    bufs.call(lib.opp_layer_norm_train_backward(gy.data_ptr(), xd.data_ptr(), g.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, C, dx.data_ptr(),
                                                dg.data_ptr(), db.data_ptr(), ws.data_ptr(), bufs.ws_bytes(ws), _s()), "opp_layer_norm_train_backward")
    torch.cuda.synchronize()
    return y, dx, dg, db


def linear_attention_train(q, k, v, q_mask, kv_mask, grad_out, short_forward=True, bufs=None):
    """opp_linear_attention_train_forward, then _backward on its KV / Ksum.  q [B,L,H,D], k, v [B,S,H,D], masks [B,L] / [B,S] or None
    -> (out, kv, ks, grad_q, grad_k, grad_v).  Each of the two calls gets a workspace of its own.  short_forward = False: only the
    backward is told `bufs.ws_bytes` (a refusal test of it)."""
    lib = _lib.load()
    bufs = bufs or DEFAULT_BUFFERS
    B, L, H, D = q.shape
    S = k.shape[1]
    qd, kd, vd, go = bufs.input(q, "q"), bufs.input(k, "k"), bufs.input(v, "v"), bufs.input(grad_out, "grad_out")
    qm = bufs.input(q_mask, "q_mask") if q_mask is not None else None
    km = bufs.input(kv_mask, "kv_mask") if kv_mask is not None else None
    out, kv, ks = bufs.output((B, L, H, D), name="out"), bufs.output((B, H, D, D), name="kv"), bufs.output((B, H, D), name="ks")
    gq, gk, gv = bufs.output((B, L, H, D), name="grad_q"), bufs.output((B, S, H, D), name="grad_k"), bufs.output((B, S, H, D), name="grad_v")
    n = lib.opp_linear_attention_train_workspace_bytes(B, L, S, H, D)
    ws = bufs.workspace(n, "ws_forward")
    bufs.call(lib.opp_linear_attention_train_forward(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), _ptr(qm), _ptr(km), B, L, S, H, D, out.data_ptr(),
                                                     kv.data_ptr(), ks.data_ptr(), ws.data_ptr(), bufs.ws_bytes(ws) if short_forward else ws.numel(),
                                                     _s()), "opp_linear_attention_train_forward")
    ws2 = bufs.workspace(n, "ws_backward")
    bufs.call(lib.opp_linear_attention_train_backward(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), _ptr(qm), _ptr(km), kv.data_ptr(), ks.data_ptr(),
                                                      go.data_ptr(), B, L, S, H, D, gq.data_ptr(), gk.data_ptr(), gv.data_ptr(), ws2.data_ptr(),
                                                      bufs.ws_bytes(ws2), _s()), "opp_linear_attention_train_backward")
    torch.cuda.synchronize()
    return out, kv, ks, gq, gk, gv


def full_attention_train(q, k, v, grad_out, precision, bufs=None):
    """opp_full_attention_train_forward, then _backward.  q [B,L,H,D], k, v [B,S,H,D]; precision 0 fp32, 3 bf16x3
    -> (out, lse [B,H,L], grad_q, grad_k, grad_v)"""
    lib = _lib.load()
    bufs = bufs or DEFAULT_BUFFERS
    B, L, H, D = q.shape
    S = k.shape[1]
    qd, kd, vd, go = bufs.input(q, "q"), bufs.input(k, "k"), bufs.input(v, "v"), bufs.input(grad_out, "grad_out")
    out, lse = bufs.output((B, L, H, D), name="out"), bufs.output((B, H, L), name="lse")
    gq, gk, gv = bufs.output((B, L, H, D), name="grad_q"), bufs.output((B, S, H, D), name="grad_k"), bufs.output((B, S, H, D), name="grad_v")
    ws = bufs.workspace(lib.opp_full_attention_train_workspace_bytes(B, L, S, H, D))
    bufs.call(lib.opp_full_attention_train_forward(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), B, L, S, H, D, precision, out.data_ptr(),
                                                   lse.data_ptr(), ws.data_ptr(), ws.numel(), _s()), "opp_full_attention_train_forward")
    bufs.call(lib.opp_full_attention_train_backward(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), lse.data_ptr(), go.data_ptr(), B, L,
                                                    S, H, D, precision, gq.data_ptr(), gk.data_ptr(), gv.data_ptr(), ws.data_ptr(),
                                                    bufs.ws_bytes(ws), _s()), "opp_full_attention_train_backward")
    torch.cuda.synchronize()
    return out, lse, gq, gk, gv


def _match_outputs(bufs, N, L):
    return (bufs.output((1, N, L), name="conf"), bufs.output(N, torch.int64, None, "i_ids"), bufs.output(N, torch.int64, None, "j_ids"),
            bufs.output(N, fill=None, name="mconf"), bufs.output((N, 2), fill=None, name="mkpts_c"), bufs.output((N, 3), fill=None, name="mkpts_3d"),
            bufs.output(1, torch.int32, 0, "count"))


def forward_coarse(model, img, pe_tokens, kpts, bank_c, base_scale=8.0, bufs=None):
    """opp_forward_coarse: img [1,1,H,W], pe_tokens [L,256], kpts [1,N,3], bank_c [1,256,N] (cpu)
    -> dict: feat_f NCHW, conf_matrix, and the first `count` entries of the match lists"""
    lib, ctx = ctx_of(model)
    bufs = bufs or DEFAULT_BUFFERS
    H, W = img.shape[2:]
    N, L = kpts.shape[1], (H // 8) * (W // 8)
    x, pe, k, b = bufs.input(img, "image"), bufs.input(pe_tokens, "pe"), bufs.input(kpts, "kpts"), bufs.input(bank_c, "bank_c")
    ff = bufs.output((H // 2, W // 2, 128), name="feat_f")
    conf, i_ids, j_ids, mconf, mkc, mk3, cnt = _match_outputs(bufs, N, L)
    ws = bufs.workspace(lib.opp_forward_coarse_workspace_bytes(ctx, H, W, N))
    bufs.call(lib.opp_forward_coarse(ctx, x.data_ptr(), H, W, pe.data_ptr(), k.data_ptr(), b.data_ptr(), None, N, base_scale, None, ff.data_ptr(),
                                     conf.data_ptr(), i_ids.data_ptr(), j_ids.data_ptr(), mconf.data_ptr(), mkc.data_ptr(), mk3.data_ptr(),
                                     cnt.data_ptr(), ws.data_ptr(), bufs.ws_bytes(ws), _s()), "forward_coarse")
    torch.cuda.synchronize()
    M = int(cnt.item())
    return {"feat_f": from_nhwc(ff, 128), "conf_matrix": conf.cpu(), "i_ids": i_ids[:M].cpu(), "j_ids": j_ids[:M].cpu(), "mconf": mconf[:M].cpu(),
            "mkpts_query_c": mkc[:M].cpu(), "mkpts_3d_db": mk3[:M].cpu()}


def backbone_fine_branch(model, x1, x2_out, H, W, bufs=None):
    """opp_backbone_fine_branch: x1 [H/2,W/2,128], x2_out [H/4,W/4,224] NHWC (pad channels zero) -> feat_f [H/2,W/2,128] NHWC (cpu)"""
    lib, ctx = ctx_of(model)
    bufs = bufs or DEFAULT_BUFFERS
    a, b = bufs.input(x1, "x1"), bufs.input(x2_out, "x2_out")
    ff = bufs.output((H // 2, W // 2, 128), name="feat_f")
    ws = bufs.workspace(lib.opp_backbone_fine_branch_workspace_bytes(ctx, H, W))
    bufs.call(lib.opp_backbone_fine_branch(ctx, a.data_ptr(), b.data_ptr(), H, W, ff.data_ptr(), ws.data_ptr(), bufs.ws_bytes(ws), _s()),
              "backbone_fine_branch")
    torch.cuda.synchronize()
    return ff.cpu()


def object_prefix(model, tokens3d, bufs=None):
    """opp_object_prefix of point tokens [N,256] -> the prefix blob as floats (cpu), or None when this configuration has none"""
    lib, ctx = ctx_of(model)
    bufs = bufs or DEFAULT_BUFFERS
    N = tokens3d.shape[0]
    nb = lib.opp_object_prefix_bytes(ctx, N)
    if nb == 0:
        return None
    t = bufs.input(tokens3d, "tokens3d")
    blob = bufs.output(nb // 4, name="prefix")
    ws = bufs.workspace(lib.opp_object_prefix_workspace_bytes(ctx, N))
    bufs.call(lib.opp_object_prefix(ctx, t.data_ptr(), N, blob.data_ptr(), nb, ws.data_ptr(), bufs.ws_bytes(ws), _s()), "object_prefix")
    torch.cuda.synchronize()
    return blob.cpu()


def backbone_train(model, imgs, bufs=None):
    """opp_backbone_train (train-mode BatchNorm, B images [B,1,H,W]) -> feat_c [B,H/8,W/8,256], feat_f [B,H/2,W/2,128], bn_stats (cpu)"""
    lib, ctx = ctx_of(model)
    model._ensure_train_packed(lib, ctx, torch.device("cuda", torch.cuda.current_device()))
    bufs = bufs or DEFAULT_BUFFERS
    B, _, H, W = imgs.shape
    x = bufs.input(imgs, "image")
    fc, ff = bufs.output((B, H // 8, W // 8, 256), name="feat_c"), bufs.output((B, H // 2, W // 2, 128), name="feat_f")
    st = bufs.output((lib.opp_num_bn_layers(ctx), 512), name="bn_stats")
    ws = bufs.workspace(lib.opp_backbone_train_workspace_bytes(ctx, B, H, W))
    bufs.call(lib.opp_backbone_train(ctx, x.data_ptr(), B, H, W, fc.data_ptr(), ff.data_ptr(), st.data_ptr(), ws.data_ptr(), bufs.ws_bytes(ws), _s()),
              "backbone_train")
    torch.cuda.synchronize()
    return fc.cpu(), ff.cpu(), st.cpu()


def fine_patches(model, x1, x2_out, H, W, bank_f, i_ids, j_ids, hw_c, mkpts_c, base_scale, run_transformer=1, spare_rows=0, bufs=None):
    """opp_fine_patches from x1 [H/2,W/2,128] and x2_out [H/4,W/4,224] (NHWC, pad channels zero) -> expec_f [M + spare_rows, 3],
    mkpts_query_f [M + spare_rows, 2], NaN-prefilled (cpu)"""
    lib, ctx = ctx_of(model)
    bufs = bufs or DEFAULT_BUFFERS
    M, N = i_ids.numel(), bank_f.shape[2]
    a, b, bk = bufs.input(x1, "x1"), bufs.input(x2_out, "x2_out"), bufs.input(bank_f, "bank_f")
    ii, jj = bufs.input(i_ids.long(), "i_ids"), bufs.input(j_ids.long(), "j_ids")
    mk = bufs.input(mkpts_c.float().reshape(M, 2), "mkpts_c")
    ex, mf = bufs.output((M + spare_rows, 3), name="expec_f"), bufs.output((M + spare_rows, 2), name="mkpts_f")
    ws = bufs.workspace(lib.opp_fine_patches_workspace_bytes(ctx, M))
    bufs.call(lib.opp_fine_patches(ctx, a.data_ptr(), b.data_ptr(), H, W, bk.data_ptr(), N, ii.data_ptr(), jj.data_ptr(), M, hw_c[0], hw_c[1],
                                   mk.data_ptr(), base_scale, None, run_transformer, ex.data_ptr(), mf.data_ptr(), ws.data_ptr(),
                                   bufs.ws_bytes(ws), _s()), "fine_patches")
    torch.cuda.synchronize()
    return ex.cpu(), mf.cpu()


def backbone_tape_backward(model, imgs, grad_fc, grad_ff, short_forward=True, bufs=None):
    """opp_backbone_train_tape, then opp_backbone_backward on its tape.  imgs [B,1,H,W], grad_fc [B,H/8,W/8,256], grad_ff [B,H/2,W/2,128]
    -> dict: feat_c, feat_f, bn_stats and "grad:<parameter>" for every backbone parameter (cpu).  The tape is a NaN-prefilled output of the
    forward and all the backward gets of it.  short_forward = False: only the backward is told `bufs.ws_bytes` (a refusal test of it)."""
    lib, ctx = ctx_of(model)
    model._ensure_train_packed(lib, ctx, torch.device("cuda", torch.cuda.current_device()))
    bufs = bufs or DEFAULT_BUFFERS
    B, _, H, W = imgs.shape
    x, gc, gf = bufs.input(imgs, "image"), bufs.input(grad_fc, "grad_feat_c"), bufs.input(grad_ff, "grad_feat_f")
    fc, ff = bufs.output((B, H // 8, W // 8, 256), name="feat_c"), bufs.output((B, H // 2, W // 2, 128), name="feat_f")
    st = bufs.output((lib.opp_num_bn_layers(ctx), 512), name="bn_stats")
    nt = lib.opp_backbone_tape_bytes(ctx, B, H, W)
    tape = bufs.output(nt // 4, name="tape")
    ws = bufs.workspace(lib.opp_backbone_train_tape_workspace_bytes(ctx, B, H, W), "ws_forward")
    bufs.call(lib.opp_backbone_train_tape(ctx, x.data_ptr(), B, H, W, fc.data_ptr(), ff.data_ptr(), st.data_ptr(), tape.data_ptr(), nt, ws.data_ptr(),
                                          bufs.ws_bytes(ws) if short_forward else ws.numel(), _s()), "opp_backbone_train_tape")
    ptrs, n = model._rt["ptrs"]
    gp = (ctypes.c_void_p * n)()
    grads = {}
    for i, name in enumerate(model._rt["names"]):
        if name.startswith("backbone.") and not name.endswith(("running_mean", "running_var")):
            grads[name] = bufs.output(tuple(model._rt["keep"][i].shape), name="grad:" + name)
            gp[i] = grads[name].data_ptr()
    ws2 = bufs.workspace(lib.opp_backbone_backward_workspace_bytes(ctx, B, H, W), "ws_backward")
    bufs.call(lib.opp_backbone_backward(ctx, x.data_ptr(), B, H, W, tape.data_ptr(), nt, ptrs, n, gc.data_ptr(), gf.data_ptr(), gp, ws2.data_ptr(),
                                        bufs.ws_bytes(ws2), _s()), "opp_backbone_backward")
    torch.cuda.synchronize()
    out = {"feat_c": fc.cpu(), "feat_f": ff.cpu(), "bn_stats": st.cpu()}
    out.update({"grad:" + k: v.cpu() for k, v in grads.items()})
    return out


# ---- entries without a workspace of their own: the provider still guards their outputs and inputs ----------------------------------
def full_attention(qkv, n_seg, len0, len1, C, nhead, cross, precision, bufs=None):
    """opp_full_attention of qkv [n_seg*(len0+len1), 3C] (plain Q | K | V) -> message [same rows, C] (cpu).  precision 0 fp32, 3 bf16x3.
    The call takes (ws, ws_bytes) and needs none: it gets the (empty) workspace its size query reports."""
    lib = _lib.load()
    bufs = bufs or DEFAULT_BUFFERS
    q = bufs.input(qkv, "qkv")
    msg = bufs.output((q.shape[0], C), name="msg")
    ws = bufs.workspace(lib.opp_full_attention_workspace_bytes(n_seg, len0, len1, C, nhead))
    bufs.call(lib.opp_full_attention(q.data_ptr(), n_seg, len0, len1, C, nhead, cross, precision, msg.data_ptr(), _ptr(ws) if ws.numel() else None,
                                     bufs.ws_bytes(ws), _s()), "opp_full_attention")
    torch.cuda.synchronize()
    return msg.cpu()


def fine_head_train(f3, win, grad_expec, bufs=None):
    """opp_fine_head_train_forward, then _backward.  f3 [M,C], win [M,W*W,C], grad_expec [M,3]
    -> (expec_f [M,3], scratch_xy [4M], grad_f3 [M,C], grad_win [M,W*W,C]) (cpu)"""
    lib = _lib.load()
    bufs = bufs or DEFAULT_BUFFERS
    M, WW, C = win.shape
    W = int(round(WW ** 0.5))
    a, b, g = bufs.input(f3, "f3"), bufs.input(win, "win"), bufs.input(grad_expec, "grad_expec_f")
    ex, xy = bufs.output((M, 3), name="expec_f"), bufs.output(4 * M, name="scratch_xy")
    g3, gw = bufs.output((M, C), name="grad_f3"), bufs.output((M, WW, C), name="grad_win")
    bufs.call(lib.opp_fine_head_train_forward(a.data_ptr(), b.data_ptr(), M, W, C, ex.data_ptr(), xy.data_ptr(), _s()), "opp_fine_head_train_forward")
    bufs.call(lib.opp_fine_head_train_backward(a.data_ptr(), b.data_ptr(), M, W, C, g.data_ptr(), g3.data_ptr(), gw.data_ptr(), _s()),
              "opp_fine_head_train_backward")
    torch.cuda.synchronize()
    return ex.cpu(), xy.cpu(), g3.cpu(), gw.cpu()


def fine_window_gather(feat_f, b_ids, j_ids, hc, wc, window, grad_windows, bufs=None):
    """opp_fine_window_gather of feat_f [B,Hf,Wf,C] (NHWC), then opp_fine_window_gather_backward of grad_windows [M,W*W,C]
    -> (windows [M,W*W,C], grad_feat_f [B,Hf,Wf,C]) (cpu)"""
    lib = _lib.load()
    bufs = bufs or DEFAULT_BUFFERS
    B, Hf, Wf, C = feat_f.shape
    M = b_ids.numel()
    f, bi, ji, gwin = bufs.input(feat_f, "feat_f"), bufs.input(b_ids.long(), "b_ids"), bufs.input(j_ids.long(), "j_ids"), bufs.input(grad_windows, "grad_windows")
    win = bufs.output((M, window * window, C), name="windows")
    gf = bufs.output((B, Hf, Wf, C), name="grad_feat_f")
    bufs.call(lib.opp_fine_window_gather(f.data_ptr(), B, Hf, Wf, C, bi.data_ptr(), ji.data_ptr(), M, hc, wc, window, win.data_ptr(), _s()),
              "opp_fine_window_gather")
    bufs.call(lib.opp_fine_window_gather_backward(gwin.data_ptr(), B, Hf, Wf, C, bi.data_ptr(), ji.data_ptr(), M, hc, wc, window, gf.data_ptr(), _s()),
              "opp_fine_window_gather_backward")
    torch.cuda.synchronize()
    return win.cpu(), gf.cpu()
