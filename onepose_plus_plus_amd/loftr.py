"""`LoFTRMatcher`: the 2D-2D matcher in front of the detector and of SfM, on libopp_hip.so.

The reference's `LoFTR_for_OnePose_Plus` (src/KeypointFreeSfM/loftr_for_sfm/loftr.py:16-128) strings together the LoFTR submodule's
backbone, sine table, coarse transformer, dual-softmax matcher, fine preprocess, fine transformer and expectation head.  Its two
consumers are SfM's `detector_free_coarse_matching` (`enable_fine_matching=False`, coarse_match_worker.py:19-24) and the demo's
first-frame detector (local_feature_2D_detector.py:25, :79-82).

The building blocks are the ones of the 2D-3D model and are pinned to the reference through it (same ResNetFPN_8_2, same sine table
-- `temp_bug_fix = False` is the formula of position_encoding.py:25-28 --, same LoFTREncoderLayer, linear attention, dual softmax and
expectation head).  The glue between them lives in the LoFTR submodule, whose directory is EMPTY in the reference checkout; four
pieces of it are therefore our reading of the published LoFTR and "parity unpinned" (tests/loftr_reference.py restates them in
float64 torch):

  * the layer schedule: one layer per name serves both images; a "cross" layer updates image 0's tokens from image 1's and then
    image 1's from the UPDATED tokens of image 0 (sequential -- unlike quirk q6 of the 2D-3D model), at both levels;
  * coarse matching: both streams / sqrt(C), temperature exactly as configured (no + 1e-4), `border_rm` cells cleared at both ends
    of both grids, mutual nearest neighbours above `thr`, the first j of a row, ascending i;
  * the fine windows: W x W cells of both 1/2-resolution maps at stride 4 with zero padding W // 2 around the matched cells;
  * the fine head: the centre token of window 0 against the W^2 tokens of window 1.

All tensor math runs in HIP kernels through the C ABI (`opp_backbone`, `opp_image_tokens`, `opp_transformer` under
`opp_config.cross_sequential`, `opp_match2d`, `opp_fine2d`); there is no CPU / PyTorch fallback.  Eval mode, batch 1, no masks.
"""
import copy
import ctypes
import warnings

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .model import GEMM_PRECISIONS, DEFAULT_GEMM_PRECISION, _Node, _init_tensor, _register, _sine_table
from .params import param_spec

__all__ = ["default_cfg", "LoFTRMatcher"]

# the values of the reference's loftr_for_onepose_plus_cfg.py:11-48, lower-cased as its lower_config() leaves them
default_cfg = {
    "backbone_type": "ResNetFPN",
    "resolution": (8, 2),
    "fine_window_size": 9,
    "fine_concat_coarse_feat": False,
    "resnetfpn": {"initial_dim": 128, "block_dims": [128, 196, 256]},
    "coarse": {"d_model": 256, "d_ffn": 256, "nhead": 8, "layer_names": ["self", "cross"] * 4, "attention": "linear",
               "temp_bug_fix": False},
    "match_coarse": {"thr": 0.2, "border_rm": 2, "match_type": "dual_softmax", "dsmax_temperature": 0.1, "skh_iters": 3,
                     "skh_init_bin_score": 1.0, "skh_prefilter": True, "train_coarse_percent": 0.4, "train_pad_num_gt_min": 200},
    "fine": {"d_model": 128, "d_ffn": 128, "nhead": 8, "layer_names": ["self", "cross"] * 1, "attention": "linear"},
}

POS_EMB_SHAPE = (256, 256)     # PositionEncodingSine's default max_shape


def check_config(cfg):
    """The configurations this matcher runs; everything else is refused here, before a device is touched."""
    if cfg["backbone_type"] != "ResNetFPN":
        raise ValueError("LoFTRMatcher: backbone_type %r is not supported (ResNetFPN)" % (cfg["backbone_type"],))
    if tuple(cfg["resolution"]) != (8, 2):
        raise NotImplementedError("LoFTRMatcher: resolution %r is not supported, only (8, 2)" % (tuple(cfg["resolution"]),))
    if cfg["fine_concat_coarse_feat"]:
        raise NotImplementedError("LoFTRMatcher: fine_concat_coarse_feat=True is not supported")
    if cfg["coarse"]["temp_bug_fix"]:
        raise NotImplementedError("LoFTRMatcher: temp_bug_fix=True (the corrected sine table) is not supported")
    if cfg["match_coarse"]["match_type"] != "dual_softmax":
        raise NotImplementedError("LoFTRMatcher: match_type %r is not supported, only dual_softmax" % (cfg["match_coarse"]["match_type"],))
    for level in ("coarse", "fine"):
        if cfg[level]["attention"] != "linear":
            raise NotImplementedError("LoFTRMatcher: %s attention %r is not supported, only linear" % (level, cfg[level]["attention"]))
        for n in cfg[level]["layer_names"]:
            if n not in ("self", "cross"):
                raise KeyError(n)
    w = cfg["fine_window_size"]
    if int(w) != w or w % 2 == 0 or not 3 <= w <= 9:
        raise ValueError("LoFTRMatcher: fine_window_size must be an odd integer in [3, 9], got %r" % (w,))
    if int(cfg["match_coarse"]["border_rm"]) < 0:
        raise ValueError("LoFTRMatcher: border_rm must not be negative")


def model_config(cfg):
    """The LoFTR config in the shape `params.param_spec` reads: no keypoint encoder, layernorm, no rezero."""
    def level(t):
        return {"d_model": t["d_model"], "nhead": t["nhead"], "layer_names": list(t["layer_names"]), "layer_iter_n": 1, "rezero": None,
                "norm_method": "layernorm"}
    return {"loftr_backbone": {"resnetfpn": {"initial_dim": cfg["resnetfpn"]["initial_dim"], "block_dims": list(cfg["resnetfpn"]["block_dims"])}},
            "keypoints_encoding": {"enable": False}, "loftr_coarse": level(cfg["coarse"]), "loftr_fine": level(cfg["fine"])}


class LoFTRMatcher(nn.Module):
    """`LoFTR_for_OnePose_Plus(config, enable_fine_matching)`.  State-dict keys: `backbone.*`, `loftr_coarse.layers.<i>.*`,
    `loftr_fine.layers.<i>.*` (names and shapes of params.py; `pos_encoding.pe` is a non-persistent buffer), so a checkpoint with its
    `matcher.` prefix stripped loads with strict=True whatever `enable_fine_matching` is (coarse_match_worker.py:21-24)."""

    def __init__(self, config=default_cfg, enable_fine_matching=True):
        super().__init__()
        check_config(config)
        self.config = copy.deepcopy(config)
        self.enable_fine_matching = bool(enable_fine_matching)
        mcfg = model_config(self.config)
        for key, shape, kind in param_spec(mcfg):
            _register(self, key, _init_tensor(shape, kind, mcfg, key), buffer=kind in ("bn_mean", "bn_var", "bn_count"))
        self.pos_encoding = _Node()
        self.pos_encoding.register_buffer("pe", _sine_table(self.config["coarse"]["d_model"], POS_EMB_SHAPE), persistent=False)
        self.gemm_precision = DEFAULT_GEMM_PRECISION
        self._reset_runtime()

    # ---- runtime state (the C context, the packed weights, cached tables) ---------------------------------------------------
    def _reset_runtime(self):
        self.__dict__["_rt"] = {"ctx": None, "packed": None, "dirty": True, "pe": {}, "ws": None, "names": None}

    def __getstate__(self):
        st = self.__dict__.copy()
        st.pop("_rt", None)
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)
        self._reset_runtime()

    def _drop_ctx(self):
        rt = self.__dict__.get("_rt")
        if rt and rt.get("ctx"):
            try:
                _lib.load().opp_destroy(rt["ctx"])
            except Exception:
                pass
            rt["ctx"] = None

    def __del__(self):
        self._drop_ctx()

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        if "_rt" in self.__dict__:
            self._rt.update(dirty=True, pe={}, ws=None)
        return out

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        self._rt["dirty"] = True
        return out

    def repack(self):
        """Call after modifying parameters in place (the packed weights are cached)."""
        self._rt["dirty"] = True

    def set_gemm_precision(self, name):
        """ "bf16x3" (default: operands carried exactly as three bf16, not narrower than fp32) or "fp32" (exact fp32 MFMA)."""
        if name not in GEMM_PRECISIONS:
            raise ValueError("gemm_precision must be one of %s" % (sorted(GEMM_PRECISIONS),))
        if name != self.gemm_precision:
            self.gemm_precision = name
            self._drop_ctx()
            self._rt.update(dirty=True, packed=None)

    def _c_config(self):
        cfg = self.config
        c = _lib.OppConfig()
        c.initial_dim = int(cfg["resnetfpn"]["initial_dim"])
        for i in range(3):
            c.block_dims[i] = int(cfg["resnetfpn"]["block_dims"][i])
        c.pos_enc_enable = 1
        for name, pre in (("coarse", "coarse"), ("fine", "fine")):
            t = cfg[name]
            names = list(t["layer_names"])
            setattr(c, pre + "_d_model", int(t["d_model"]))
            setattr(c, pre + "_nhead", int(t["nhead"]))
            setattr(c, pre + "_n_layers", len(names))
            arr = getattr(c, pre + "_is_cross")
            for i, n in enumerate(names):
                arr[i] = 1 if n == "cross" else 0
        c.fine_window = int(cfg["fine_window_size"])
        c.match_thr = float(cfg["match_coarse"]["thr"])
        c.match_border_rm = int(cfg["match_coarse"]["border_rm"])
        c.match_temperature = float(cfg["match_coarse"]["dsmax_temperature"])
        c.gemm_precision = GEMM_PRECISIONS[self.gemm_precision]
        c.encoder_fusion = 0           # the sequential schedule runs one launch per Linear ("2D-2D matching")
        c.cross_sequential = 1
        return c

    def _ensure_ready(self, device):
        lib = _lib.load()
        rt = self._rt
        if rt["ctx"] is None:
            ctx = ctypes.c_void_p()
            ccfg = self._c_config()
            _lib.check(lib.opp_create(ctypes.byref(ccfg), ctypes.byref(ctx)), "opp_create")
            rt["ctx"] = ctx
            rt["names"] = [lib.opp_weight_name(ctx, i).decode() for i in range(lib.opp_num_weights(ctx))]
        if rt["dirty"] or rt["packed"] is None or rt["packed"].device != device:
            sd = dict(self.named_parameters())
            sd.update(dict(self.named_buffers()))
            n = len(rt["names"])
            ptrs = (ctypes.c_void_p * n)()
            keep = []
            for i, name in enumerate(rt["names"]):
                t = sd[name].detach()
                if t.device != device:
                    raise RuntimeError("parameter %s is on %s, input on %s" % (name, t.device, device))
                if t.dtype != torch.float32 or not t.is_contiguous():
                    t = t.float().contiguous()
                if t.numel() != lib.opp_weight_numel(rt["ctx"], i):
                    raise RuntimeError("parameter %s has %d elements, expected %d" % (name, t.numel(), lib.opp_weight_numel(rt["ctx"], i)))
                keep.append(t)
                ptrs[i] = t.data_ptr()
            nbytes = lib.opp_packed_weights_bytes(rt["ctx"])
            blob = torch.empty(nbytes, dtype=torch.uint8, device=device)
            stream = torch.cuda.current_stream(device).cuda_stream
            _lib.check(lib.opp_pack_weights(rt["ctx"], ptrs, n, blob.data_ptr(), nbytes, stream), "opp_pack_weights")
            rt.update(packed=blob, dirty=False, keep=keep)
        return lib, rt["ctx"]

    def _pe_tokens(self, hc, wc, device):
        key = (hc, wc)
        if key not in self._rt["pe"]:
            pe = self.pos_encoding.pe
            if hc > pe.shape[2] or wc > pe.shape[3]:
                raise RuntimeError("feature map %dx%d exceeds the sine table %s" % (hc, wc, POS_EMB_SHAPE))
            self._rt["pe"][key] = pe[0, :, :hc, :wc].permute(1, 2, 0).reshape(hc * wc, -1).contiguous().to(device)
        return self._rt["pe"][key]

    def _workspace(self, nbytes, device):
        ws = self._rt["ws"]
        if ws is None or ws.numel() < nbytes or ws.device != device:
            ws = torch.empty(max(int(nbytes), 4096), dtype=torch.uint8, device=device)
            self._rt["ws"] = ws
        return ws

    # ---- forward -------------------------------------------------------------------------------------------------------------
    def _refuse(self, data, kwargs):
        """Every unsupported call, named, before anything is launched (and before a device is needed)."""
        if self.training:
            raise NotImplementedError("LoFTRMatcher: train()-mode forward is not supported (eval only)")
        for k in kwargs:
            if k in ("extract_coarse_feature", "extract_fine_feature"):
                raise NotImplementedError("LoFTRMatcher: %s (descriptor extraction at the matches) is not supported" % k)
            raise TypeError("LoFTRMatcher.forward got an unexpected keyword %r" % k)
        if "mask0" in data or "mask1" in data:
            raise NotImplementedError("LoFTRMatcher: mask0 / mask1 (padding masks) are not supported")
        if "mkpts0_c" in data:
            raise NotImplementedError("LoFTRMatcher: the fine level on given coarse matches ('mkpts0_c' in data) is not supported")
        for k in ("image0", "image1"):
            t = data[k]
            if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 1:
                raise ValueError("LoFTRMatcher: %s must be a [1, 1, H, W] tensor" % k)
            if t.shape[0] != 1:
                raise NotImplementedError("LoFTRMatcher: batch > 1 is not supported (%s has batch %d)" % (k, t.shape[0]))
            if t.shape[2] % 8 or t.shape[3] % 8 or t.shape[2] < 8 or t.shape[3] < 8:
                raise ValueError("LoFTRMatcher: %s size %dx%d is not a multiple of 8" % (k, t.shape[2], t.shape[3]))
        for k in ("scale0", "scale1"):
            if k in data and tuple(data[k].shape) != (1, 2):
                raise ValueError("LoFTRMatcher: %s must be [1, 2] = (h_scale, w_scale)" % k)

    @staticmethod
    def _f32(t, name, device):
        if not t.is_cuda:
            raise RuntimeError("%s must be a CUDA/ROCm tensor: the HIP path has no CPU fallback" % name)
        if t.device != device:
            raise RuntimeError("%s is on %s, expected %s" % (name, t.device, device))
        return t.float().contiguous()

    def forward(self, data, **kwargs):
        """`LoFTR_for_OnePose_Plus.forward` (loftr.py:34-128), in place on `data`; returns `data`."""
        self._refuse(data, kwargs)
        device = data["image0"].device
        if device.type != "cuda":
            raise RuntimeError("image0 must be a CUDA/ROCm tensor: the HIP path has no CPU fallback")
        cfg = self.config
        dC, dF, W = cfg["coarse"]["d_model"], cfg["fine"]["d_model"], int(cfg["fine_window_size"])
        with torch.cuda.device(device):
            lib, ctx = self._ensure_ready(device)
            stream = torch.cuda.current_stream(device).cuda_stream
            imgs = [self._f32(data[k], k, device) for k in ("image0", "image1")]
            scales = [self._f32(data[k], k, device) if k in data else None for k in ("scale0", "scale1")]
            hw_i = [tuple(int(v) for v in im.shape[2:]) for im in imgs]
            hw_c = [(h // 8, w // 8) for h, w in hw_i]
            hw_f = [(h // 2, w // 2) for h, w in hw_i]
            L = [h * w for h, w in hw_c]
            data.update({"bs": 1, "hw0_i": imgs[0].shape[2:], "hw1_i": imgs[1].shape[2:],
                         "hw0_c": torch.Size(hw_c[0]), "hw1_c": torch.Size(hw_c[1]), "hw0_f": torch.Size(hw_f[0]), "hw1_f": torch.Size(hw_f[1])})

            def ptr(t):
                return t.data_ptr() if t is not None else None

            # 1. backbone per image (eval: the reference's concatenation of equal-sized images gives the same values), tokens = feat_c + pe
            tokens = torch.empty((L[0] + L[1], dC), dtype=torch.float32, device=device)
            feat_c = torch.empty((max(L), dC), dtype=torch.float32, device=device)
            feat_f = [torch.empty((h * w, dF), dtype=torch.float32, device=device) for h, w in hw_f]
            for k in range(2):
                H, Wd = hw_i[k]
                ws = self._workspace(lib.opp_backbone_workspace_bytes(ctx, H, Wd), device)
                _lib.check(lib.opp_backbone(ctx, imgs[k].data_ptr(), H, Wd, feat_c.data_ptr(), feat_f[k].data_ptr(), ws.data_ptr(), ws.numel(), stream),
                           "opp_backbone")
                pe = self._pe_tokens(hw_c[k][0], hw_c[k][1], device)
                _lib.check(lib.opp_image_tokens(ctx, feat_c.data_ptr(), pe.data_ptr(), L[k], tokens[k * L[0]:].data_ptr(), stream), "opp_image_tokens")
            # 2. coarse transformer, sequential cross layers
            ws = self._workspace(lib.opp_transformer_workspace_bytes(ctx, 0, 1, L[0], L[1]), device)
            _lib.check(lib.opp_transformer(ctx, 0, tokens.data_ptr(), 1, L[0], L[1], ws.data_ptr(), ws.numel(), stream), "opp_transformer")
            # 3. coarse matching
            conf = torch.empty((1, L[0], L[1]), dtype=torch.float32, device=device)
            i_ids = torch.empty(L[0], dtype=torch.int64, device=device)
            j_ids = torch.empty(L[0], dtype=torch.int64, device=device)
            mconf = torch.empty(L[0], dtype=torch.float32, device=device)
            mk0 = torch.empty((L[0], 2), dtype=torch.float32, device=device)
            mk1 = torch.empty((L[0], 2), dtype=torch.float32, device=device)
            count = torch.zeros(1, dtype=torch.int32, device=device)
            ws = self._workspace(lib.opp_match2d_workspace_bytes(ctx, L[0], L[1]), device)
            _lib.check(lib.opp_match2d(ctx, tokens.data_ptr(), tokens[L[0]:].data_ptr(), hw_c[0][0], hw_c[0][1], hw_c[1][0], hw_c[1][1],
                                       float(hw_i[0][0]) / float(hw_c[0][0]), ptr(scales[0]), ptr(scales[1]), conf.data_ptr(), i_ids.data_ptr(),
                                       j_ids.data_ptr(), mconf.data_ptr(), mk0.data_ptr(), mk1.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(),
                                       stream), "opp_match2d")
            M = int(count.item())                                        # the one device-to-host synchronisation
            b_ids = torch.zeros(M, dtype=torch.int64, device=device)
            data.update({"conf_matrix": conf, "b_ids": b_ids, "i_ids": i_ids[:M], "j_ids": j_ids[:M], "m_bids": b_ids,
                         "gt_mask": torch.zeros(M, dtype=torch.bool, device=device), "mkpts0_c": mk0[:M], "mkpts1_c": mk1[:M], "mconf": mconf[:M]})
            self._rt["last"] = (imgs, scales, tokens, feat_c, feat_f)     # what the stream was handed stays alive until the next call
            if not self.enable_fine_matching:                            # loftr.py:125-128
                data.update({"mkpts0_f": data["mkpts0_c"], "mkpts1_f": data["mkpts1_c"]})
                return data
            # 4. / 5. fine level
            data["W"] = W
            if M == 0:
                warnings.warn("No matches found in coarse-level.")
                data.update({"expec_f": torch.empty(0, 3, device=device), "mkpts0_f": data["mkpts0_c"], "mkpts1_f": data["mkpts1_c"]})
                return data
            expec = torch.empty((M, 3), dtype=torch.float32, device=device)
            mk1_f = torch.empty((M, 2), dtype=torch.float32, device=device)
            ws = self._workspace(lib.opp_fine2d_workspace_bytes(ctx, M), device)
            _lib.check(lib.opp_fine2d(ctx, feat_f[0].data_ptr(), hw_f[0][0], hw_f[0][1], feat_f[1].data_ptr(), hw_f[1][0], hw_f[1][1], i_ids.data_ptr(),
                                      j_ids.data_ptr(), M, hw_c[0][1], hw_c[1][1], hw_f[0][0] // hw_c[0][0], mk1.data_ptr(),
                                      float(hw_i[0][0]) / float(hw_f[0][0]), ptr(scales[1]), expec.data_ptr(), mk1_f.data_ptr(), ws.data_ptr(),
                                      ws.numel(), stream), "opp_fine2d")
            data.update({"expec_f": expec, "mkpts0_f": data["mkpts0_c"], "mkpts1_f": mk1_f})
            return data

    # ---- convenience -----------------------------------------------------------------------------------------------------------
    def match(self, image0, image1, **scales):
        """(image0, image1 [1,1,H,W] device tensors; scale0= / scale1= optional) -> (mkpts0_f, mkpts1_f, mconf), device tensors."""
        for k in scales:
            if k not in ("scale0", "scale1"):
                raise TypeError("LoFTRMatcher.match got an unexpected keyword %r" % k)
        data = {"image0": image0, "image1": image1}
        data.update(scales)
        self.forward(data)
        return data["mkpts0_f"], data["mkpts1_f"], data["mconf"]

    def as_detector_matcher(self, device=None):
        """The callable `AffineBoxDetector(matcher, ref_images)` expects: (ref view, frame) -> (mkpts0 [k,2], mkpts1 [k,2]) in the pixels of
        the views as given.  A view is a [h, w] uint8 image (numpy, CPU or device tensor: uploaded and divided by 255 on the device by
        the ingest kernel) or a float image in [0, 1].  A side that is no multiple of 8 is resized down to one, as the reference's
        `read_grayscale(df=8)` does, and the scale goes into scale0 / scale1."""
        from .ingest import read_grayscale_u8

        def to_image(view):
            if isinstance(view, np.ndarray):
                view = torch.from_numpy(np.ascontiguousarray(view))
            view = view.reshape(view.shape[-2], view.shape[-1])
            dev = torch.device(device) if device is not None else (view.device if view.is_cuda else torch.device("cuda", torch.cuda.current_device()))
            h, w = int(view.shape[0]), int(view.shape[1])
            if view.dtype == torch.uint8:
                img, scale = read_grayscale_u8(view.contiguous(), resize=[-1], df=8, ret_scales=True, device=dev)
                return img[None], scale[None].to(dev)
            if h % 8 or w % 8:
                raise ValueError("LoFTRMatcher: a float view must have sides that are multiples of 8, got %dx%d" % (h, w))
            return view.to(dev, torch.float32)[None, None].contiguous(), None

        def matcher(ref, frame):
            data = {}
            for k, view in (("0", ref), ("1", frame)):
                img, scale = to_image(view)
                data["image" + k] = img
                if scale is not None:
                    data["scale" + k] = scale
            with torch.no_grad():
                self.forward(data)
            return data["mkpts0_f"], data["mkpts1_f"]

        return matcher
