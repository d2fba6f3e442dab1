"""The 2D-2D matcher without a device: its fixtures against the float64 restatement, the module's state-dict contract, its default
config against the reference's settings (tests/golden/loftr_default_cfg.json: the values of loftr_for_onepose_plus_cfg.py:11-48 as
data), and every refusal, raised before a device is needed."""
import json
import os

import numpy as np
import pytest
import torch

from onepose_plus_plus_amd.loftr import LoFTRMatcher, default_cfg, model_config
from onepose_plus_plus_amd.params import param_spec
from tests import helpers as H
from tests import loftr_reference as R
from tests.golden.loftr_cases import (LOFTR_PAIRS, VARIANTS, WINDOWS, content_state_dict, detector_case, loftr_cfg, loftr_pair,
                                      loftr_state_dict)


@pytest.fixture(scope="module")
def sd():
    return loftr_state_dict()


def test_default_cfg_has_the_reference_values():
    with open(os.path.join(H.GOLDEN, "loftr_default_cfg.json")) as f:
        ref = json.load(f)
    assert json.loads(json.dumps(default_cfg)) == ref


@pytest.mark.parametrize("name", list(LOFTR_PAIRS))
def test_fixture_is_the_float64_restatement(name, sd):
    """the stored results are what tests/loftr_reference.py computes today (to float64 rounding across thread counts), at the default
    window and every threshold; the float32 restatement selects the same sets and stays within TOL_CONF"""
    gold = H.load_golden(name)
    data = loftr_pair(name, "thr0005s")
    r64 = R.forward(sd, data, loftr_cfg(VARIANTS["thr0005s"][0], 9))
    assert np.abs(r64["conf_matrix"][0].numpy() - gold["conf_matrix"]).max() < 1e-7          # the fixture stores conf_matrix as float32
    for k in ("i_ids", "j_ids"):
        assert np.array_equal(r64[k].numpy(), gold["thr0005s/w9/" + k]), k
    assert len(gold["thr0005s/w9/i_ids"]) >= 6
    for k in ("mconf", "mkpts0_c", "mkpts1_c", "mkpts1_f", "expec_f"):
        assert np.abs(r64[k].numpy() - gold["thr0005s/w9/" + k]).max() < 1e-8, k
    r32 = R.forward(sd, data, loftr_cfg(VARIANTS["thr0005s"][0], 9), dtype=torch.float32)
    assert np.abs(r32["conf_matrix"][0].double().numpy() - gold["conf_matrix"]).max() < H.TOL_CONF
    for vname, (thr, _) in VARIANTS.items():
        i, j, _ = R.select(r32["conf_matrix"], r64["hw0_c"], r64["hw1_c"], thr, default_cfg["match_coarse"]["border_rm"])
        for W in WINDOWS:
            assert np.array_equal(i.numpy(), gold["%s/w%d/i_ids" % (vname, W)]) and np.array_equal(j.numpy(), gold["%s/w%d/j_ids" % (vname, W)])
    assert len(gold["thr09/w9/i_ids"]) == 0 and gold["thr09/w9/expec_f"].shape == (0, 3)


def test_content_weights_match_by_the_known_shift():
    """the detector case (tests/test_loftr_gpu.py): with `content_state_dict` most coarse matches of the float32 restatement are the
    known shift of the view inside the frame -- what the affine estimator behind the matcher needs"""
    view, frame, (dy, dx) = detector_case()
    data = {"image0": view[None, None].float() / 255, "image1": frame[None, None].float() / 255}
    r = R.forward(content_state_dict(), data, loftr_cfg(default_cfg["match_coarse"]["thr"], 9), enable_fine=False, dtype=torch.float32)
    d = r["mkpts1_c"] - r["mkpts0_c"]
    good = int(((d - torch.tensor([dx, dy])).abs().max(1)[0] < 0.5).sum())
    assert len(d) >= 60 and good >= 0.6 * len(d), (len(d), good)


def test_state_dict_keys_and_strict_load(sd):
    spec = param_spec(model_config(default_cfg))
    for fine in (True, False):
        m = LoFTRMatcher(enable_fine_matching=fine)
        keys = list(m.state_dict().keys())
        assert keys == [k for k, _, _ in spec]
        assert all(k.split(".")[0] in ("backbone", "loftr_coarse", "loftr_fine") for k in keys)
        assert sum(k.startswith("loftr_coarse.layers.") for k in keys) == 8 * 10 and sum(k.startswith("loftr_fine.layers.") for k in keys) == 2 * 10
        assert not any("kpt_3d_pos_encoding" in k or k.startswith("pos_encoding") for k in keys)
        assert tuple(m.pos_encoding.pe.shape) == (1, 256, 256, 256)
        for k, shape, _ in spec:
            assert tuple(m.state_dict()[k].shape) == tuple(shape), k
        # the checkpoint as SfM loads it (coarse_match_worker.py:21-24): `matcher.` stripped, strict, whatever enable_fine_matching is
        ckpt = {"matcher." + k: v for k, v in sd.items()}
        m.load_state_dict({k[len("matcher."):]: v for k, v in ckpt.items()}, strict=True)
        assert torch.equal(m.state_dict()["loftr_fine.layers.1.mlp.2.weight"], sd["loftr_fine.layers.1.mlp.2.weight"])
        with pytest.raises(RuntimeError):
            m.load_state_dict({k: v for k, v in sd.items() if "loftr_fine" not in k}, strict=True)


def _cfg(**kw):
    cfg = loftr_cfg(0.2, 9)
    for path, v in kw.items():
        d = cfg
        keys = path.split("__")
        for k in keys[:-1]:
            d = d[k]
        d[keys[-1]] = v
    return cfg


@pytest.mark.parametrize("kw,exc,word", [
    (dict(fine_concat_coarse_feat=True), NotImplementedError, "fine_concat_coarse_feat"),
    (dict(coarse__temp_bug_fix=True), NotImplementedError, "temp_bug_fix"),
    (dict(match_coarse__match_type="sinkhorn"), NotImplementedError, "match_type"),
    (dict(coarse__attention="full"), NotImplementedError, "attention"),
    (dict(fine__attention="full"), NotImplementedError, "attention"),
    (dict(resolution=(16, 4)), NotImplementedError, "resolution"),
    (dict(fine_window_size=8), ValueError, "fine_window_size"),
    (dict(fine_window_size=11), ValueError, "fine_window_size"),
    (dict(fine_window_size=1), ValueError, "fine_window_size"),
])
def test_config_refusals(kw, exc, word):
    with pytest.raises(exc, match=word):
        LoFTRMatcher(_cfg(**kw))


def test_forward_refusals_need_no_device():
    m = LoFTRMatcher().eval()
    img = torch.zeros(1, 1, 64, 64)

    def call(extra=None, **kwargs):
        d = {"image0": img, "image1": img}
        d.update(extra or {})
        return m(d, **kwargs)

    with pytest.raises(NotImplementedError, match="mask0"):
        call({"mask0": torch.ones(1, 8, 8), "mask1": torch.ones(1, 8, 8)})
    with pytest.raises(NotImplementedError, match="batch > 1"):
        call({"image1": torch.zeros(2, 1, 64, 64)})
    with pytest.raises(NotImplementedError, match="mkpts0_c"):
        call({"mkpts0_c": torch.zeros(3, 2), "mkpts1_c": torch.zeros(3, 2)})
    with pytest.raises(NotImplementedError, match="extract_coarse_feature"):
        call(extract_coarse_feature=True)
    with pytest.raises(NotImplementedError, match="extract_fine_feature"):
        call(extract_fine_feature=True)
    with pytest.raises(ValueError, match="multiple of 8"):
        call({"image0": torch.zeros(1, 1, 60, 64)})
    with pytest.raises(NotImplementedError, match="train"):
        LoFTRMatcher().train()({"image0": img, "image1": img})
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # everything above came first: a CPU tensor is the last refusal
        call()
