"""Full attention (`attention` != "linear" in loftr_coarse / loftr_fine, transformer.py:32-40): configuration, C ABI layout, the
fp64 restatement against the reference's fixtures and the static code-generation checks of csrc/full_attention.hip.  No GPU."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from onepose_plus_plus_amd import OnePosePlus_model, _lib
from onepose_plus_plus_amd.config import default_config
from tests import helpers as H
from tests import full_attention_oracle as FO
from tests.golden.fullattn_cases import FULLATTN_TRANSFORMER_CASES, fullattn_transformer_setup, full_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAS_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")


@pytest.mark.parametrize("coarse,fine", [(True, False), (False, True), (True, True)])
def test_model_builds_with_full_attention_and_keeps_the_state_dict(coarse, fine):
    lin = OnePosePlus_model(default_config())
    m = OnePosePlus_model(full_config(default_config(), coarse, fine))
    assert list(m.state_dict()) == list(lin.state_dict())
    m.load_state_dict(lin.state_dict(), strict=True)     # FullAttention has no parameters: a linear checkpoint loads strictly


def test_any_non_linear_value_selects_full_attention_and_kernel_fn_is_not_checked():
    cfg = default_config()
    cfg["loftr_coarse"]["attention"] = "softmax"
    cfg["loftr_fine"]["attention"] = "full"
    cfg["loftr_coarse"]["kernel_fn"] = "foo"              # build_feature_map is never reached by FullAttention
    cfg["loftr_fine"]["kernel_fn"] = "foo"
    m = OnePosePlus_model(cfg)
    c = m._c_config()
    assert (c.coarse_attention, c.fine_attention) == (1, 1)
    lin = default_config()
    lin["loftr_coarse"]["kernel_fn"] = "foo"
    with pytest.raises(ValueError):
        OnePosePlus_model(lin)
    bad = full_config(default_config())
    bad["loftr_coarse"]["redraw_interval"] = 3             # the LocalFeatureTransformer assertion holds for both attentions
    with pytest.raises(AssertionError):
        OnePosePlus_model(bad)


@pytest.mark.parametrize("coarse,fine", [(False, False), (True, False), (False, True), (True, True)])
def test_c_config_sets_the_attention_fields(coarse, fine):
    c = OnePosePlus_model(full_config(default_config(), coarse, fine))._c_config()
    assert (c.coarse_attention, c.fine_attention) == (int(coarse), int(fine))


@pytest.mark.skipif(shutil.which("cc") is None and shutil.which("gcc") is None, reason="needs a host C compiler")
def test_opp_config_layout_matches_the_header():
    cc = shutil.which("cc") or shutil.which("gcc")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "opp_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(opp_config), '
           'offsetof(opp_config, coarse_attention), offsetof(opp_config, fine_attention)); return 0; }\n')
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "t.c"), "w") as f:
            f.write(src)
        exe = os.path.join(tmp, "t")
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "t.c"), "-o", exe])
        size, off_c, off_f = map(int, subprocess.check_output([exe]).split())
    assert size == ctypes.sizeof(_lib.OppConfig)
    assert off_c == _lib.OppConfig.coarse_attention.offset and off_f == _lib.OppConfig.fine_attention.offset
    assert off_c == _lib.OppConfig.fpn_overlap.offset + 4 and off_f == off_c + 4     # appended: a zeroed config stays linear


@pytest.mark.parametrize("name", list(FULLATTN_TRANSFORMER_CASES))
def test_fp64_restatement_reproduces_the_reference_fixtures(name):
    """pins tests/full_attention_oracle.py to the reference: within 1e-5 relative on random weights; the peaked case gets 2e-5 (the
    reference's own fp32 result is measured 1.5e-5 away from fp64 there: the sharp softmax amplifies the fp32 rounding of the logits)"""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    cfg, sd, tokens2d, bank = fullattn_transformer_setup(name)
    with torch.no_grad():
        f3, f2 = FO.local_feature_transformer(sd, "loftr_coarse", cfg["loftr_coarse"], bank.double(), tokens2d.double())
    rel = 1e-5 if FULLATTN_TRANSFORMER_CASES[name][3] == 1.0 else 2e-5
    H.assert_transformer_digest(H.transformer_digest(f3[0], f2[0]), H.load_golden(name), rel=rel, where=name)


def test_fp64_full_attention_of_one_token_is_v():
    q, k, v = torch.randn(1, 5, 8, 16, dtype=torch.float64), torch.randn(1, 1, 8, 16, dtype=torch.float64), torch.randn(1, 1, 8, 16, dtype=torch.float64)
    assert torch.equal(FO.full_attention(q, k, v), v.expand(1, 5, 8, 16))


@pytest.mark.skipif(not HAS_HIPCC, reason="needs hipcc")
def test_full_attention_kernels_have_no_scratch_and_no_waterfall():
    from tools import isa_audit
    with tempfile.TemporaryDirectory() as tmp:
        src, rows, err = isa_audit.audit_source("full_attention.hip", False, tmp)
    assert rows is not None, err
    names = [r[0] for r in rows]
    assert any("full_attn_flash_kernel" in k for k in names) and any("full_attn_small_kernel" in k for k in names)
    for k, vg, ag, sc, water, mfma, pk in rows:
        assert sc == 0 and water == 0, (k, sc, water)
        if "full_attn_flash_kernel" in k:
            assert mfma > 0, k
            assert vg + ag <= 256, (k, vg, ag)
