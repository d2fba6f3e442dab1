"""Static guard on the bf16x3 convolution instances of gemm_mfma.hip (CPU: hipcc cross-compiles gfx950).  Every bf16x3 convolution kernel
(opp_gemm_kernel<..., CONV = true, ..., PREC = 2> and the pre-split opp_gemm_asp_kernel) runs its K loop on v_mfma_f32_16x16x32_bf16 only:
the tiles are bit-identical to each other only while they all share one MFMA shape and K grouping.  No scratch, no waterfall loops, and the
register budget of a two-waves-per-SIMD kernel."""
import os
import re
import shutil
import tempfile

import pytest

from tools import isa_audit

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


def _body(text, k):
    m = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(k), text, re.S | re.M)
    return m.group(0) if m else ""


def _is_b3_conv(k):
    # opp_gemm_kernel<BM, BN, WM, WN, CONV, ABL, DEPTH, PREC> / opp_gemm_asp_kernel<BM, BN, WM, WN, ABL, DEPTH, PREC>
    m = re.match(r"_ZN12_GLOBAL__N_115opp_gemm_kernelILi\d+ELi\d+ELi\d+ELi\d+ELb1ELi\d+ELi\d+ELi2EEEv", k)
    return m is not None or k.startswith("_ZN12_GLOBAL__N_119opp_gemm_asp_kernel")


@pytest.mark.parametrize("tuning", [False, True])
def test_bf16x3_convolutions_run_on_16x16x32_mfma(tuning):
    with tempfile.TemporaryDirectory() as tmp:
        src, rows, err = isa_audit.audit_source("gemm_mfma.hip", tuning, tmp)
        assert rows is not None, err
        text = open(os.path.join(tmp, src + ".s")).read()
    convs = [r for r in rows if _is_b3_conv(r[0])]
    assert len(convs) >= 10, [r[0] for r in rows]
    for k, vg, ag, sc, water, mfma, pk in convs:
        body = _body(text, k)
        n16 = len(re.findall(r"\bv_mfma_f32_16x16x32_bf16\b", body))
        assert n16 > 0 and n16 == mfma, (k, n16, mfma)
        assert "v_mfma_f32_32x32x16_bf16" not in body, k
        assert sc == 0 and water == 0, (k, sc, water)
        assert vg + ag <= 256, (k, vg, ag)
    # the dense bf16x3 GEMMs keep the 32 x 32 shape (the encoder chain and the im2col stem are bit-identical to them)
    dense = [r for r in rows if re.match(r"_ZN12_GLOBAL__N_115opp_gemm_kernelILi\d+ELi\d+ELi\d+ELi\d+ELb0ELi0ELi2ELi2EEEv", r[0])]
    assert dense and all("v_mfma_f32_16x16x32_bf16" not in _body(text, r[0]) for r in dense)
