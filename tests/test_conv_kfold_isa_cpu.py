"""Static guard on opp_gemm_kfold_kernel (gemm_mfma.hip: the four K slices of a bf16x3 convolution summed inside one 128 x 128 workgroup;
CPU: hipcc cross-compiles gfx950), after the pattern of test_conv_n208_isa_cpu.py: the symbol exists, and its second accumulator set fits."""
import os
import re
import shutil
import tempfile

import pytest

from tools import isa_audit

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

SYMBOL = "_ZN12_GLOBAL__N_121opp_gemm_kfold_kernelE7OppGemm"


def test_kfold_kernel_is_built_without_scratch_on_16x16_mfmas():
    with tempfile.TemporaryDirectory() as tmp:
        src, rows, err = isa_audit.audit_source("gemm_mfma.hip", False, tmp)
        assert rows is not None, err
        text = open(os.path.join(tmp, src + ".s")).read()
    found = [r for r in rows if r[0] == SYMBOL]
    assert len(found) == 1, [r[0] for r in rows if "kfold" in r[0]]
    k, vg, ag, sc, water, mfma, pk = found[0]
    body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(k), text, re.S | re.M).group(0)
    assert sc == 0 and water == 0, (sc, water)
    assert vg + ag <= 256, (vg, ag)
    n16 = len(re.findall(r"\bv_mfma_f32_16x16x32_bf16\b", body))
    assert n16 == mfma and n16 > 0, (n16, mfma)
    # one chunk pair, six products per 16 x 16 block, 8 blocks per wave (32 x 64): the body of the unsplit 128 x 128 tile, once
    assert n16 == 2 * 6 * 8, n16
