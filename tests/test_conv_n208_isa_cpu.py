"""Static guard on the two-role 128 x 224 bf16x3 convolution tile (gemm_mfma.hip, kRoles; CPU: hipcc cross-compiles gfx950).  The generic
check in test_conv_isa_cpu.py covers every opp_gemm_kernel<..., true, ..., 2> instance it finds; this one makes sure the new instance is
among them, so that guard cannot pass by matching nothing."""
import os
import re
import shutil
import tempfile

import pytest

from tools import isa_audit

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

# opp_gemm_kernel<128, 224, 2, 4, true, 0, 2, OPP_PREC_BF16X3>
SYMBOL = "_ZN12_GLOBAL__N_115opp_gemm_kernelILi128ELi224ELi2ELi4ELb1ELi0ELi2ELi2EEEv7OppGemm"


def test_two_role_conv_tile_is_built_without_scratch():
    with tempfile.TemporaryDirectory() as tmp:
        src, rows, err = isa_audit.audit_source("gemm_mfma.hip", False, tmp)
        assert rows is not None, err
        text = open(os.path.join(tmp, src + ".s")).read()
    found = [r for r in rows if r[0] == SYMBOL]
    assert len(found) == 1, [r[0] for r in rows if "opp_gemm_kernel" in r[0]]
    k, vg, ag, sc, water, mfma, pk = found[0]
    body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(k), text, re.S | re.M).group(0)
    assert sc == 0 and water == 0, (sc, water)
    assert vg + ag <= 256, (vg, ag)
    n16 = len(re.findall(r"\bv_mfma_f32_16x16x32_bf16\b", body))
    assert n16 == mfma and "v_mfma_f32_32x32x16_bf16" not in body, (n16, mfma)
    # both roles' chunk pairs, six products per 16 x 16 block: 2 x 6 x (16 + 10) -- 26 blocks per SIMD and chunk, not the 32 of 128 x 256
    assert n16 == 2 * 6 * (16 + 10), n16
