"""Static guard on the batched store loop of opp_gemm_body (gemm_mfma.hip; CPU: hipcc cross-compiles gfx950).  vmcnt counts stores too, so a
vmcnt wait between two stores of a batch puts a store round trip back into the epilogue; and a residual address the compiler cannot trace to
g.R becomes a flat load, which also counts on lgkmcnt and is waited for by the next item's LDS read.  Neither shows in any result.
The store-run check reads the assembly in text order, so it can also fail for a harmless reason -- the compiler unrolling the two-batch loop
(runs of 8) or laying the instances out so that two of them touch (a run of 6 or 8): then look at the listing and update the expected runs; a run
SHORTER than a batch (1s and 3s) is the real regression.  That the direct residual's loads have no lgkmcnt wait between them is not pinned
beyond the absence of flat accesses."""
import os
import re
import shutil
import tempfile

import pytest

from tools import isa_audit

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

# opp_gemm_kernel<128, 128, 4, 2, true, 0, 2, OPP_PREC_BF16X3>: 8 float4 items per thread, batches of 4 (2 with the bilinear residual)
SYMBOL = "_ZN12_GLOBAL__N_115opp_gemm_kernelILi128ELi128ELi4ELi2ELb1ELi0ELi2ELi2EEEv7OppGemm"


@pytest.fixture(scope="module")
def asm():
    with tempfile.TemporaryDirectory() as tmp:
        src, rows, err = isa_audit.audit_source("gemm_mfma.hip", False, tmp)
        assert rows is not None, err
        return open(os.path.join(tmp, src + ".s")).read()


def test_no_flat_memory_access_in_the_gemm_kernels(asm):
    assert not re.findall(r"^\s*flat_(?:load|store)_\w+", asm, re.M)


def test_no_vmcnt_wait_between_the_stores_of_a_batch(asm):
    body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(SYMBOL), asm, re.S | re.M).group(0).split("\n")
    last_mfma = max(i for i, ln in enumerate(body) if "v_mfma_" in ln)
    runs, cur = [], 0       # 16-byte stores in text order, cut wherever a vmcnt wait stands between two of them
    for ln in body[last_mfma:]:
        if re.search(r"\bglobal_store_dwordx4\b", ln):
            cur += 1
        elif re.search(r"s_waitcnt.*vmcnt", ln) and cur:
            runs.append(cur)
            cur = 0
    if cur:
        runs.append(cur)
    # the four 16-byte instances of the loop: no loads in the items, bias / row mask per item, direct residual (4 stores each), bilinear (2)
    assert sorted(runs) == [2, 4, 4, 4], runs
