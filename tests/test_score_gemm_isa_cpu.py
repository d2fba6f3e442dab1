"""Static guard on the five score GEMM kernels of csrc/gemm_ss.hip (CPU: hipcc cross-compiles gfx950): the register budgets their occupancy
needs, the scratch and the MFMA counts of the build in which every kernel stated its own tile setup, K stage and epilogue."""
import os
import shutil
import tempfile

import pytest

from tools import isa_audit

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

NS = "_ZN12_GLOBAL__N_1"
# symbol -> (VGPR + AGPR budget, scratch bytes, v_mfma count)
#   three residents: three workgroups of four waves = three waves per SIMD, 512 / 3 rounded down to the allocation granule = 168; its 12 bytes
#   of spills lie outside the K loop.  The others: two waves per SIMD = 256.
#   48 MFMAs = the two-stage K loop body, 24 = the one-stage body: neither re-rolled nor duplicated
KERNELS = {
    NS + "14gemm_ss_kernelILi1EEEv9OppGemmSS": (256, 0, 48),      # OPP_SS_STATS
    NS + "14gemm_ss_kernelILi3EEEv9OppGemmSS": (256, 0, 48),      # OPP_SS_STATS_STORE
    NS + "14gemm_ss_kernelILi2EEEv9OppGemmSS": (256, 0, 48),      # OPP_SS_CONF
    NS + "22gemm_ss_persist_kernelE9OppGemmSS": (256, 0, 48),
    NS + "19gemm_ss_res3_kernelE9OppGemmSS": (168, 12, 24),
}


def test_score_gemm_kernels_keep_their_registers_scratch_and_mfma_counts():
    with tempfile.TemporaryDirectory() as tmp:
        _, rows, err = isa_audit.audit_source("gemm_ss.hip", False, tmp)
    assert rows is not None, err
    found = {r[0]: r for r in rows}
    assert set(found) == set(KERNELS), sorted(found)
    for k, (budget, scratch, n_mfma) in KERNELS.items():
        _, vg, ag, sc, water, mfma, _ = found[k]
        assert vg + ag <= budget, (k, vg, ag)
        assert sc == scratch, (k, sc)
        assert mfma == n_mfma, (k, mfma)
        assert water == 0, (k, water)
