"""Static audit of csrc/pointcloud.hip (CPU: hipcc cross-compiles gfx950): no kernel uses scratch or a waterfall loop, and the
kernels that decide a comparison -- the pair search and the box mask -- hold no fused multiply-add: their float64 products and sums
round one by one like the numpy restatement (build.SOURCE_FLAGS compiles the file with contraction off).  The emit kernel's
correctly rounded division expands into FMAs by design and is not part of that check."""
import os
import re
import shutil
import tempfile

import pytest

from tools import isa_audit

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

KERNELS = ("pc_box_mask_kernel", "pc_neighbor_kernelILb0", "pc_neighbor_kernelILb1", "pc_select_kernel", "pc_emit_kernel")


@pytest.fixture(scope="module")
def audit():
    with tempfile.TemporaryDirectory() as tmp:
        src, rows, err = isa_audit.audit_source("pointcloud.hip", False, tmp)
        assert rows is not None, err
        return rows, open(os.path.join(tmp, src + ".s")).read()


def test_every_kernel_is_there_without_scratch_or_waterfall(audit):
    rows, _ = audit
    names = [r[0] for r in rows]
    for k in KERNELS:
        assert sum(k in n for n in names) == 1, (k, names)
    assert len(rows) == len(KERNELS)
    for name, vgpr, agpr, scratch, waterfall, mfma, pk in rows:
        assert scratch == 0, (name, scratch)
        assert waterfall == 0, (name, waterfall)


def test_no_contraction_where_a_threshold_is_decided(audit):
    rows, asm = audit
    for name in (r[0] for r in rows):
        if "pc_neighbor_kernel" not in name and "pc_box_mask_kernel" not in name:
            continue
        body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), asm, re.S | re.M).group(0)
        assert re.search(r"\bv_mul_f64\b", body) and re.search(r"\bv_add_f64\b", body), name
        assert not re.search(r"\bv_fma_f64\b|\bv_fmac_f64\b", body), name
