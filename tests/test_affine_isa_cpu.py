"""Static audit of csrc/affine.hip (CPU: hipcc cross-compiles gfx950): the five kernels of the batched affine RANSAC are there and
none of them uses scratch or a waterfall loop -- the 2 x 3 models stay in LDS or scalars, the per-group counters in registers."""
import os
import shutil
import tempfile

import pytest

from tools import isa_audit

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

KERNELS = ("affine_hypotheses_kernel", "affine_score_kernel", "affine_stop_kernel", "affine_final_kernel", "affine_select_kernel")


@pytest.fixture(scope="module")
def audit():
    with tempfile.TemporaryDirectory() as tmp:
        src, rows, err = isa_audit.audit_source("affine.hip", False, tmp)
        assert rows is not None, err
        return rows, open(os.path.join(tmp, src + ".s")).read()


def test_every_kernel_is_there_without_scratch_or_waterfall(audit):
    rows, text = audit
    names = [r[0] for r in rows]
    for k in KERNELS:
        assert sum(k in n for n in names) == 1, (k, names)
    assert len(rows) == len(KERNELS)
    for name, vgpr, agpr, scratch, waterfall, mfma, pk in rows:
        assert scratch == 0, (name, scratch)
        assert waterfall == 0, (name, waterfall)
        assert mfma == 0, name
        # the metadata as well: the private segment is not an expression over callees there
        meta = text[text.index(".name:           " + name):]
        assert ".private_segment_fixed_size: 0\n" in meta[:meta.index(".vgpr_count")], name
