"""GPU: `opp_affine2d_ransac_batch` held to the workspace contract ("The workspace contract") with the harness of
tests/memory_contract.py on `tests.hip_ops.GuardedBuffers`: a zero-filled, a NaN-filled and a left-over workspace give bit-identical
outputs with intact guard bands, and a workspace declared half as large, or empty, is refused with the workspace code before
anything is written."""
import pytest

from tests import affine_cases as AC
from tests import affine_ops as AO
from tests import memory_contract as MC

pytestmark = pytest.mark.gpu


def _views(sizes, seed0):
    return [AC.scene(seed0 + k, n, 0.3)[:2] for k, n in enumerate(sizes)]


def _stage(bufs):
    """V = 3, n = (65, 0, 7), 257 iterations"""
    return AO.run_raw(_views((65, 0, 7), 70), [3, 4, 5], 257, 0.99, bufs=bufs)


def _larger(bufs):
    """the strictly larger predecessor of the left-over fill: more views, more matches, more iterations"""
    return AO.run_raw(_views((80, 3, 9, 70), 80), [6, 7, 8, 9], 300, 0.99, bufs=bufs)


def test_size_query_grows_with_the_predecessor():
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    assert lib.opp_affine2d_batch_workspace_bytes(300, 4, 162) > lib.opp_affine2d_batch_workspace_bytes(257, 3, 72) > 0


def test_workspace_fills_give_the_same_bits():
    assert MC.fill_problems(_stage, _larger) == []


def test_too_small_a_workspace_is_refused_before_any_write():
    assert MC.refusal_problems(_stage) == []
