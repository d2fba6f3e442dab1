"""GPU: the three score GEMM kernels of csrc/gemm_ss.hip behind `opp_coarse_match` -- two residents per CU (statistics, statistics + score
tile, confidences), three residents (the default) and the persistent kernel (OPP_SS_PERSIST=1) -- are built from one tile setup, one K stage
and one set of epilogue pieces.  Sharing them changes no arithmetic, so the bar is equality with the build in which every kernel restated
them: sha256 digests of every output, for every case x leg of tests/golden/score_gemm_cases.py."""
import pytest

from tests import helpers as H
from tests.golden import score_gemm_cases as SC


@pytest.fixture(scope="module")
def digests():
    """every leg once: `res3`, `res2` and `two` in this process, `persist` in a child (its switch is read once per process).  all_digests()
    itself checks that every case finds more than a quarter of its planted matches, that conf_matrix is finite everywhere (the NaN
    prefill is overwritten) and that OPP_SS_RES3 acted (somewhere the `res3` and `res2` confidences differ)."""
    return SC.all_digests()


def test_golden_file_holds_every_case_and_leg():
    """(no GPU: the CPU suite checks the fixture's key set)"""
    gold = H.load_golden(SC.PARENT_DIGEST)
    assert set(gold) == {"%s.%s.%s" % (c, leg, k) for c, leg in SC.pairs() for k in SC.KEYS}


@pytest.mark.gpu
@pytest.mark.parametrize("case,leg", SC.pairs(), ids=["%s-%s" % p for p in SC.pairs()])
def test_outputs_equal_the_preceding_build(digests, case, leg):
    """tests/golden/score_gemm_parent_digest.npz (gen_score_gemm_digest.py, run on the build with three self-contained kernels): conf_matrix,
    i_ids, j_ids, mconf and mkpts_query_c bit for bit."""
    skip = digests.get("%s.%s.skip" % (case, leg))
    if skip:
        pytest.skip(skip)
    gold = H.load_golden(SC.PARENT_DIGEST)
    for k in SC.KEYS:
        name = "%s.%s.%s" % (case, leg, k)
        assert digests[name] == str(gold[name]), name
