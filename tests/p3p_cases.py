"""Shared by tests/test_p3p_cpu.py and tests/test_p3p_gpu.py: the cases on which the default P3P PnP-RANSAC is compared with its
float64 restatement (tests/p3p_reference.py), their scenes, and the restatement's results, computed once per case.

The shapes are the smallest at which the kernels take another path: n = 4 and 5 (the sampler's retry loop), 63 / 64 / 65 (the
64-lane tail of the scoring wave), 257 and 700 (the 256-thread tail and more than one chunk of the refinement's point loop);
iterations = 1, 3 (one scoring block of 4 waves), 255 / 257 (the 256-thread hypothesis grid, ransac_scan's chunk 1 -> 2) and 601
(chunk 3).  The scene and hash seeds were searched on the CPU with the restatement alone (tests/test_p3p_cpu.py asserts what
they were searched for): at most 1 % undecided hypotheses and scoring decisions per case, no undecided decision in the selected
hypothesis or its refinement, and for the four special cases their stated property."""
import collections
import functools

import numpy as np

from tests import p3p_reference as PR
from tests.loransac_cases import MARGIN
from tests.test_pnp_gpu import _scene

THR = 3.3
THR2 = THR * THR

# The float64 conditioning noise of the restatement's hypothesis poses: the largest difference, over every decided valid
# hypothesis of every case below (`single_cases()` included), between `PR.hypothesis` and its second evaluation (`precise=True`: long double, every accepted
# root Newton-polished, the alignment from the triangle frames), in the returned form [R | t / scale].  Measured by
# tests/test_p3p_cpu.py::test_hypothesis_pose_bar, which prints it and fails when it no longer matches.  The bar on a device
# hypothesis pose is 16 x that noise: the device contracts to FMA, orders its operations differently and takes the roots from
# a Ferrari solve.  Measured: 1.126e-08 (case "tie", hypothesis 131; the other cases stay below 5e-9), so the bar is 1.92e-07.
# The noise is the conditioning of Grunert's equations, not of `np.roots`: polishing the float64 roots does not lower it.  Scene
# seeds whose hypotheses include a nearly fourfold root (noise 8e-7 was seen) were passed over, so that the bar stays below 1e-6.
HYP_POSE_NOISE = 1.2e-8
HYP_POSE_TOL = 16 * HYP_POSE_NOISE

Case = collections.namedtuple("Case", "name n outliers noise scale iterations refine_iters confidence scene_seed seed behind")

CASES = [
    Case("n4", 4, 0.0, 0.3, 1000, 3, 1, 1.0, 1, 5, 0),
    Case("n5", 5, 0.0, 0.3, 1, 1, 8, 1.0, 2, 5, 0),
    Case("tie", 12, 0.25, 0.5, 1000, 255, 0, 1.0, 303, 5, 0),
    Case("n12", 12, 0.25, 0.5, 1000, 601, 1, 0.99, 4, 5, 0),
    Case("n63", 63, 0.3, 0.5, 1000, 255, 8, 0.99, 5, 5, 0),
    Case("n64", 64, 0.3, 0.5, 1, 257, 1, 1.0, 6, 5, 0),
    Case("n65_behind", 65, 0.3, 0.5, 1000, 257, 8, 1.0, 107, 5, 5),
    Case("stop", 257, 0.5, 1.5, 1000, 601, 8, 0.99, 8, 5, 0),
    Case("n700_behind", 700, 0.4, 0.5, 1, 601, 8, 1.0, 9, 5, 9),
    Case("few", 50, 1.0, 0.0, 1000, 601, 8, 1.0, 310, 5, 0),
    Case("none", 5, 1.0, 0.0, 1000, 3, 8, 1.0, 11, 5, 0),
]
BY_NAME = {c.name: c for c in CASES}
# one hypothesis at a time: iterations = 1 and no refinement return the hypothesis's own pose; hash seeds 0..39 on each scene
SINGLE_SCENES = [Case("one70", 70, 0.2, 0.5, 1, 1, 0, 1.0, 21, 0, 0), Case("one257_behind", 257, 0.2, 0.5, 1000, 1, 0, 1.0, 22, 0, 7)]
SINGLE_SEEDS = range(40)


def single_cases():
    return [c._replace(seed=s) for c in SINGLE_SCENES for s in SINGLE_SEEDS]


def scene(case):
    """-> K [3,3], uv [n,2] float32, X [n,3] float32, indices of the matches planted behind the camera.  `behind` matches get a
    3D point at negative depth under the true pose and the pixel its projection formula gives there: without the z > 1e-12 test
    they would be perfect inliers of the true pose."""
    rng = np.random.default_rng(case.scene_seed)
    K, uv, X, R, t, _ = _scene(rng, case.n, case.outliers, case.noise)
    if case.outliers >= 1.0:
        uv = rng.uniform(0, 512, size=uv.shape)
    planted = np.arange(case.behind) * (case.n // max(case.behind, 1))
    for i in planted:
        Xc = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), -rng.uniform(0.3, 0.8)])
        X[i] = R.T @ (Xc - t)
        uv[i] = [K[0, 0] * Xc[0] / Xc[2] + K[0, 2], K[1, 1] * Xc[1] / Xc[2] + K[1, 2]]
    return K, uv.astype(np.float32), X.astype(np.float32), planted


@functools.lru_cache(maxsize=None)
def reference(case):
    """the restatement on `case`, once; callers leave it unchanged.  -> (K, uv, X, planted, uv64, X64, K4, PR.run's dict)"""
    K, uv, X, planted = scene(case)
    uv64, X64 = PR.f64(uv, X, case.scale)
    K4 = PR.K4_of(K)
    out = PR.run(X64, uv64, K4, THR2, case.seed, case.iterations, case.refine_iters, case.confidence, case.scale)
    return K, uv, X, planted, uv64, X64, K4, out


def undecided_shares(case, out):
    """(share of undecided hypotheses, share of undecided (hypothesis, point) scoring decisions, the selected hypothesis or its
    refinement is undecided)"""
    hyps = float(np.mean(out["undecided"])) if len(out["undecided"]) else 0.0
    points = float(np.sum(out["point_undecided"])) / max(1, len(out["undecided"]) * case.n)
    b = out["best"]
    sel = b >= 0 and (out["undecided"][b] or out["point_undecided"][b] > 0 or any(m < MARGIN for _, m in out["refine_margins"]))
    return hyps, points, bool(sel)


def pose_distance(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


def tied(out):
    """the hypotheses before the stop index that reach the highest score, in index order"""
    sc = out["scores"][:out["stop"]]
    return np.nonzero(sc == sc.max())[0] if sc.size and sc.max() >= 0 else np.zeros(0, dtype=np.int64)
