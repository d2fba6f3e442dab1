"""CPU: the affine RANSAC behind the 2D detector (onepose_plus_plus_amd/detect.py, csrc/affine.hip) without a GPU -- the float64
restatement (tests/affine_reference.py) recovers the planted map and decides its own case list, the pure logic of
csrc/affine_batch.h built for the host with g++ agrees with it, and the front end refuses bad arguments before it touches a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import affine_cases as AC
from tests import affine_reference as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = ctypes.POINTER(ctypes.c_double)


def _p(a):
    return a.ctypes.data_as(dp)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("affine") / "libaffine_host.so")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "affine_host.cpp")])
    L = ctypes.CDLL(out)
    L.t_affine_layout.restype = None
    L.t_affine_from3.restype = None
    L.t_affine_count.argtypes = [dp, dp, dp, ctypes.c_int, ctypes.c_double]
    return L


def _run(case, **kw):
    n, out, iters, conf, scene_seed, seed = case
    p0, p1, M, outl = AC.scene(scene_seed, n, out)
    r = AR.estimate_view(p0, p1, seed, iters, AC.THR, conf, True, AC.corners_of(AC.REF_HW), AC.FALLBACK, **kw)
    return r, p0, p1, M, outl


def _corner_gap(A, B):
    c = AC.corners_of(AC.REF_HW)
    return float(np.abs((c @ A[:, :2].T + A[:, 2]) - (c @ B[:, :2].T + B[:, 2])).max())


@pytest.mark.parametrize("n,out", [(300, 0.0), (300, 0.3), (300, 0.6), (65, 0.3), (7, 0.0)])
def test_restatement_recovers_the_planted_map(n, out):
    r, p0, p1, M, outl = _run((n, out, 2000, 0.99, 31 + n, 9))
    assert r["ok"] == 1 and not r["undecided"]
    # 0.5 px noise on n (1 - out) inliers over a 640 x 480 image: the corners land well within 3 px (7 matches) / 1 px
    assert _corner_gap(r["affine"], M) < (3.0 if n < 60 else 1.0)
    assert r["n_inliers"] >= 0.9 * round(n * (1 - out)) and r["mask"][outl].sum() == 0
    assert np.array_equal(r["box"], AR.box_of(r["affine"], AC.corners_of(AC.REF_HW)))
    e2 = AR.errors2(r["ransac_affine"], AR.f64(p0), AR.f64(p1))
    assert np.array_equal(r["mask"], (e2 <= AC.THR ** 2).astype(np.int32))          # the inliers of the RANSAC model, not of the refit


def test_restatement_failures_and_small_views():
    c, fb = AC.corners_of(AC.REF_HW), AC.FALLBACK
    p0, p1, M, _ = AC.scene(5, 12, 0.0)
    for k in (0, 1, 2):
        r = AR.estimate_view(p0[:k], p1[:k], 1, 64, corners=c, fallback_box=fb)
        assert (r["ok"], r["stop"], r["n_inliers"]) == (0, 0, 0) and np.array_equal(r["box"], fb) and np.array_equal(r["affine"], np.eye(3)[:2])
    r = AR.estimate_view(p0[:3], p1[:3], 1, 64, corners=c, fallback_box=fb)        # n == 3: one hypothesis on 0, 1, 2
    assert r["ok"] == 1 and r["stop"] == 1 and r["best"] == 0 and r["samples"][0].tolist() == [0, 1, 2] and (r["samples"][1:] == -1).all()
    assert r["n_inliers"] == 3 and r["cond"] is None and _corner_gap(r["affine"], r["ransac_affine"]) == 0.0
    line = np.stack([15.0 * np.arange(40), 30.0 * np.arange(40) + 3], axis=1).astype(np.float32)       # exact in float32
    r = AR.estimate_view(line, p1[:1].repeat(40, 0), 1, 64, corners=c, fallback_box=fb)
    assert r["ok"] == 0 and (r["scores"] == -1).all() and r["stop"] == 64 and np.array_equal(r["box"], fb)
    same = p0[:1].repeat(40, 0)
    r = AR.estimate_view(same, same, 1, 64, corners=c, fallback_box=fb)
    assert r["ok"] == 0 and (r["scores"] == -1).all() and not r["undecided"]


@pytest.mark.parametrize("cases", [AC.GPU_CASES, AC.GRID_CASES], ids=["gpu_cases", "grid"])
def test_undecided_cap_and_conditioning(cases):
    """the restatement alone: at most 1 case in 20 of the list undecided, every refit well conditioned"""
    undecided, worst = 0, 0.0
    for case in cases:
        r = _run(case)[0]
        undecided += bool(r["undecided"])
        if r["cond"] is not None:
            worst = max(worst, r["cond"])
            assert r["cond"] <= 1e3, (case, r["cond"])
    print("undecided %d of %d, largest condition number %.3g" % (undecided, len(cases), worst))
    assert undecided * 20 <= len(cases), (undecided, len(cases))


def test_case_list_covers_the_shapes():
    assert {c[0] for c in AC.GPU_CASES} == set(AC.SIZES) and {c[2] for c in AC.GPU_CASES} == set(AC.ITERATIONS)
    assert {c[3] for c in AC.GPU_CASES} == {0.99, 1.0} and 36 <= len(AC.GPU_CASES) <= 44 and len(AC.GRID_CASES) == 96
    for n in AC.SIZES:
        assert {c[2] for c in AC.GPU_CASES if c[0] == n and c[3] == 0.99} == set(AC.ITERATIONS)


# ---- csrc/affine_batch.h on the host ---------------------------------------------------------------------------------------------
def test_modes(lib):
    assert [lib.t_affine_mode(n) for n in range(6)] == [0, 0, 0, 1, 2, 2] and lib.t_affine_mode(100000) == 2
    for iters in (1, 64, 2000):
        assert [lib.t_affine_hypotheses(n, iters) for n in (0, 2, 3, 4, 300)] == [0, 0, 1, iters, iters]
        for n in (0, 2, 3, 4, 300):                                                # the restatement evaluates as many
            p0, p1, _, _ = AC.scene(3, n, 0.0)
            r = AR.estimate_view(p0, p1, 5, iters)
            assert int((r["samples"][:, 0] >= 0).sum()) == lib.t_affine_hypotheses(n, iters)


def _align(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("iterations", [1, 63, 64, 257, 2000])
@pytest.mark.parametrize("V", [1, 3, 16])
def test_workspace_layout(lib, iterations, V):
    out = (ctypes.c_ulonglong * 8)()
    lib.t_affine_layout(iterations, V, 123, out)
    hyp, valid, score, score2, hs, is_, total, returned = (int(x) for x in out)
    assert total == returned == V * (_align(48 * iterations) + 3 * _align(4 * iterations))
    spans = []
    for base, stride, per in ((hyp, hs, 48), (valid, is_, 4), (score, is_, 4), (score2, is_, 4)):
        assert base % 256 == 0 and stride % 256 == 0
        spans += [(base + v * stride, base + v * stride + per * iterations) for v in range(V)]
    spans.sort()
    assert spans[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= total
    lib.t_affine_layout(0, 0, 0, out)
    clamp = list(out)
    lib.t_affine_layout(1, 1, 1, out)
    assert clamp == list(out)


def test_library_size_query_is_the_layout(lib):
    from onepose_plus_plus_amd import _lib
    L = _lib.load()
    for I in (0, 1, 257, 2000):
        for V in (0, 1, 3, 1024):
            for n in (0, 5, 30000):
                assert L.opp_affine2d_batch_workspace_bytes(I, V, n) == max(V, 1) * (_align(48 * max(I, 1)) + 3 * _align(4 * max(I, 1)))


def test_collinearity_model_and_counts_agree_with_the_restatement(lib):
    rng = np.random.default_rng(4)
    p0, p1, _, _ = AC.scene(17, 300, 0.4)
    p0, p1 = AR.f64(p0), AR.f64(p1)
    for _ in range(200):
        idx = rng.choice(300, 3, replace=False)
        s, d = np.ascontiguousarray(p0[idx]), np.ascontiguousarray(p1[idx])
        col, margin = AR.collinear(s[None])
        assert bool(lib.t_affine_collinear(_p(s))) == bool(col[0]) and margin[0] > 1e-3
        M = np.zeros(6)
        lib.t_affine_from3(_p(s), _p(d), _p(M))
        ref = np.linalg.solve(np.concatenate([s, np.ones((3, 1))], axis=1), d).T
        e2 = AR.errors2(ref, p0, p1)
        assert _corner_gap(M.reshape(2, 3), ref) <= 1e-9 * max(1.0, np.abs(ref).max() * 640)
        if AR._rel(e2, 36.0).min() > 1e-6:
            assert lib.t_affine_count(_p(M), _p(np.ascontiguousarray(p0)), _p(np.ascontiguousarray(p1)), 300, 36.0) == int((e2 <= 36.0).sum())
    for s in ([[0, 0], [1, 1], [2, 2]], [[5, 5], [5, 5], [9, 1]], [[3, 4], [3, 4], [3, 4]], [[0, 0], [100, 0], [200, 0]]):
        s = np.array(s, np.float64)
        assert lib.t_affine_collinear(_p(s)) == 1 and AR.collinear(s[None])[0][0]
    s = np.array([[0, 0], [100, 0], [200, 1e-3]])
    assert lib.t_affine_collinear(_p(s)) == 0 and not AR.collinear(s[None])[0][0]


def test_refit_agrees_with_lstsq(lib):
    for seed, n in ((1, 4), (2, 7), (3, 300)):
        p0, p1, _, _ = AC.scene(seed, n, 0.0)
        p0, p1 = np.ascontiguousarray(AR.f64(p0)), np.ascontiguousarray(AR.f64(p1))
        M = np.zeros(6)
        assert lib.t_affine_refit(_p(p0), _p(p1), n, _p(M)) == 1
        ref, cond = AR.refit(p0, p1)
        assert cond <= 1e3 and _corner_gap(M.reshape(2, 3), ref) <= 1e-6
    line = np.stack([np.arange(5.0), 2 * np.arange(5.0)], axis=1).copy()
    keep = np.full(6, 7.0)
    assert lib.t_affine_refit(_p(line), _p(line), 5, _p(keep)) == 0 and (keep == 7.0).all()     # singular: the model is kept


def test_box_truncates_towards_zero_and_refuses_what_int32_cannot_hold(lib):
    c = np.ascontiguousarray(AC.corners_of(AC.REF_HW))
    box = (ctypes.c_int * 4)(9, 9, 9, 9)
    M = np.array([0.5, -0.25, -10.7, 0.1, 0.9, -0.6])
    assert lib.t_affine_box(_p(M), _p(c), box) == 1
    assert list(box) == AR.box_of(M.reshape(2, 3), c).tolist() == [-130, 0, 309, 495]
    for bad in (np.nan, np.inf, 2.0 ** 31, -2.0 ** 31):
        M2 = M.copy()
        M2[2] = bad
        box = (ctypes.c_int * 4)(9, 9, 9, 9)
        assert lib.t_affine_box(_p(M2), _p(c), box) == 0 and list(box) == [9, 9, 9, 9] and AR.box_of(M2.reshape(2, 3), c) is None
    M2 = M.copy()
    M2[2] = 2.0 ** 31 - 700.0                                     # the largest corner stays below 2^31
    assert lib.t_affine_box(_p(M2), _p(c), box) == 1 and list(box) == AR.box_of(M2.reshape(2, 3), c).tolist()


# ---- the front end -----------------------------------------------------------------------------------------------------------------
def test_front_end_refuses_bad_arguments_before_any_device_work():
    from onepose_plus_plus_amd import detect_box, estimate_affine_2d_batch
    from onepose_plus_plus_amd.detect import AffineBoxDetector
    p = np.zeros((8, 2), np.float32)
    bad = [dict(pts1=np.zeros((7, 2))), dict(pts0=np.zeros((8, 3))), dict(view_ids=np.zeros(8), offsets=[0, 8]), dict(view_ids=np.zeros(8)),
           dict(offsets=[0, 4, 8], n_views=3), dict(corners=np.zeros((2, 4, 3))), dict(offsets=[0, 8], corners=np.zeros((2, 4, 2))),
           dict(n_views=0, view_ids=np.zeros(8)), dict(n_views=1025, view_ids=np.zeros(8)), dict(max_iters=0), dict(max_iters=(1 << 20) + 1),
           dict(ransac_reproj_threshold=0.0), dict(confidence=0.0), dict(seed=[1, 2]), dict(fallback_box=[1, 2, 3]),
           dict(fallback_box=[0.5, 0, 1, 1]), dict(fallback_box=[0, 0, 0, 2 ** 31])]
    for kw in bad:
        args = dict(pts0=p, pts1=p)
        args.update(kw)
        with pytest.raises(ValueError):
            estimate_affine_2d_batch(**args)
    with pytest.raises(ValueError):
        detect_box([], (480, 640), (960, 1280))
    with pytest.raises(ValueError):
        detect_box([(p, p[:5])], (480, 640), (960, 1280))
    with pytest.raises(ValueError):
        detect_box([(p, p), (p, p)], [(480, 640)] * 3, (960, 1280))
    with pytest.raises(ValueError):
        AffineBoxDetector(lambda a, b: (p, p), [])


def test_ctypes_table_declares_the_entry_points():
    from onepose_plus_plus_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "opp_hip.h")).read(), flags=re.S)
    counts = {name: args.count(",") + 1 for name, args in re.findall(r"\b(opp_affine2d_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}
    assert counts == {"opp_affine2d_batch_workspace_bytes": 3, "opp_affine2d_ransac_batch": 25}
    for name, k in counts.items():
        assert len(_lib.SIGNATURES[name][1]) == k
    assert _lib.SIGNATURES["opp_affine2d_batch_workspace_bytes"][0] is ctypes.c_size_t
    assert "affine.hip" in build.SOURCES and "affine_batch.h" in build.HEADERS                 # the source hash covers them
