"""CPU: what pose.py decides before any C call -- the solver a name resolves to, the default confidence, the batch call a solver
has and the keyword arguments it takes -- pinned as tables against what the five front doors did when each wrote it out.  Pure
Python: the library is never loaded."""
import numpy as np
import pytest

from onepose_plus_plus_amd import pose


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def load():
        raise AssertionError("the solver resolution must not need the library")
    monkeypatch.setattr(pose._lib, "load", load)


def test_solver_names():
    for name in ("p3p", "epnp", "loransac"):
        for flag in (False, True):
            assert pose._resolve_solver(name, flag) == name
        assert pose._resolve_solver(name, auto=False) == name
    assert pose._resolve_solver("auto", False) == "epnp"
    assert pose._resolve_solver("auto", True) == "loransac"
    with pytest.raises(ValueError) as e:
        pose._resolve_solver("dlt", False)
    assert str(e.value) == "solver must be one of 'p3p', 'epnp', 'loransac', 'auto', got 'dlt'"
    with pytest.raises(ValueError) as e:                    # ransac_PnP_ex has no "auto"
        pose._resolve_solver("auto", auto=False)
    assert str(e.value) == "solver must be one of 'p3p', 'epnp', 'loransac', got 'auto'"


def test_front_doors_refuse_a_bad_name_before_the_library():
    K, uv, X = np.eye(3), np.zeros((8, 2)), np.zeros((8, 3))
    with pytest.raises(ValueError, match="'auto', got 'dlt'"):
        pose.ransac_PnP(K, uv, X, solver="dlt")
    with pytest.raises(ValueError, match="'loransac', got 'auto'"):
        pose.ransac_PnP_ex(K, uv, X, solver="auto")
    with pytest.raises(ValueError, match="'auto', got 'dlt'"):
        pose.ransac_PnP_batch(K[None], uv, X, offsets=[0, 8], solver="dlt")
    for kw in (dict(solver="loransac"), dict(solver="auto", use_pycolmap_ransac=True)):
        with pytest.raises(NotImplementedError, match="loransac_PnP_batch"):
            pose.ransac_PnP_batch(K[None], uv, X, offsets=[0, 8], **kw)


def test_default_confidence():
    assert [pose._confidence(s, None) for s in ("p3p", "epnp", "loransac")] == [1.0, 0.99, 0.9999]
    assert [pose._confidence(s, 0.5) for s in ("p3p", "epnp", "loransac")] == [0.5, 0.5, 0.5]


OPTIONS = {"scale": 1000, "refine_iters": 3, "min_trials": 300, "min_inlier_ratio": 0.05, "seed": 7, "iterations": 1500, "confidence": 0.9}
RANSAC_KEYS = {"solver", "scale", "refine_iters", "seed", "iterations", "confidence"}
LORANSAC_KEYS = {"min_trials", "min_inlier_ratio", "seed", "iterations", "confidence"}


@pytest.mark.parametrize("solver,flag,call,keys,resolved", [
    ("p3p", False, "ransac_PnP_batch", RANSAC_KEYS, "p3p"),
    ("p3p", True, "ransac_PnP_batch", RANSAC_KEYS, "p3p"),
    ("epnp", False, "ransac_PnP_batch", RANSAC_KEYS, "epnp"),
    ("auto", False, "ransac_PnP_batch", RANSAC_KEYS, "epnp"),
    ("loransac", False, "loransac_PnP_batch", LORANSAC_KEYS, None),
    ("auto", True, "loransac_PnP_batch", LORANSAC_KEYS, None),
])
def test_batch_call_and_its_keyword_arguments(solver, flag, call, keys, resolved):
    fn, kw = pose._batch_call(dict(OPTIONS, solver=solver), flag, batch_loransac=True)
    assert fn is getattr(pose, call)
    assert set(kw) == keys
    assert kw.get("solver") == resolved
    assert all(kw[k] == OPTIONS[k] for k in keys - {"solver"})
    if call == "loransac_PnP_batch":                        # off unless asked for: the per-sample loop runs
        assert pose._batch_call(dict(OPTIONS, solver=solver), flag, batch_loransac=False) is None


def test_batch_call_defaults_and_unknown_names():
    fn, kw = pose._batch_call({"scale": 2}, False, batch_loransac=False)
    assert fn is pose.ransac_PnP_batch and kw == {"scale": 2, "solver": "p3p"}
    assert pose._batch_call({"solver": "dlt"}, False) is None          # left to ransac_PnP, which raises
    fn, kw = pose._batch_call({"solver": "loransac", "simple_pinhole": False, "max_batch": 2}, False)
    assert fn is pose.loransac_PnP_batch and kw == {"simple_pinhole": False, "max_batch": 2}      # anything else passes through


def test_failure_tuple_and_homogeneous_pose():
    pose34, homo, inliers, state = pose._failure()
    assert np.array_equal(pose34, np.eye(4)[:3]) and np.array_equal(homo, np.eye(4)) and state is False
    assert inliers.dtype == bool and inliers.shape == (0,)
    P = np.arange(12.0).reshape(3, 4)
    assert np.array_equal(pose._homo(P), np.vstack([P, [0, 0, 0, 1]])) and pose._homo(P).dtype == np.float64
    PB = np.arange(24.0).reshape(2, 3, 4)
    assert pose._homo(PB).shape == (2, 4, 4) and all(np.array_equal(pose._homo(PB)[b], pose._homo(PB[b])) for b in range(2))
