"""CPU: the numpy restatement of the pose metrics (tests/pose_metrics_reference.py, what the GPU tests can compute on a machine
without the reference) against the fixtures the reference's own functions produced (tests/golden/gen_pose_metrics_golden.py), and
against the live reference where its checkout is present; `aggregate_metrics` against the reference's; the import plumbing."""
import os
import sys

import numpy as np
import pytest

from tests import pose_metrics_reference as R
from tests.golden import pose_metrics_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF = os.environ.get("OPP_REFERENCE_ROOT", "/root/reference")


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= 1e-12 * np.abs(b)))


@pytest.fixture(scope="module")
def single():
    g = np.load(os.path.join(GOLDEN, "pose_metrics_single.npz"))
    assert list(g["names"]) == list(C.SINGLE_CASES) and tuple(g["units"]) == C.UNITS and tuple(g["diameters"]) == C.DIAMETERS
    return {k: g[k] for k in g.files}


def _check_row(model, pred, gt, K, g, i, where):
    for u, unit in enumerate(C.UNITS):
        r, t = R.query_pose_error(pred, gt, unit)
        assert _close(r, g["R_err"][i]) and _close(t, g["t_err"][i][u]), (where, unit, r, t)
    for si, syn in enumerate((False, True)):
        md = R.add_mean_dist(model, pred, gt, syn)
        assert _close(md, g["mean_dist"][i][si]), (where, syn, md, g["mean_dist"][i][si])
        for di, diameter in enumerate(C.DIAMETERS):
            assert R.add_metric(model, diameter, pred, gt, syn=syn) == bool(g["add"][i][di][si]), (where, syn, diameter)
    assert _close(R.projection_2d_error(model, pred, gt, K), g["proj2D"][i]), where


@pytest.mark.parametrize("name", list(C.SINGLE_CASES))
def test_restatement_matches_fixture(single, name):
    i = list(C.SINGLE_CASES).index(name)
    _check_row(*C.single_inputs(name), single, i, name)


def test_restatement_matches_batch_fixture():
    g = np.load(os.path.join(GOLDEN, "pose_metrics_batch.npz"))
    model, preds, gts, Ks, syn, valid = C.batch_inputs()
    for b in range(len(preds)):
        _check_row(model, preds[b], gts[b], Ks[b], g, b, "batch row %d" % b)


def test_fixture_covers_the_cases_with_margins(single):
    """what the generator asserted before it wrote the files: every vertex count has an ADD that passes and one that fails, no mean
    distance within 1e-6 of a threshold, no rotation error within 1e-3 rad of pi"""
    names = list(C.SINGLE_CASES)
    assert sorted({C.SINGLE_CASES[n][0] for n in names}) == sorted(C.P_LIST) and len(names) == 3 * len(C.P_LIST)
    for P in C.P_LIST:
        rows = [i for i, n in enumerate(names) if C.SINGLE_CASES[n][0] == P]
        assert single["add"][rows, :, 0].any() and not single["add"][rows, :, 0].all()
    thr = np.array(C.DIAMETERS)[None, :, None] * 0.1
    assert np.all(np.abs(single["mean_dist"][:, None, :] - thr) >= 1e-6 * thr)
    assert np.all(np.abs(np.deg2rad(single["R_err"]) - np.pi) > 1e-3)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src", "utils")), reason="reference checkout not present")
def test_restatement_matches_live_reference():
    from tests.golden.gen_pose_metrics_golden import load_reference_metric_utils
    saved = {k: sys.modules.get(k) for k in ("cv2", "open3d", "plyfile", "loguru")}
    saved_src = {k: v for k, v in sys.modules.items() if k == "src" or k.startswith("src.")}
    saved_path = list(sys.path)
    try:
        for k in saved_src:
            sys.modules.pop(k, None)
        mu = load_reference_metric_utils()
        for name in ("p65_small", "p257_large", "p1025_small"):
            model, pred, gt, K = C.single_inputs(name)
            for unit in C.UNITS:
                assert _close(R.query_pose_error(pred, gt, unit), mu.query_pose_error(pred, gt, unit=unit))
            assert _close(R.projection_2d_error(model, pred, gt, K), mu.projection_2d_error(model, pred, gt, K))
            for syn in (False, True):
                for diameter in C.DIAMETERS:
                    assert R.add_metric(model, diameter, pred, gt, syn=syn) == mu.add_metric(model, diameter, pred, gt, syn=syn)
        # 4x4 poses: the "dim check" of all three functions
        homo = lambda p: np.concatenate([p, [[0.0, 0.0, 0.0, 1.0]]])      # noqa: E731
        assert _close(R.query_pose_error(homo(pred), homo(gt)), mu.query_pose_error(homo(pred), homo(gt)))
        with pytest.raises(NotImplementedError):
            mu.query_pose_error(pred, gt, unit="km")
        # the drop-in replaces the reference's compute_query_pose_errors in the imported module AND in a caller that bound the
        # name before install() ran (`from src.utils.metric_utils import compute_query_pose_errors`, worker.py:4)
        import importlib
        import types
        for name in ("ray", "tqdm"):
            if name not in sys.modules:
                saved[name] = None
                sys.modules[name] = types.ModuleType(name)
        sys.modules["ray"].remote = getattr(sys.modules["ray"], "remote", lambda *a, **k: (lambda f: f))
        sys.modules["tqdm"].tqdm = getattr(sys.modules["tqdm"], "tqdm", lambda x, **k: x)
        worker = importlib.import_module("src.inference.inference_OnePosePlus_worker")
        upstream = mu.compute_query_pose_errors
        assert worker.compute_query_pose_errors is upstream
        from onepose_plus_plus_amd import dropin
        done = dropin.install(metrics=True)
        assert done["src.utils.metric_utils:compute_query_pose_errors"] == "compute_query_pose_errors"
        assert done["src.inference.inference_OnePosePlus_worker:compute_query_pose_errors"] == "compute_query_pose_errors"
        assert "src.lightning_model.OnePosePlus_lightning_model:compute_query_pose_errors" not in done      # never imported here
        assert done["src.utils.metric_utils"] == "ransac_PnP"
        assert mu.compute_query_pose_errors.__module__ == "onepose_plus_plus_amd.dropin"
        assert worker.compute_query_pose_errors is mu.compute_query_pose_errors is not upstream
    finally:
        sys.path[:] = saved_path
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[k]
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
        sys.modules.update(saved_src)


def test_aggregate_metrics_matches_fixture():
    from onepose_plus_plus_amd.metrics import aggregate_metrics
    g = np.load(os.path.join(GOLDEN, "pose_metrics_aggregate.npz"))
    agg = aggregate_metrics(C.aggregate_inputs())
    assert list(agg) == list(g["keys"])
    assert np.array_equal(np.array([agg[k] for k in agg]), g["values"])
    pose_only = aggregate_metrics({k: v for k, v in C.aggregate_inputs().items() if k in ("R_errs", "t_errs")}, pose_thres=[2, 4])
    assert list(pose_only) == list(g["keys_pose_only"])
    assert np.array_equal(np.array([pose_only[k] for k in pose_only]), g["values_pose_only"])


def test_unknown_unit_raises_before_anything_else():
    from onepose_plus_plus_amd.metrics import pose_metrics, query_pose_error
    pose = np.eye(4)[None, :3]
    with pytest.raises(NotImplementedError):
        pose_metrics(None, pose, pose, unit="km")
    with pytest.raises(NotImplementedError):
        query_pose_error(pose[0], pose[0], unit="inch")


def test_public_names_are_exported():
    import onepose_plus_plus_amd as pkg
    from onepose_plus_plus_amd import metrics
    for name in ("pose_metrics", "query_pose_error", "projection_2d_error", "add_metric", "compute_query_pose_errors",
                 "aggregate_metrics"):
        assert getattr(pkg, name) is getattr(metrics, name) and name in pkg.__all__


def test_install_without_metrics_returns_what_it_returned_before():
    """`metrics` defaults to off: the same keys and values as before, no wrapper recorded; with it the new key appears and the
    existing "src.utils.metric_utils" entry keeps its value"""
    from onepose_plus_plus_amd import dropin
    saved = {k: v for k, v in sys.modules.items() if k == "src" or k.startswith("src.")}
    saved_path = list(sys.path)
    key = "src.utils.metric_utils:compute_query_pose_errors"
    try:
        for k in saved:
            sys.modules.pop(k, None)
        done = dropin.install()
        assert key not in done
        assert set(done) == {"src.models.OnePosePlus.OnePosePlusModel", "src.models.OnePosePlus", "src.utils.metric_utils",
                             "src.lightning_model.losses", "src.models.OnePosePlus.utils.fine_supervision"}
        assert done["src.models.OnePosePlus"] == "OnePosePlus_model" and done["src.lightning_model.losses"] == "Loss"
        assert dropin.install(pnp=False, loss=False) == {"src.models.OnePosePlus.OnePosePlusModel": "OnePosePlus_model",
                                                         "src.models.OnePosePlus": "OnePosePlus_model"}
        with_metrics = dropin.install(metrics=True)
        assert key in with_metrics and {k: v for k, v in with_metrics.items() if k != key} == done
    finally:
        sys.path[:] = saved_path
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_metrics_module_does_not_import_the_oracle():
    import types

    from onepose_plus_plus_amd import metrics
    src = open(os.path.join(ROOT, "onepose_plus_plus_amd", "metrics.py")).read()
    assert "oracle" not in src
    mods = [v.__name__ for v in vars(metrics).values() if isinstance(v, types.ModuleType)]
    assert not [m for m in mods if m.split(".")[0] == "oracle"], mods
