"""GPU: the batched LO-RANSAC (csrc/pnp_lo_batch.hip through opp_pnp_loransac_batch / pose.loransac_PnP_batch) against the
single-sample call on each sample's slice -- byte for byte -- on one batch whose sizes hit every device-side branch
(tests/loransac_batch_cases.py): n = 300 with 70 % outliers, 0 (empty, between non-empty ones), 2 (the failure), 3 (P3P models
only), 4 (no LO), 5, 70 with 40 % outliers, 130 clean.  The single-sample results are computed once per module."""
import numpy as np
import pytest
import torch

from tests import loransac_batch_cases as BC
from tests.golden import pose_metrics_cases as PC
from tests.test_loransac_gpu import _errs
from tests.test_pnp_gpu import _scene

pytestmark = pytest.mark.gpu

SIZES, SEEDS, THR = BC.SIZES, BC.SEEDS, BC.THR
B = len(SIZES)


@pytest.fixture(scope="module")
def scene():
    """the batch, and per setting the single-sample results on each sample's slice; computed once, never modified"""
    from onepose_plus_plus_amd.pose import ransac_PnP_ex
    K, uvs, Xs, gts = BC.make_batch()
    singles = {name: [ransac_PnP_ex(K[b], uvs[b], Xs[b], seed=SEEDS[b], solver="loransac", pnp_reprojection_error=THR, **kw)
                      for b in range(B)] for name, kw in BC.SETTINGS.items()}
    return {"K": K, "uv": uvs, "X": Xs, "gt": gts, "singles": singles}


def _concat(scene, order):
    return BC.concat(scene["K"], scene["uv"], scene["X"], order)


def _batch(K, uv, X, **kw):
    from onepose_plus_plus_amd.pose import loransac_PnP_batch
    return loransac_PnP_batch(K, uv, X, pnp_reprojection_error=THR, **kw)


def _same_as_single(r, i, ref):
    """sample i of the batch result r against ransac_PnP_ex's dict"""
    assert r["pose"][i].dtype == np.float64 and r["pose"][i].tobytes() == ref["pose"].tobytes()
    assert bool(r["state"][i]) == ref["state"] and int(r["stop"][i]) == ref["stop"]
    if ref["state"]:
        assert r["inliers"][i].dtype == np.int32 and r["inliers"][i].shape == (len(ref["inliers"]), 1)
        assert np.array_equal(r["inliers"][i][:, 0], ref["inliers"])
    else:
        assert r["inliers"][i].dtype == bool and r["inliers"][i].size == 0
        assert np.array_equal(r["pose"][i], np.eye(4)[:3])
    assert np.array_equal(r["pose_homo"][i], np.concatenate([r["pose"][i], [[0.0, 0.0, 0.0, 1.0]]]))


def _same_results(a, b):
    assert a["pose"].tobytes() == b["pose"].tobytes() and a["pose_homo"].tobytes() == b["pose_homo"].tobytes()
    assert np.array_equal(a["state"], b["state"]) and np.array_equal(a["stop"], b["stop"])
    assert torch.equal(a["pose_dev"], b["pose_dev"])
    assert all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a["inliers"], b["inliers"]))


@pytest.mark.parametrize("setting", list(BC.SETTINGS))
def test_every_sample_equals_the_single_call(scene, setting):
    kw = BC.SETTINGS[setting]
    singles = scene["singles"][setting]
    stops = [s["stop"] for s in singles]
    print(setting, "single-call stops", stops, "states", [s["state"] for s in singles], "inliers", [len(s["inliers"]) for s in singles])
    if setting == "two_pass":            # both branches of the second pass in one batch: a sample that runs it, one that skips it
        assert any(s > kw["min_trials"] for s in stops) and stops[0] > kw["min_trials"]
        assert any(s == kw["min_trials"] for s in stops)
    if setting == "one_pass":
        assert all(s == kw["iterations"] for s, n in zip(stops, SIZES) if n >= 3)
    K, uv, X, off, seeds = _concat(scene, range(B))
    r = _batch(K, uv, X, offsets=off, seed=seeds, **kw)
    assert r["pose"].shape == (B, 3, 4) and r["pose_homo"].shape == (B, 4, 4) and r["state"].shape == (B,) and r["state"].dtype == bool
    assert len(r["inliers"]) == B and len(r["stop"]) == B
    assert r["pose_dev"].is_cuda and r["pose_dev"].dtype == torch.float64 and r["pose_dev"].shape == (B, 3, 4)
    assert np.array_equal(r["pose_dev"].cpu().numpy(), r["pose"])
    for b in range(B):
        _same_as_single(r, b, singles[b])
    for b, n in enumerate(SIZES):
        if n < 3:                                                 # the failure convention: identity, no inliers, state False, stop 0
            assert not r["state"][b] and r["stop"][b] == 0 and np.array_equal(r["pose"][b], np.eye(4)[:3]) and r["inliers"][b].size == 0
        assert n < 70 or r["state"][b]


def test_position_and_chunking_do_not_matter(scene):
    kw = BC.SETTINGS["two_pass"]
    singles = scene["singles"]["two_pass"]
    order = list(range(B))[::-1]
    K, uv, X, off, seeds = _concat(scene, order)
    r = _batch(K, uv, X, offsets=off, seed=seeds, **kw)
    for i, b in enumerate(order):
        _same_as_single(r, i, singles[b])
    K, uv, X, off, seeds = _concat(scene, [0])                    # sample 0 alone, B = 1
    r = _batch(K, uv, X, offsets=off, seed=seeds[0], batch_size=1, **kw)
    _same_as_single(r, 0, singles[0])
    K, uv, X, off, seeds = _concat(scene, range(B))
    one = _batch(K, uv, X, offsets=off, seed=seeds, **kw)
    for max_batch in (3, 1):                                      # chunks of 3, 3, 2 and of one sample each
        _same_results(_batch(K, uv, X, offsets=off, seed=seeds, max_batch=max_batch, **kw), one)


def test_m_bids_offsets_and_host_inputs_agree(scene):
    from onepose_plus_plus_amd.pose import BatchIdsError
    kw = BC.SETTINGS["two_pass"]
    K, uv, X, off, seeds = _concat(scene, range(B))
    ids = torch.from_numpy(np.repeat(np.arange(B), SIZES).astype(np.int64)).cuda()
    uv_d, X_d = torch.from_numpy(uv).cuda(), torch.from_numpy(X).cuda()
    a = _batch(K, uv_d, X_d, m_bids=ids, seed=seeds, **kw)
    _same_results(_batch(K, uv_d, X_d, offsets=torch.from_numpy(off).cuda(), seed=seeds, **kw), a)
    _same_results(_batch(K, uv, X, offsets=off, seed=seeds, **kw), a)                         # host inputs
    _same_results(_batch(K, uv, X, m_bids=ids.cpu().numpy(), seed=seeds, max_batch=5, **kw), a)
    for b in range(B):
        _same_as_single(a, b, scene["singles"]["two_pass"][b])
    bad = ids.clone()
    bad[10], bad[11] = 1, 0                                       # a decreasing pair
    with pytest.raises(BatchIdsError):
        _batch(K, uv_d, X_d, m_bids=bad, seed=seeds, **kw)
    with pytest.raises(ValueError):
        _batch(K, uv_d, X_d, m_bids=ids, offsets=off, **kw)
    with pytest.raises(ValueError):
        _batch(K, uv_d, X_d, **kw)
    Kbad = K.copy()
    Kbad[3, 0, 0] = 0.0
    with pytest.raises(ValueError, match="focal"):
        _batch(Kbad, uv_d, X_d, m_bids=ids, seed=seeds, **kw)


def test_simple_pinhole_switch():
    """K[b] with fx != fy: each setting equals the single call with the same setting, and the two differ"""
    from onepose_plus_plus_amd.pose import ransac_PnP_ex
    rng = np.random.default_rng(61)
    Ks, uvs, Xs = [], [], []
    for n in (120, 60):
        K, uv, X, R, t, _ = _scene(rng, n, 0.2, 0.3)
        assert K[0, 0] != K[1, 1]
        Ks.append(K)
        uvs.append(uv.astype(np.float32))
        Xs.append(X.astype(np.float32))
    K, uv, X, off = np.stack(Ks), np.concatenate(uvs), np.concatenate(Xs), np.array([0, 120, 180], np.int32)
    kw = dict(iterations=600, min_trials=200)
    res = {}
    for simple in (True, False):
        res[simple] = _batch(K, uv, X, offsets=off, seed=(3, 4), simple_pinhole=simple, **kw)
        for b in range(2):
            ref = ransac_PnP_ex(K[b], uvs[b], Xs[b], seed=3 + b, solver="loransac", pnp_reprojection_error=THR, simple_pinhole=simple, **kw)
            _same_as_single(res[simple], b, ref)
    assert res[True]["state"].all() and res[False]["state"].all()
    assert all(res[True]["pose"][b].tobytes() != res[False]["pose"][b].tobytes() for b in range(2))


def _raw(scene, n_samples=None, ws_short=0, iterations=1500, min_trials=300):
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    K, uv, X, off, seeds = _concat(scene, range(B))
    n = len(uv)
    p2, p3 = torch.from_numpy(uv).to(dev), torch.from_numpy(X).to(dev)
    off_d = torch.from_numpy(off).to(dev)
    K4 = torch.from_numpy(np.ascontiguousarray(np.stack([K[:, 0, 0], K[:, 0, 0], K[:, 0, 2], K[:, 1, 2]], 1))).to(dev)
    seeds_d = torch.tensor(seeds, dtype=torch.int32, device=dev)
    pose = torch.full((B, 12), float("nan"), dtype=torch.float64, device=dev)
    mask = torch.full((n,), 7, dtype=torch.int32, device=dev)
    cnt = torch.full((3, B), -5, dtype=torch.int32, device=dev)
    nbytes = lib.opp_pnp_loransac_batch_workspace_bytes(max(iterations, 1), B, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = lib.opp_pnp_loransac_batch(p2.data_ptr(), p3.data_ptr(), off_d.data_ptr(), B if n_samples is None else n_samples, n, K4.data_ptr(),
                                    seeds_d.data_ptr(), THR, iterations, 0.9999, min_trials, 0.01, pose.data_ptr(), mask.data_ptr(),
                                    cnt[0].data_ptr(), cnt[1].data_ptr(), cnt[2].data_ptr(), ws.data_ptr(), nbytes - ws_short,
                                    torch.cuda.current_stream().cuda_stream)
    err = lib.opp_last_error()
    torch.cuda.synchronize()
    return rc, err, pose.cpu().numpy(), mask.cpu().numpy(), cnt.cpu().numpy(), off


def test_raw_abi_outputs(scene):
    rc, _, pose, mask, cnt, off = _raw(scene)
    assert rc == 0
    assert np.isin(mask, (0, 1)).all()                            # every entry written, failed segments included
    eye = np.eye(4)[:3].reshape(-1)
    for b, n in enumerate(SIZES):
        seg = mask[off[b]:off[b + 1]]
        assert seg.sum() == cnt[0, b]
        assert cnt[1, b] in (0, 1) and (n >= 3 or cnt[1, b] == 0) and (n < 70 or cnt[1, b] == 1)
        if cnt[1, b] == 0:                                        # a failed sample: identity, no inliers
            assert np.array_equal(pose[b], eye) and cnt[0, b] == 0 and not seg.any()
        else:
            assert np.isfinite(pose[b]).all()
        assert cnt[2, b] == scene["singles"]["two_pass"][b]["stop"] and (n >= 3 or cnt[2, b] == 0)
        assert pose[b].tobytes() == scene["singles"]["two_pass"][b]["pose"].tobytes()


def test_raw_abi_refusals(scene):
    rc, err, pose, mask, cnt, _ = _raw(scene, ws_short=1)
    assert rc != 0 and b"workspace" in err
    assert np.isnan(pose).all() and (mask == 7).all() and (cnt == -5).all()      # nothing was launched
    for kwargs in ({"n_samples": 0}, {"n_samples": 1025}, {"iterations": 0}, {"min_trials": -1}):
        rc, err, pose, mask, cnt, _ = _raw(scene, **kwargs)
        assert rc != 0 and err, kwargs
        assert np.isnan(pose).all() and (mask == 7).all() and (cnt == -5).all(), kwargs


def _planted(rng, n, K, pose):
    X = rng.uniform(-0.1, 0.1, size=(n, 3))
    Xc = X @ pose[:, :3].T + pose[:, 3]
    uv = np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[0, 0] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], 1)     # SIMPLE_PINHOLE: fx on both axes
    return X.astype(np.float32), uv.astype(np.float32)


def test_compute_query_pose_errors_opt_in(monkeypatch):
    """B = 3, the middle sample with 2 matches (it fails): `batch_loransac=True` against the per-sample loop, forced by passing
    the single-sample function as `ransac_PnP=`; the per-sample estimator is patched to raise, so the batch pass alone ran"""
    import onepose_plus_plus_amd.pose as pose_mod
    from onepose_plus_plus_amd.metrics import compute_query_pose_errors
    single = pose_mod.ransac_PnP
    rng = np.random.default_rng(5)
    K = PC.intrinsics()
    gts = np.stack([np.concatenate([PC.gt_pose(rng), [[0.0, 0.0, 0.0, 1.0]]]) for _ in range(3)])
    sizes = (200, 2, 150)
    Xs, uvs = zip(*[_planted(rng, n, K, gts[b, :3]) for b, n in enumerate(sizes)])
    base = {"m_bids": torch.from_numpy(np.repeat(np.arange(3), sizes)).cuda(), "mkpts_3d_db": torch.from_numpy(np.concatenate(Xs)).cuda(),
            "mkpts_query_f": torch.from_numpy(np.concatenate(uvs)).cuda(), "q_hw_i": (480, 640),
            "query_image_scale": torch.ones(3, 2), "query_intrinsic": torch.from_numpy(np.stack([K] * 3)),
            "query_pose_gt": torch.from_numpy(gts)}
    configs = {"point_cloud_rescale": 1000, "pnp_reprojection_error": 3.3, "use_pycolmap_ransac": True, "model_unit": "m"}

    def boom(*a, **k):
        raise RuntimeError("the per-sample estimator was called")

    monkeypatch.setattr(pose_mod, "ransac_PnP", boom)
    for solver, extra in (("loransac", {}), ("auto", {}), ("loransac", {"min_trials": 200, "min_inlier_ratio": 0.05, "refine_iters": 3})):
        got, ref = dict(base), dict(base)
        compute_query_pose_errors(got, configs, solver=solver, iterations=1500, seed=4, batch_loransac=True, **extra)
        compute_query_pose_errors(ref, configs, solver=solver, iterations=1500, seed=4, ransac_PnP=single, **extra)
        assert isinstance(got["pose_pred"], np.ndarray) and got["pose_pred"].shape == (3, 4, 4)
        assert got["pose_pred"].dtype == ref["pose_pred"].dtype and got["pose_pred"].tobytes() == ref["pose_pred"].tobytes()
        for k in ("R_errs", "t_errs"):
            assert len(got[k]) == 3 and got[k] == ref[k], k
        for a, b in zip(got["inliers"], ref["inliers"]):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
        assert got["R_errs_c"] == [] and got["t_errs_c"] == [] and got["inliers_c"] == []
        assert got["R_errs"][1] == np.inf and got["t_errs"][1] == np.inf
        assert got["inliers"][1].dtype == bool and got["inliers"][1].size == 0 and np.array_equal(got["pose_pred"][1], np.eye(4))
        assert got["R_errs"][0] < 0.05 and got["t_errs"][2] < 0.05 and len(got["inliers"][0]) >= 190
    with pytest.raises(RuntimeError, match="per-sample estimator"):          # without the keyword LO-RANSAC still loops
        compute_query_pose_errors(dict(base), configs, solver="loransac")
    with pytest.raises(RuntimeError, match="per-sample estimator"):
        compute_query_pose_errors(dict(base), configs, solver="loransac", batch_loransac=False)


def test_two_calls_return_the_same_bytes(scene):
    K, uv, X, off, seeds = _concat(scene, range(B))
    for kw in BC.SETTINGS.values():
        _same_results(_batch(K, uv, X, offsets=off, seed=seeds, **kw), _batch(K, uv, X, offsets=off, seed=seeds, **kw))


def test_large_samples_recover_the_ground_truth(scene):
    """a sanity check only, with the bounds of test_loransac_gpu.py::test_loransac_recovers_pose: at least 85 % of the true
    inliers found, at most 5 % of n + 2 others, and on the clean sample a pose within 1e-6 degrees and 1e-6 cm"""
    K, uv, X, off, seeds = _concat(scene, range(B))
    r = _batch(K, uv, X, offsets=off, seed=seeds, **BC.SETTINGS["defaults"])
    checked = 0
    for b, n in enumerate(SIZES):
        if n >= 70:
            R, t, out_idx = scene["gt"][b]
            inl = set(r["inliers"][b][:, 0].tolist())
            true_in = set(range(n)) - set(out_idx.tolist())
            ang, tcm = _errs(r["pose"][b], R, t)
            print("sample %d (n = %d, %.0f %% outliers): %d inliers, %d of the %d true ones, %.3g deg, %.3g cm"
                  % (b, n, 100 * BC.OUTLIERS[b], len(inl), len(inl & true_in), len(true_in), ang, tcm))
            assert r["state"][b] and len(inl & true_in) >= 0.85 * len(true_in) and len(inl - true_in) <= 0.05 * n + 2
            if BC.NOISE[b] == 0 and BC.OUTLIERS[b] == 0:
                assert ang < 1e-6 and tcm < 1e-6, (ang, tcm)
            checked += 1
    assert checked == 3
