"""GPU: the batched PnP-RANSAC (csrc/pnp_batch.hip through opp_pnp_ransac_batch / pose.ransac_PnP_batch) against the
single-sample call on each sample's slice -- byte for byte -- on one batch whose sizes hit every device-side branch:
n = 700 (more than one 256-thread chunk per point loop), 0 (empty, between non-empty ones), 3 (failure), 4 (EPnP's switch to
P3P), 5 (EPnP's single solve), 6 (the first sampled size), 120.  The single-sample results are computed once per module."""
import ctypes

import numpy as np
import pytest
import torch

from tests.golden import pose_metrics_cases as C
from tests.test_epnp_gpu import _errs
from tests.test_pnp_gpu import _scene

pytestmark = pytest.mark.gpu

SIZES = (700, 0, 3, 4, 5, 6, 120)
SEEDS = (9, 9, 1, 2, 3, 4, 5)
SCALE = 1000
THR = 3.3
ITERS = 1500
SOLVERS = ("p3p", "epnp")
KW = dict(scale=SCALE, pnp_reprojection_error=THR, iterations=ITERS)


def _make_batch():
    rng = np.random.default_rng(77)
    Ks, uvs, Xs, gts = [], [], [], []
    for b, n in enumerate(SIZES):
        K0, uv, X, R, t, _ = _scene(rng, max(n, 1), 0.4 if n >= 6 else 0.0, 0.5 if n >= 6 else 0.0)
        K = K0.copy()                                  # a different camera per sample: remap the pixels of the scene's K0 to it
        K[0, 0] += 11.0 * b
        K[1, 1] -= 7.0 * b
        K[0, 2] += 3.0 * b
        K[1, 2] -= 2.0 * b
        uv = np.stack([(uv[:, 0] - K0[0, 2]) / K0[0, 0] * K[0, 0] + K[0, 2], (uv[:, 1] - K0[1, 2]) / K0[1, 1] * K[1, 1] + K[1, 2]], 1)
        Ks.append(K)
        uvs.append(uv[:n].astype(np.float32))
        Xs.append(X[:n].astype(np.float32))
        gts.append((R, t))
    return np.stack(Ks), uvs, Xs, gts


@pytest.fixture(scope="module")
def scene():
    """the batch, and per (solver, confidence) the single-sample results on each sample's slice; computed once, never modified"""
    from onepose_plus_plus_amd.pose import ransac_PnP_ex
    Ks, uvs, Xs, gts = _make_batch()
    singles = {}
    for solver in SOLVERS:
        for conf in (1.0, None, 0.99):
            singles[solver, conf] = [ransac_PnP_ex(Ks[b], uvs[b], Xs[b], seed=SEEDS[b], solver=solver, confidence=conf, **KW)
                                     for b in range(len(SIZES))]
    return {"K": Ks, "uv": uvs, "X": Xs, "gt": gts, "singles": singles}


def _concat(scene, order):
    uv = np.concatenate([scene["uv"][b] for b in order]).reshape(-1, 2)
    X = np.concatenate([scene["X"][b] for b in order]).reshape(-1, 3)
    off = np.concatenate([[0], np.cumsum([SIZES[b] for b in order])]).astype(np.int32)
    return scene["K"][list(order)], uv, X, off, tuple(SEEDS[b] for b in order)


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


@pytest.mark.parametrize("conf", [1.0, None, 0.99])
@pytest.mark.parametrize("solver", SOLVERS)
def test_every_sample_equals_the_single_call(scene, solver, conf):
    from onepose_plus_plus_amd.pose import ransac_PnP, ransac_PnP_batch
    B = len(SIZES)
    K, uv, X, off, seeds = _concat(scene, range(B))
    r = ransac_PnP_batch(K, uv, X, offsets=off, seed=seeds, solver=solver, confidence=conf, **KW)
    assert r["pose"].shape == (B, 3, 4) and r["pose_homo"].shape == (B, 4, 4) and r["state"].shape == (B,) and r["state"].dtype == bool
    assert len(r["inliers"]) == B and len(r["stop"]) == B
    assert r["pose_dev"].is_cuda and r["pose_dev"].dtype == torch.float64 and np.array_equal(r["pose_dev"].cpu().numpy(), r["pose"])
    for b in range(B):
        _same_as_single(r, b, scene["singles"][solver, conf][b])
    for b, n in enumerate(SIZES):
        assert n >= 4 or not r["state"][b]                        # fewer than 4 matches: the failure convention
        assert n < 100 or r["state"][b]
    if solver == "p3p" and conf == 0.99:                          # pnp_batch_stop_kernel with an early stop on the P3P path
        assert any(int(r["stop"][b]) < ITERS for b in range(B) if SIZES[b] >= 4)
    if solver == "p3p" and conf is None:                          # the default path against ransac_PnP's tuple
        for b in range(B):
            pose, homo, inl, ok = ransac_PnP(scene["K"][b], scene["uv"][b], scene["X"][b], seed=SEEDS[b], **KW)
            assert ok == bool(r["state"][b]) and pose.tobytes() == r["pose"][b].tobytes() and np.array_equal(homo, r["pose_homo"][b])
            assert inl.dtype == r["inliers"][b].dtype and np.array_equal(inl, r["inliers"][b])


@pytest.mark.parametrize("solver", SOLVERS)
def test_order_and_neighbours_do_not_matter(scene, solver):
    from onepose_plus_plus_amd.pose import ransac_PnP_batch
    B = len(SIZES)
    order = list(range(B))[::-1]
    K, uv, X, off, seeds = _concat(scene, order)
    r = ransac_PnP_batch(K, uv, X, offsets=off, seed=seeds, solver=solver, **KW)
    for i, b in enumerate(order):
        _same_as_single(r, i, scene["singles"][solver, None][b])
    K, uv, X, off, seeds = _concat(scene, [0])                    # sample 0 alone, B = 1
    r = ransac_PnP_batch(K, uv, X, offsets=off, seed=seeds[0], solver=solver, batch_size=1, **KW)
    _same_as_single(r, 0, scene["singles"][solver, None][0])


def test_m_bids_and_offsets_agree(scene):
    from onepose_plus_plus_amd.pose import ransac_PnP_batch
    B = len(SIZES)
    K, uv, X, off, seeds = _concat(scene, range(B))
    ids = torch.from_numpy(np.repeat(np.arange(B), SIZES).astype(np.int64)).cuda()
    uv_d, X_d = torch.from_numpy(uv).cuda(), torch.from_numpy(X).cuda()
    for solver in SOLVERS:
        a = ransac_PnP_batch(K, uv_d, X_d, m_bids=ids, seed=seeds, solver=solver, **KW)
        b = ransac_PnP_batch(K, uv_d, X_d, offsets=torch.from_numpy(off).cuda(), seed=seeds, solver=solver, **KW)
        c = ransac_PnP_batch(K, uv, X, offsets=off, seed=seeds, solver=solver, **KW)          # host inputs
        for r in (b, c):
            assert a["pose"].tobytes() == r["pose"].tobytes() and np.array_equal(a["state"], r["state"])
            assert np.array_equal(a["stop"], r["stop"])
            assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a["inliers"], r["inliers"]))
    bad = ids.clone()
    bad[10], bad[11] = 1, 0                                       # a decreasing pair
    with pytest.raises(ValueError):
        ransac_PnP_batch(K, uv_d, X_d, m_bids=bad, seed=seeds, **KW)
    with pytest.raises(ValueError):
        ransac_PnP_batch(K, uv_d, X_d, m_bids=ids, offsets=off, **KW)
    with pytest.raises(NotImplementedError, match="ransac_PnP"):
        ransac_PnP_batch(K, uv_d, X_d, m_bids=ids, solver="loransac", **KW)
    with pytest.raises(NotImplementedError, match="ransac_PnP"):
        ransac_PnP_batch(K, uv_d, X_d, m_bids=ids, solver="auto", use_pycolmap_ransac=True, **KW)


def _raw(scene, solver, n_samples=None, ws_short=0, iterations=ITERS):
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    B = len(SIZES)
    K, uv, X, off, seeds = _concat(scene, range(B))
    n = len(uv)
    p2, p3 = torch.from_numpy(uv).to(dev), torch.from_numpy(X).to(dev)
    off_d = torch.from_numpy(off).to(dev)
    K4 = torch.from_numpy(np.ascontiguousarray(np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], 1))).to(dev)
    seeds_d = torch.tensor(seeds, dtype=torch.int32, device=dev)
    pose = torch.full((B, 12), float("nan"), dtype=torch.float64, device=dev)
    mask = torch.full((n,), 7, dtype=torch.int32, device=dev)
    cnt = torch.full((3, B), -5, dtype=torch.int32, device=dev)
    nbytes = lib.opp_pnp_batch_workspace_bytes(iterations, B, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = lib.opp_pnp_ransac_batch(p2.data_ptr(), p3.data_ptr(), off_d.data_ptr(), B if n_samples is None else n_samples, n, K4.data_ptr(),
                                  seeds_d.data_ptr(), THR, float(SCALE), iterations, 8, solver, 0.99, pose.data_ptr(), mask.data_ptr(),
                                  cnt[0].data_ptr(), cnt[1].data_ptr(), cnt[2].data_ptr(), ws.data_ptr(), nbytes - ws_short,
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, pose.cpu().numpy(), mask.cpu().numpy(), cnt.cpu().numpy(), off


@pytest.mark.parametrize("solver", [0, 1])
def test_raw_abi_outputs(scene, solver):
    rc, pose, mask, cnt, off = _raw(scene, solver)
    assert rc == 0
    assert np.isin(mask, (0, 1)).all()                            # every entry written, failed segments included
    eye = np.eye(4)[:3].reshape(-1)
    for b, n in enumerate(SIZES):
        seg = mask[off[b]:off[b + 1]]
        assert seg.sum() == cnt[0, b]
        assert cnt[1, b] in (0, 1) and (n >= 4 or cnt[1, b] == 0) and (n < 100 or cnt[1, b] == 1)
        if cnt[1, b] == 0:                                        # a failed sample: identity, no inliers
            assert np.array_equal(pose[b], eye) and cnt[0, b] == 0 and not seg.any()
        else:
            assert np.isfinite(pose[b]).all()
    assert (cnt[2] >= 0).all() and (cnt[2] <= ITERS).all()


def test_raw_abi_refusals(scene):
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    rc, pose, mask, cnt, _ = _raw(scene, 0, ws_short=1)
    assert rc != 0 and b"workspace" in lib.opp_last_error()
    assert np.isnan(pose).all() and (mask == 7).all() and (cnt == -5).all()      # nothing was launched
    for kwargs in ({"n_samples": 0}, {"n_samples": 1025}, {"solver": 2}, {"iterations": 0}):
        args = {"solver": 0}
        args.update(kwargs)
        rc, pose, mask, cnt, _ = _raw(scene, args.pop("solver"), **args)
        assert rc != 0 and lib.opp_last_error(), kwargs
        assert np.isnan(pose).all() and (mask == 7).all()


@pytest.mark.parametrize("solver", SOLVERS)
def test_large_samples_recover_the_ground_truth(scene, solver):
    """a sanity check only, with the bounds of test_epnp_gpu.py::test_epnp_recovers_pose for noisy scenes"""
    from onepose_plus_plus_amd.pose import ransac_PnP_batch
    B = len(SIZES)
    K, uv, X, off, seeds = _concat(scene, range(B))
    r = ransac_PnP_batch(K, uv, X, offsets=off, seed=seeds, solver=solver, **KW)
    checked = 0
    for b, n in enumerate(SIZES):
        if n >= 100:
            R, t = scene["gt"][b]
            ang, tcm = _errs(r["pose"][b], R, t)
            assert ang < 0.8 and tcm < 1.0, (b, ang, tcm)
            checked += 1
    assert checked == 2


def _planted(rng, n, K, pose):
    X = rng.uniform(-0.1, 0.1, size=(n, 3))
    Xc = X @ pose[:, :3].T + pose[:, 3]
    uv = np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], 1)
    return X.astype(np.float32), uv.astype(np.float32)


def test_compute_query_pose_errors_goes_through_the_batch(monkeypatch):
    """B = 3, the middle sample with 2 matches (it fails): the batch call inside compute_query_pose_errors against the
    per-sample loop, forced by passing the single-sample function as `ransac_PnP=`"""
    import onepose_plus_plus_amd.pose as pose_mod
    from onepose_plus_plus_amd.metrics import compute_query_pose_errors
    single = pose_mod.ransac_PnP
    rng = np.random.default_rng(5)
    K = C.intrinsics()
    gts = np.stack([np.concatenate([C.gt_pose(rng), [[0.0, 0.0, 0.0, 1.0]]]) for _ in range(3)])
    sizes = (200, 2, 150)
    Xs, uvs = zip(*[_planted(rng, n, K, gts[b, :3]) for b, n in enumerate(sizes)])
    base = {"m_bids": torch.from_numpy(np.repeat(np.arange(3), sizes)).cuda(), "mkpts_3d_db": torch.from_numpy(np.concatenate(Xs)).cuda(),
            "mkpts_query_f": torch.from_numpy(np.concatenate(uvs)).cuda(), "q_hw_i": (480, 640),
            "query_image_scale": torch.ones(3, 2), "query_intrinsic": torch.from_numpy(np.stack([K] * 3)),
            "query_pose_gt": torch.from_numpy(gts)}
    configs = {"point_cloud_rescale": 1000, "pnp_reprojection_error": 3.3, "use_pycolmap_ransac": False, "model_unit": "m"}

    def boom(*a, **k):
        raise RuntimeError("the per-sample estimator was called")

    monkeypatch.setattr(pose_mod, "ransac_PnP", boom)
    for solver in SOLVERS:
        got, ref = dict(base), dict(base)
        compute_query_pose_errors(got, configs, solver=solver, iterations=ITERS, seed=4)
        compute_query_pose_errors(ref, configs, solver=solver, iterations=ITERS, seed=4, ransac_PnP=single)
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
    with pytest.raises(RuntimeError, match="per-sample estimator"):          # LO-RANSAC still loops
        compute_query_pose_errors(dict(base), configs, solver="loransac")
    with pytest.raises(RuntimeError, match="per-sample estimator"):
        compute_query_pose_errors(dict(base), dict(configs, use_pycolmap_ransac=True), solver="auto")


def test_compute_query_pose_errors_with_unordered_ids_falls_back_to_the_loop():
    """ids that are not in the matcher's order: the batch pass is discarded with a warning and the per-sample loop, which
    selects by `m_bids == b`, gives what it gave before"""
    import onepose_plus_plus_amd.pose as pose_mod
    from onepose_plus_plus_amd.metrics import compute_query_pose_errors
    rng = np.random.default_rng(6)
    K = C.intrinsics()
    gts = np.stack([np.concatenate([C.gt_pose(rng), [[0.0, 0.0, 0.0, 1.0]]]) for _ in range(2)])
    sizes = (120, 90)
    Xs, uvs = zip(*[_planted(rng, n, K, gts[b, :3]) for b, n in enumerate(sizes)])
    perm = rng.permutation(sum(sizes))
    ids = np.repeat(np.arange(2), sizes)[perm]
    assert (np.diff(ids) < 0).any()
    base = {"m_bids": torch.from_numpy(ids).cuda(), "mkpts_3d_db": torch.from_numpy(np.concatenate(Xs)[perm]).cuda(),
            "mkpts_query_f": torch.from_numpy(np.concatenate(uvs)[perm]).cuda(), "q_hw_i": (480, 640),
            "query_image_scale": torch.ones(2, 2), "query_intrinsic": torch.from_numpy(np.stack([K] * 2)),
            "query_pose_gt": torch.from_numpy(gts)}
    configs = {"point_cloud_rescale": 1000, "pnp_reprojection_error": 3.3, "use_pycolmap_ransac": False, "model_unit": "m"}
    got, ref = dict(base), dict(base)
    with pytest.warns(RuntimeWarning, match="per sample"):
        compute_query_pose_errors(got, configs, iterations=ITERS, seed=4)
    compute_query_pose_errors(ref, configs, iterations=ITERS, seed=4, ransac_PnP=pose_mod.ransac_PnP)
    assert got["pose_pred"].tobytes() == ref["pose_pred"].tobytes() and got["R_errs"] == ref["R_errs"] and got["t_errs"] == ref["t_errs"]
    assert all(np.array_equal(a, b) for a, b in zip(got["inliers"], ref["inliers"]))
    assert max(got["R_errs"]) < 0.05 and max(got["t_errs"]) < 0.05
    assert all(len(i) >= 0.95 * n for i, n in zip(got["inliers"], sizes))


def test_raw_single_call_takes_zero_matches_as_the_failure():
    """opp_pnp_ransac with n_points = 0 and the null pointers of an empty tensor: the n < 4 failure, not an argument error"""
    from onepose_plus_plus_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    K4 = (ctypes.c_double * 4)(560.0, 555.0, 256.0, 250.0)
    pose = torch.full((12,), float("nan"), dtype=torch.float64, device=dev)
    mask = torch.full((1,), 7, dtype=torch.int32, device=dev)
    cnt = torch.full((2,), -5, dtype=torch.int32, device=dev)
    nbytes = lib.opp_pnp_workspace_bytes(ITERS)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = lib.opp_pnp_ransac(None, None, 0, K4, THR, float(SCALE), ITERS, 1, 8, pose.data_ptr(), mask.data_ptr(), cnt.data_ptr(),
                            cnt.data_ptr() + 4, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.opp_last_error()
    assert np.array_equal(pose.cpu().numpy(), np.eye(4)[:3].reshape(-1)) and cnt.cpu().tolist() == [0, 0] and mask.item() == 7
    rc = lib.opp_pnp_ransac(None, None, 5, K4, THR, float(SCALE), ITERS, 1, 8, pose.data_ptr(), mask.data_ptr(), cnt.data_ptr(),
                            cnt.data_ptr() + 4, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"null" in lib.opp_last_error()          # matches without an address are still refused


def test_two_calls_return_the_same_bytes(scene):
    from onepose_plus_plus_amd.pose import ransac_PnP_batch
    K, uv, X, off, seeds = _concat(scene, range(len(SIZES)))
    for solver in SOLVERS:
        a = ransac_PnP_batch(K, uv, X, offsets=off, seed=seeds, solver=solver, **KW)
        b = ransac_PnP_batch(K, uv, X, offsets=off, seed=seeds, solver=solver, **KW)
        assert a["pose"].tobytes() == b["pose"].tobytes() and np.array_equal(a["stop"], b["stop"]) and np.array_equal(a["state"], b["state"])
        assert all(np.array_equal(x, y) for x, y in zip(a["inliers"], b["inliers"]))


@pytest.mark.parametrize("solver", ["p3p", "epnp", "loransac"])
def test_the_three_front_doors_agree_with_the_batch_at_one_sample(solver):
    """ransac_PnP's tuple, ransac_PnP_ex's dict and sample 0 of the solver's batch call at B = 1, byte for byte in pose, inliers
    and state: the single calls share one Python helper, the batch path does not.  n = 70 carries 30 % outliers and 0.5 px noise
    and every solver succeeds on it; below the solver's minimum (4 matches, 3 for "loransac") every door reports the failure."""
    from onepose_plus_plus_amd.pose import loransac_PnP_batch, ransac_PnP, ransac_PnP_batch, ransac_PnP_ex
    rng = np.random.default_rng(2024)
    kw = dict(pnp_reprojection_error=THR, iterations=500, seed=3)
    for n in (0, 3, 4, 5, 6, 70):
        K, uv, X = _scene(rng, max(n, 1), 0.3 if n == 70 else 0.0, 0.5 if n == 70 else 0.0)[:3]
        uv[:, 1] = (uv[:, 1] - K[1, 2]) / K[1, 1] * K[0, 0] + K[1, 2]     # one focal length: "loransac" puts fx on both axes
        K[1, 1] = K[0, 0]
        uv, X = uv[:n].astype(np.float32), X[:n].astype(np.float32)
        pose, homo, inl, ok = ransac_PnP(K, uv, X, solver=solver, **kw)
        ex = ransac_PnP_ex(K, uv, X, solver=solver, **kw)
        if solver == "loransac":
            r = loransac_PnP_batch(K[None], uv, X, offsets=[0, n], **kw)
        else:
            r = ransac_PnP_batch(K[None], uv, X, offsets=[0, n], solver=solver, **kw)
        assert ok is ex["state"] and ok == bool(r["state"][0]), n
        assert pose.dtype == np.float64 and pose.tobytes() == r["pose"][0].tobytes(), n
        assert homo.tobytes() == r["pose_homo"][0].tobytes(), n
        assert inl.dtype == r["inliers"][0].dtype and inl.shape == r["inliers"][0].shape and np.array_equal(inl, r["inliers"][0]), n
        _same_as_single(r, 0, ex)
        if n == 70:
            assert ok and len(inl) >= 40, n        # 49 matches carry noise alone, 0.5 px against a 3.3 px threshold
        if n < (3 if solver == "loransac" else 4):
            assert not ok and np.array_equal(pose, np.eye(4)[:3]) and inl.size == 0, n
