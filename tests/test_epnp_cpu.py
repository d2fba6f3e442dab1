"""CPU: the EPnP solver shared with the HIP kernels (csrc/pnp_math.h, built for the host with g++) against synthetic
ground truth and the float64 restatement (tests/epnp_reference.py); the 12x12 Jacobi against numpy.linalg.eigh; the
RANSAC stopping rule; the EPnP kernels' code generation; dropin routing of pnp="epnp".  No GPU."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import epnp_reference as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K4 = np.array([560.0, 555.0, 256.0, 250.0])
dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("epnp") / "libepnp_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "epnp_host.cpp")])
    L = ctypes.CDLL(out)
    L.t_epnp.restype = ctypes.c_int
    L.t_stop.restype = ctypes.c_int
    L.t_update_iters.restype = ctypes.c_int
    L.t_update_iters.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int]
    return L


def _p(a):
    return a.ctypes.data_as(dp)


def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def scene(rng, n, zscale=1.0):
    R = random_rotation(rng)
    X = rng.uniform(-150, 150, size=(n, 3))       # millimetres, like the reference's scaled point clouds
    X[:, 2] *= zscale
    t = np.array([rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(500, 1000)])
    Xc = X @ R.T + t
    uv = np.stack([K4[0] * Xc[:, 0] / Xc[:, 2] + K4[2], K4[1] * Xc[:, 1] / Xc[:, 2] + K4[3]], 1)
    return np.ascontiguousarray(X), np.ascontiguousarray(uv), R, t


def host_epnp(lib, X, uv):
    pose, errs = np.zeros(12), np.zeros(3)
    best = lib.t_epnp(_p(X), _p(uv), ctypes.c_int(len(X)), _p(K4), _p(pose), _p(errs))
    R, t = pose[:9].reshape(3, 3), pose[9:]
    return best, np.concatenate([R, t[:, None]], 1), errs


def rot_err(R1, R2):
    # rotation angle of R1^T R2 (radians), from the chord: exact near zero, unlike arccos of the trace
    return 2 * np.arcsin(min(1.0, np.linalg.norm(R1 - R2) / (2 * np.sqrt(2))))


@pytest.mark.parametrize("n", [5, 6, 20, 200])
def test_epnp_noise_free(lib, n):
    rng = np.random.default_rng(n)
    for _ in range(6):
        X, uv, R, t = scene(rng, n)
        best, pose, errs = host_epnp(lib, X, uv)
        assert best in (1, 2, 3)
        assert rot_err(pose[:, :3], R) < 1e-9 and np.abs(pose[:, 3] - t).max() < 1e-9 * np.linalg.norm(t)
        ref, ref_errs = ER.epnp(X, uv, K4)
        assert np.abs(pose - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
        assert np.allclose(errs, ref_errs, rtol=1e-9, atol=1e-12)


def test_epnp_near_planar(lib):
    rng = np.random.default_rng(11)
    for n in (6, 50, 300):
        X, uv, R, t = scene(rng, n, zscale=0.01)
        best, pose, _ = host_epnp(lib, X, uv)
        assert best > 0 and rot_err(pose[:, :3], R) < 1e-6 and np.abs(pose[:, 3] - t).max() < 1e-6 * np.linalg.norm(t)


@pytest.mark.parametrize("kind", ["planar", "collinear", "coincident"])
def test_epnp_degenerate_stays_finite(lib, kind):
    rng = np.random.default_rng(3)
    for n in (5, 12, 100):
        X, uv, R, t = scene(rng, n)
        if kind == "planar":
            X[:, 2] = 0.0
        elif kind == "collinear":
            X = np.outer(rng.uniform(-1, 1, n), [100.0, 40.0, -30.0]) + 5.0
        else:
            X[:] = X[0]
        X = np.ascontiguousarray(X)
        Xc = X @ R.T + t
        uv = np.ascontiguousarray(np.stack([K4[0] * Xc[:, 0] / Xc[:, 2] + K4[2], K4[1] * Xc[:, 1] / Xc[:, 2] + K4[3]], 1))
        best, pose, errs = host_epnp(lib, X, uv)
        assert best == 0 or np.all(np.isfinite(pose))       # a pose, or a reported failure -- never NaN
        assert not np.any(np.isnan(errs))


def test_jacobi12_against_eigh(lib):
    rng = np.random.default_rng(5)
    for trial in range(20):
        # M^T M-like spectra: a cluster near zero (a null space of dimension 1..4) beside large eigenvalues
        k0 = 1 + trial % 4
        lam = np.concatenate([rng.uniform(0, 1e-10, k0), 10.0 ** rng.uniform(-2, 6, 12 - k0)])
        Q, _ = np.linalg.qr(rng.normal(size=(12, 12)))
        A = np.ascontiguousarray((Q * lam) @ Q.T)
        A = 0.5 * (A + A.T)
        ev, V = np.zeros(12), np.zeros(144)
        lib.t_jacobi12(_p(A), _p(ev), _p(V))
        V = V.reshape(12, 12)
        w, U = np.linalg.eigh(A)
        scale = np.abs(w).max()
        assert np.allclose(np.sort(ev), w, rtol=0, atol=1e-13 * scale)
        assert np.abs(V.T @ V - np.eye(12)).max() < 1e-12
        # spanned subspaces of the 4 smallest (EPnP's kernel) and of the rest: principal angles
        o = np.argsort(ev, kind="stable")
        for cols_j, cols_e in ((o[:4], slice(0, 4)), (o[4:], slice(4, 12))):
            if cols_e == slice(0, 4) and w[4] - w[3] < 1e-6 * scale:
                continue
            s = np.linalg.svd(V[:, cols_j].T @ U[:, cols_e], compute_uv=False)
            assert s.min() > 1 - 1e-9
        # the restatement runs the same rotations
        Ar, Vr = ER.jacobi12(A)
        assert np.array_equal(np.diag(Ar), ev) and np.array_equal(Vr, V)


def test_stop_rule_matches_restatement(lib):
    rng = np.random.default_rng(9)
    for trial in range(300):
        iters = int(rng.integers(1, 400))
        n = int(rng.integers(6, 500))
        m = 4 if trial % 5 == 0 else 5
        conf = [0.99, 0.5, 0.999, 1.0][trial % 4]
        hi = int(rng.integers(1, n + 1))
        sc = rng.integers(-1, hi + 1, size=iters).astype(np.int32)
        sc[rng.random(iters) < 0.2] = -1
        best = ctypes.c_int(0)
        stop = lib.t_stop(sc.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), iters, n, m, ctypes.c_double(conf), ctypes.byref(best))
        assert (stop, best.value) == ER.ransac_stop(sc, n, m, conf)
        if conf >= 1.0:
            assert stop == iters
    # OpenCV's RANSACUpdateNumIters at a few points: all inliers stops at once, a degenerate denominator keeps niters
    assert lib.t_update_iters(0.99, 0.0, 5, 10000) == 0 == ER.update_iters(0.99, 0.0, 5, 10000)
    assert lib.t_update_iters(0.99, 1.0, 5, 10000) == 10000 == ER.update_iters(0.99, 1.0, 5, 10000)
    assert lib.t_update_iters(0.99, 0.5, 5, 10000) == 145 == ER.update_iters(0.99, 0.5, 5, 10000)


def test_epnp_kernels_isa():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import tempfile
    import isa_audit
    with tempfile.TemporaryDirectory() as tmp:
        src, rows, err = isa_audit.audit_source("pnp.hip", False, tmp)
        assert rows is not None, err
        text = open(os.path.join(tmp, "pnp.hip.s")).read()
    by = {k: r for k, *r in rows}
    for name in ("pnp_epnp_hypotheses_kernel", "pnp_epnp_final_kernel", "pnp_stop_kernel"):
        ks = [k for k in by if name in k]
        assert len(ks) == 1, (name, list(by))
        vg, ag, sc, water, mfma, pk = by[ks[0]]
        assert sc == 0 and water == 0, (name, sc, water)
        # the metadata as well: the private segment is not an expression over callees there
        meta = text[text.index(".name:           " + ks[0]):]
        assert ".private_segment_fixed_size: 0\n" in meta[:meta.index(".vgpr_count")]


def test_dropin_routes_epnp(monkeypatch):
    import onepose_plus_plus_amd.dropin as dropin
    from onepose_plus_plus_amd import pose
    saved = {k: v for k, v in sys.modules.items() if k == "src" or k.startswith("src.")}
    try:
        for k in saved:
            monkeypatch.delitem(sys.modules, k)
        for name in ("src", "src.utils"):
            m = types.ModuleType(name)
            m.__path__ = []
            monkeypatch.setitem(sys.modules, name, m)
        mu = types.ModuleType("src.utils.metric_utils")
        mu.ransac_PnP = None
        monkeypatch.setitem(sys.modules, "src.utils.metric_utils", mu)
        sys.modules["src.utils"].metric_utils = mu
        done = dropin.install(pnp="epnp", loss=False)
        assert done["src.utils.metric_utils"] == "ransac_PnP (epnp)"
        f = mu.ransac_PnP
        assert f is not pose.ransac_PnP and f.func is pose.ransac_PnP and f.keywords == {"solver": "epnp"}
        dropin.install(pnp=True, loss=False)
        assert mu.ransac_PnP is pose.ransac_PnP
        with pytest.raises(ValueError):
            dropin.install(pnp="dls", loss=False)
    finally:
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[k]
        sys.modules.update(saved)
