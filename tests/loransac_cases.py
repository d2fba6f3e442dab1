"""Shared by tests/test_loransac_cpu.py and tests/test_loransac_gpu.py: the scenes of the LO-RANSAC tests, a numpy copy of the
device's hash sampler, and the replay cases with the seeds chosen for a decision margin >= 1e-6 (checked on the CPU)."""
import ctypes

import numpy as np

from tests.test_pnp_gpu import _scene

THR = 3.3
MARGIN = 1e-6
# (n, outlier fraction, confidence, iterations, scene seed, sampler seed) of the replay against the restatement
REPLAY_CASES = [(120, 0.5, 0.9999, 3000, 21, 5), (60, 0.3, 1.0, 1500, 22, 5), (400, 0.7, 0.9999, 10000, 23, 5)]


def sp_scene(rng, n, outlier_frac, noise_px, planar=False):
    """`tests.test_pnp_gpu._scene` as a SIMPLE_PINHOLE scene: its K has fx != fy, and the reference's pycolmap branch uses
    K[0,0] for both axes, so the v coordinates are rescaled about cy to the focal length fx (and K is returned with fy = fx)"""
    K, uv, X, R, t, out_idx = _scene(rng, n, outlier_frac, noise_px, planar)
    uv = uv.copy()
    uv[:, 1] = (uv[:, 1] - K[1, 2]) * (K[0, 0] / K[1, 1]) + K[1, 2]
    K = K.copy()
    K[1, 1] = K[0, 0]
    return K, uv, X, R, t, out_idx


def f64(uv, X):
    """what the device sees: float32 inputs widened to double (no rescaling of the points)"""
    return uv.astype(np.float32).astype(np.float64), X.astype(np.float32).astype(np.float64)


def _hash32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def draw_sample(seed, h, n, k=3):
    """csrc/pnp_sample.h: draw_sample<k>"""
    s = _hash32(seed ^ ((0x9e3779b9 * (h + 1)) & 0xFFFFFFFF))
    idx = []
    for _ in range(k):
        c = 0
        for _tries in range(64):
            s = _hash32((s + 0x632be5ab) & 0xFFFFFFFF)
            c = s % n
            if c not in idx:
                break
        idx.append(c)
    return idx


def host_trials(lib, LR, X64, uv64, K4, thr, seed, trials):
    """what the hypotheses / scoring kernels produce, on the host: samples, P3P models (host build), numpy supports"""
    dp = ctypes.POINTER(ctypes.c_double)
    K4 = np.ascontiguousarray(K4, dtype=np.float64)
    models = np.zeros((trials, 4, 3, 4))
    counts = np.full((trials, 4), -1, dtype=np.int64)
    sums = np.zeros((trials, 4))
    n = X64.shape[0]
    for t in range(trials):
        idx = draw_sample(seed, t, n)
        if len(set(idx)) < 3:
            continue
        Xs, us, buf = np.ascontiguousarray(X64[idx]), np.ascontiguousarray(uv64[idx]), np.zeros(48)
        ns = lib.t_p3p(Xs.ctypes.data_as(dp), us.ctypes.data_as(dp), K4.ctypes.data_as(dp), buf.ctypes.data_as(dp))
        for m in range(ns):
            p = buf[12 * m:12 * m + 12]
            models[t, m] = np.concatenate([p[:9].reshape(3, 3), p[9:, None]], 1)
            counts[t, m], sums[t, m], _, _ = LR.support(models[t, m], X64, uv64, K4, thr * thr)
    return models, counts, sums
