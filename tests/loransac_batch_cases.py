"""Shared by tests/test_loransac_batch_cpu.py and tests/test_loransac_batch_gpu.py: the one batch whose sizes hit every
device-side branch of the batched LO-RANSAC, and the parameter settings it runs under.  numpy only."""
import numpy as np

from tests import loransac_cases as C

THR = C.THR
# n = 300 with 70 % outliers (its bound after the first pass lies past min_trials: the second pass runs), 0 (empty, between
# non-empty ones), 2 (the failure), 3 (P3P models only, no LO), 4 (LO needs more than 4 inliers), 5, 70 with 40 % outliers (more
# than one 64-lane stride), 130 clean (its bound is min_trials: the second pass is skipped)
SIZES = (300, 0, 2, 3, 4, 5, 70, 130)
OUTLIERS = (0.7, 0.0, 0.0, 0.0, 0.0, 0.0, 0.4, 0.0)
NOISE = (0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5, 0.0)
SEEDS = (5, 9, 1, 2, 3, 4, 6, 7)
SCENE_SEED = 91
# (iterations, min_trials, confidence): the two-pass path; t1 = iterations, a single pass; the defaults
SETTINGS = {"two_pass": dict(iterations=1500, min_trials=300),
            "one_pass": dict(iterations=600, confidence=1.0),
            "defaults": dict(iterations=1500)}


def make_batch():
    """-> K [B,3,3] (a different SIMPLE_PINHOLE camera per sample), uv / X: B float32 arrays, gt: B (R, t, outlier indices)"""
    rng = np.random.default_rng(SCENE_SEED)
    Ks, uvs, Xs, gts = [], [], [], []
    for b, n in enumerate(SIZES):
        K0, uv, X, R, t, out_idx = C.sp_scene(rng, max(n, 30), OUTLIERS[b], NOISE[b])
        K = K0.copy()                                  # remap the pixels of the scene's camera K0 to this sample's
        K[0, 0] = K[1, 1] = K0[0, 0] + 11.0 * b
        K[0, 2] += 3.0 * b
        K[1, 2] -= 2.0 * b
        uv = np.stack([(uv[:, 0] - K0[0, 2]) / K0[0, 0] * K[0, 0] + K[0, 2], (uv[:, 1] - K0[1, 2]) / K0[1, 1] * K[1, 1] + K[1, 2]], 1)
        Ks.append(K)
        uvs.append(uv[:n].astype(np.float32))
        Xs.append(X[:n].astype(np.float32))
        gts.append((R, t, out_idx[out_idx < n]))
    return np.stack(Ks), uvs, Xs, gts


def concat(K, uvs, Xs, order):
    """the samples `order` as one batch call's inputs -> K, uv [M,2], X [M,3], offsets [len(order) + 1], seeds"""
    uv = np.concatenate([uvs[b] for b in order]).reshape(-1, 2)
    X = np.concatenate([Xs[b] for b in order]).reshape(-1, 3)
    off = np.concatenate([[0], np.cumsum([SIZES[b] for b in order])]).astype(np.int32)
    return K[list(order)], uv, X, off, tuple(SEEDS[b] for b in order)
