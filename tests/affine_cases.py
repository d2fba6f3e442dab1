"""Scenes and the case list of the affine RANSAC tests (tests/test_affine_cpu.py, tests/test_affine_gpu.py).

A scene: source points uniform over a 640 x 480 database image, a random similarity-plus-shear map that puts the image about the
centre of a 1280 x 960 query frame (a corner may leave it: negative coordinates are part of the box test), 0.5 px Gaussian noise on the mapped points, and outliers whose query points are uniform over the frame."""
import numpy as np

REF_HW = (480, 640)
QUERY_HW = (960, 1280)
NOISE_PX = 0.5
THR = 6.0
FALLBACK = (140, -20, 1140, 980)          # the reference's centre +- 500 on a 1280 x 960 frame


def corners_of(hw):
    """the reference's (0,0), (W,0), (0,H), (W,H)"""
    h, w = hw
    return np.array([[0, 0], [w, 0], [0, h], [w, h]], np.float64)


def planted_map(rng):
    th = rng.uniform(-0.6, 0.6)
    s = rng.uniform(0.7, 1.3)
    shear = rng.uniform(-0.15, 0.15)
    L = s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]) @ np.array([[1.0, shear], [0.0, 1.0]])
    centre = np.array([REF_HW[1] / 2.0, REF_HW[0] / 2.0])
    target = np.array([QUERY_HW[1] / 2.0, QUERY_HW[0] / 2.0]) + rng.uniform(-60, 60, 2)
    return np.concatenate([L, (target - L @ centre)[:, None]], axis=1)


def scene(seed, n, outlier_frac):
    """-> (p0 [n,2] float32, p1 [n,2] float32, planted map [2,3], outlier mask [n])"""
    rng = np.random.default_rng(seed)
    M = planted_map(rng)
    p0 = rng.uniform(0, 1, (n, 2)) * np.array([REF_HW[1], REF_HW[0]])
    p1 = p0 @ M[:, :2].T + M[:, 2] + rng.normal(0, NOISE_PX, (n, 2))
    out = np.zeros(n, bool)
    n_out = int(round(outlier_frac * n))
    if n_out:
        out[rng.choice(n, n_out, replace=False)] = True
        p1[out] = rng.uniform(0, 1, (n_out, 2)) * np.array([QUERY_HW[1], QUERY_HW[0]])
    return p0.astype(np.float32), p1.astype(np.float32), M, out


SIZES = (3, 5, 6, 7, 63, 64, 65, 300)
ITERATIONS = (1, 64, 257, 2000)
OUTLIERS = (0.0, 0.3, 0.6)


def _cases():
    """(n, outlier share, iterations, confidence, scene seed, sampler seed): every size at every iteration count with the outlier
    share cycling (32 cases at confidence 0.99), and every size once more without the early stop (8 cases at 1.0)"""
    cases, k = [], 0
    for iters in ITERATIONS:
        for n in SIZES:
            cases.append((n, OUTLIERS[k % 3], iters, 0.99, 100 + k, 7 + k))
            k += 1
    for j, n in enumerate(SIZES):
        cases.append((n, OUTLIERS[(j + 1) % 3], ITERATIONS[1 + j % 3], 1.0, 200 + j, 50 + j))
    return cases


GPU_CASES = _cases()

# the prototype's grid of the issue, for the undecided cap of the restatement alone
GRID_CASES = [(n, o, it, 0.99, 1000 + 97 * a + 13 * b + c, 3 + a + b + c) for a, n in enumerate(SIZES) for b, o in enumerate(OUTLIERS)
              for c, it in enumerate(ITERATIONS)]


def groups(cases):
    """cases grouped by (iterations, confidence): one device call per group, its cases as the views -> {key: [case index]}"""
    g = {}
    for i, c in enumerate(cases):
        g.setdefault((c[2], c[3]), []).append(i)
    return g
