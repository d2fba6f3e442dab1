"""Seeded inputs of the point-cloud post-processing tests (tests/test_pointcloud_cpu.py, tests/test_pointcloud_gpu.py) and of the
fixture generator gen_pointcloud_golden.py: inputs only, the expected results are in tests/golden/pointcloud_*.npz.

Every cloud is built from the distance threshold THR = 1e-3 of filter_points.merge: isolated seeds, satellites 0.3-0.7 THR from a
seed, chains spaced 0.8 THR (each link a neighbour of the next, the ends not of each other -- this is what makes the reference's
row walk order-dependent and drops points).  Ids are sparse int64 values above 2**31."""
import numpy as np

THR = 1e-3
ID_BASE = (1 << 31) + 12345


def _ids(n, rng):
    return ID_BASE + np.cumsum(rng.integers(1, 1000, size=n)).astype(np.int64)


def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def mixed_cloud(n, seed):
    """about n points: isolated seeds, seeds with 1-3 satellites, chains of 3-11 points, shuffled; exactly n are returned"""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < n:
        kind = rng.integers(0, 4)
        base = rng.uniform(-0.5, 0.5, size=3)
        if kind == 0:
            pts.append(base)
        elif kind in (1, 2):
            pts.append(base)
            for _ in range(int(rng.integers(1, 4))):
                pts.append(base + _unit(rng) * rng.uniform(0.3, 0.7) * THR)
        else:
            step = _unit(rng) * 0.8 * THR
            for k in range(int(rng.integers(3, 12))):
                pts.append(base + k * step)
    pts = np.array(pts[:n])
    return pts[rng.permutation(n)], _ids(n, rng)


def line_cloud(order):
    """200 points spaced 0.8 THR on a line, in index order, reversed or permuted"""
    rng = np.random.default_rng(77)
    direction = np.array([0.6, 0.64, 0.48])
    pts = np.array([0.1, -0.2, 0.3]) + np.arange(200)[:, None] * (0.8 * THR) * direction
    if order == "reversed":
        pts = pts[::-1].copy()
    elif order == "permuted":
        pts = pts[rng.permutation(200)]
    return pts, _ids(200, rng)


def blob_cloud():
    """40 points within 0.2 THR of each other: every point is every point's neighbour, one cluster of degree 40"""
    rng = np.random.default_rng(40)
    pts = np.array([0.25, 0.5, -0.125]) + rng.uniform(-0.1, 0.1, size=(40, 3)) * THR / np.sqrt(3.0)
    return pts, _ids(40, rng)


def duplicate_cloud():
    """30 distinct points, 12 of them present two or three times (distance exactly 0), shuffled"""
    rng = np.random.default_rng(5)
    base = rng.uniform(-0.5, 0.5, size=(30, 3))
    pts = np.concatenate([base, base[:12], base[:5]])
    pts = pts[rng.permutation(len(pts))]
    return pts, _ids(len(pts), rng)


def _pair(distance):
    rng = np.random.default_rng(2)
    a = rng.uniform(-0.5, 0.5, size=3)
    return np.stack([a, a + _unit(rng) * distance]), _ids(2, rng)


# name -> (builder of (xyzs, ids), threshold)
MERGE_CASES = {
    "n1": (lambda: (np.array([[0.125, -0.25, 0.5]]), np.array([ID_BASE], dtype=np.int64)), THR),
    "n2_close": (lambda: _pair(0.4 * THR), THR),
    "n2_far": (lambda: _pair(3.0 * THR), THR),
    "n63": (lambda: mixed_cloud(63, 63), THR),
    "n64": (lambda: mixed_cloud(64, 64), THR),
    "n65": (lambda: mixed_cloud(65, 65), THR),
    "n257": (lambda: mixed_cloud(257, 257), THR),
    "duplicates": (duplicate_cloud, THR),
    "blob40": (blob_cloud, THR),
    "line200": (lambda: line_cloud("index"), THR),
    "line200_reversed": (lambda: line_cloud("reversed"), THR),
    "line200_permuted": (lambda: line_cloud("permuted"), THR),
    "mixed1500": (lambda: mixed_cloud(1500, 1500), THR),
    "mixed1500_thr5e-3": (lambda: mixed_cloud(1500, 1500), 5e-3),
}
MIXED_CASES = ("mixed1500", "mixed1500_thr5e-3")      # more than 100 multi-member clusters and at least 5 dropped points each


def merge_inputs(name):
    build, thr = MERGE_CASES[name]
    xyzs, ids = build()
    return np.ascontiguousarray(xyzs, dtype=np.float64), np.asarray(ids, dtype=np.int64), thr


def box_corners(rotated):
    """corners in the order of the reference's get_3d_box: (-,-,-) (-,-,+) (-,+,+) (-,+,-) (+,-,-) (+,-,+) (+,+,+) (+,+,-)"""
    sx, sy, sz = 0.11, 0.07, 0.05
    c = np.array([[-sx, -sy, -sz], [-sx, -sy, sz], [-sx, sy, sz], [-sx, sy, -sz],
                  [sx, -sy, -sz], [sx, -sy, sz], [sx, sy, sz], [sx, sy, -sz]])
    if not rotated:
        return c + np.array([0.02, -0.01, 0.03])
    rng = np.random.default_rng(9)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.linalg.det(q))
    return c @ q.T + np.array([-0.3, 0.2, 0.05])


BOX_CASES = {"%s_n%d" % ("rotated" if rot else "axis", n): (rot, n) for rot in (False, True) for n in (1, 65, 1000)}


def box_inputs(name):
    """points spread over 2.5 box lengths along every edge: both sides of all six faces are populated from n = 65 on;
    the single point of n = 1 lies inside"""
    rotated, n = BOX_CASES[name]
    corners = box_corners(rotated)
    rng = np.random.default_rng(1000 + n + rotated)
    u = rng.uniform(-0.75, 1.75, size=(n, 3)) if n > 1 else np.array([[0.4, 0.6, 0.5]])
    c4 = corners[4]
    xyz = c4 + u[:, :1] * (corners[5] - c4) + u[:, 1:2] * (corners[0] - c4) + u[:, 2:] * (corners[7] - c4)
    return np.ascontiguousarray(xyz), corners


# name -> (track lengths, thres, percent_thres)
TKL_CASES = {
    "ties": ([2, 2, 3, 3, 3, 4, 4, 5, 7, 7], 4, 1.0),
    "ties_exact": ([2, 2, 3, 3, 3, 4, 4, 5, 7, 7], 5, 1.0),
    "thres_above_n": ([2, 3, 3, 9, 4], 100, 1.0),
    "percent_half": ([2, 2, 3, 3, 3, 4, 4, 5, 7, 7], 100, 0.5),
    "single_length": ([6, 6, 6, 6], 2, 1.0),
    "single_length_loose": ([6, 6, 6, 6], 10, 1.0),
    "thres_zero": ([2, 5, 5, 8], 0, 1.0),
}

POSTPROCESS = dict(n=300, seed=300, dim=16, max_num_kp3d=60, rotated=True)


def postprocess_inputs():
    """a 300-point mixed cloud scaled into and around the rotated box, unordered sparse ids, track lengths 2-9 and per-point
    16-channel features -> (ids, xyz, track_lengths, corners, kp3d_id_feature, kp3d_id_score)"""
    p = POSTPROCESS
    rng = np.random.default_rng(p["seed"])
    cloud, ids = mixed_cloud(p["n"], p["seed"])
    corners = box_corners(p["rotated"])
    centre = corners.mean(0)
    xyz = np.ascontiguousarray(centre + cloud * 0.2)           # a cube of side 0.2 around a box of 0.22 x 0.14 x 0.10: most points fall outside
    ids = ids[rng.permutation(p["n"])]
    track_lengths = rng.integers(2, 10, size=p["n"])
    feature = {int(i): rng.standard_normal((int(t), p["dim"])).astype(np.float32) for i, t in zip(ids, track_lengths)}
    score = {int(i): rng.uniform(0.1, 1.0, size=(int(t), 1)) for i, t in zip(ids, track_lengths)}
    return ids, xyz, track_lengths, corners, feature, score
