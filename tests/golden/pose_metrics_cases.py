"""Seeded inputs of the pose-metric fixtures (tests/golden/pose_metrics_*.npz, written by gen_pose_metrics_golden.py from the
reference's own `query_pose_error` / `add_metric` / `projection_2d_error` / `aggregate_metrics`).  Only results are stored; the
generator and the tests rebuild the inputs from here (numpy only).

Vertex counts are the tile and chunk edges of the two device sweeps (256 vertices per workgroup, 1024 predicted points per
ADD-S chunk, one wave = 64).  Every count is scored under three perturbations of the ground-truth pose: the identical pose, a
small one (0.03 rad, about 1 cm) and a large one (2.5 rad, 30 cm; 0.64 rad away from pi, where upstream's acos without a
lower clamp would turn NaN)."""
import numpy as np

P_LIST = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500)
PERTURBATIONS = {"same": (0.0, 0.0), "small": (0.03, 0.01), "large": (2.5, 0.30)}     # rotation (rad), translation (model units)
UNITS = ("m", "cm", "mm")
DIAMETER_PASS, DIAMETER_FAIL = 0.3, 0.05     # thresholds 0.03 / 0.005 around the small perturbation's ADD of about 0.01
DIAMETERS = (DIAMETER_PASS, DIAMETER_FAIL)

# name -> (P, perturbation, seed)
SINGLE_CASES = {"p%d_%s" % (P, kind): (P, kind, 1000 + 10 * i + k)
                for i, P in enumerate(P_LIST) for k, kind in enumerate(PERTURBATIONS)}
# one call over three poses with mixed flags
BATCH_P, BATCH_SEED = 257, 77
BATCH_KINDS = ("small", "large", "small")
BATCH_SYN = (0, 1, 1)
BATCH_VALID = (1, 0, 1)
AGGREGATE_SEED, AGGREGATE_N = 5, 200


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * (Kx @ Kx)


def vertices(P, rng):
    return ((rng.random((P, 3)) - 0.5) * 0.2).astype(np.float32)


def gt_pose(rng):
    """[3,4] float64: an axis-angle rotation of about 1 rad, t about (0.02, -0.01, 0.6)"""
    R = rodrigues(rng.normal(size=3), 1.0 + 0.1 * rng.normal())
    t = np.array([0.02, -0.01, 0.6]) + 0.005 * rng.normal(size=3)
    return np.concatenate([R, t[:, None]], axis=1)


def perturbed(pose, kind, rng):
    ang, trans = PERTURBATIONS[kind]
    if ang == 0.0 and trans == 0.0:
        return pose.copy()
    dR = rodrigues(rng.normal(size=3), ang)
    d = rng.normal(size=3)
    t = pose[:, 3] + trans * d / np.linalg.norm(d)
    return np.concatenate([dR @ pose[:, :3], t[:, None]], axis=1)


def intrinsics():
    return np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])


def single_inputs(name):
    """-> model [P,3] float32, pose_pred [3,4], pose_gt [3,4], K [3,3] (float64)"""
    P, kind, seed = SINGLE_CASES[name]
    rng = np.random.default_rng(seed)
    model = vertices(P, rng)
    gt = gt_pose(rng)
    return model, perturbed(gt, kind, rng), gt, intrinsics()


def batch_inputs():
    """-> model [P,3], pose_pred [3,3,4], pose_gt [3,3,4], K [3,3,3], syn [3] bool, valid [3] bool"""
    rng = np.random.default_rng(BATCH_SEED)
    model = vertices(BATCH_P, rng)
    gts = [gt_pose(rng) for _ in BATCH_KINDS]
    preds = [perturbed(g, kind, rng) for g, kind in zip(gts, BATCH_KINDS)]
    Ks = np.stack([intrinsics() * np.array([[1.0 + 0.01 * b], [1.0 + 0.01 * b], [1.0]]) for b in range(len(gts))])
    return model, np.stack(preds), np.stack(gts), Ks, np.array(BATCH_SYN, bool), np.array(BATCH_VALID, bool)


def aggregate_inputs():
    """a seeded per-frame metric list as the reference's evaluation collects it (some failed poses = inf)"""
    rng = np.random.default_rng(AGGREGATE_SEED)
    R = np.abs(rng.normal(size=AGGREGATE_N)) * 3.0
    t = np.abs(rng.normal(size=AGGREGATE_N)) * 3.0
    fail = rng.random(AGGREGATE_N) < 0.05
    R[fail], t[fail] = np.inf, np.inf
    return {"R_errs": list(R), "t_errs": list(t), "ADD_metric": list(rng.random(AGGREGATE_N) < 0.7),
            "proj2D_metric": list(np.abs(rng.normal(size=AGGREGATE_N - int(fail.sum()))) * 6.0)}
