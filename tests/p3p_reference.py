"""float64 restatement of the default PnP-RANSAC (solver "p3p" of pose.ransac_PnP: csrc/pnp_body.h, csrc/pnp_math.h), for the
tests.  Written from the published algorithm (Grunert's P3P as reviewed by Haralick et al., IJCV 1994) and this project's headers,
and independent of the device code where it can be: the quartic's roots come from `np.roots` (the device: Ferrari + Newton), the
pose from an SVD alignment of the three points (the device: two orthonormal frames), the normal equations from `np.linalg.solve`
(the device: its own elimination).  The sampler is tests/loransac_cases.draw_sample, the stop index tests/epnp_reference.ransac_stop.

Inputs are what the device sees: the float32 matches widened to double, the 3D points multiplied by `scale` (`f64`).  Poses are
[3,4] = [R | t] in the scaled unit until `out_pose` divides t by the scale, as the device does on output.

Every decision records its margin in the list `margins` as (kind, margin): how far the compared numbers were apart, relative to
the larger one (to max(1, |root|) for a quartic root).  A hypothesis with a margin below MARGIN is "undecided": a correctly
rounded implementation may decide it either way.  The per-point decisions (e^2 <= thr2, z > 1e-12) are too many for a list;
`point_margins` gives them as an array."""
import math

import numpy as np

from tests import epnp_reference as ER
from tests.loransac_cases import MARGIN, draw_sample

Z_MIN = 1e-12
IDENTITY = np.eye(4)[:3]


def f64(uv, X, scale):
    return uv.astype(np.float32).astype(np.float64), X.astype(np.float32).astype(np.float64) * float(scale)


def K4_of(K):
    return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], dtype=np.float64)


def sample4(seed, h, n):
    """the 4 match indices of hypothesis h (csrc/pnp_sample.h: draw_sample<4>)"""
    return draw_sample(int(seed) & 0xFFFFFFFF, h, n, k=4)


def _note(margins, kind, a, b):
    if margins is not None:
        a, b = float(a), float(b)
        den = max(abs(a), abs(b))
        margins.append((kind, abs(a - b) / den if den > 0 and math.isfinite(den) else float("inf")))


def _note_abs(margins, kind, v):
    if margins is not None:
        margins.append((kind, float(v)))


def undecided(margins):
    return any(m < MARGIN for _, m in margins)


def residuals(pose, X, uv, K4):
    """(squared reprojection errors [n], inf for a point that is not in front of the camera; camera depths [n])"""
    Xc = X @ pose[:, :3].T + pose[:, 3]
    with np.errstate(all="ignore"):
        du = K4[0] * Xc[:, 0] / Xc[:, 2] + K4[2] - uv[:, 0]
        dv = K4[1] * Xc[:, 1] / Xc[:, 2] + K4[3] - uv[:, 1]
        e = du * du + dv * dv
    return np.where(Xc[:, 2] > Z_MIN, e, np.inf), Xc[:, 2]


def point_margins(e, z, thr2):
    """per point: the relative distance of e^2 from thr2, or (smaller) the distance of the depth from the z > 1e-12 bar"""
    with np.errstate(all="ignore"):
        m = np.where(np.isfinite(e), np.abs(e - thr2) / np.maximum(e, thr2), np.inf)
    return np.minimum(m, np.abs(z - Z_MIN))


def _align_svd(x, p):
    """the proper rotation and translation that take the three world points x [3,3] onto the camera points p [3,3] (Kabsch)"""
    xm, pm = x.mean(0), p.mean(0)
    U, _, Vt = np.linalg.svd((x - xm).T @ (p - pm))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, pm - R @ xm


def _align_frames(x, p):
    """the same from the orthonormal frames of the two triangles, in the dtype of the inputs (np.linalg has no long double)"""
    def frame(q):
        e1 = q[1] - q[0]
        e1 = e1 / np.sqrt((e1 * e1).sum())
        e3 = np.cross(e1, q[2] - q[0])
        e3 = e3 / np.sqrt((e3 * e3).sum())
        return np.stack([e1, np.cross(e3, e1), e3])
    R = frame(p).T @ frame(x)
    return R, p[0] - R @ x[0]


def hypothesis(X, uv, K4, idx, thr2, margins=None, precise=False):
    """Grunert's P3P on the matches idx[:3], the candidate pose chosen by the squared reprojection error of match idx[3] and
    valid when that error <= 4 thr2 -> (pose [3,4] or None, margins).  None where the device has no model: coincident (or
    repeated) or collinear points among the three, a vanishing leading coefficient, no admissible root, an error above the bar.
    precise: the measurement of this function's own rounding noise -- long double throughout, every accepted root polished by
    Newton steps on the quartic, the alignment from the triangle frames."""
    margins = [] if margins is None else margins
    T = np.longdouble if precise else np.float64
    i3 = [int(i) for i in idx[:3]]
    x = X[i3].astype(T)
    K4t = np.asarray(K4, dtype=T)
    b = np.stack([(uv[i3, 0].astype(T) - K4t[2]) / K4t[0], (uv[i3, 1].astype(T) - K4t[3]) / K4t[1], np.ones(3, dtype=T)], 1)
    y = b / np.sqrt((b * b).sum(1))[:, None]
    a2, b2, c2 = ((x[1] - x[2]) ** 2).sum(), ((x[0] - x[2]) ** 2).sum(), ((x[0] - x[1]) ** 2).sum()
    if len(set(i3)) < 3 or min(a2, b2, c2) < 1e-24:
        return None, margins
    e1 = (x[1] - x[0]) / np.sqrt(c2)
    if np.sqrt((np.cross(e1, x[2] - x[0]) ** 2).sum()) < 1e-18:
        return None, margins
    ca, cb, cg = y[1] @ y[2], y[0] @ y[2], y[0] @ y[1]
    k1, k2, k3, k4 = (a2 - c2) / b2, (a2 + c2) / b2, (b2 - c2) / b2, (b2 - a2) / b2
    A = [(k1 - 1) ** 2 - 4 * (c2 / b2) * ca * ca,
         4 * (k1 * (1 - k1) * cb - (1 - k2) * ca * cg + 2 * (c2 / b2) * ca * ca * cb),
         2 * (k1 * k1 - 1 + 2 * k1 * k1 * cb * cb + 2 * k3 * ca * ca - 4 * k2 * ca * cb * cg + 2 * k4 * cg * cg),
         4 * (-k1 * (1 + k1) * cb + 2 * (a2 / b2) * cg * cg * cb - (1 - k2) * ca * cg),
         (1 + k1) ** 2 - 4 * (a2 / b2) * cg * cg]
    _note(margins, "leading", abs(A[0]), 1e-14)
    if abs(A[0]) < 1e-14:
        return None, margins
    roots = np.roots(np.array([float(a) for a in A]))
    X4 = X[int(idx[3])][None].astype(np.float64)
    uv4 = uv[int(idx[3])][None].astype(np.float64)
    cands = []
    for j, r in enumerate(roots):
        size = max(1.0, abs(r))
        if r.imag != 0.0:                                  # a complex pair: how far from a double real root
            _note_abs(margins, "imag", abs(r.imag) / size)
            continue
        others = np.delete(roots, j)
        if others.size:                                    # a real root: how far from merging with another and turning complex
            _note_abs(margins, "root_gap", np.abs(others - r).min() / size)
        v = T(r.real)
        if precise:
            for _ in range(4):
                f = (((A[0] * v + A[1]) * v + A[2]) * v + A[3]) * v + A[4]
                fp = ((4 * A[0] * v + 3 * A[1]) * v + 2 * A[2]) * v + A[3]
                if fp == 0:
                    break
                v = v - f / fp
        _note_abs(margins, "v_sign", abs(v) / size)
        if not v > 0:
            continue
        den = 2 * (cg - v * ca)
        _note(margins, "den", abs(den), 1e-12)
        if abs(den) < 1e-12:
            continue
        u = ((k1 - 1) * v * v - 2 * k1 * cb * v + 1 + k1) / den
        _note_abs(margins, "u_sign", abs(u) / max(1.0, abs(u)))
        if not u > 0:
            continue
        s1sq = b2 / (1 + v * v - 2 * v * cb)
        if not s1sq > 0:
            continue
        s1 = np.sqrt(s1sq)
        p = np.stack([s1 * y[0], u * s1 * y[1], v * s1 * y[2]])
        R, t = _align_frames(x, p) if precise else _align_svd(x, p)
        pose = np.concatenate([R, t[:, None]], 1)
        e, _ = residuals(pose.astype(np.float64), X4, uv4, K4)
        cands.append((float(e[0]), pose))
    cands = [c for c in cands if math.isfinite(c[0])]      # behind the camera for the 4th match: 1e300 on the device, never < 1e300
    if not cands:
        return None, margins
    cands.sort(key=lambda c: c[0])
    if len(cands) > 1:
        _note(margins, "fourth_gap", cands[0][0], cands[1][0])
    _note(margins, "fourth_bar", cands[0][0], 4.0 * thr2)
    if not cands[0][0] <= 4.0 * thr2:
        return None, margins
    return cands[0][1], margins


def score(pose, X, uv, K4, thr2):
    """the scoring kernel's count: points with z > 1e-12 and e^2 <= thr2 -> (count, inlier mask, per-point margins)"""
    e, z = residuals(pose, X, uv, K4)
    inl = e <= thr2
    return int(inl.sum()), inl, point_margins(e, z, thr2)


def select(scores):
    """the lowest index of the highest score; -1 (the failure) when every score is -1 or there is none"""
    scores = np.asarray(scores)
    if scores.size == 0 or scores.max() < 0:
        return -1
    return int(np.argmax(scores))


def stop_and_select(scores, n, conf):
    """(stop index of the sequential loop, the hypothesis the refinement starts from: `select` over the scores before it)"""
    stop, _ = ER.ransac_stop(scores, n, 4, conf)
    return stop, select(np.asarray(scores)[:stop])


def _rodrigues(w):
    th = math.sqrt(float(w @ w))
    Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + Kx
    Kx = Kx / th
    return np.eye(3) + math.sin(th) * Kx + (1.0 - math.cos(th)) * (Kx @ Kx)


def _gn_system(pose, X, uv, K4):
    """J^T J and -J^T r of the pixel residuals with respect to (w, dt) of X_cam' = exp([w]x) (R X + t) + dt"""
    Xc = X @ pose[:, :3].T + pose[:, 3]
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    r = np.concatenate([K4[0] * x / z + K4[2] - uv[:, 0], K4[1] * y / z + K4[3] - uv[:, 1]])
    o = np.zeros_like(z)
    dpu = np.stack([K4[0] / z, o, -K4[0] * x / (z * z)], 1)       # d u / d X_cam
    dpv = np.stack([o, K4[1] / z, -K4[1] * y / (z * z)], 1)
    # d X_cam / d w = -[X_cam]x : the rows of J are dp . (-[X_cam]x) = X_cam x dp
    J = np.concatenate([np.concatenate([np.cross(Xc, dpu), dpu], 1), np.concatenate([np.cross(Xc, dpv), dpv], 1)])
    return J.T @ J, -(J.T @ r)


def refine(pose, X, uv, K4, thr2, iters, scale, margins=None):
    """the device's Gauss-Newton loop from `pose` (scaled unit): every iteration re-evaluates the inliers, solves the normal
    equations on them and left-multiplies the update, R <- exp(w) R, t <- exp(w) t + dt; an iteration with fewer than 4 inliers or
    a singular system changes nothing.  -> (pose [R | t / scale], inlier mask after a last evaluation).  margins: list that
    receives the smallest per-point margin of every evaluation as ("refine_point", margin)"""
    P = np.array(pose, dtype=np.float64)
    for _ in range(int(iters)):
        e, z = residuals(P, X, uv, K4)
        inl = e <= thr2
        _note_abs(margins, "refine_point", point_margins(e, z, thr2).min())
        if inl.sum() < 4:
            continue
        H, g = _gn_system(P, X[inl], uv[inl], K4)
        try:
            d = np.linalg.solve(H, g)
        except np.linalg.LinAlgError:
            continue
        if not np.all(np.isfinite(d)):
            continue
        E = _rodrigues(d[:3])
        P = np.concatenate([E @ P[:, :3], (E @ P[:, 3] + d[3:])[:, None]], 1)
    e, z = residuals(P, X, uv, K4)
    _note_abs(margins, "refine_point", point_margins(e, z, thr2).min())
    return out_pose(P, scale), e <= thr2


def out_pose(pose, scale):
    """[R | t / scale], the form the device returns"""
    P = np.array(pose, dtype=np.float64)
    P[:, 3] /= float(scale)
    return P


def run(X, uv, K4, thr2, seed, iterations, refine_iters, conf, scale):
    """The whole estimator on one sample -> dict: per hypothesis `samples`, `poses` (None: invalid), `undecided`, `scores` (-1:
    invalid), `point_undecided` (number of undecided points); `stop`, `best` (-1: the failure), `pose` [3,4] as returned,
    `inliers` (mask), `state`, `refine_margins`."""
    n = X.shape[0]
    out = {"samples": [], "poses": [], "undecided": [], "scores": [], "point_undecided": []}
    for h in range(iterations if n >= 4 else 0):
        idx = sample4(seed, h, n)
        pose, m = hypothesis(X, uv, K4, idx, thr2)
        out["samples"].append(idx)
        out["poses"].append(pose)
        out["undecided"].append(undecided(m))
        if pose is None:
            out["scores"].append(-1)
            out["point_undecided"].append(0)
        else:
            c, _, pm = score(pose, X, uv, K4, thr2)
            out["scores"].append(c)
            out["point_undecided"].append(int((pm < MARGIN).sum()))
    out["scores"] = np.array(out["scores"], dtype=np.int64)
    out["stop"], out["best"] = stop_and_select(out["scores"], n, conf) if n >= 4 else (0, -1)
    out["refine_margins"] = []
    if out["best"] < 0:
        out.update(pose=IDENTITY.copy(), inliers=np.zeros(n, dtype=bool), state=False)
    else:
        out["pose"], out["inliers"] = refine(out["poses"][out["best"]], X, uv, K4, thr2, refine_iters, scale, out["refine_margins"])
        out["state"] = True
    return out
