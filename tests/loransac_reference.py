"""float64 restatement of the LO-RANSAC pose estimator with robust refinement (solver "loransac" of pose.ransac_PnP: the
reference's pycolmap branch, COLMAP's LORANSAC<P3P, EPnP> + a Cauchy-loss refinement), written from its description in
pose.py's docstring, for the tests.  EPnP is tests/epnp_reference.py; the P3P models are an input (recorded from the device, or
from a host build of opp_p3p_grunert).

Every function that decides something appends (kind, relative margin) to `margins` when given a list: how far the two compared
numbers were apart, relative to the larger one.  A run whose smallest margin is far above rounding took the same decisions as
any correctly rounded implementation."""
import math

import numpy as np

from tests import epnp_reference as ER

NOSUM = 1.7976931348623157e308
LO_ROUNDS = 10
LO_MIN = 4
LM_ITERS = 100
LM_LAMBDA0 = 1e-4
LM_FACTOR = 10.0
LM_LAMBDA_MIN = 1e-12
LM_LAMBDA_MAX = 1e16
LM_GTOL = 1.0
LM_MIN_GAIN = 1e-3


def _note(margins, kind, a, b):
    if margins is not None:
        den = max(abs(a), abs(b))
        margins.append((kind, abs(a - b) / den if den > 0 and math.isfinite(den) else float("inf")))


def residuals(pose, X, uv, K4):
    """squared reprojection errors [n]; inf for a point that is not in front of the camera"""
    Xc = X @ pose[:, :3].T + pose[:, 3]
    with np.errstate(all="ignore"):
        du = K4[0] * Xc[:, 0] / Xc[:, 2] + K4[2] - uv[:, 0]
        dv = K4[1] * Xc[:, 1] / Xc[:, 2] + K4[3] - uv[:, 1]
        e = du * du + dv * dv
    return np.where(Xc[:, 2] > 1e-12, e, np.inf)


def support(pose, X, uv, K4, thr2):
    """-> (inlier count, sum of the inliers' residuals, inlier indices, residuals)"""
    e = residuals(pose, X, uv, K4)
    inl = np.nonzero(e <= thr2)[0]
    return int(inl.size), float(e[inl].sum()), inl, e


def better(a, b, margins=None):
    """support a = (count, sum) is better than b"""
    if a[0] != b[0]:
        return a[0] > b[0]
    if b[1] < NOSUM:
        _note(margins, "support", a[1], b[1])
    return a[1] < b[1]


def dyn_trials(confidence, cnt, n, cap):
    if not confidence < 1.0:
        return cap
    if cnt >= n:
        return 0
    r = cnt / n
    den = math.log(1.0 - r * r * r)
    if not den < 0.0:
        return cap
    v = 3.0 * math.log(1.0 - confidence) / den
    return cap if v >= cap else int(math.ceil(v))


def local_optimise(pose, sup, X, uv, K4, thr2, margins=None):
    """the LO rounds from a model with support `sup` = (count, sum) -> (support, pose)"""
    best, best_pose = sup, pose
    if sup[0] <= LO_MIN:
        return best, best_pose
    for _ in range(LO_ROUNDS):
        prev = best[0]
        inl = np.nonzero(residuals(best_pose, X, uv, K4) <= thr2)[0]
        if inl.size <= LO_MIN:
            break
        cand, _ = ER.epnp(X[inl], uv[inl], K4)
        if cand is None:
            break
        c, s, _, _ = support(cand, X, uv, K4, thr2)
        if better((c, s), best, margins):
            best, best_pose = (c, s), cand
        if best[0] <= prev:
            break
    return best, best_pose


def resolve(cand_idx, raw, lo, n, confidence, min_trials, cap, margins=None):
    """the sequential loop over candidate models given their raw and locally optimised supports (lists of (count, sum));
    cand_idx[c] = 4 * trial + model -> (stop, index of the best candidate or -1, taken flags)"""
    best, b, dyn, last, taken, ended = (0, NOSUM), -1, cap, -1, [], False
    for c, idx in enumerate(cand_idx):
        t = int(idx) >> 2
        ended = ended or t >= max(dyn, min_trials, last + 1)
        live = (not ended) and better(raw[c], best, margins)
        taken.append(1 if live else 0)
        if live:
            best, b, last = lo[c], c, t
            dyn = dyn_trials(confidence, best[0], n, cap)
    return min(cap, max(dyn, min_trials, last + 1)), b, taken


def lo_ransac(models, counts, sums, X, uv, K4, thr, confidence=0.9999, min_trials=1000, cap=10000, min_inlier_ratio=0.01,
              margins=None):
    """The trial loop, literally.  models [T][4][3,4]; counts / sums [T][4]: the support of every model (count < 0: no such
    model).  -> dict(stop, best (trial, model) or None, candidates [4 * trial + model], lo [(count, sum)] per candidate, taken,
    pose (before refinement), inliers, state)"""
    n, thr2 = X.shape[0], thr * thr
    best, best_pose, best_tm = (0, NOSUM), None, None
    record = (0, NOSUM)                      # the best raw support so far: the candidate list does not know about LO
    cands, lo, taken = [], [], []
    dyn, t = cap, 0
    while t < cap:
        if t >= dyn and t >= min_trials:
            break
        for m in range(4):
            if counts[t][m] < 0:
                continue
            s = (int(counts[t][m]), float(sums[t][m]))
            is_cand = better(s, record)
            if is_cand:
                record = s
                cands.append(4 * t + m)
            if better(s, best, margins):
                assert is_cand
                best, best_pose = local_optimise(np.asarray(models[t][m], dtype=np.float64), s, X, uv, K4, thr2, margins)
                best_tm = (t, m)
                dyn = dyn_trials(confidence, best[0], n, cap)
                lo.append(best)
                taken.append(1)
            elif is_cand:
                lo.append(None)              # never optimised by the sequential loop
                taken.append(0)
        t += 1
    out = {"stop": t, "best": best_tm, "candidates": cands, "lo": lo, "taken": taken, "support": best}
    out["state"] = best_pose is not None and best[0] > 0 and best[0] >= min_inlier_ratio * n
    if out["state"]:
        out["pose"] = best_pose
        out["inliers"] = np.nonzero(residuals(best_pose, X, uv, K4) <= thr2)[0]
    return out


def _rodrigues(w):
    th = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + Kx
    Kx = Kx / th
    return np.eye(3) + math.sin(th) * Kx + (1.0 - math.cos(th)) * (Kx @ Kx)


def _lm_rows(pose, X, uv, K4):
    """Jacobians Ju, Jv [n,6] of the projection with respect to (w, dt) of X_cam' = exp([w]x)(R X + t) + dt, residuals [n,2]"""
    Xc = X @ pose[:, :3].T + pose[:, 3]
    xc, yc, zc = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    ok = zc > 1e-12
    with np.errstate(all="ignore"):
        iz = 1.0 / zc
        r = np.stack([K4[0] * xc * iz + K4[2] - uv[:, 0], K4[1] * yc * iz + K4[3] - uv[:, 1]], 1)
        ju = np.stack([K4[0] * iz, np.zeros_like(iz), -K4[0] * xc * iz * iz], 1)
        jv = np.stack([np.zeros_like(iz), K4[1] * iz, -K4[1] * yc * iz * iz], 1)
    # d(Xc)/d(w) = -[Xc]x
    cross = np.zeros((X.shape[0], 3, 3))
    cross[:, 0, 1], cross[:, 0, 2] = zc, -yc
    cross[:, 1, 0], cross[:, 1, 2] = -zc, xc
    cross[:, 2, 0], cross[:, 2, 1] = yc, -xc
    Ju = np.concatenate([np.einsum("nk,nkj->nj", ju, cross), ju], 1)
    Jv = np.concatenate([np.einsum("nk,nkj->nj", jv, cross), jv], 1)
    return Ju, Jv, r, ok


def robust_cost(pose, X, uv, K4):
    Ju, Jv, r, ok = _lm_rows(pose, X, uv, K4)
    s = (r * r).sum(1)
    with np.errstate(all="ignore"):
        rho = np.where(ok, np.log(1.0 + s), 1e300)
    return float(np.cumsum(rho)[-1]) if rho.size else 0.0


def _normal_equations(pose, X, uv, K4):
    Ju, Jv, r, ok = _lm_rows(pose, X, uv, K4)
    s = (r * r).sum(1)
    with np.errstate(all="ignore"):
        w = np.where(ok, 1.0 / (1.0 + s), 0.0)
    Ju, Jv, r = np.where(ok[:, None], Ju, 0.0), np.where(ok[:, None], Jv, 0.0), np.where(ok[:, None], r, 0.0)
    H = np.cumsum(w[:, None, None] * (Ju[:, :, None] * Ju[:, None, :] + Jv[:, :, None] * Jv[:, None, :]), 0)[-1]
    g = -np.cumsum(w[:, None] * (Ju * r[:, :1] + Jv * r[:, 1:]), 0)[-1]
    return H, g


def cauchy_lm(pose, X, uv, K4, margins=None):
    """Levenberg-Marquardt on sum log(1 + residual) from `pose` [3,4] -> (pose, damped systems solved, cost before, cost after)"""
    P = np.array(pose, dtype=np.float64)
    if X.shape[0] == 0:
        return P, 0, 0.0, 0.0
    cost = cost0 = robust_cost(P, X, uv, K4)
    H, g = _normal_equations(P, X, uv, K4)
    lam, iters = LM_LAMBDA0, 0
    for _ in range(LM_ITERS):
        gm = float(np.abs(g).max())
        _note(margins, "gradient", gm, LM_GTOL)
        if not gm > LM_GTOL:
            break
        iters += 1
        A = H + lam * np.diag(np.diag(H))
        N, pred = None, 0.0
        try:
            d = np.linalg.solve(A, g)
            if np.all(np.isfinite(d)) and np.abs(np.diag(A)).min() >= 1e-18:
                E = _rodrigues(d[:3])
                N = np.concatenate([E @ P[:, :3], (E @ P[:, 3] + d[3:])[:, None]], 1)
                pred = float(np.sum(d * (g + lam * np.diag(H) * d)))     # decrease predicted by the linearised model
        except np.linalg.LinAlgError:
            pass
        accept = False
        if N is not None:
            cost_new = robust_cost(N, X, uv, K4)
            _note(margins, "accept", cost - cost_new, LM_MIN_GAIN * pred)
            accept = pred > 0.0 and cost - cost_new > LM_MIN_GAIN * pred
        if accept:
            P, cost = N, cost_new
            lam = max(lam / LM_FACTOR, LM_LAMBDA_MIN)
            H, g = _normal_equations(P, X, uv, K4)
        else:
            lam = lam * LM_FACTOR
            if lam > LM_LAMBDA_MAX:
                break
    return P, iters, cost0, cost


def estimate(models, counts, sums, X, uv, K4, thr, margins=None, **kw):
    """lo_ransac + the refinement on the best model's inliers -> its dict plus refined `pose_refined`, `lm_iters`, costs"""
    out = lo_ransac(models, counts, sums, X, uv, K4, thr, margins=margins, **kw)
    if out["state"]:
        inl = out["inliers"]
        out["pose_refined"], out["lm_iters"], out["cost0"], out["cost"] = cauchy_lm(out["pose"], X[inl], uv[inl], K4, margins)
    return out


def smallest_margin(margins):
    return min((m for _, m in margins), default=float("inf"))
