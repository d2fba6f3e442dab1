"""float64 restatement of the batched affine RANSAC (csrc/affine.hip), independent of the device code where it can be: the minimal
model from np.linalg.solve, the refit from np.linalg.lstsq, the sampler restated in tests.loransac_cases.draw_sample(k=3), the
stop rule in tests.epnp_reference.ransac_stop(m=3).  No GPU.

Like tests/p3p_reference.py it records a margin for every floating-point decision, as (kind, margin); a view with a margin below
MARGIN is "undecided": a correctly rounded implementation in another order of operations may decide it the other way, so an
exact comparison of counts, masks and boxes proves nothing there.  The decisions and their margins:
  collinear   OpenCV's haveCollinearPoints on the sample's source points: |cross| against FLT_EPSILON * (|dx1| + ...), relative
              to the larger of the two (both zero -- repeated points -- is decided)
  point       e2 against thr^2 for every match under every hypothesis, relative to the larger
  corner      the distance in px of a mapped corner coordinate to the nearest non-zero integer (truncation towards zero does not
              change at 0), and to 2^31
Ties between hypotheses or views of equal inlier count are not floating-point decisions: the sequential loop takes a later
hypothesis only on a strictly larger count, the selection takes the first view, and both sides apply exactly these rules on
integers.  `n_tied_hyp` / `n_tied_view` report how many candidates shared the best count.
`cond` is the 2-norm condition number of the centred [n_inliers, 2] design matrix of the refit."""
import numpy as np

from tests.epnp_reference import ransac_stop
from tests.loransac_cases import MARGIN, draw_sample

FLT_EPSILON = float(np.finfo(np.float32).eps)


def f64(p):
    """what the device sees: float32 inputs widened to double"""
    return np.asarray(p).astype(np.float32).astype(np.float64).reshape(-1, 2)


def _rel(a, b):
    den = np.maximum(np.abs(a), np.abs(b))
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.abs(a - b) / den
    return np.where(den > 0, m, np.inf)


def collinear(src):
    """src [H,3,2] -> (collinear [H], margin [H])"""
    d1 = src[:, 1] - src[:, 2]
    d2 = src[:, 0] - src[:, 2]
    cross = np.abs(d2[:, 0] * d1[:, 1] - d2[:, 1] * d1[:, 0])
    bound = FLT_EPSILON * (np.abs(d1).sum(axis=1) + np.abs(d2).sum(axis=1))
    return cross <= bound, _rel(cross, bound)


def errors2(M, p0, p1):
    """M [...,2,3] -> squared distances [..., n]"""
    proj = np.einsum("...ij,nj->...ni", M[..., :, :2], p0) + M[..., None, :, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return ((proj - p1) ** 2).sum(axis=-1)


def box_of(M, corners, margins=None):
    """-> (box int32 [4] or None when a coordinate is not finite or does not fit int32)"""
    pts = np.asarray(corners, np.float64).reshape(4, 2) @ M[:, :2].T + M[:, 2]
    if not np.isfinite(pts).all() or (np.abs(pts) >= 2.0 ** 31).any():
        return None
    if margins is not None:
        r = np.rint(pts)
        d = np.where(r != 0, np.abs(pts - r), np.inf)
        margins.append(("corner", float(min(d.min(), (2.0 ** 31 - np.abs(pts)).min()))))
    t = pts.astype(np.int32)
    return np.array([t[:, 0].min(), t[:, 1].min(), t[:, 0].max(), t[:, 1].max()], np.int32)


def refit(p0, p1):
    """least-squares affine map on coordinates centred on the means -> (M [2,3], condition number of the design matrix)"""
    m0, m1 = p0.mean(axis=0), p1.mean(axis=0)
    A, B = p0 - m0, p1 - m1
    sol = np.linalg.lstsq(A, B, rcond=None)[0]            # [2,2]: columns = the rows of the linear part
    L = sol.T
    return np.concatenate([L, (m1 - L @ m0)[:, None]], axis=1), float(np.linalg.cond(A))


def estimate_view(p0, p1, seed, iterations, thr=6.0, confidence=0.99, refine=True, corners=None, fallback_box=(0, 0, 0, 0)):
    """One view -> dict: samples [iterations,3], scores [iterations], stop, best, ok, affine [2,3], ransac_affine, mask [n],
    n_inliers, box [4], margins, undecided, cond (None without a refit), sample_cond (the same number for the three source points
    of the best sample), n_tied_hyp"""
    p0, p1 = f64(p0), f64(p1)
    n, thr2 = p0.shape[0], float(thr) * float(thr)
    corners = np.zeros((4, 2)) if corners is None else np.asarray(corners, np.float64).reshape(4, 2)
    out = {"n": n, "samples": np.full((iterations, 3), -1, np.int32), "scores": np.full(iterations, -1, np.int32), "stop": 0, "best": -1,
           "ok": 0, "affine": np.eye(3)[:2].copy(), "ransac_affine": None, "mask": np.zeros(n, np.int32), "n_inliers": 0,
           "box": np.asarray(fallback_box, np.int32).copy(), "margins": [], "cond": None, "sample_cond": None, "n_tied_hyp": 0}
    margins = out["margins"]

    def done():
        out["undecided"] = any(m < MARGIN for _, m in margins)
        return out

    if n < 3:
        return done()
    H = 1 if n == 3 else iterations
    idx = np.array([[0, 1, 2]] if n == 3 else [draw_sample(int(seed), h, n, 3) for h in range(H)], np.int64)
    out["samples"][:H] = idx
    col, cm = collinear(p0[idx])
    margins.append(("collinear", float(cm.min())))
    models = np.zeros((H, 2, 3))
    good = np.nonzero(~col)[0]
    if good.size:
        A = np.concatenate([p0[idx[good]], np.ones((good.size, 3, 1))], axis=2)      # [G,3,3]
        models[good] = np.transpose(np.linalg.solve(A, p1[idx[good]]), (0, 2, 1))
        e2 = errors2(models[good], p0, p1)                                           # [G,n]
        out["scores"][good] = (e2 <= thr2).sum(axis=1)
        margins.append(("point", float(_rel(e2, thr2).min())))
    stop, best = ransac_stop(out["scores"][:H], n, 3, confidence)
    out["stop"], out["best"] = stop, best
    if best < 0:
        return done()
    out["n_tied_hyp"] = int((out["scores"][:stop] == out["scores"][best]).sum())
    M = models[best]
    mask = errors2(M, p0, p1) <= thr2
    out["ransac_affine"] = M.copy()
    out["sample_cond"] = float(np.linalg.cond(p0[idx[best]] - p0[idx[best]].mean(axis=0)))
    if refine and mask.sum() > 3:
        M, out["cond"] = refit(p0[mask], p1[mask])
    box = box_of(M, corners, margins)
    if box is None:
        return done()
    out.update(ok=1, affine=M, mask=mask.astype(np.int32), n_inliers=int(mask.sum()), box=box)
    return done()


def estimate_batch(views, seeds, iterations, thr=6.0, confidence=0.99, refine=True, corners=None, fallback_box=(0, 0, 0, 0)):
    """views: list of (p0 [n,2], p1 [n,2]) -> (list of `estimate_view` dicts, best_view, best_box, n_tied_view)"""
    res = [estimate_view(p0, p1, seeds[v], iterations, thr, confidence, refine, None if corners is None else corners[v], fallback_box)
           for v, (p0, p1) in enumerate(views)]
    counts = [r["n_inliers"] if r["ok"] else -1 for r in res]
    top = max(counts)
    if top < 0:
        return res, -1, np.asarray(fallback_box, np.int32), 0
    best = counts.index(top)
    return res, best, res[best]["box"], counts.count(top)
