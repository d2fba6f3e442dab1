"""float64 restatement of the EPnP solver and the RANSAC stopping rule of csrc/pnp_math.h (the reference's
cv2.solvePnPRansac(flags=SOLVEPNP_EPNP), V. Lepetit, F. Moreno-Noguer, P. Fua, IJCV 81(2), 2009), for the tests.

Every operation is written in the device's order: sums over points run sequentially (np.cumsum), the 12x12 eigen-solve is the
same cyclic Jacobi with the same round-robin pivot order (not numpy.linalg.eigh: for 5-point samples the null space of M is
2-dimensional, and EPnP's rank-1 beta extraction depends on the basis a solver picks in it)."""
import math

import numpy as np

F = np.float64
SWEEPS12 = 10
SWEEPS3 = 10
GN_ITERS = 5
BAD = 1e300


def _seqsum(a):
    return F(np.cumsum(np.asarray(a, dtype=np.float64))[-1])


def _rot(app, aqq, apq):
    if apq == 0.0:
        return F(1.0), F(0.0)
    with np.errstate(all="ignore"):
        th = (aqq - app) / (F(2.0) * apq)
        t = F(1.0) / (np.abs(th) + np.sqrt(th * th + F(1.0)))
        if th < 0.0:
            t = -t
        c = F(1.0) / np.sqrt(t * t + F(1.0))
    return c, t * c


def _jacobi_step(A, V, pairs):
    N = A.shape[0]
    pr = np.arange(N)
    jd = np.ones(N)
    jo = np.zeros(N)
    for p, q in pairs:
        c, s = _rot(A[p, p], A[q, q], A[p, q])
        pr[p], pr[q] = q, p
        jd[p] = jd[q] = c
        jo[p], jo[q] = -s, s
    with np.errstate(all="ignore"):
        B = jd[:, None] * A + jo[:, None] * A[pr, :]
        A2 = B * jd[None, :] + B[:, pr] * jo[None, :]
        V2 = V * jd[None, :] + V[:, pr] * jo[None, :]
    return A2, V2


def rr_pairs12(s):
    out = []
    for k in range(6):
        a, b = (0, 1 + s % 11) if k == 0 else (1 + (s + k) % 11, 1 + (s + 11 - k) % 11)
        out.append((min(a, b), max(a, b)))
    return out


def jacobi12(A):
    """-> (A after the sweeps: eigenvalues on the diagonal, V: eigenvectors as columns)"""
    A = np.array(A, dtype=np.float64)
    V = np.eye(12)
    for _ in range(SWEEPS12):
        for st in range(11):
            A, V = _jacobi_step(A, V, rr_pairs12(st))
    return A, V


def jacobi3(S):
    A = np.array(S, dtype=np.float64)
    V = np.eye(3)
    for _ in range(SWEEPS3):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            A, V = _jacobi_step(A, V, [(p, q)])
    return A, V


def _order_desc3(d):
    o = [0, 1, 2]
    for i in range(3):
        for j in range(2 - i):
            if d[o[j + 1]] > d[o[j]]:
                o[j], o[j + 1] = o[j + 1], o[j]
    return o


def qr_solve(A, b):
    """OpenCV epnp::qr_solve (Householder); None when singular"""
    A = [[F(x) for x in row] for row in np.asarray(A, dtype=np.float64)]
    b = [F(x) for x in b]
    nr, nc = len(A), len(A[0])
    a1, a2 = [F(0)] * nc, [F(0)] * nc
    with np.errstate(all="ignore"):
        for k in range(nc):
            eta = abs(A[k][k])
            for i in range(k + 1, nr):
                if abs(A[i][k]) > eta:
                    eta = abs(A[i][k])
            if not eta > 0.0:
                return None
            s = F(0.0)
            for i in range(k, nr):
                A[i][k] = A[i][k] / eta
                s = s + A[i][k] * A[i][k]
            sigma = np.sqrt(s)
            if A[k][k] < 0.0:
                sigma = -sigma
            A[k][k] = A[k][k] + sigma
            a1[k] = sigma * A[k][k]
            a2[k] = -eta * sigma
            for j in range(k + 1, nc):
                s = F(0.0)
                for i in range(k, nr):
                    s = s + A[i][k] * A[i][j]
                tau = s / a1[k]
                for i in range(k, nr):
                    A[i][j] = A[i][j] - tau * A[i][k]
        for j in range(nc):
            tau = F(0.0)
            for i in range(j, nr):
                tau = tau + A[i][j] * b[i]
            tau = tau / a1[j]
            for i in range(j, nr):
                b[i] = b[i] - tau * A[i][j]
        x = [F(0)] * nc
        x[nc - 1] = b[nc - 1] / a2[nc - 1]
        for i in range(nc - 2, -1, -1):
            s = F(0.0)
            for j in range(i + 1, nc):
                s = s + A[i][j] * x[j]
            x[i] = (b[i] - s) / a2[i]
    return x


def _dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _gauss_newton(L, rho, bt):
    with np.errstate(all="ignore"):
        for _ in range(GN_ITERS):
            A, b = [], []
            for i in range(6):
                l = L[i]
                A.append([F(2) * l[0] * bt[0] + l[1] * bt[1] + l[3] * bt[2] + l[6] * bt[3],
                          l[1] * bt[0] + F(2) * l[2] * bt[1] + l[4] * bt[2] + l[7] * bt[3],
                          l[3] * bt[0] + l[4] * bt[1] + F(2) * l[5] * bt[2] + l[8] * bt[3],
                          l[6] * bt[0] + l[7] * bt[1] + l[8] * bt[2] + F(2) * l[9] * bt[3]])
                b.append(rho[i] - (l[0] * bt[0] * bt[0] + l[1] * bt[0] * bt[1] + l[2] * bt[1] * bt[1] + l[3] * bt[0] * bt[2] +
                                   l[4] * bt[1] * bt[2] + l[5] * bt[2] * bt[2] + l[6] * bt[0] * bt[3] + l[7] * bt[1] * bt[3] +
                                   l[8] * bt[2] * bt[3] + l[9] * bt[3] * bt[3]))
            x = qr_solve(A, b)
            if x is None:
                return bt
            bt = [bt[k] + x[k] for k in range(4)]
    return bt


def _betas(v, cw):
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    L, rho = [], []
    for pa, pb in pairs:
        dv = [[v[k][3 * pa + c] - v[k][3 * pb + c] for c in range(3)] for k in range(4)]
        L.append([_dot3(dv[0], dv[0]), F(2) * _dot3(dv[0], dv[1]), _dot3(dv[1], dv[1]), F(2) * _dot3(dv[0], dv[2]),
                  F(2) * _dot3(dv[1], dv[2]), _dot3(dv[2], dv[2]), F(2) * _dot3(dv[0], dv[3]), F(2) * _dot3(dv[1], dv[3]),
                  F(2) * _dot3(dv[2], dv[3]), _dot3(dv[3], dv[3])])
        a, b = cw[pa], cw[pb]
        rho.append((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]))
    betas = {1: [F(0)] * 4, 2: [F(0)] * 4, 3: [F(0)] * 4}
    with np.errstate(all="ignore"):
        x = qr_solve([[L[i][c] for c in (0, 1, 3, 6)] for i in range(6)], rho)
        if x is not None:
            b0 = np.sqrt(-x[0]) if x[0] < 0 else np.sqrt(x[0])
            sg = -1 if x[0] < 0 else 1
            betas[1] = _gauss_newton(L, rho, [b0, sg * x[1] / b0, sg * x[2] / b0, sg * x[3] / b0])
        for cand, cols in ((2, (0, 1, 2)), (3, (0, 1, 2, 3, 4))):
            x = qr_solve([[L[i][c] for c in cols] for i in range(6)], rho)
            if x is None:
                continue
            if x[0] < 0:
                b0 = np.sqrt(-x[0])
                b1 = np.sqrt(-x[2]) if x[2] < 0 else F(0.0)
            else:
                b0 = np.sqrt(x[0])
                b1 = np.sqrt(x[2]) if x[2] > 0 else F(0.0)
            if x[1] < 0:
                b0 = -b0
            b2 = x[3] / b0 if cand == 3 else F(0.0)
            betas[cand] = _gauss_newton(L, rho, [b0, b1, b2, F(0.0)])
    return betas


def _procrustes(B):
    S = np.empty((3, 3))
    for a in range(3):
        for b in range(3):
            S[a, b] = B[0, a] * B[0, b] + B[1, a] * B[1, b] + B[2, a] * B[2, b]
    A3, V3 = jacobi3(S)
    o = _order_desc3(np.diag(A3))
    sg = [np.sqrt(A3[o[k], o[k]]) if A3[o[k], o[k]] > 0.0 else F(0.0) for k in range(3)]
    Vs = V3[:, o]
    if not (sg[0] > 0.0) or not (sg[1] > 1e-14 * sg[0]):
        return None
    U = np.zeros((3, 3))
    with np.errstate(all="ignore"):
        for k in range(3):
            if k == 2 and not (sg[2] > 1e-12 * sg[0]):
                break
            for m in range(3):
                U[m, k] = (B[m, 0] * Vs[0, k] + B[m, 1] * Vs[1, k] + B[m, 2] * Vs[2, k]) / sg[k]
        if not (sg[2] > 1e-12 * sg[0]):
            U[0, 2] = U[1, 0] * U[2, 1] - U[2, 0] * U[1, 1]
            U[1, 2] = U[2, 0] * U[0, 1] - U[0, 0] * U[2, 1]
            U[2, 2] = U[0, 0] * U[1, 1] - U[1, 0] * U[0, 1]
        R = np.empty((3, 3))
        for a in range(3):
            for b in range(3):
                R[a, b] = U[a, 0] * Vs[b, 0] + U[a, 1] * Vs[b, 1] + U[a, 2] * Vs[b, 2]
    r = R.reshape(-1)
    det = r[0] * r[4] * r[8] + r[1] * r[5] * r[6] + r[2] * r[3] * r[7] - r[2] * r[4] * r[6] - r[1] * r[3] * r[8] - r[0] * r[5] * r[7]
    if det < 0:
        R[2] = -R[2]
    return R


def epnp(X, uv, K4):
    """X [n,3] world points (scaled), uv [n,2] pixels, K4 = fx, fy, cx, cy -> (pose [3,4] or None, errs [3])"""
    X = np.asarray(X, dtype=np.float64)
    uv = np.asarray(uv, dtype=np.float64)
    fx, fy, cx, cy = [F(k) for k in K4]
    n = X.shape[0]
    with np.errstate(all="ignore"):
        cw0 = np.array([_seqsum(X[:, e]) / n for e in range(3)])
        S = np.empty((3, 3))
        for a in range(3):
            for b in range(a, 3):
                S[a, b] = S[b, a] = _seqsum((X[:, a] - cw0[a]) * (X[:, b] - cw0[b]))
        A3, V3 = jacobi3(S)
        o = _order_desc3(np.diag(A3))
        sg = [np.sqrt(A3[o[k], o[k]] / n) if A3[o[k], o[k]] > 0.0 else F(0.0) for k in range(3)]
        isg = [F(1.0) / sg[k] if (sg[k] > 1e-12 * sg[0] and sg[k] > 0.0) else F(0.0) for k in range(3)]
        ax = [V3[:, o[k]] for k in range(3)]
        cw = [cw0] + [np.array([cw0[c] + sg[k] * ax[k][c] for c in range(3)]) for k in range(3)]
        d0, d1, d2 = X[:, 0] - cw0[0], X[:, 1] - cw0[1], X[:, 2] - cw0[2]
        a = [(ax[k][0] * d0 + ax[k][1] * d1 + ax[k][2] * d2) * isg[k] for k in range(3)]
        alph = np.stack([1.0 - a[0] - a[1] - a[2], a[0], a[1], a[2]], 1)
        du, dv = cx - uv[:, 0], cy - uv[:, 1]
        Mu = np.zeros((n, 12))
        Mv = np.zeros((n, 12))
        for j in range(4):
            Mu[:, 3 * j] = alph[:, j] * fx
            Mu[:, 3 * j + 2] = alph[:, j] * du
            Mv[:, 3 * j + 1] = alph[:, j] * fy
            Mv[:, 3 * j + 2] = alph[:, j] * dv
        T = np.empty((2 * n, 12, 12))
        T[0::2] = Mu[:, :, None] * Mu[:, None, :]
        T[1::2] = Mv[:, :, None] * Mv[:, None, :]
        MtM = np.cumsum(T, axis=0)[-1]
        MtM = np.triu(MtM) + np.triu(MtM, 1).T
        A, V = jacobi12(MtM)
        ordv = list(range(12))
        for i in range(12):
            for j in range(11 - i):
                if A[ordv[j + 1], ordv[j + 1]] < A[ordv[j], ordv[j]]:
                    ordv[j], ordv[j + 1] = ordv[j + 1], ordv[j]
        v = [V[:, ordv[k]] for k in range(4)]
        betas = _betas(v, cw)
        poses, errs = {}, {}
        for cand in (1, 2, 3):
            bt = betas[cand]
            ccs = bt[0] * v[0] + bt[1] * v[1] + bt[2] * v[2] + bt[3] * v[3]
            pcs = np.stack([alph[:, 0] * ccs[c] + alph[:, 1] * ccs[3 + c] + alph[:, 2] * ccs[6 + c] + alph[:, 3] * ccs[9 + c]
                            for c in range(3)], 1)
            sgn = F(-1.0) if pcs[0, 2] < 0.0 else F(1.0)
            pc0 = np.array([_seqsum(sgn * pcs[:, e]) / n for e in range(3)])
            B = np.empty((3, 3))
            for e in range(9):
                ea, eb = e // 3, e % 3
                B[ea, eb] = _seqsum((sgn * pcs[:, ea] - pc0[ea]) * (X[:, eb] - cw0[eb]))
            R = _procrustes(B)
            ok = R is not None
            if R is None:
                R = np.zeros((3, 3))   # the device leaves R unspecified here; the candidate is rejected either way
            t = np.array([pc0[r] - (R[r, 0] * cw0[0] + R[r, 1] * cw0[1] + R[r, 2] * cw0[2]) for r in range(3)])
            xc = R[0, 0] * X[:, 0] + R[0, 1] * X[:, 1] + R[0, 2] * X[:, 2] + t[0]
            yc = R[1, 0] * X[:, 0] + R[1, 1] * X[:, 1] + R[1, 2] * X[:, 2] + t[1]
            zc = R[2, 0] * X[:, 0] + R[2, 1] * X[:, 1] + R[2, 2] * X[:, 2] + t[2]
            iz = 1.0 / zc
            ue, ve = cx + fx * xc * iz, cy + fy * yc * iz
            perr = np.sqrt((uv[:, 0] - ue) * (uv[:, 0] - ue) + (uv[:, 1] - ve) * (uv[:, 1] - ve))
            s = _seqsum(perr) / n
            fin = np.isfinite(s) and abs(s) < 1e300 and np.all(np.isfinite(R)) and np.all(np.isfinite(t)) and \
                np.all(np.abs(R) < 1e300) and np.all(np.abs(t) < 1e300)
            errs[cand] = s if (ok and fin) else F(BAD)
            poses[cand] = np.concatenate([R, t[:, None]], 1)
    N = 1
    if errs[2] < errs[1]:
        N = 2
    if errs[3] < errs[N]:
        N = 3
    return (poses[N] if errs[N] < BAD else None), np.array([errs[1], errs[2], errs[3]])


def update_iters(p, ep, m, max_iters):
    """OpenCV's RANSACUpdateNumIters ((1 - ep)^m by repeated multiplication)"""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, 2.2250738585072014e-308)
    q, qm = 1.0 - ep, 1.0
    for _ in range(m):
        qm = qm * q
    denom = 1.0 - qm
    if denom < 2.2250738585072014e-308:
        return 0
    num, denom = math.log(num), math.log(denom)
    return max_iters if (denom >= 0 or -num >= max_iters * (-denom)) else int(np.rint(num / denom))


def ransac_stop(scores, n, m, confidence):
    """the sequential RANSAC loop over per-hypothesis inlier counts -> (stop index, best hypothesis or -1)"""
    niters, bc, b, it = len(scores), 0, -1, 0
    while it < niters:
        s = int(scores[it])
        if s > max(bc, m - 1):
            b, bc = it, s
            if confidence < 1.0:
                niters = update_iters(confidence, (n - s) / n, m, niters)
        it += 1
    return it, b
