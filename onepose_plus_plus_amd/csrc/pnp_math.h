// Perspective-three-point solver + pose utilities shared by the HIP PnP-RANSAC kernels
// (pnp.hip) and the host unit tests (compiled with g++: tests/test_pnp_cpu.py).
//
// Replaces, on the GPU, the pose step that follows the matcher on every caller of the hot path:
//   ransac_PnP   /root/reference/src/utils/metric_utils.py:121-204
//   (cv2.solvePnPRansac(EPNP, 10000 iterations) -> R|t ; accuracy-level parity only: OpenCV's
//    RANSAC draws from its own RNG)
// Minimal solvers: Grunert's P3P (quartic in the depth ratio, as reviewed by Haralick et al.,
// IJCV 1994) and EPnP (Lepetit et al., IJCV 2009; the reference's own, second half of this file),
// all arithmetic in double.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define OPP_HD __host__ __device__ inline
#else
#define OPP_HD inline
#endif

struct OppPose {
  double R[9];  // row-major, X_cam = R * X_world + t
  double t[3];
};

OPP_HD double opp_dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
OPP_HD void opp_cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
OPP_HD double opp_norm3(const double* a) { return sqrt(opp_dot3(a, a)); }

// real roots of x^4 + b x^3 + c x^2 + d x + e = 0 (Ferrari via the resolvent cubic), polished by
// Newton steps on the original polynomial.  Returns the number of real roots written.
OPP_HD int opp_solve_quartic(double b, double c, double d, double e, double* roots) {
  // depressed quartic y^4 + p y^2 + q y + r, x = y - b/4
  const double b2 = b * b;
  const double p = c - 0.375 * b2;
  const double q = d - 0.5 * b * c + 0.125 * b2 * b;
  const double r = e - 0.25 * b * d + 0.0625 * b2 * c - (3.0 / 256.0) * b2 * b2;
  int n = 0;
  double ys[4];
  if (fabs(q) < 1e-14 * (1.0 + fabs(p) + fabs(r))) {  // biquadratic
    const double disc = p * p - 4.0 * r;
    if (disc >= 0.0) {
      const double sq = sqrt(disc);
      const double z1 = 0.5 * (-p + sq), z2 = 0.5 * (-p - sq);
      if (z1 >= 0.0) {
        ys[n++] = sqrt(z1);
        ys[n++] = -sqrt(z1);
      }
      if (z2 >= 0.0) {
        ys[n++] = sqrt(z2);
        ys[n++] = -sqrt(z2);
      }
    }
  } else {
    // resolvent cubic  m^3 + p m^2 + (p^2/4 - r) m - q^2/8 = 0 ; take a positive real root
    const double A = p, B = 0.25 * p * p - r, C = -0.125 * q * q;
    // depressed cubic t^3 + P t + Q, m = t - A/3
    const double P = B - A * A / 3.0;
    const double Q = 2.0 * A * A * A / 27.0 - A * B / 3.0 + C;
    const double disc = 0.25 * Q * Q + P * P * P / 27.0;
    double m;
    if (disc >= 0.0) {
      const double sq = sqrt(disc);
      m = cbrt(-0.5 * Q + sq) + cbrt(-0.5 * Q - sq) - A / 3.0;
    } else {
      const double rr = sqrt(-P * P * P / 27.0);
      const double phi = acos(fmax(-1.0, fmin(1.0, -0.5 * Q / rr)));
      const double mag = 2.0 * sqrt(-P / 3.0);
      double best = -1e300;
      for (int k = 0; k < 3; ++k) {
        const double cand = mag * cos((phi + 2.0 * M_PI * k) / 3.0) - A / 3.0;
        if (cand > best) best = cand;
      }
      m = best;
    }
    if (m <= 0.0) return 0;
    const double s = sqrt(2.0 * m);
    const double t1 = -(2.0 * p + 2.0 * m) - 2.0 * q / s;  // discriminants of the two quadratics
    const double t2 = -(2.0 * p + 2.0 * m) + 2.0 * q / s;
    if (t1 >= 0.0) {
      ys[n++] = 0.5 * (s + sqrt(t1));
      ys[n++] = 0.5 * (s - sqrt(t1));
    }
    if (t2 >= 0.0) {
      ys[n++] = 0.5 * (-s + sqrt(t2));
      ys[n++] = 0.5 * (-s - sqrt(t2));
    }
  }
  for (int i = 0; i < n; ++i) {
    double x = ys[i] - 0.25 * b;
    for (int it = 0; it < 3; ++it) {  // Newton polish
      const double f = (((x + b) * x + c) * x + d) * x + e;
      const double fp = ((4.0 * x + 3.0 * b) * x + 2.0 * c) * x + d;
      if (fabs(fp) < 1e-300) break;
      x -= f / fp;
    }
    roots[i] = x;
  }
  return n;
}

// P3P.  y[3][3]: unit bearing vectors in the camera frame; x[3][3]: world points.
// Writes up to 4 poses; returns their number.
OPP_HD int opp_p3p_grunert(const double y[3][3], const double x[3][3], OppPose* out) {
  double d12[3], d13[3], d23[3];
  for (int k = 0; k < 3; ++k) {
    d12[k] = x[0][k] - x[1][k];
    d13[k] = x[0][k] - x[2][k];
    d23[k] = x[1][k] - x[2][k];
  }
  const double a2 = opp_dot3(d23, d23), b2 = opp_dot3(d13, d13), c2 = opp_dot3(d12, d12);  // a=|x2x3| b=|x1x3| c=|x1x2|
  if (a2 < 1e-24 || b2 < 1e-24 || c2 < 1e-24) return 0;
  const double ca = opp_dot3(y[1], y[2]), cb = opp_dot3(y[0], y[2]), cg = opp_dot3(y[0], y[1]);
  const double k1 = (a2 - c2) / b2, k2 = (a2 + c2) / b2, k3 = (b2 - c2) / b2, k4 = (b2 - a2) / b2;
  const double A4 = (k1 - 1.0) * (k1 - 1.0) - 4.0 * (c2 / b2) * ca * ca;
  const double A3 = 4.0 * (k1 * (1.0 - k1) * cb - (1.0 - k2) * ca * cg + 2.0 * (c2 / b2) * ca * ca * cb);
  const double A2 = 2.0 * (k1 * k1 - 1.0 + 2.0 * k1 * k1 * cb * cb + 2.0 * k3 * ca * ca - 4.0 * k2 * ca * cb * cg + 2.0 * k4 * cg * cg);
  const double A1 = 4.0 * (-k1 * (1.0 + k1) * cb + 2.0 * (a2 / b2) * cg * cg * cb - (1.0 - k2) * ca * cg);
  const double A0 = (1.0 + k1) * (1.0 + k1) - 4.0 * (a2 / b2) * cg * cg;
  if (fabs(A4) < 1e-14) return 0;
  double vs[4];
  const int nr = opp_solve_quartic(A3 / A4, A2 / A4, A1 / A4, A0 / A4, vs);
  int n = 0;
  for (int i = 0; i < nr; ++i) {
    const double v = vs[i];
    if (!(v > 0.0)) continue;
    const double den = 2.0 * (cg - v * ca);
    if (fabs(den) < 1e-12) continue;
    const double u = ((k1 - 1.0) * v * v - 2.0 * k1 * cb * v + 1.0 + k1) / den;
    if (!(u > 0.0)) continue;
    const double s1sq = b2 / (1.0 + v * v - 2.0 * v * cb);
    if (!(s1sq > 0.0)) continue;
    const double s1 = sqrt(s1sq), s2 = u * s1, s3 = v * s1;
    // camera-frame points
    double p[3][3];
    for (int k = 0; k < 3; ++k) {
      p[0][k] = s1 * y[0][k];
      p[1][k] = s2 * y[1][k];
      p[2][k] = s3 * y[2][k];
    }
    // orthonormal frames of the two triangles -> R = Fc * Fw^T
    double fw[3][3], fc[3][3], tmp[3];
    for (int f = 0; f < 2; ++f) {
      const double(*q)[3] = f == 0 ? x : p;
      double(*F)[3] = f == 0 ? fw : fc;
      double e1[3], e2[3], e3[3], w[3];
      for (int k = 0; k < 3; ++k) {
        e1[k] = q[1][k] - q[0][k];
        w[k] = q[2][k] - q[0][k];
      }
      const double n1 = opp_norm3(e1);
      for (int k = 0; k < 3; ++k) e1[k] /= n1;
      opp_cross3(e1, w, e3);
      const double n3 = opp_norm3(e3);
      if (n3 < 1e-18) return n;
      for (int k = 0; k < 3; ++k) e3[k] /= n3;
      opp_cross3(e3, e1, e2);
      for (int k = 0; k < 3; ++k) {
        F[0][k] = e1[k];
        F[1][k] = e2[k];
        F[2][k] = e3[k];
      }
    }
    OppPose P;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) P.R[r * 3 + c] = fc[0][r] * fw[0][c] + fc[1][r] * fw[1][c] + fc[2][r] * fw[2][c];
    for (int r = 0; r < 3; ++r) {
      tmp[r] = P.R[r * 3 + 0] * x[0][0] + P.R[r * 3 + 1] * x[0][1] + P.R[r * 3 + 2] * x[0][2];
      P.t[r] = p[0][r] - tmp[r];
    }
    out[n++] = P;
  }
  return n;
}

// squared reprojection error (pixels) of world point X under pose P and intrinsics K (fx, fy, cx, cy);
// returns a huge value for points behind the camera
OPP_HD double opp_reproj_err2(const OppPose& P, const double* K4, const double* X, const double* uv) {
  const double xc = P.R[0] * X[0] + P.R[1] * X[1] + P.R[2] * X[2] + P.t[0];
  const double yc = P.R[3] * X[0] + P.R[4] * X[1] + P.R[5] * X[2] + P.t[1];
  const double zc = P.R[6] * X[0] + P.R[7] * X[1] + P.R[8] * X[2] + P.t[2];
  if (!(zc > 1e-12)) return 1e300;
  const double du = K4[0] * xc / zc + K4[2] - uv[0];
  const double dv = K4[1] * yc / zc + K4[3] - uv[1];
  return du * du + dv * dv;
}

// R <- exp([w]x) * R  (Rodrigues)
OPP_HD void opp_rot_update(double* R, const double* w) {
  const double th = opp_norm3(w);
  double E[9];
  if (th < 1e-12) {
    E[0] = 1; E[1] = -w[2]; E[2] = w[1];
    E[3] = w[2]; E[4] = 1; E[5] = -w[0];
    E[6] = -w[1]; E[7] = w[0]; E[8] = 1;
  } else {
    const double k[3] = {w[0] / th, w[1] / th, w[2] / th};
    const double c = cos(th), s = sin(th), v = 1.0 - c;
    E[0] = c + k[0] * k[0] * v;        E[1] = k[0] * k[1] * v - k[2] * s; E[2] = k[0] * k[2] * v + k[1] * s;
    E[3] = k[1] * k[0] * v + k[2] * s; E[4] = c + k[1] * k[1] * v;        E[5] = k[1] * k[2] * v - k[0] * s;
    E[6] = k[2] * k[0] * v - k[1] * s; E[7] = k[2] * k[1] * v + k[0] * s; E[8] = c + k[2] * k[2] * v;
  }
  double N[9];
  for (int r = 0; r < 3; ++r)
    for (int c2 = 0; c2 < 3; ++c2) N[r * 3 + c2] = E[r * 3] * R[c2] + E[r * 3 + 1] * R[3 + c2] + E[r * 3 + 2] * R[6 + c2];
  for (int i = 0; i < 9; ++i) R[i] = N[i];
}

// solves the symmetric positive (semi-)definite 6x6 system H d = g in place (Gaussian elimination with
// partial pivoting); returns false if singular
OPP_HD bool opp_solve6(double* H, double* g) {
  for (int i = 0; i < 6; ++i) {
    int piv = i;
    for (int r = i + 1; r < 6; ++r)
      if (fabs(H[r * 6 + i]) > fabs(H[piv * 6 + i])) piv = r;
    if (fabs(H[piv * 6 + i]) < 1e-18) return false;
    if (piv != i) {
      for (int c = 0; c < 6; ++c) {
        const double t = H[i * 6 + c];
        H[i * 6 + c] = H[piv * 6 + c];
        H[piv * 6 + c] = t;
      }
      const double t = g[i];
      g[i] = g[piv];
      g[piv] = t;
    }
    for (int r = i + 1; r < 6; ++r) {
      const double f = H[r * 6 + i] / H[i * 6 + i];
      for (int c = i; c < 6; ++c) H[r * 6 + c] -= f * H[i * 6 + c];
      g[r] -= f * g[i];
    }
  }
  for (int i = 5; i >= 0; --i) {
    double s = g[i];
    for (int c = i + 1; c < 6; ++c) s -= H[i * 6 + c] * g[c];
    g[i] = s / H[i * 6 + i];
  }
  return true;
}

// accumulates one correspondence into the Gauss-Newton normal equations (upper triangle of H 6x6, g 6)
// for the update (w, dt): X_cam' = exp([w]x) (R X + t) + dt ; residual in pixels
OPP_HD void opp_gn_accumulate(const OppPose& P, const double* K4, const double* X, const double* uv, double* H, double* g) {
  const double xc = P.R[0] * X[0] + P.R[1] * X[1] + P.R[2] * X[2] + P.t[0];
  const double yc = P.R[3] * X[0] + P.R[4] * X[1] + P.R[5] * X[2] + P.t[1];
  const double zc = P.R[6] * X[0] + P.R[7] * X[1] + P.R[8] * X[2] + P.t[2];
  const double iz = 1.0 / zc;
  const double ru = K4[0] * xc * iz + K4[2] - uv[0];
  const double rv = K4[1] * yc * iz + K4[3] - uv[1];
  // d(u,v)/d(Xc)
  const double ju[3] = {K4[0] * iz, 0.0, -K4[0] * xc * iz * iz};
  const double jv[3] = {0.0, K4[1] * iz, -K4[1] * yc * iz * iz};
  // d(Xc)/d(w) = -[Xc]x ; d(Xc)/d(dt) = I
  double Ju[6], Jv[6];
  // -[Xc]x = [[0, zc, -yc], [-zc, 0, xc], [yc, -xc, 0]]
  Ju[0] = ju[0] * 0.0 + ju[1] * (-zc) + ju[2] * yc;
  Ju[1] = ju[0] * zc + ju[1] * 0.0 + ju[2] * (-xc);
  Ju[2] = ju[0] * (-yc) + ju[1] * xc + ju[2] * 0.0;
  Jv[0] = jv[0] * 0.0 + jv[1] * (-zc) + jv[2] * yc;
  Jv[1] = jv[0] * zc + jv[1] * 0.0 + jv[2] * (-xc);
  Jv[2] = jv[0] * (-yc) + jv[1] * xc + jv[2] * 0.0;
  for (int k = 0; k < 3; ++k) {
    Ju[3 + k] = ju[k];
    Jv[3 + k] = jv[k];
  }
  for (int r = 0; r < 6; ++r) {
    for (int c = r; c < 6; ++c) H[r * 6 + c] += Ju[r] * Ju[c] + Jv[r] * Jv[c];
    g[r] -= Ju[r] * ru + Jv[r] * rv;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// EPnP (V. Lepetit, F. Moreno-Noguer, P. Fua, "EPnP: An Accurate O(n) Solution to the PnP Problem", IJCV 81(2), 2009),
// structured like OpenCV's `epnp` class (the minimal and refit solver of cv2.solvePnPRansac(flags=SOLVEPNP_EPNP)).
//
// Written once for the device and the host: every stage takes (tid, nt) -- the calling thread and the number of threads
// that run it together -- and separates its phases with OPP_BARRIER() (a no-op on the host, where tid = 0, nt = 1).
// All arrays live in an OppEpnpWs (LDS on the device) or in caller-provided per-point buffers, so the kernels keep no
// indexed local arrays (no scratch).  Every sum over points runs sequentially in point order, one thread per entry, and
// FP contraction is off, so a numpy restatement with the same operation order (tests/epnp_reference.py) rounds identically.
// ---------------------------------------------------------------------------------------------------------------------
#if defined(__clang__)
#define OPP_NOFMA _Pragma("clang fp contract(off)")
#else
#define OPP_NOFMA
#endif
#if defined(__HIPCC__)
#define OPP_HDI __host__ __device__ __attribute__((always_inline)) inline
#else
#define OPP_HDI inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define OPP_BARRIER() __syncthreads()
#else
#define OPP_BARRIER() ((void)0)
#endif

#define OPP_EPNP_SWEEPS12 10   // cyclic Jacobi sweeps of the 12x12 M^T M (fixed count: deterministic, converged in <= 7)
#define OPP_EPNP_SWEEPS3 10    // sweeps of the 3x3 solves
#define OPP_EPNP_GN_ITERS 5    // Gauss-Newton iterations on the betas (OpenCV: 5)
#define OPP_EPNP_BAD 1e300     // reprojection error of a degenerate candidate

struct OppEpnpWs {
  double cw[12];              // control points, world frame [4][3]; cw[0..2] = centroid
  double ax[9];               // principal axes of the world points (rows, descending eigenvalue)
  double isg[3];              // pseudo-inverse of sqrt(lambda_k / n) (0 for a vanishing axis)
  double A[2][144], V[2][144];  // Jacobi of M^T M, double-buffered (A -> eigenvalues on the diagonal, V -> eigenvectors)
  double jd[12], jo[12];      // one parallel Jacobi step: J[i][i] and J[partner(i)][i]
  int pr[12];                 // partner index of each row / column in the step
  int ord[12];                // eigenvalues of M^T M, ascending
  double s3[9], v3[9], t3[9], u3[9];   // 3x3 symmetric eigen-solves (matrix, vectors, double-buffer partners)
  double L[60], rho[6];       // L_6x10, rho
  double qa[30], qb[6], qx[5], q1[5], q2[5];   // Householder QR least squares
  double betas[4][4];         // per candidate 1..3
  double ccs[12];             // control points, camera frame
  double pc0[3], abt[9];      // Procrustes
  double dv[12], sg[3], U[9], Vs[9];   // scratch of the serial stages
  int o3[3], cols[5];
  double Rt[4][12];           // per candidate 1..3: R row-major | t
  double err[4];              // mean reprojection error per candidate
  int best;                   // chosen candidate, 0 = degenerate
};

OPP_HDI double opp_dot3_nc(const double* a, const double* b) {
  OPP_NOFMA
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

// one symmetric Jacobi rotation (Numerical Recipes convention): J[p][p] = J[q][q] = c, J[p][q] = s, J[q][p] = -s zeroes apq
OPP_HDI void opp_jacobi_rot(double app, double aqq, double apq, double* c, double* s) {
  OPP_NOFMA
  if (apq == 0.0) {
    *c = 1.0;
    *s = 0.0;
    return;
  }
  const double th = (aqq - app) / (2.0 * apq);
  double t = 1.0 / (fabs(th) + sqrt(th * th + 1.0));
  if (th < 0.0) t = -t;
  *c = 1.0 / sqrt(t * t + 1.0);
  *s = t * *c;
}

// element e of A' = J^T A J and V' = V J for a step of disjoint rotations (pr / jd / jo describe J)
OPP_HDI void opp_jacobi_elem(const double* A, const double* V, double* A2, double* V2, int N, const int* pr, const double* jd,
                            const double* jo, int e) {
  OPP_NOFMA
  const int i = e / N, j = e % N, pi = pr[i], pj = pr[j];
  const double bij = jd[i] * A[i * N + j] + jo[i] * A[pi * N + j];
  const double bipj = jd[i] * A[i * N + pj] + jo[i] * A[pi * N + pj];
  A2[e] = bij * jd[j] + bipj * jo[j];
  V2[e] = V[i * N + j] * jd[j] + V[i * N + pj] * jo[j];
}

// round-robin (circle method) pivot order of the 12x12 solve: step s (0..10), slot k (0..5) -> pair p < q; every pair once per sweep
OPP_HDI void opp_rr_pair12(int s, int k, int* p, int* q) {
  int a, b;
  if (k == 0) {
    a = 0;
    b = 1 + s % 11;
  } else {
    a = 1 + (s + k) % 11;
    b = 1 + (s + 11 - k) % 11;
  }
  *p = a < b ? a : b;
  *q = a < b ? b : a;
}

// sets up the J of one rotation on (p, q) in pr / jd / jo
OPP_HDI void opp_jacobi_set(const double* A, int N, int p, int q, int* pr, double* jd, double* jo) {
  double c, s;
  opp_jacobi_rot(A[p * N + p], A[q * N + q], A[p * N + q], &c, &s);
  pr[p] = q;
  pr[q] = p;
  jd[p] = c;
  jd[q] = c;
  jo[p] = -s;
  jo[q] = s;
}

// serial cyclic Jacobi of a symmetric 3x3 (pivots (0,1), (0,2), (1,2)); S is destroyed, V receives the eigenvectors (columns),
// T / U are buffers of 9, pr / jd / jo of 3; on return the eigenvalues are on the diagonal of the returned matrix (S or T)
OPP_HDI const double* opp_jacobi3(double* S, double* V, double* T, double* U, int* pr, double* jd, double* jo) {
  for (int k = 0; k < 9; ++k) V[k] = (k % 4 == 0) ? 1.0 : 0.0;
  double *a = S, *v = V, *a2 = T, *v2 = U;
  for (int sw = 0; sw < OPP_EPNP_SWEEPS3; ++sw)
    for (int st = 0; st < 3; ++st) {
      const int p = st == 2 ? 1 : 0, q = st == 0 ? 1 : 2, r = 3 - p - q;
      opp_jacobi_set(a, 3, p, q, pr, jd, jo);
      pr[r] = r;
      jd[r] = 1.0;
      jo[r] = 0.0;
      for (int e = 0; e < 9; ++e) opp_jacobi_elem(a, v, a2, v2, 3, pr, jd, jo, e);
      double* t = a; a = a2; a2 = t;
      t = v; v = v2; v2 = t;
    }
  if (v != V)
    for (int k = 0; k < 9; ++k) V[k] = v[k];
  return a;
}

// order[0..2] = indices of the diagonal of a 3x3, descending (ties: lower index first)
OPP_HDI void opp_order3_desc(const double* a, int* o) {
  o[0] = 0; o[1] = 1; o[2] = 2;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 2 - i; ++j)
      if (a[o[j + 1] * 4] > a[o[j] * 4]) {
        const int t = o[j]; o[j] = o[j + 1]; o[j + 1] = t;
      }
}

// Householder QR least squares (OpenCV epnp::qr_solve): A [nr][nc] row-major (destroyed), b [nr] (destroyed) -> x [nc].
// a1 / a2: buffers of nc.  Returns false when A is singular.
OPP_HDI bool opp_qr_solve(double* A, int nr, int nc, double* b, double* x, double* a1, double* a2) {
  OPP_NOFMA
  for (int k = 0; k < nc; ++k) {
    double eta = fabs(A[k * nc + k]);
    for (int i = k + 1; i < nr; ++i)
      if (fabs(A[i * nc + k]) > eta) eta = fabs(A[i * nc + k]);
    if (!(eta > 0.0)) return false;
    double sum = 0.0;
    for (int i = k; i < nr; ++i) {
      A[i * nc + k] = A[i * nc + k] / eta;
      sum = sum + A[i * nc + k] * A[i * nc + k];
    }
    double sigma = sqrt(sum);
    if (A[k * nc + k] < 0.0) sigma = -sigma;
    A[k * nc + k] = A[k * nc + k] + sigma;
    a1[k] = sigma * A[k * nc + k];
    a2[k] = -eta * sigma;
    for (int j = k + 1; j < nc; ++j) {
      double s = 0.0;
      for (int i = k; i < nr; ++i) s = s + A[i * nc + k] * A[i * nc + j];
      const double tau = s / a1[k];
      for (int i = k; i < nr; ++i) A[i * nc + j] = A[i * nc + j] - tau * A[i * nc + k];
    }
  }
  for (int j = 0; j < nc; ++j) {
    double tau = 0.0;
    for (int i = j; i < nr; ++i) tau = tau + A[i * nc + j] * b[i];
    tau = tau / a1[j];
    for (int i = j; i < nr; ++i) b[i] = b[i] - tau * A[i * nc + j];
  }
  x[nc - 1] = b[nc - 1] / a2[nc - 1];
  for (int i = nc - 2; i >= 0; --i) {
    double s = 0.0;
    for (int j = i + 1; j < nc; ++j) s = s + A[i * nc + j] * x[j];
    x[i] = (b[i] - s) / a2[i];
  }
  return true;
}

// least squares rho ~ L[:, cols] x  (cols: the columns of L_6x10 used by one beta approximation)
OPP_HDI bool opp_epnp_ls(OppEpnpWs* w, int nc) {
  const int* cols = w->cols;
  for (int i = 0; i < 6; ++i) {
    for (int j = 0; j < nc; ++j) w->qa[i * nc + j] = w->L[i * 10 + cols[j]];
    w->qb[i] = w->rho[i];
  }
  return opp_qr_solve(w->qa, 6, nc, w->qb, w->qx, w->q1, w->q2);
}

// Gauss-Newton on the four betas (OpenCV epnp::gauss_newton / compute_A_and_b_gauss_newton)
OPP_HDI void opp_epnp_gauss_newton(OppEpnpWs* w, double* bt) {
  OPP_NOFMA
  for (int it = 0; it < OPP_EPNP_GN_ITERS; ++it) {
    for (int i = 0; i < 6; ++i) {
      const double* l = w->L + i * 10;
      double* a = w->qa + i * 4;
      a[0] = 2 * l[0] * bt[0] + l[1] * bt[1] + l[3] * bt[2] + l[6] * bt[3];
      a[1] = l[1] * bt[0] + 2 * l[2] * bt[1] + l[4] * bt[2] + l[7] * bt[3];
      a[2] = l[3] * bt[0] + l[4] * bt[1] + 2 * l[5] * bt[2] + l[8] * bt[3];
      a[3] = l[6] * bt[0] + l[7] * bt[1] + l[8] * bt[2] + 2 * l[9] * bt[3];
      w->qb[i] = w->rho[i] - (l[0] * bt[0] * bt[0] + l[1] * bt[0] * bt[1] + l[2] * bt[1] * bt[1] + l[3] * bt[0] * bt[2] +
                              l[4] * bt[1] * bt[2] + l[5] * bt[2] * bt[2] + l[6] * bt[0] * bt[3] + l[7] * bt[1] * bt[3] +
                              l[8] * bt[2] * bt[3] + l[9] * bt[3] * bt[3]);
    }
    if (!opp_qr_solve(w->qa, 6, 4, w->qb, w->qx, w->q1, w->q2)) return;
    for (int k = 0; k < 4; ++k) bt[k] = bt[k] + w->qx[k];
  }
}

// eigenvector k (0 = smallest eigenvalue) of M^T M, component m
#define OPP_EPNP_V(w, vb, k, m) ((vb)[(m) * 12 + (w)->ord[k]])

// L_6x10, rho, the three beta initialisations (approx_1 / 2 / 3) and their Gauss-Newton refinement.  Serial.
OPP_HDI void opp_epnp_betas(OppEpnpWs* w, const double* vb) {
  OPP_NOFMA
  for (int i = 0; i < 6; ++i) {   // control-point pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
    const int pa = i < 3 ? 0 : (i < 5 ? 1 : 2), pb = i < 3 ? i + 1 : (i < 5 ? i - 1 : 3);
    double* dv = w->dv;
    for (int k = 0; k < 4; ++k)
      for (int c = 0; c < 3; ++c) dv[3 * k + c] = OPP_EPNP_V(w, vb, k, 3 * pa + c) - OPP_EPNP_V(w, vb, k, 3 * pb + c);
    double* r = w->L + i * 10;
    r[0] = opp_dot3_nc(dv, dv);
    r[1] = 2 * opp_dot3_nc(dv, dv + 3);
    r[2] = opp_dot3_nc(dv + 3, dv + 3);
    r[3] = 2 * opp_dot3_nc(dv, dv + 6);
    r[4] = 2 * opp_dot3_nc(dv + 3, dv + 6);
    r[5] = opp_dot3_nc(dv + 6, dv + 6);
    r[6] = 2 * opp_dot3_nc(dv, dv + 9);
    r[7] = 2 * opp_dot3_nc(dv + 3, dv + 9);
    r[8] = 2 * opp_dot3_nc(dv + 6, dv + 9);
    r[9] = opp_dot3_nc(dv + 9, dv + 9);
    const double* a = w->cw + 3 * pa;
    const double* b = w->cw + 3 * pb;
    w->rho[i] = (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
  }
  for (int c = 1; c <= 3; ++c)
    for (int k = 0; k < 4; ++k) w->betas[c][k] = 0.0;
  {  // approx_1: B11 B12 B13 B14
    w->cols[0] = 0; w->cols[1] = 1; w->cols[2] = 3; w->cols[3] = 6;
    double* bt = w->betas[1];
    if (opp_epnp_ls(w, 4)) {
      const double* x = w->qx;
      if (x[0] < 0) {
        bt[0] = sqrt(-x[0]);
        bt[1] = -x[1] / bt[0];
        bt[2] = -x[2] / bt[0];
        bt[3] = -x[3] / bt[0];
      } else {
        bt[0] = sqrt(x[0]);
        bt[1] = x[1] / bt[0];
        bt[2] = x[2] / bt[0];
        bt[3] = x[3] / bt[0];
      }
      opp_epnp_gauss_newton(w, bt);
    }
  }
  {  // approx_2: B11 B12 B22
    w->cols[0] = 0; w->cols[1] = 1; w->cols[2] = 2;
    double* bt = w->betas[2];
    if (opp_epnp_ls(w, 3)) {
      const double* x = w->qx;
      if (x[0] < 0) {
        bt[0] = sqrt(-x[0]);
        bt[1] = (x[2] < 0) ? sqrt(-x[2]) : 0.0;
      } else {
        bt[0] = sqrt(x[0]);
        bt[1] = (x[2] > 0) ? sqrt(x[2]) : 0.0;
      }
      if (x[1] < 0) bt[0] = -bt[0];
      opp_epnp_gauss_newton(w, bt);
    }
  }
  {  // approx_3: B11 B12 B22 B13 B23
    for (int k = 0; k < 5; ++k) w->cols[k] = k;
    double* bt = w->betas[3];
    if (opp_epnp_ls(w, 5)) {
      const double* x = w->qx;
      if (x[0] < 0) {
        bt[0] = sqrt(-x[0]);
        bt[1] = (x[2] < 0) ? sqrt(-x[2]) : 0.0;
      } else {
        bt[0] = sqrt(x[0]);
        bt[1] = (x[2] > 0) ? sqrt(x[2]) : 0.0;
      }
      if (x[1] < 0) bt[0] = -bt[0];
      bt[2] = x[3] / bt[0];
      opp_epnp_gauss_newton(w, bt);
    }
  }
}

// R (row-major) = U V^T from the 3x3 cross-covariance abt (camera x world) via the eigen-solve of abt^T abt; OpenCV's sign fix
// (negate the last row when det R < 0).  Serial.  Returns false for a rank <= 1 cross-covariance.
OPP_HDI bool opp_epnp_procrustes(OppEpnpWs* w, double* R) {
  OPP_NOFMA
  const double* B = w->abt;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) w->s3[a * 3 + b] = B[0 * 3 + a] * B[0 * 3 + b] + B[1 * 3 + a] * B[1 * 3 + b] + B[2 * 3 + a] * B[2 * 3 + b];
  const double* ev = opp_jacobi3(w->s3, w->v3, w->t3, w->u3, w->pr, w->jd, w->jo);
  int* o = w->o3;
  opp_order3_desc(ev, o);
  double *sg = w->sg, *U = w->U, *Vs = w->Vs;
  for (int k = 0; k < 3; ++k) {
    const double l = ev[o[k] * 4];
    sg[k] = l > 0.0 ? sqrt(l) : 0.0;
    for (int m = 0; m < 3; ++m) Vs[m * 3 + k] = w->v3[m * 3 + o[k]];
  }
  if (!(sg[0] > 0.0) || !(sg[1] > 1e-14 * sg[0])) return false;
  for (int k = 0; k < 3; ++k) {
    if (k == 2 && !(sg[2] > 1e-12 * sg[0])) break;
    for (int m = 0; m < 3; ++m) U[m * 3 + k] = (B[m * 3 + 0] * Vs[0 * 3 + k] + B[m * 3 + 1] * Vs[1 * 3 + k] + B[m * 3 + 2] * Vs[2 * 3 + k]) / sg[k];
  }
  if (!(sg[2] > 1e-12 * sg[0])) {   // (near-)coplanar camera points: complete the frame
    U[0 * 3 + 2] = U[1 * 3 + 0] * U[2 * 3 + 1] - U[2 * 3 + 0] * U[1 * 3 + 1];
    U[1 * 3 + 2] = U[2 * 3 + 0] * U[0 * 3 + 1] - U[0 * 3 + 0] * U[2 * 3 + 1];
    U[2 * 3 + 2] = U[0 * 3 + 0] * U[1 * 3 + 1] - U[1 * 3 + 0] * U[0 * 3 + 1];
  }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) R[a * 3 + b] = U[a * 3 + 0] * Vs[b * 3 + 0] + U[a * 3 + 1] * Vs[b * 3 + 1] + U[a * 3 + 2] * Vs[b * 3 + 2];
  const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] -
                     R[0] * R[5] * R[7];
  if (det < 0) {
    R[6] = -R[6];
    R[7] = -R[7];
    R[8] = -R[8];
  }
  return true;
}

OPP_HDI bool opp_finite(double x) { return x == x && fabs(x) < 1e300; }

// cyclic Jacobi of w->A[0] (V[0] = I), six disjoint rotations per step (round-robin order), 11 steps per sweep; the buffers
// alternate every step.  Returns the buffer index holding the result.  Every one of the nt threads calls it.
OPP_HDI int opp_jacobi12(OppEpnpWs* w, int tid, int nt) {
  int cur = 0;
  for (int sw = 0; sw < OPP_EPNP_SWEEPS12; ++sw)
    for (int st = 0; st < 11; ++st) {
      for (int k = tid; k < 6; k += nt) {
        int p, q;
        opp_rr_pair12(st, k, &p, &q);
        opp_jacobi_set(w->A[cur], 12, p, q, w->pr, w->jd, w->jo);
      }
      OPP_BARRIER();
      for (int e = tid; e < 144; e += nt) opp_jacobi_elem(w->A[cur], w->V[cur], w->A[cur ^ 1], w->V[cur ^ 1], 12, w->pr, w->jd, w->jo, e);
      OPP_BARRIER();
      cur ^= 1;
    }
  return cur;
}

// EPnP on n >= 4 correspondences.  X [n][3] world points (already scaled), uv [n][2] pixels, K4 = fx, fy, cx, cy.
// alph [n][4], pcs [n][3], perr [n]: per-point buffers.  Every one of the nt threads calls it (it contains barriers).
// On return (all threads) w->best > 0 and w->Rt[w->best] holds the pose, or w->best == 0 for a degenerate input.
OPP_HDI void opp_epnp_solve(const double* X, const double* uv, int n, const double* K4, OppEpnpWs* w, double* alph, double* pcs,
                           double* perr, int tid, int nt) {
  OPP_NOFMA
  // centroid and scatter matrix of the world points (sequential in point order, one thread per entry)
  for (int e = tid; e < 3; e += nt) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s = s + X[3 * i + e];
    w->cw[e] = s / n;
  }
  OPP_BARRIER();
  for (int e = tid; e < 6; e += nt) {
    const int a = e < 3 ? 0 : (e < 5 ? 1 : 2), b = e < 3 ? e : (e < 5 ? e - 2 : 2);
    double s = 0.0;
    for (int i = 0; i < n; ++i) s = s + (X[3 * i + a] - w->cw[a]) * (X[3 * i + b] - w->cw[b]);
    w->s3[a * 3 + b] = s;
    w->s3[b * 3 + a] = s;
  }
  OPP_BARRIER();
  // control points: centroid + sqrt(lambda_k / n) e_k along the principal axes; pseudo-inverse of their offsets
  if (tid == 0) {
    const double* ev = opp_jacobi3(w->s3, w->v3, w->t3, w->u3, w->pr, w->jd, w->jo);
    int* o = w->o3;
    opp_order3_desc(ev, o);
    double* sg = w->sg;
    for (int k = 0; k < 3; ++k) {
      const double l = ev[o[k] * 4];
      sg[k] = l > 0.0 ? sqrt(l / n) : 0.0;
    }
    for (int k = 0; k < 3; ++k) {
      w->isg[k] = (sg[k] > 1e-12 * sg[0] && sg[k] > 0.0) ? 1.0 / sg[k] : 0.0;
      for (int c = 0; c < 3; ++c) {
        w->ax[k * 3 + c] = w->v3[c * 3 + o[k]];
        w->cw[3 * (k + 1) + c] = w->cw[c] + sg[k] * w->ax[k * 3 + c];
      }
    }
  }
  OPP_BARRIER();
  // barycentric coordinates
  for (int i = tid; i < n; i += nt) {
    const double d0 = X[3 * i] - w->cw[0], d1 = X[3 * i + 1] - w->cw[1], d2 = X[3 * i + 2] - w->cw[2];
    const double a0 = (w->ax[0] * d0 + w->ax[1] * d1 + w->ax[2] * d2) * w->isg[0];
    const double a1 = (w->ax[3] * d0 + w->ax[4] * d1 + w->ax[5] * d2) * w->isg[1];
    const double a2 = (w->ax[6] * d0 + w->ax[7] * d1 + w->ax[8] * d2) * w->isg[2];
    alph[4 * i + 0] = 1.0 - a0 - a1 - a2;
    alph[4 * i + 1] = a0;
    alph[4 * i + 2] = a1;
    alph[4 * i + 3] = a2;
  }
  OPP_BARRIER();
  // M^T M: upper triangle, one thread per entry, rows of M in point order (u row, then v row)
  for (int e = tid; e < 78; e += nt) {
    int r = 0, f = e;
    while (f >= 12 - r) {
      f -= 12 - r;
      ++r;
    }
    const int c = r + f;
    const int jr = r / 3, kr = r % 3, jc = c / 3, kc = c % 3;
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
      const double ar = alph[4 * i + jr], ac = alph[4 * i + jc];
      const double du = K4[2] - uv[2 * i], dv = K4[3] - uv[2 * i + 1];
      const double mur = kr == 0 ? ar * K4[0] : (kr == 1 ? 0.0 : ar * du);
      const double muc = kc == 0 ? ac * K4[0] : (kc == 1 ? 0.0 : ac * du);
      const double mvr = kr == 0 ? 0.0 : (kr == 1 ? ar * K4[1] : ar * dv);
      const double mvc = kc == 0 ? 0.0 : (kc == 1 ? ac * K4[1] : ac * dv);
      s = s + mur * muc;
      s = s + mvr * mvc;
    }
    w->A[0][r * 12 + c] = s;
    w->A[0][c * 12 + r] = s;
    w->V[0][r * 12 + c] = r == c ? 1.0 : 0.0;
    w->V[0][c * 12 + r] = r == c ? 1.0 : 0.0;
  }
  OPP_BARRIER();
  const int cur = opp_jacobi12(w, tid, nt);
  const double* vb = w->V[cur];
  if (tid == 0) {
    for (int k = 0; k < 12; ++k) w->ord[k] = k;   // ascending eigenvalues, ties: lower index first
    for (int i = 0; i < 12; ++i)
      for (int j = 0; j < 11 - i; ++j)
        if (w->A[cur][w->ord[j + 1] * 13] < w->A[cur][w->ord[j] * 13]) {
          const int t = w->ord[j]; w->ord[j] = w->ord[j + 1]; w->ord[j + 1] = t;
        }
    opp_epnp_betas(w, vb);
  }
  OPP_BARRIER();
  for (int cand = 1; cand <= 3; ++cand) {
    if (tid == 0) {   // control points in the camera frame
      for (int m = 0; m < 12; ++m) {
        const double* bt = w->betas[cand];
        w->ccs[m] = bt[0] * OPP_EPNP_V(w, vb, 0, m) + bt[1] * OPP_EPNP_V(w, vb, 1, m) + bt[2] * OPP_EPNP_V(w, vb, 2, m) +
                    bt[3] * OPP_EPNP_V(w, vb, 3, m);
      }
    }
    OPP_BARRIER();
    for (int i = tid; i < n; i += nt)
      for (int c = 0; c < 3; ++c)
        pcs[3 * i + c] = alph[4 * i] * w->ccs[c] + alph[4 * i + 1] * w->ccs[3 + c] + alph[4 * i + 2] * w->ccs[6 + c] +
                         alph[4 * i + 3] * w->ccs[9 + c];
    OPP_BARRIER();
    const double sgn = pcs[2] < 0.0 ? -1.0 : 1.0;   // solve_for_sign: the first point in front of the camera
    for (int e = tid; e < 3; e += nt) {
      double s = 0.0;
      for (int i = 0; i < n; ++i) s = s + sgn * pcs[3 * i + e];
      w->pc0[e] = s / n;
    }
    OPP_BARRIER();
    for (int e = tid; e < 9; e += nt) {
      const int a = e / 3, b = e % 3;
      double s = 0.0;
      for (int i = 0; i < n; ++i) s = s + (sgn * pcs[3 * i + a] - w->pc0[a]) * (X[3 * i + b] - w->cw[b]);
      w->abt[e] = s;
    }
    OPP_BARRIER();
    if (tid == 0) {
      double* P = w->Rt[cand];
      const bool ok = opp_epnp_procrustes(w, P);
      for (int a = 0; a < 3; ++a) P[9 + a] = w->pc0[a] - (P[a * 3] * w->cw[0] + P[a * 3 + 1] * w->cw[1] + P[a * 3 + 2] * w->cw[2]);
      w->err[cand] = ok ? 0.0 : OPP_EPNP_BAD;
    }
    OPP_BARRIER();
    for (int i = tid; i < n; i += nt) {
      const double* P = w->Rt[cand];
      const double* x = X + 3 * i;
      const double xc = P[0] * x[0] + P[1] * x[1] + P[2] * x[2] + P[9];
      const double yc = P[3] * x[0] + P[4] * x[1] + P[5] * x[2] + P[10];
      const double zc = P[6] * x[0] + P[7] * x[1] + P[8] * x[2] + P[11];
      const double iz = 1.0 / zc;
      const double ue = K4[2] + K4[0] * xc * iz, ve = K4[3] + K4[1] * yc * iz;
      perr[i] = sqrt((uv[2 * i] - ue) * (uv[2 * i] - ue) + (uv[2 * i + 1] - ve) * (uv[2 * i + 1] - ve));
    }
    OPP_BARRIER();
    if (tid == 0) {
      double s = 0.0;
      for (int i = 0; i < n; ++i) s = s + perr[i];
      s = s / n;
      bool fin = opp_finite(s);
      for (int k = 0; k < 12; ++k) fin = fin && opp_finite(w->Rt[cand][k]);
      if (w->err[cand] == 0.0) w->err[cand] = fin ? s : OPP_EPNP_BAD;
    }
    OPP_BARRIER();
  }
  if (tid == 0) {
    int N = 1;
    if (w->err[2] < w->err[1]) N = 2;
    if (w->err[3] < w->err[N]) N = 3;
    w->best = w->err[N] < OPP_EPNP_BAD ? N : 0;
  }
  OPP_BARRIER();
}

// OpenCV's RANSACUpdateNumIters (repeated multiplication in place of std::pow)
OPP_HDI int opp_ransac_update_iters(double p, double ep, int m, int max_iters) {
  OPP_NOFMA
  p = fmax(p, 0.0);
  p = fmin(p, 1.0);
  ep = fmax(ep, 0.0);
  ep = fmin(ep, 1.0);
  double num = 1.0 - p;
  if (num < 2.2250738585072014e-308) num = 2.2250738585072014e-308;
  const double q = 1.0 - ep;
  double qm = 1.0;
  for (int k = 0; k < m; ++k) qm = qm * q;
  double denom = 1.0 - qm;
  if (denom < 2.2250738585072014e-308) return 0;
  num = log(num);
  denom = log(denom);
  return (denom >= 0 || -num >= max_iters * (-denom)) ? max_iters : (int)rint(num / denom);
}

// the sequential RANSAC loop over per-hypothesis inlier counts (score < 0: no model): a hypothesis becomes the best when its
// count > max(best count, m - 1); after each new best niters = update(...) unless confidence >= 1.  Returns the number of
// hypotheses the loop evaluates (the stop index); *best = the best hypothesis, -1 if none qualified.
OPP_HDI int opp_ransac_stop(const int* score, int iters, int n, int m, double confidence, int* best) {
  int niters = iters, bc = 0, b = -1, it = 0;
  for (; it < niters; ++it) {
    const int s = score[it];
    if (s > (bc > m - 1 ? bc : m - 1)) {
      b = it;
      bc = s;
      if (confidence < 1.0) niters = opp_ransac_update_iters(confidence, (double)(n - s) / n, m, niters);
    }
  }
  *best = b;
  return it;
}

// ---------------------------------------------------------------------------------------------------------------------
// LO-RANSAC with robust refinement (COLMAP 3.8 EstimateAbsolutePose: LORANSAC<P3PEstimator, EPNPEstimator>, then
// RefineAbsolutePose under a Cauchy loss -- the reference's `use_pycolmap_ransac=True` branch, metric_utils.py:137-170).
// The pieces that decide something -- support order, trial bound, the sequential walk over the candidate models, the
// Levenberg-Marquardt refinement -- are written once for the device (pnp_lo.hip) and the host (tests/loransac_host.cpp).
// ---------------------------------------------------------------------------------------------------------------------
#define OPP_LO_ROUNDS 10          // local optimisations per new best (COLMAP kMaxNumLocalTrials)
#define OPP_LO_MIN_INLIERS 4      // LO runs with more inliers than this (the EPnP estimator's minimal sample)
#define OPP_LO_NOSUM 1.7976931348623157e308   // residual sum of "no model yet"
#define OPP_LM_MAX_ITERS 100
#define OPP_LM_LAMBDA0 1e-4       // initial damping (Ceres' initial trust-region radius 1e4)
#define OPP_LM_FACTOR 10.0        // the damping is divided by it after an accepted step, multiplied after a rejected one
#define OPP_LM_LAMBDA_MIN 1e-12
#define OPP_LM_LAMBDA_MAX 1e16    // "the damping overflows"
#define OPP_LM_MIN_GAIN 1e-3      // a step is taken when the cost falls by this fraction of the predicted decrease (Ceres' min_relative_decrease)
#define OPP_LM_GRAD_TOL 1.0       // COLMAP's gradient_tolerance on the max-norm of the gradient
#define OPP_LM_ROW 16             // doubles per point: Ju[6], Jv[6], ru, rv, weight, rho

// support (inlier count, sum of the inliers' squared residuals) a is better than b
OPP_HDI bool opp_support_better(int ca, double sa, int cb, double sb) { return ca > cb || (ca == cb && sa < sb); }

// trials needed so that an all-inlier 3-sample was drawn with probability `confidence`, times COLMAP's multiplier 3:
// ceil(3 log(1 - confidence) / log(1 - r^3)), r = cnt / n.  confidence >= 1: the cap; r = 1: 0; log(1 - r^3) = 0: the cap.
OPP_HDI int opp_lo_dyn(double confidence, int cnt, int n, int cap) {
  OPP_NOFMA
  if (!(confidence < 1.0)) return cap;
  if (cnt >= n) return 0;
  const double r = (double)cnt / n;
  const double den = log(1.0 - r * r * r);
  if (!(den < 0.0)) return cap;
  const double v = 3.0 * log(1.0 - confidence) / den;
  return v >= (double)cap ? cap : (int)ceil(v);
}

// The sequential loop over the candidate models.  cand_idx[c] = 4 * trial + model, ascending; (rc, rs)[c] the support of the
// model itself, (lc, ls)[c] its support after local optimisation (equal to the raw one when LO did not run or did not help).
// A candidate is taken when the loop has not ended before its trial and its raw support beats the best so far; the best then
// becomes its LO support and the bound follows.  The loop ends at the first trial t >= dyn and >= min_trials (checked before a
// trial starts, so the models of the current trial are all seen).  Returns the stop index; *best = the last candidate taken
// (-1: none); taken[c] (may be NULL) = 1 for the candidates taken.
OPP_HDI int opp_lo_resolve(const int* cand_idx, const int* rc, const double* rs, const int* lc, const double* ls, int ncand, int n,
                           double confidence, int min_trials, int cap, int* best, int* taken) {
  int bc = 0, b = -1, dyn = cap, last = -1;
  double bs = OPP_LO_NOSUM;
  bool ended = false;
  for (int c = 0; c < ncand; ++c) {
    const int t = cand_idx[c] >> 2;
    int end = dyn > min_trials ? dyn : min_trials;
    if (last + 1 > end) end = last + 1;
    ended = ended || t >= end;
    const bool live = !ended && opp_support_better(rc[c], rs[c], bc, bs);
    if (taken) taken[c] = live ? 1 : 0;
    if (live) {
      bc = lc[c];
      bs = ls[c];
      b = c;
      last = t;
      dyn = opp_lo_dyn(confidence, bc, n, cap);
    }
  }
  int end = dyn > min_trials ? dyn : min_trials;
  if (last + 1 > end) end = last + 1;
  *best = b;
  return end < cap ? end : cap;
}

struct OppLmWs {
  OppPose P, N;            // the accepted pose, the trial pose
  double H[36], g[6];      // normal equations at P (H symmetric, H d = g)
  double A[36], d[6];      // the damped system and its solution
  double cost, cost_new;   // sum of log(1 + s_i) at P / at N
  double pred;             // decrease of the cost that the linearised model predicts for the step: d . (g + lambda diag(H) d)
  double lambda;
  int iters;               // damped systems solved
  int done, ok, acc;
};

// one point of the robust problem at pose P: the Jacobian rows of (u, v) with respect to the update (w, dt) of
// X_cam' = exp([w]x) (R X + t) + dt, the residual, the first-order Cauchy weight 1 / (1 + s) and rho = log(1 + s), s = |r|^2.
// A point at or behind the camera gets weight 0 and rho 1e300, so a step that puts one there is rejected.
OPP_HDI void opp_lm_row(const OppPose& P, const double* K4, const double* X, const double* uv, double* row) {
  OPP_NOFMA
  const double xc = P.R[0] * X[0] + P.R[1] * X[1] + P.R[2] * X[2] + P.t[0];
  const double yc = P.R[3] * X[0] + P.R[4] * X[1] + P.R[5] * X[2] + P.t[1];
  const double zc = P.R[6] * X[0] + P.R[7] * X[1] + P.R[8] * X[2] + P.t[2];
  if (!(zc > 1e-12)) {
    for (int k = 0; k < 15; ++k) row[k] = 0.0;
    row[15] = 1e300;
    return;
  }
  const double iz = 1.0 / zc;
  const double ru = K4[0] * xc * iz + K4[2] - uv[0];
  const double rv = K4[1] * yc * iz + K4[3] - uv[1];
  const double ju0 = K4[0] * iz, ju2 = -K4[0] * xc * iz * iz;
  const double jv1 = K4[1] * iz, jv2 = -K4[1] * yc * iz * iz;
  row[0] = ju2 * yc;
  row[1] = ju0 * zc - ju2 * xc;
  row[2] = -ju0 * yc;
  row[3] = ju0;
  row[4] = 0.0;
  row[5] = ju2;
  row[6] = -jv1 * zc + jv2 * yc;
  row[7] = -jv2 * xc;
  row[8] = jv1 * xc;
  row[9] = 0.0;
  row[10] = jv1;
  row[11] = jv2;
  const double s = ru * ru + rv * rv;
  row[12] = ru;
  row[13] = rv;
  row[14] = 1.0 / (1.0 + s);
  row[15] = log(1.0 + s);
}

// entry e of the sums over the rows, in point order: e < 21 the upper triangle of H (row-major), 21..26 g, 27 the cost
OPP_HDI double opp_lm_sum(const double* rows, int n, int e) {
  OPP_NOFMA
  double s = 0.0;
  if (e == 27) {
    for (int i = 0; i < n; ++i) s = s + rows[(size_t)i * OPP_LM_ROW + 15];
    return s;
  }
  if (e >= 21) {
    const int k = e - 21;
    for (int i = 0; i < n; ++i) {
      const double* r = rows + (size_t)i * OPP_LM_ROW;
      s = s - r[14] * (r[k] * r[12] + r[6 + k] * r[13]);
    }
    return s;
  }
  int a = 0, f = e;
  while (f >= 6 - a) {
    f -= 6 - a;
    ++a;
  }
  const int b = a + f;
  for (int i = 0; i < n; ++i) {
    const double* r = rows + (size_t)i * OPP_LM_ROW;
    s = s + r[14] * (r[a] * r[b] + r[6 + a] * r[6 + b]);
  }
  return s;
}

OPP_HDI void opp_lm_store(OppLmWs* w, int e, double v) {
  if (e >= 21) {
    w->g[e - 21] = v;
    return;
  }
  int a = 0, f = e;
  while (f >= 6 - a) {
    f -= 6 - a;
    ++a;
  }
  w->H[a * 6 + a + f] = v;
  w->H[(a + f) * 6 + a] = v;
}

// the damped step from w->P: (H + lambda diag H) d = g, N = the updated pose.  Serial.  False when the system is singular.
OPP_HDI bool opp_lm_step(OppLmWs* w) {
  for (int k = 0; k < 36; ++k) w->A[k] = w->H[k];
  for (int k = 0; k < 6; ++k) {
    w->A[k * 7] = w->H[k * 7] + w->lambda * w->H[k * 7];
    w->d[k] = w->g[k];
  }
  if (!opp_solve6(w->A, w->d)) return false;
  for (int k = 0; k < 6; ++k)
    if (!opp_finite(w->d[k])) return false;
  double pred = 0.0;
  for (int k = 0; k < 6; ++k) pred = pred + w->d[k] * (w->g[k] + w->lambda * w->H[k * 7] * w->d[k]);
  w->pred = pred;
  w->N = w->P;
  opp_rot_update(w->N.R, w->d);
  double E[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  opp_rot_update(E, w->d);
  for (int r = 0; r < 3; ++r) w->N.t[r] = E[r * 3] * w->P.t[0] + E[r * 3 + 1] * w->P.t[1] + E[r * 3 + 2] * w->P.t[2] + w->d[3 + r];
  return true;
}

// accept / reject: the step is taken only when the robust cost decreases, by at least OPP_LM_MIN_GAIN of the predicted decrease
// (near convergence cost - cost_new is a difference of nearly equal sums; against the prediction the decision stays far from
// its rounding error, where a bare cost_new < cost would not)
OPP_HDI void opp_lm_accept(OppLmWs* w) {
  w->acc = (w->pred > 0.0 && w->cost - w->cost_new > OPP_LM_MIN_GAIN * w->pred) ? 1 : 0;
  if (w->acc) {
    w->P = w->N;
    w->cost = w->cost_new;
    w->lambda = w->lambda / OPP_LM_FACTOR;
    if (w->lambda < OPP_LM_LAMBDA_MIN) w->lambda = OPP_LM_LAMBDA_MIN;
  } else {
    w->lambda = w->lambda * OPP_LM_FACTOR;
    if (w->lambda > OPP_LM_LAMBDA_MAX) w->done = 1;
  }
}

// Levenberg-Marquardt on sum_i log(1 + |pi(R X_i + t) - uv_i|^2) over the n points X [n][3], uv [n][2], from w->P.
// rows: n * OPP_LM_ROW doubles.  Every one of the nt threads calls it (it contains barriers); on return w->P is the refined
// pose, w->iters the damped systems solved, w->cost the robust cost at w->P.  Stops at |g|_inf <= OPP_LM_GRAD_TOL, after
// OPP_LM_MAX_ITERS iterations or when the damping passes OPP_LM_LAMBDA_MAX.
OPP_HDI void opp_lm_refine(const double* X, const double* uv, int n, const double* K4, OppLmWs* w, double* rows, int tid, int nt) {
  if (tid == 0) {
    w->lambda = OPP_LM_LAMBDA0;
    w->iters = 0;
    w->done = 0;
  }
  for (int i = tid; i < n; i += nt) opp_lm_row(w->P, K4, X + 3 * (size_t)i, uv + 2 * (size_t)i, rows + (size_t)i * OPP_LM_ROW);
  OPP_BARRIER();
  for (int e = tid; e < 28; e += nt) {
    const double v = opp_lm_sum(rows, n, e);
    if (e == 27) w->cost = v; else opp_lm_store(w, e, v);
  }
  OPP_BARRIER();
  for (int it = 0; it < OPP_LM_MAX_ITERS; ++it) {
    if (tid == 0) {
      double gm = 0.0;
      for (int k = 0; k < 6; ++k) gm = fmax(gm, fabs(w->g[k]));
      if (!(gm > OPP_LM_GRAD_TOL)) w->done = 1;
      if (!w->done) {
        w->iters = w->iters + 1;
        w->ok = opp_lm_step(w) ? 1 : 0;
      }
    }
    OPP_BARRIER();
    const int done = w->done, ok = w->ok;
    OPP_BARRIER();   // every thread has read them before thread 0 writes again
    if (done) break;
    if (ok) {
      for (int i = tid; i < n; i += nt) opp_lm_row(w->N, K4, X + 3 * (size_t)i, uv + 2 * (size_t)i, rows + (size_t)i * OPP_LM_ROW);
      OPP_BARRIER();
      if (tid == 0) {
        w->cost_new = opp_lm_sum(rows, n, 27);
        opp_lm_accept(w);
      }
      OPP_BARRIER();
      if (w->acc)
        for (int e = tid; e < 27; e += nt) opp_lm_store(w, e, opp_lm_sum(rows, n, e));
    } else if (tid == 0) {   // a singular damped system: more damping
      w->cost_new = w->cost;
      w->pred = 0.0;
      opp_lm_accept(w);
    }
    OPP_BARRIER();
  }
  OPP_BARRIER();
}
