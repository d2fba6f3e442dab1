// Host build of the PnP math (onepose_plus_plus_amd/csrc/pnp_math.h) for CPU unit tests.
#include "../onepose_plus_plus_amd/csrc/pnp_math.h"

extern "C" {
int t_quartic(double b, double c, double d, double e, double* roots) { return opp_solve_quartic(b, c, d, e, roots); }

// y [3][3] unit bearings, x [3][3] world points -> poses as 12 doubles each (R row-major | t)
int t_p3p(const double* y, const double* x, double* out) {
  double yy[3][3], xx[3][3];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) {
      yy[i][k] = y[i * 3 + k];
      xx[i][k] = x[i * 3 + k];
    }
  OppPose P[4];
  const int n = opp_p3p_grunert(yy, xx, P);
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < 9; ++k) out[i * 12 + k] = P[i].R[k];
    for (int k = 0; k < 3; ++k) out[i * 12 + 9 + k] = P[i].t[k];
  }
  return n;
}

// Gauss-Newton refinement over n correspondences; pose in/out as 12 doubles
int t_refine(double* pose, const double* K4, const double* X, const double* uv, int n, int iters) {
  OppPose P;
  for (int k = 0; k < 9; ++k) P.R[k] = pose[k];
  for (int k = 0; k < 3; ++k) P.t[k] = pose[9 + k];
  for (int it = 0; it < iters; ++it) {
    double H[36] = {0}, g[6] = {0};
    for (int i = 0; i < n; ++i) opp_gn_accumulate(P, K4, X + 3 * i, uv + 2 * i, H, g);
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < r; ++c) H[r * 6 + c] = H[c * 6 + r];
    if (!opp_solve6(H, g)) return -1;
    opp_rot_update(P.R, g);
    double nt[3];
    double E[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    opp_rot_update(E, g);
    for (int r = 0; r < 3; ++r) nt[r] = E[r * 3] * P.t[0] + E[r * 3 + 1] * P.t[1] + E[r * 3 + 2] * P.t[2] + g[3 + r];
    for (int r = 0; r < 3; ++r) P.t[r] = nt[r];
  }
  for (int k = 0; k < 9; ++k) pose[k] = P.R[k];
  for (int k = 0; k < 3; ++k) pose[9 + k] = P.t[k];
  return 0;
}

double t_reproj(const double* pose, const double* K4, const double* X, const double* uv) {
  OppPose P;
  for (int k = 0; k < 9; ++k) P.R[k] = pose[k];
  for (int k = 0; k < 3; ++k) P.t[k] = pose[9 + k];
  return opp_reproj_err2(P, K4, X, uv);
}

// The steps of the P3P kernels (csrc/pnp_body.h) after the sampling, on the host, for tests/test_p3p_cpu.py.
// X [n][3] (already scaled) and uv [n][2] in double, idx: the 4 sampled matches -> 1 and the pose (12 doubles) when valid
int t_hypothesis(const double* X, const double* uv, const double* K4, const int* idx, double thr2, double* pose) {
  double y[3][3], x[3][3];
  for (int k = 0; k < 3; ++k) {
    const double u = (uv[2 * idx[k]] - K4[2]) / K4[0];
    const double v = (uv[2 * idx[k] + 1] - K4[3]) / K4[1];
    const double inv = 1.0 / sqrt(u * u + v * v + 1.0);
    y[k][0] = u * inv;
    y[k][1] = v * inv;
    y[k][2] = inv;
    for (int c = 0; c < 3; ++c) x[k][c] = X[3 * idx[k] + c];
  }
  OppPose sol[4];
  const int ns = opp_p3p_grunert(y, x, sol);
  int best = -1;
  double best_e = 1e300;
  for (int i = 0; i < ns; ++i) {
    const double e = opp_reproj_err2(sol[i], K4, X + 3 * idx[3], uv + 2 * idx[3]);
    if (e < best_e) {
      best_e = e;
      best = i;
    }
  }
  if (!(best >= 0 && best_e <= thr2 * 4.0)) return 0;
  for (int k = 0; k < 9; ++k) pose[k] = sol[best].R[k];
  for (int k = 0; k < 3; ++k) pose[9 + k] = sol[best].t[k];
  return 1;
}

// inlier count of a pose over n matches; mask (may be null) receives the per-point decision
int t_score(const double* pose, const double* K4, const double* X, const double* uv, int n, double thr2, int* mask) {
  OppPose P;
  for (int k = 0; k < 9; ++k) P.R[k] = pose[k];
  for (int k = 0; k < 3; ++k) P.t[k] = pose[9 + k];
  int cnt = 0;
  for (int i = 0; i < n; ++i) {
    const int in = opp_reproj_err2(P, K4, X + 3 * i, uv + 2 * i) <= thr2 ? 1 : 0;
    if (mask) mask[i] = in;
    cnt += in;
  }
  return cnt;
}

// the refinement loop of pnp_refine_body, points summed in index order: inliers re-evaluated every iteration, no step below 4
// inliers or on a singular system; pose in/out in the scaled unit; returns the final inlier count and writes the final mask
int t_refine_inliers(double* pose, const double* K4, const double* X, const double* uv, int n, double thr2, int iters, int* mask) {
  OppPose P;
  for (int k = 0; k < 9; ++k) P.R[k] = pose[k];
  for (int k = 0; k < 3; ++k) P.t[k] = pose[9 + k];
  for (int it = 0; it < iters; ++it) {
    double H[36] = {0}, g[6] = {0};
    int total = 0;
    for (int i = 0; i < n; ++i)
      if (opp_reproj_err2(P, K4, X + 3 * i, uv + 2 * i) <= thr2) {
        opp_gn_accumulate(P, K4, X + 3 * i, uv + 2 * i, H, g);
        ++total;
      }
    if (total < 4) continue;
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < r; ++c) H[r * 6 + c] = H[c * 6 + r];
    if (!opp_solve6(H, g)) continue;
    OppPose N = P;
    opp_rot_update(N.R, g);
    double E[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    opp_rot_update(E, g);
    for (int r = 0; r < 3; ++r) N.t[r] = E[r * 3] * P.t[0] + E[r * 3 + 1] * P.t[1] + E[r * 3 + 2] * P.t[2] + g[3 + r];
    P = N;
  }
  for (int k = 0; k < 9; ++k) pose[k] = P.R[k];
  for (int k = 0; k < 3; ++k) pose[9 + k] = P.t[k];
  return t_score(pose, K4, X, uv, n, thr2, mask);
}
}
