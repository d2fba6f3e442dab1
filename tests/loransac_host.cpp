// Host build of the LO-RANSAC decisions and the robust refinement (onepose_plus_plus_amd/csrc/pnp_math.h) for CPU unit tests
// (tests/test_loransac_cpu.py) and for the stand-alone sanitizer program (tests/loransac_host_main.cpp).
#include <vector>

#include "../onepose_plus_plus_amd/csrc/pnp_math.h"

extern "C" {
int t_lo_better(int ca, double sa, int cb, double sb) { return opp_support_better(ca, sa, cb, sb) ? 1 : 0; }

int t_lo_dyn(double confidence, int cnt, int n, int cap) { return opp_lo_dyn(confidence, cnt, n, cap); }

int t_lo_resolve(const int* cand_idx, const int* rc, const double* rs, const int* lc, const double* ls, int ncand, int n, double confidence,
                 int min_trials, int cap, int* best, int* taken) {
  return opp_lo_resolve(cand_idx, rc, rs, lc, ls, ncand, n, confidence, min_trials, cap, best, taken);
}

// pose: 12 doubles R row-major | t, refined in place on X [n][3], uv [n][2].  Returns the damped systems solved; cost[0] = the
// robust cost at the refined pose.
int t_lm_refine(const double* X, const double* uv, int n, const double* K4, double* pose, double* cost) {
  OppLmWs* w = new OppLmWs();
  std::vector<double> rows((size_t)(n > 0 ? n : 1) * OPP_LM_ROW);
  for (int k = 0; k < 9; ++k) w->P.R[k] = pose[k];
  for (int k = 0; k < 3; ++k) w->P.t[k] = pose[9 + k];
  opp_lm_refine(X, uv, n, K4, w, rows.data(), 0, 1);
  for (int k = 0; k < 9; ++k) pose[k] = w->P.R[k];
  for (int k = 0; k < 3; ++k) pose[9 + k] = w->P.t[k];
  cost[0] = w->cost;
  const int it = w->iters;
  delete w;
  return it;
}

// `iters` unweighted Gauss-Newton steps of opp_gn_accumulate on the same points (the refinement of solver "p3p")
void t_gn_refine(const double* X, const double* uv, int n, const double* K4, double* pose, int iters) {
  OppPose P;
  for (int k = 0; k < 9; ++k) P.R[k] = pose[k];
  for (int k = 0; k < 3; ++k) P.t[k] = pose[9 + k];
  for (int it = 0; it < iters; ++it) {
    double H[36] = {0}, g[6] = {0};
    for (int i = 0; i < n; ++i) opp_gn_accumulate(P, K4, X + 3 * i, uv + 2 * i, H, g);
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < r; ++c) H[r * 6 + c] = H[c * 6 + r];
    if (!opp_solve6(H, g)) break;
    OppPose N = P;
    opp_rot_update(N.R, g);
    double E[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    opp_rot_update(E, g);
    for (int r = 0; r < 3; ++r) N.t[r] = E[r * 3] * P.t[0] + E[r * 3 + 1] * P.t[1] + E[r * 3 + 2] * P.t[2] + g[3 + r];
    P = N;
  }
  for (int k = 0; k < 9; ++k) pose[k] = P.R[k];
  for (int k = 0; k < 3; ++k) pose[9 + k] = P.t[k];
}

// P3P on 3 matches: X [3][3], uv [3][2] -> up to 4 poses (12 doubles each); returns their number
int t_p3p(const double* X, const double* uv, const double* K4, double* poses) {
  double y[3][3], x[3][3];
  for (int k = 0; k < 3; ++k) {
    const double u = (uv[2 * k] - K4[2]) / K4[0], v = (uv[2 * k + 1] - K4[3]) / K4[1];
    const double inv = 1.0 / sqrt(u * u + v * v + 1.0);
    y[k][0] = u * inv;
    y[k][1] = v * inv;
    y[k][2] = inv;
    for (int c = 0; c < 3; ++c) x[k][c] = X[3 * k + c];
  }
  OppPose sol[4];
  const int ns = opp_p3p_grunert(y, x, sol);
  for (int i = 0; i < ns; ++i) {
    for (int k = 0; k < 9; ++k) poses[12 * i + k] = sol[i].R[k];
    for (int k = 0; k < 3; ++k) poses[12 * i + 9 + k] = sol[i].t[k];
  }
  return ns;
}
}
