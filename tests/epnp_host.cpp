// Host build of the EPnP math (onepose_plus_plus_amd/csrc/pnp_math.h) for CPU unit tests (tests/test_epnp_cpu.py).
#include <vector>

#include "../onepose_plus_plus_amd/csrc/pnp_math.h"

extern "C" {
// X [n][3] world points, uv [n][2] pixels, K4 = fx, fy, cx, cy -> pose [12] (R row-major | t), errs [3] (mean reprojection error
// of the candidates 1..3).  Returns the chosen candidate, 0 for a degenerate input.
int t_epnp(const double* X, const double* uv, int n, const double* K4, double* pose, double* errs) {
  OppEpnpWs* w = new OppEpnpWs();
  std::vector<double> alph(4 * n), pcs(3 * n), perr(n);
  opp_epnp_solve(X, uv, n, K4, w, alph.data(), pcs.data(), perr.data(), 0, 1);
  const int best = w->best;
  for (int k = 0; k < 12; ++k) pose[k] = best ? w->Rt[best][k] : 0.0;
  for (int k = 0; k < 3; ++k) errs[k] = w->err[k + 1];
  delete w;
  return best;
}

// the 12x12 symmetric Jacobi of the solver: A [144] -> diagonal [12] and eigenvectors V [144] (columns)
void t_jacobi12(const double* A, double* evals, double* V) {
  OppEpnpWs* w = new OppEpnpWs();
  for (int e = 0; e < 144; ++e) {
    w->A[0][e] = A[e];
    w->V[0][e] = (e % 13 == 0) ? 1.0 : 0.0;
  }
  const int cur = opp_jacobi12(w, 0, 1);
  for (int k = 0; k < 12; ++k) evals[k] = w->A[cur][k * 13];
  for (int e = 0; e < 144; ++e) V[e] = w->V[cur][e];
  delete w;
}

int t_stop(const int* score, int iters, int n, int m, double conf, int* best) { return opp_ransac_stop(score, iters, n, m, conf, best); }

int t_update_iters(double p, double ep, int m, int max_iters) { return opp_ransac_update_iters(p, ep, m, max_iters); }
}
