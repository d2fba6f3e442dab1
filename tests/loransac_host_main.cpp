// Stand-alone program around tests/loransac_host.cpp for sanitizer runs on the CPU (not part of the pytest suite):
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o loransac_host_main tests/loransac_host_main.cpp && ./loransac_host_main
// Runs the robust refinement on synthetic scenes (clean, noisy, with displaced points, behind-the-camera start, n = 0..3) and the
// sequential walk on random candidate lists; prints a summary and returns 0.
#include <stdio.h>
#include <stdlib.h>

#include "loransac_host.cpp"

static unsigned long long g_state = 88172645463325252ull;
static double urand() {   // xorshift64*, uniform in [0, 1)
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (double)((g_state * 2685821657736338717ull) >> 11) / 9007199254740992.0;
}

int main() {
  const double K4[4] = {560.0, 560.0, 256.0, 250.0};
  int total_iters = 0;
  for (int scene = 0; scene < 24; ++scene) {
    const int n = scene < 4 ? scene : 5 + (int)(urand() * 400);
    std::vector<double> X(3 * (size_t)(n + 1)), uv(2 * (size_t)(n + 1));
    double w[3] = {urand() - 0.5, urand() - 0.5, urand() - 0.5};
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    opp_rot_update(R, w);
    const double t[3] = {urand() * 0.1 - 0.05, urand() * 0.1 - 0.05, 0.5 + 0.5 * urand()};
    const double noise = scene % 3 == 0 ? 0.0 : 0.5;
    for (int i = 0; i < n; ++i) {
      double xc[3];
      for (int c = 0; c < 3; ++c) X[3 * i + c] = 0.3 * urand() - 0.15;
      for (int r = 0; r < 3; ++r) xc[r] = R[r * 3] * X[3 * i] + R[r * 3 + 1] * X[3 * i + 1] + R[r * 3 + 2] * X[3 * i + 2] + t[r];
      uv[2 * i] = K4[0] * xc[0] / xc[2] + K4[2] + noise * (urand() - 0.5) + (scene % 4 == 1 && i % 10 == 0 ? 5.0 : 0.0);
      uv[2 * i + 1] = K4[1] * xc[1] / xc[2] + K4[3] + noise * (urand() - 0.5);
    }
    double pose[12], cost = 0.0;
    double dw[3] = {0.01 * (urand() - 0.5), 0.01 * (urand() - 0.5), 0.01 * (urand() - 0.5)};
    for (int k = 0; k < 9; ++k) pose[k] = R[k];
    opp_rot_update(pose, dw);
    for (int k = 0; k < 3; ++k) pose[9 + k] = t[k] + 0.002 * (urand() - 0.5);
    if (scene == 5) pose[11] = -t[2];   // every point behind the camera at the start
    total_iters += t_lm_refine(X.data(), uv.data(), n, K4, pose, &cost);
    t_gn_refine(X.data(), uv.data(), n, K4, pose, 2);
  }
  int total_stop = 0;
  for (int rep = 0; rep < 200; ++rep) {
    const int ncand = (int)(urand() * 40), n = 10 + (int)(urand() * 500), cap = 1 + (int)(urand() * 3000);
    std::vector<int> idx(ncand + 1), rc(ncand + 1), lc(ncand + 1), taken(ncand + 1);
    std::vector<double> rs(ncand + 1), ls(ncand + 1);
    int e = 0;
    for (int c = 0; c < ncand; ++c) {
      e += 1 + (int)(urand() * 200);
      idx[c] = e;
      rc[c] = (int)(urand() * (n + 1));
      rs[c] = urand() * 100.0;
      lc[c] = rc[c] + (int)(urand() * (n + 1 - rc[c]));
      ls[c] = lc[c] == rc[c] ? rs[c] * urand() : urand() * 100.0;
    }
    int best = 0;
    total_stop += t_lo_resolve(idx.data(), rc.data(), rs.data(), lc.data(), ls.data(), ncand, n, rep % 3 ? 0.9999 : 1.0, (int)(urand() * 1500), cap,
                               &best, taken.data());
  }
  printf("loransac_host_main: ok (%d LM iterations, stop sum %d)\n", total_iters, total_stop);
  return 0;
}
