// Host build of the batched affine RANSAC's pure logic (onepose_plus_plus_amd/csrc/affine_batch.h) for CPU unit tests.
#include "../onepose_plus_plus_amd/csrc/affine_batch.h"

extern "C" {
int t_affine_mode(int n) { return opp_affine_mode(n); }

int t_affine_hypotheses(int n, int iterations) { return opp_affine_hypotheses(opp_affine_mode(n), iterations); }

// the layout as 8 numbers: the 4 array offsets, the 2 strides, the total, and what opp_affine_layout returns
void t_affine_layout(int iterations, int n_views, int n_total, unsigned long long* out) {
  OppAffineLayout L;
  const size_t bytes = opp_affine_layout(iterations, n_views, n_total, &L);
  const size_t v[8] = {L.hyp, L.valid, L.score, L.score2, L.hyp_stride, L.int_stride, L.bytes, bytes};
  for (int k = 0; k < 8; ++k) out[k] = v[k];
}

// src [3][2]
int t_affine_collinear(const double* s) { return opp_affine_collinear(s[0], s[1], s[2], s[3], s[4], s[5]) ? 1 : 0; }

// src, dst [3][2] -> M [6]
void t_affine_from3(const double* s, const double* d, double* M) {
  opp_affine_from3(s[0], s[1], s[2], s[3], s[4], s[5], d[0], d[1], d[2], d[3], d[4], d[5], M);
}

// inlier counts of one model over n matches
int t_affine_count(const double* M, const double* p0, const double* p1, int n, double thr2) {
  int c = 0;
  for (int i = 0; i < n; ++i) c += opp_affine_err2(M[0], M[1], M[2], M[3], M[4], M[5], p0[2 * i], p0[2 * i + 1], p1[2 * i], p1[2 * i + 1]) <= thr2;
  return c;
}

int t_affine_box(const double* M, const double* corners, int* box) { return opp_affine_box(M, corners, box) ? 1 : 0; }

// the refit as affine_final_kernel runs it, with the sums taken in match order
int t_affine_refit(const double* p0, const double* p1, int n, double* M) {
  double mx = 0, my = 0, mX = 0, mY = 0;
  for (int i = 0; i < n; ++i) mx += p0[2 * i], my += p0[2 * i + 1], mX += p1[2 * i], mY += p1[2 * i + 1];
  mx /= n, my /= n, mX /= n, mY /= n;
  double S[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const double x = p0[2 * i] - mx, y = p0[2 * i + 1] - my, X = p1[2 * i] - mX, Y = p1[2 * i + 1] - mY;
    S[0] += x * x, S[1] += x * y, S[2] += y * y, S[3] += x * X, S[4] += y * X, S[5] += x * Y, S[6] += y * Y;
  }
  return opp_affine_refit(mx, my, mX, mY, S[0], S[1], S[2], S[3], S[4], S[5], S[6], M) ? 1 : 0;
}
}
