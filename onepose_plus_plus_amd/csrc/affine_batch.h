// The pure logic of the batched affine RANSAC (affine.hip), written once for the device and the host (compiled with g++:
// tests/test_affine_cpu.py): what a view of n matches runs, the layout of the workspace, OpenCV's collinearity test on a minimal
// sample, the closed-form 3-match model, the inlier error and the box of the mapped image corners.
#pragma once
#include <math.h>
#include <stddef.h>

#include "pnp_batch.h"   // OPP_BHD, opp_ws_align, opp_pnp_extent: the offsets convention of the batched PnP

#define OPP_AFFINE_MODEL_POINTS 3      // cv::estimateAffine2D: RANSACPointSetRegistrator with modelPoints = 3
#define OPP_AFFINE_FLT_EPSILON 1.1920928955078125e-07

// what a view runs
enum OppAffineMode {
  OPP_AFFINE_FAIL = 0,     // n < 3: no model
  OPP_AFFINE_ONE = 1,      // n == 3: one hypothesis on matches 0, 1, 2, no sampling
  OPP_AFFINE_RANSAC = 2    // n > 3: `iterations` hypotheses on 3-match samples
};

OPP_BHD int opp_affine_mode(int n) { return n < 3 ? OPP_AFFINE_FAIL : (n == 3 ? OPP_AFFINE_ONE : OPP_AFFINE_RANSAC); }

// hypotheses a view evaluates: the entries of its slabs that the call writes and reads
OPP_BHD int opp_affine_hypotheses(int mode, int iterations) {
  return mode == OPP_AFFINE_FAIL ? 0 : (mode == OPP_AFFINE_ONE ? 1 : iterations);
}

// byte offsets into the workspace: hyp | valid | score | score2, per-view slabs, view v's at <array> + v * <stride>
struct OppAffineLayout {
  size_t hyp, valid, score, score2;
  size_t hyp_stride;   // hyp: [iterations][6] doubles, the 2 x 3 map row-major
  size_t int_stride;   // valid, score, score2: [iterations] ints
  size_t bytes;
};

OPP_BHD size_t opp_affine_layout(int iterations, int n_views, int n_total, OppAffineLayout* L) {
  const size_t I = (size_t)(iterations < 1 ? 1 : iterations), V = (size_t)(n_views < 1 ? 1 : n_views);
  (void)n_total;   // nothing in the workspace is per match: the refit sums in registers
  OppAffineLayout l;
  l.hyp_stride = opp_ws_align(I * 6 * sizeof(double));
  l.int_stride = opp_ws_align(I * sizeof(int));
  size_t off = 0;
  l.hyp = off, off += V * l.hyp_stride;
  l.valid = off, off += V * l.int_stride;
  l.score = off, off += V * l.int_stride;
  l.score2 = off, off += V * l.int_stride;
  l.bytes = off;
  if (L) *L = l;
  return l.bytes;
}

// OpenCV's haveCollinearPoints on a 3-point set (the third point against the pair before it), as we read ptsetreg.cpp
OPP_BHD bool opp_affine_collinear(double x0, double y0, double x1, double y1, double x2, double y2) {
  const double dx1 = x1 - x2, dy1 = y1 - y2, dx2 = x0 - x2, dy2 = y0 - y2;
  return fabs(dx2 * dy1 - dy2 * dx1) <= OPP_AFFINE_FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2));
}

// the affine map through three matches (x_k, y_k) -> (X_k, Y_k), Cramer on coordinates relative to match 0.
// M = a b c | d e f.  The caller has excluded collinear source points, so the determinant is not zero.
OPP_BHD void opp_affine_from3(double x0, double y0, double x1, double y1, double x2, double y2, double X0, double Y0, double X1, double Y1,
                              double X2, double Y2, double* M) {
  const double ux = x1 - x0, uy = y1 - y0, vx = x2 - x0, vy = y2 - y0;
  const double det = ux * vy - uy * vx;
  const double pX = X1 - X0, qX = X2 - X0, pY = Y1 - Y0, qY = Y2 - Y0;
  const double a = (pX * vy - qX * uy) / det, b = (ux * qX - vx * pX) / det;
  const double d = (pY * vy - qY * uy) / det, e = (ux * qY - vx * pY) / det;
  M[0] = a;
  M[1] = b;
  M[2] = X0 - (a * x0 + b * y0);
  M[3] = d;
  M[4] = e;
  M[5] = Y0 - (d * x0 + e * y0);
}

// squared distance of the mapped source point to the query point
OPP_BHD double opp_affine_err2(double a, double b, double c, double d, double e, double f, double x, double y, double X, double Y) {
  const double rx = a * x + b * y + c - X, ry = d * x + e * y + f - Y;
  return rx * rx + ry * ry;
}

// box = min x, min y, max x, max y of the four corners mapped through M and truncated towards zero (numpy's .astype(int32)).
// false, and the box untouched, when a mapped coordinate is not finite or does not fit int32.
OPP_BHD bool opp_affine_box(const double* M, const double* corners /* [4][2] */, int* box) {
  int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
  for (int k = 0; k < 4; ++k) {
    const double cx = corners[2 * k], cy = corners[2 * k + 1];
    const double px = M[0] * cx + M[1] * cy + M[2], py = M[3] * cx + M[4] * cy + M[5];
    if (!(fabs(px) < 2147483648.0) || !(fabs(py) < 2147483648.0)) return false;   // NaN and infinity fail both comparisons
    const int ix = (int)px, iy = (int)py;
    x0 = (k == 0 || ix < x0) ? ix : x0;
    y0 = (k == 0 || iy < y0) ? iy : y0;
    x1 = (k == 0 || ix > x1) ? ix : x1;
    y1 = (k == 0 || iy > y1) ? iy : y1;
  }
  box[0] = x0;
  box[1] = y0;
  box[2] = x1;
  box[3] = y1;
  return true;
}

// the least-squares affine map from the centred sums of the inliers (means mx, my, mX, mY; S** = sums of products of centred
// coordinates).  false when the 2 x 2 normal matrix is singular or the result not finite: the caller keeps its model.
OPP_BHD bool opp_affine_refit(double mx, double my, double mX, double mY, double Sxx, double Sxy, double Syy, double SxX, double SyX,
                              double SxY, double SyY, double* M) {
  const double det = Sxx * Syy - Sxy * Sxy;
  if (!(fabs(det) > 0.0)) return false;
  const double a = (SxX * Syy - SyX * Sxy) / det, b = (Sxx * SyX - Sxy * SxX) / det;
  const double d = (SxY * Syy - SyY * Sxy) / det, e = (Sxx * SyY - Sxy * SxY) / det;
  const double c = mX - (a * mx + b * my), f = mY - (d * mx + e * my);
  if (!(fabs(a) + fabs(b) + fabs(c) + fabs(d) + fabs(e) + fabs(f) < INFINITY)) return false;
  M[0] = a;
  M[1] = b;
  M[2] = c;
  M[3] = d;
  M[4] = e;
  M[5] = f;
  return true;
}
