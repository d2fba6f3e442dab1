// PnP-RANSAC on the GPU: the pose step that follows the 2D-3D matcher on every caller of the hot
// path.
//
// Replaces  ransac_PnP / cv2.solvePnPRansac(EPNP, 10000 iterations)
//           /root/reference/src/utils/metric_utils.py:121-204 (called from :251-259, demo.py:132)
// so that the matches never leave the device: at a few hundred images/s the reference's CPU
// RANSAC + D2H sync is the end-to-end limiter.  Accuracy-level parity only (OpenCV draws its
// samples from its own RNG); validated against synthetic ground-truth poses (tests/test_pnp_gpu.py).
//
//   1. hypotheses : one thread per hypothesis: 4 distinct matches from a counter-based hash RNG,
//                   Grunert P3P on three (double), the 4th disambiguates
//   2. scoring    : one wave per hypothesis counts reprojection inliers over all matches
//   3. selection  : arg-max inlier count (ties -> lowest hypothesis index: deterministic)
//   4. refinement : Gauss-Newton on the inlier set (re-evaluated every iteration), one workgroup
//
// opp_pnp_ransac_ex adds the reference's own estimator (solver 1, EPnP as in cv2.solvePnPRansac(flags=SOLVEPNP_EPNP)):
//   1. hypotheses : one wave per hypothesis: 5 distinct matches (same hash RNG), EPnP (pnp_math.h) with M^T M, its 12x12
//                   Jacobi and every other array in LDS (no scratch); n == 4 runs the P3P hypotheses above (OpenCV's switch)
//   2. scoring    : pnp_score_kernel, unchanged
//   3. final      : one workgroup: the sequential RANSAC loop over the scores with OpenCV's adaptive stop (a scan of the
//                   per-hypothesis counts in index order, skipping 256ths of the range whose maximum cannot be a new best),
//                   the best hypothesis's inlier mask, and an EPnP refit on those inliers (reductions in point order)
//
// The kernel bodies live in pnp_body.h, which the batched kernels (pnp_batch.hip) call as well.  Both entries are one launch
// routine (pnp_launch); what a sample of n matches runs and where its buffers lie in the workspace are opp_pnp_mode and
// opp_pnp_layout of pnp_batch.h, which the batch reads too.
#include "opp_common.h"
#include "pnp_args.h"
#include "pnp_batch.h"
#include "pnp_body.h"

namespace {

__global__ __launch_bounds__(256) void pnp_hypotheses_kernel(const float* __restrict__ p2, const float* __restrict__ p3,
                                                             PnpParams prm, double* __restrict__ hyp, int* __restrict__ valid) {
  pnp_hypotheses_body(p2, p3, prm, hyp, valid, blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ __launch_bounds__(256) void pnp_score_kernel(const float* __restrict__ p2, const float* __restrict__ p3, PnpParams prm,
                                                        const double* __restrict__ hyp, const int* __restrict__ valid,
                                                        int* __restrict__ score) {
  pnp_score_body(p2, p3, prm, hyp, valid, score, blockIdx.x);
}

// single workgroup: best hypothesis, Gauss-Newton refinement on its inliers, final inlier mask
__global__ __launch_bounds__(256) void pnp_refine_kernel(const float* __restrict__ p2, const float* __restrict__ p3, PnpParams prm,
                                                         const double* __restrict__ hyp, const int* __restrict__ score,
                                                         int gn_iters, double* __restrict__ pose_out, int* __restrict__ mask,
                                                         int* __restrict__ n_inl, int* __restrict__ ok_out) {
  pnp_refine_body(p2, p3, prm, hyp, score, gn_iters, pose_out, mask, n_inl, ok_out);
}


// ---- EPnP (opp_pnp_ransac_ex, solver 1) ------------------------------------------------------------------------------

// sample indices of the P3P hypotheses (4 per hypothesis, the 5th column -1), for opp_pnp_ransac_ex's optional output
__global__ __launch_bounds__(256) void pnp_p3p_samples_kernel(PnpParams prm, int* __restrict__ samples) {
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= prm.iters) return;
  int idx[4];
  draw_sample<4>(prm.seed, h, prm.n, idx);
#pragma unroll
  for (int k = 0; k < 4; ++k) samples[(size_t)h * 5 + k] = idx[k];
  samples[(size_t)h * 5 + 4] = -1;
}

// one 64-thread workgroup (one wave) per hypothesis: 5 distinct matches -> EPnP -> hyp[h] (R | t), valid[h]
__global__ __launch_bounds__(64) void pnp_epnp_hypotheses_kernel(const float* __restrict__ p2, const float* __restrict__ p3, PnpParams prm,
                                                                 double* __restrict__ hyp, int* __restrict__ valid, int* __restrict__ samples) {
  pnp_epnp_hypotheses_body(p2, p3, prm, hyp, valid, samples, blockIdx.x);
}

// P3P under opp_pnp_ransac_ex: the stop index, and the scores with every hypothesis past it masked out (-1) for pnp_refine_kernel
__global__ __launch_bounds__(256) void pnp_stop_kernel(const int* __restrict__ score, PnpParams prm, int m, double conf,
                                                       int* __restrict__ score_masked, int* __restrict__ stop_out) {
  pnp_stop_body(score, prm, m, conf, score_masked, stop_out);
}

// single workgroup, the end of the EPnP path (modes and `pts`: pnp_epnp_final_body)
__global__ __launch_bounds__(256) void pnp_epnp_final_kernel(const float* __restrict__ p2, const float* __restrict__ p3, PnpParams prm,
                                                             const double* __restrict__ hyp, const int* __restrict__ score, int mode, int m,
                                                             double conf, double* __restrict__ pts, double* __restrict__ pose_out,
                                                             int* __restrict__ mask, int* __restrict__ n_inl, int* __restrict__ ok_out,
                                                             int* __restrict__ stop_out) {
  pnp_epnp_final_body(p2, p3, prm, hyp, score, mode, m, conf, pts, pose_out, mask, n_inl, ok_out, stop_out);
}

}  // namespace

extern "C" size_t opp_pnp_workspace_bytes(int iterations) {
  if (iterations < 1) return 1024;   // no slab is rounded up to a trial here, unlike in opp_pnp_ex_workspace_bytes
  OppPnpLayout L;
  opp_pnp_layout(iterations, 1, 1, &L);
  return L.score2 + 1024;   // hyp | valid | score
}

extern "C" size_t opp_pnp_ex_workspace_bytes(int iterations, int n_points) { return opp_pnp_layout(iterations, 1, n_points, nullptr); }

namespace {

struct PnpBuffers {   // the workspace, carved (opp_pnp_layout at B = 1); opp_pnp_ransac's ends before score2
  double* hyp;
  int *valid, *score, *score2;
  double* pts;
};

PnpBuffers pnp_carve(void* ws, int iterations, int n_points) {
  OppPnpLayout L;
  opp_pnp_layout(iterations, 1, n_points, &L);
  char* base = (char*)ws;
  return {(double*)(base + L.hyp), (int*)(base + L.valid), (int*)(base + L.score), (int*)(base + L.score2), (double*)(base + L.pts)};
}

PnpParams pnp_params(const double* K4, double reproj_error_px, double scale, int n_points, int iterations, unsigned seed) {
  PnpParams prm;
  for (int k = 0; k < 4; ++k) prm.K4[k] = K4[k];
  prm.thr2 = reproj_error_px * reproj_error_px;
  prm.scale = scale;
  prm.n = n_points;
  prm.iters = iterations;
  prm.seed = seed;
  return prm;
}

// The launches of both entries; what a sample of prm.n matches runs is opp_pnp_mode's table.  stop_stage: solver 0 masks the
// hypotheses past the stop index (into b.score2) before the refinement; without it b.score2 and b.pts are not touched.
// stop_out, samples_out, scores_out: optional.  -> false when the copy of the scores could not be enqueued
bool pnp_launch(hipStream_t stream, const float* pts2d, const float* pts3d, PnpParams prm, const PnpBuffers& b, int solver, bool stop_stage,
                double confidence, int refine_iters, double* pose_out, int* inlier_mask, int* n_inliers, int* ok, int* stop_out,
                int* samples_out, int* scores_out) {
  const int iterations = prm.iters;
  int m;
  const int mode = opp_pnp_mode(solver, prm.n, &m);
  if (mode == OPP_PNP_P3P_RANSAC || mode == OPP_PNP_EPNP_RANSAC) {
    if (mode == OPP_PNP_EPNP_RANSAC)
      hipLaunchKernelGGL(pnp_epnp_hypotheses_kernel, dim3(iterations), dim3(64), 0, stream, pts2d, pts3d, prm, b.hyp, b.valid, samples_out);
    else
      hipLaunchKernelGGL(pnp_hypotheses_kernel, dim3(opp_cdiv(iterations, 256)), dim3(256), 0, stream, pts2d, pts3d, prm, b.hyp, b.valid);
    hipLaunchKernelGGL(pnp_score_kernel, dim3(opp_cdiv(iterations, 4)), dim3(256), 0, stream, pts2d, pts3d, prm, b.hyp, b.valid, b.score);
    if (samples_out && mode == OPP_PNP_P3P_RANSAC)
      hipLaunchKernelGGL(pnp_p3p_samples_kernel, dim3(opp_cdiv(iterations, 256)), dim3(256), 0, stream, prm, samples_out);
    if (scores_out && hipMemcpyAsync(scores_out, b.score, (size_t)iterations * sizeof(int), hipMemcpyDeviceToDevice, stream) != hipSuccess)
      return false;
  }
  if (solver == 0) {
    const int* score = b.score;
    if (mode == OPP_PNP_FAIL) {   // cv2.solvePnPRansac raises -> reference returns identity / no inliers / state False
      prm.iters = 0;
      (void)hipMemsetAsync(b.score, 0, sizeof(int), stream);
      if (stop_out) (void)hipMemsetAsync(stop_out, 0, sizeof(int), stream);
    } else if (stop_stage) {   // the refinement sees only the hypotheses before the stop index
      hipLaunchKernelGGL(pnp_stop_kernel, dim3(1), dim3(256), 0, stream, b.score, prm, m, confidence, b.score2, stop_out);
      score = b.score2;
    }
    hipLaunchKernelGGL(pnp_refine_kernel, dim3(1), dim3(256), 0, stream, pts2d, pts3d, prm, b.hyp, score, refine_iters, pose_out, inlier_mask,
                       n_inliers, ok);
  } else {
    hipLaunchKernelGGL(pnp_epnp_final_kernel, dim3(1), dim3(256), 0, stream, pts2d, pts3d, prm, b.hyp, b.score, opp_pnp_final_mode(mode), m,
                       confidence, b.pts, pose_out, inlier_mask, n_inliers, ok, stop_out);
  }
  return true;
}

}  // namespace

extern "C" int opp_pnp_ransac(const float* pts2d, const float* pts3d, int n_points, const double* K4, double reproj_error_px,
                              double scale, int iterations, unsigned seed, int refine_iters, double* pose_out,
                              int* inlier_mask, int* n_inliers, int* ok, void* ws, size_t ws_bytes, void* stream_) {
  OPP_TRY(opp_pnp_check_args("pnp", pts2d, pts3d, n_points, K4, pose_out, inlier_mask, n_inliers, ok, ws, iterations, reproj_error_px, scale > 0,
                             1.0));
  OPP_CHECK_WS(ws_bytes >= opp_pnp_workspace_bytes(iterations), "pnp: workspace too small");
  // solver 0 over every hypothesis: no stop stage, no optional output
  pnp_launch((hipStream_t)stream_, pts2d, pts3d, pnp_params(K4, reproj_error_px, scale, n_points, iterations, seed),
             pnp_carve(ws, iterations, n_points), 0, false, 1.0, refine_iters, pose_out, inlier_mask, n_inliers, ok, nullptr, nullptr, nullptr);
  OPP_CHECK_LAUNCH("pnp kernels");
  return OPP_OK;
}

extern "C" int opp_pnp_ransac_ex(const float* pts2d, const float* pts3d, int n_points, const double* K4, double reproj_error_px,
                                 double scale, int iterations, unsigned seed, int refine_iters, int solver, double confidence,
                                 double* pose_out, int* inlier_mask, int* n_inliers, int* ok, int* stop_out, int* samples_out,
                                 int* scores_out, void* ws, size_t ws_bytes, void* stream_) {
  OPP_TRY(opp_pnp_check_args("pnp_ex", pts2d, pts3d, n_points, K4, pose_out, inlier_mask, n_inliers, ok, ws, iterations, reproj_error_px,
                             scale > 0, confidence));
  OPP_TRY(opp_pnp_check_solver("pnp_ex", solver));
  OPP_CHECK_WS(ws_bytes >= opp_pnp_ex_workspace_bytes(iterations, n_points), "pnp_ex: workspace too small");
  if (!pnp_launch((hipStream_t)stream_, pts2d, pts3d, pnp_params(K4, reproj_error_px, scale, n_points, iterations, seed),
                  pnp_carve(ws, iterations, n_points), solver, true, confidence, refine_iters, pose_out, inlier_mask, n_inliers, ok, stop_out,
                  samples_out, scores_out)) {
    opp_set_error("pnp_ex: copy of the scores failed");
    return OPP_ERR_LAUNCH;
  }
  OPP_CHECK_LAUNCH("pnp_ex kernels");
  return OPP_OK;
}
