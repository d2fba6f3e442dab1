// LO-RANSAC with robust refinement on the GPU: the pose step of the reference's `use_pycolmap_ransac=True` branch
// (pycolmap.absolute_pose_estimation, src/utils/metric_utils.py:137-170; demo.py:132, inference_LINEMOD.yaml:117), i.e.
// COLMAP 3.8 EstimateAbsolutePose = LORANSAC<P3PEstimator, EPNPEstimator> + RefineAbsolutePose under a Cauchy loss.
// Everything runs in parallel and the result is that of the sequential loop over trials 0, 1, ... (pnp_math.h: opp_lo_resolve):
//
//   1. hypotheses : one thread per trial: 3 distinct matches (the hash sampler of pnp.hip), Grunert P3P -> 0..4 models
//      scoring    : one wave per (trial, model): inlier count and sum of the inliers' squared residuals, lane l summing the
//                   points l, l + 64, ... in order and a butterfly over the lanes (one fixed order everywhere a model is scored)
//   2. candidates : one workgroup lists, in (trial, model) order, the models whose support beats every earlier model's.  Local
//                   optimisation only raises the bar, so these are a superset of the models the sequential loop optimises
//   3. LO         : a fixed grid of one-wave workgroups strides over the list: up to OPP_LO_ROUNDS rounds of EPnP on the
//                   inliers of the candidate's current best model (compacted in point order), kept while the support improves
//   4. final      : one workgroup: the sequential walk over the candidates (a candidate whose raw support no longer beats the
//                   running best is dropped), the bound on the trials and the stop index, the inlier mask of the best model,
//                   and the Levenberg-Marquardt refinement (pnp_math.h: opp_lm_refine) on those inliers
//
// The first min_trials trials run 1-4 first; their bound on the trials (it only falls afterwards) is left in device memory, and the
// launches over the remaining trials read it and return early past it.  Every loop has a fixed bound, no workgroup waits on
// another, and all arrays live in LDS or in the workspace (no private-segment memory).
// The kernels below are wrappers: their bodies are in pnp_lo_body.h, which the batched kernels of pnp_lo_batch.hip call too.
// The workspace is the batch's at one sample (opp_lo_batch_layout, pnp_lo_batch.h, with opp_lo_mode and opp_lo_first_pass).
#include "opp_common.h"
#include "pnp_args.h"
#include "pnp_lo_body.h"

namespace {

// trials [t0, min(t1, *bound))
__global__ __launch_bounds__(256) void loransac_hypotheses_kernel(const float* __restrict__ p2, const float* __restrict__ p3, LoParams prm,
                                                                  int t0, int t1, const int* __restrict__ bound, double* __restrict__ hyp,
                                                                  int* __restrict__ nmod, int* __restrict__ samples) {
  lo_hypotheses_body(p2, p3, prm, t0, t1, bound, hyp, nmod, samples, blockIdx.x * 256 + threadIdx.x);
}

// one workgroup per trial, one wave per model
__global__ __launch_bounds__(256) void loransac_score_kernel(const float* __restrict__ p2, const float* __restrict__ p3, LoParams prm, int t0,
                                                             int t1, const int* __restrict__ bound, const double* __restrict__ hyp,
                                                             const int* __restrict__ nmod, int* __restrict__ cnt, double* __restrict__ sum,
                                                             OppLoRecord rec) {
  lo_score_body(p2, p3, prm, t0, t1, bound, hyp, nmod, cnt, sum, rec, blockIdx.x);
}

// one workgroup
__global__ __launch_bounds__(256) void loransac_candidates_kernel(int t1, const int* __restrict__ bound, int skip_t1, LoBuffers b) {
  lo_candidates_body(t1, bound, skip_t1, b);
}

// one wave per workgroup, workgroup g takes the candidates g, g + gridDim.x, ...
__global__ __launch_bounds__(64) void loransac_optimise_kernel(const float* __restrict__ p2, const float* __restrict__ p3, LoParams prm,
                                                               const int* __restrict__ bound, int skip_t1, LoBuffers b) {
  lo_optimise_body(p2, p3, prm, bound, skip_t1, b, blockIdx.x, gridDim.x);
}

// one workgroup; mode 0 / 1 / 2 as in lo_final_body
__global__ __launch_bounds__(256) void loransac_final_kernel(const float* __restrict__ p2, const float* __restrict__ p3, LoParams prm, int mode,
                                                             LoBuffers b, double* __restrict__ pose_out, int* __restrict__ mask,
                                                             int* __restrict__ n_inl, int* __restrict__ ok_out, int* __restrict__ stop_out,
                                                             OppLoRecord rec) {
  lo_final_body(p2, p3, prm, mode, b, pose_out, mask, n_inl, ok_out, stop_out, rec);
}

}  // namespace

extern "C" size_t opp_pnp_loransac_workspace_bytes(int iterations, int n_points) {
  return opp_lo_batch_layout(iterations, 1, n_points, nullptr);
}

extern "C" int opp_pnp_loransac(const float* pts2d, const float* pts3d, int n_points, const double* K4, double reproj_error_px,
                                int iterations, unsigned seed, double confidence, int min_trials, double min_inlier_ratio, double* pose_out,
                                int* inlier_mask, int* n_inliers, int* ok, int* stop_out, const OppLoRecord* record, void* ws, size_t ws_bytes,
                                void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OPP_TRY(opp_pnp_check_args("pnp_loransac", pts2d, pts3d, n_points, K4, pose_out, inlier_mask, n_inliers, ok, ws, iterations, reproj_error_px,
                             min_trials >= 0 && min_inlier_ratio >= 0.0, confidence));
  OPP_CHECK_ARG(K4[0] > 0.0 && K4[1] > 0.0, "pnp_loransac: focal lengths must be positive");
  OPP_CHECK_WS(ws_bytes >= opp_pnp_loransac_workspace_bytes(iterations, n_points), "pnp_loransac: workspace too small");
  LoParams prm;
  for (int k = 0; k < 4; ++k) prm.K4[k] = K4[k];
  prm.thr2 = reproj_error_px * reproj_error_px;
  prm.conf = confidence;
  prm.min_ratio = min_inlier_ratio;
  prm.n = n_points;
  prm.iters = iterations;
  prm.min_trials = min_trials;
  prm.seed = seed;
  OppLoBatchLayout L;
  opp_lo_batch_layout(iterations, 1, n_points, &L);
  const LoBuffers b = lo_buffers((char*)ws, L, 0, 0);
  const OppLoRecord rec = record ? *record : OppLoRecord{};
  if (opp_lo_mode(n_points) == OPP_LO_FAIL) {   // pycolmap reports failure: identity / no inliers / state False
    hipLaunchKernelGGL(loransac_final_kernel, dim3(1), dim3(256), 0, stream, pts2d, pts3d, prm, 2, b, pose_out, inlier_mask, n_inliers, ok,
                       stop_out, rec);
    OPP_CHECK_LAUNCH("pnp_loransac kernels");
    return OPP_OK;
  }
  const int t1 = opp_lo_first_pass(min_trials, iterations);
  // first pass: the trials every run evaluates
  hipLaunchKernelGGL(loransac_hypotheses_kernel, dim3(opp_cdiv(t1, 256)), dim3(256), 0, stream, pts2d, pts3d, prm, 0, t1, (const int*)nullptr,
                     b.hyp, b.nmod, rec.samples);
  hipLaunchKernelGGL(loransac_score_kernel, dim3(t1), dim3(256), 0, stream, pts2d, pts3d, prm, 0, t1, (const int*)nullptr, b.hyp, b.nmod, b.cnt,
                     b.sum, rec);
  hipLaunchKernelGGL(loransac_candidates_kernel, dim3(1), dim3(256), 0, stream, t1, (const int*)nullptr, -1, b);
  hipLaunchKernelGGL(loransac_optimise_kernel, dim3(OPP_LO_GRID), dim3(64), 0, stream, pts2d, pts3d, prm, (const int*)nullptr, -1, b);
  if (t1 < iterations) {   // the trials up to the first pass's bound (read on the device; nothing runs past it)
    const int* bound = b.ctl + 1;
    hipLaunchKernelGGL(loransac_final_kernel, dim3(1), dim3(256), 0, stream, pts2d, pts3d, prm, 0, b, pose_out, inlier_mask, n_inliers, ok,
                       stop_out, rec);
    hipLaunchKernelGGL(loransac_hypotheses_kernel, dim3(opp_cdiv(iterations - t1, 256)), dim3(256), 0, stream, pts2d, pts3d, prm, t1, iterations,
                       bound, b.hyp, b.nmod, rec.samples);
    hipLaunchKernelGGL(loransac_score_kernel, dim3(iterations - t1), dim3(256), 0, stream, pts2d, pts3d, prm, t1, iterations, bound, b.hyp, b.nmod,
                       b.cnt, b.sum, rec);
    hipLaunchKernelGGL(loransac_candidates_kernel, dim3(1), dim3(256), 0, stream, iterations, bound, t1, b);
    hipLaunchKernelGGL(loransac_optimise_kernel, dim3(OPP_LO_GRID), dim3(64), 0, stream, pts2d, pts3d, prm, bound, t1, b);
  }
  hipLaunchKernelGGL(loransac_final_kernel, dim3(1), dim3(256), 0, stream, pts2d, pts3d, prm, 1, b, pose_out, inlier_mask, n_inliers, ok, stop_out,
                     rec);
  OPP_CHECK_LAUNCH("pnp_loransac kernels");
  return OPP_OK;
}
