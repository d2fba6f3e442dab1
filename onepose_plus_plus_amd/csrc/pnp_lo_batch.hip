// LO-RANSAC for a whole batch in one pass: the kernels of pnp_lo.hip (their bodies, pnp_lo_body.h) with the sample taken from
// blockIdx.y (blockIdx.x for the one-workgroup stages), so that B images cost one set of launches and no host sync instead of B
// serial runs whose candidate list, walk and Levenberg-Marquardt refinement each occupy ONE workgroup of the chip.
//
// The matches of all samples lie concatenated in sample order, delimited by a device array offsets [B+1] (pnp_batch.hip): the
// sizes n_b are known on the device only, so the one thing opp_pnp_loransac decides on the host from n_points -- n < 3 is the
// failure -- is decided per sample in the kernels (opp_lo_mode, pnp_lo_batch.h), and a workgroup whose sample does not use a
// kernel returns at once.  Each sample reads its own K4 and seed from device arrays and owns an `iterations`-sized slab of
// every array of LoBuffers that scales with the trials, and a ctl of its own; its LO points start OPP_LO_GRID * 13 * offsets[b]
// doubles into one array, its final-stage points 21 * offsets[b] doubles into another (opp_lo_batch_layout).  Offsets that do
// not describe a segment of [0, n_total] make an empty sample (opp_pnp_extent): nothing is read or written outside the
// caller's arrays.
//
// The two passes of pnp_lo.hip: the first covers the t1 trials every run evaluates (a number the host knows), a mode-0 final
// kernel leaves each sample's bound on the trials in its ctl[1], and every workgroup of the second pass over [t1, iterations)
// reads its sample's bound and returns past it; a sample whose bound did not pass t1 skips the second candidates / LO stage.
//
//   grid (ceil(trials / 256), B)  loransac_batch_hypotheses_kernel
//   grid (trials, B) x 256        loransac_batch_score_kernel
//   grid (B)                      loransac_batch_candidates_kernel
//   grid (OPP_LO_GRID, B) x 64        loransac_batch_optimise_kernel
//   grid (B)                      loransac_batch_final_kernel
//
// Per sample the result is that of opp_pnp_loransac on its slice, bit for bit (tests/test_loransac_batch_gpu.py).  Every loop
// has a fixed bound, no workgroup waits on another, and all arrays live in LDS or in the workspace.
#include "opp_common.h"
#include "pnp_args.h"
#include "pnp_lo_body.h"

namespace {

struct LoBatch {
  const float* p2;
  const float* p3;
  const int* offsets;      // [B+1]
  const double* K4;        // [B][4] fx, fy, cx, cy
  const unsigned* seeds;   // [B]
  double thr2, conf, min_ratio;
  int n_total, iters, min_trials;
  char* ws;
  OppLoBatchLayout L;
  double* pose_out;        // [B][12]
  int* mask;               // [n_total]
  int* n_inl;              // [B]
  int* ok;                 // [B]
  int* stop;               // [B]
};

struct LoSample {
  LoParams prm;
  int first, mode;
};

__device__ __forceinline__ LoSample lo_load_sample(const LoBatch& a, int b) {
  LoSample s;
  opp_pnp_extent(a.offsets[b], a.offsets[b + 1], a.n_total, &s.first, &s.prm.n);
  for (int k = 0; k < 4; ++k) s.prm.K4[k] = a.K4[4 * b + k];
  s.prm.thr2 = a.thr2;
  s.prm.conf = a.conf;
  s.prm.min_ratio = a.min_ratio;
  s.prm.iters = a.iters;
  s.prm.min_trials = a.min_trials;
  s.prm.seed = a.seeds[b];
  s.mode = opp_lo_mode(s.prm.n);
  return s;
}

// second != 0: the second pass, bounded by the sample's ctl[1]
__global__ __launch_bounds__(256) void loransac_batch_hypotheses_kernel(LoBatch a, int t0, int t1, int second) {
  const int b = blockIdx.y;
  const LoSample s = lo_load_sample(a, b);
  if (s.mode != OPP_LO_RUN) return;
  const LoBuffers bf = lo_buffers(a.ws, a.L, b, s.first);
  lo_hypotheses_body(a.p2 + (size_t)2 * s.first, a.p3 + (size_t)3 * s.first, s.prm, t0, t1, second ? bf.ctl + 1 : nullptr, bf.hyp, bf.nmod,
                     nullptr, blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(256) void loransac_batch_score_kernel(LoBatch a, int t0, int t1, int second) {
  const int b = blockIdx.y;
  const LoSample s = lo_load_sample(a, b);
  if (s.mode != OPP_LO_RUN) return;
  const LoBuffers bf = lo_buffers(a.ws, a.L, b, s.first);
  lo_score_body(a.p2 + (size_t)2 * s.first, a.p3 + (size_t)3 * s.first, s.prm, t0, t1, second ? bf.ctl + 1 : nullptr, bf.hyp, bf.nmod, bf.cnt,
                bf.sum, OppLoRecord{}, blockIdx.x);
}

// one workgroup per sample.  skip_t1 >= 0: the second pass
__global__ __launch_bounds__(256) void loransac_batch_candidates_kernel(LoBatch a, int t1, int skip_t1) {
  const int b = blockIdx.x;
  const LoSample s = lo_load_sample(a, b);
  if (s.mode != OPP_LO_RUN) return;
  const LoBuffers bf = lo_buffers(a.ws, a.L, b, s.first);
  lo_candidates_body(t1, skip_t1 >= 0 ? bf.ctl + 1 : nullptr, skip_t1, bf);
}

__global__ __launch_bounds__(64) void loransac_batch_optimise_kernel(LoBatch a, int skip_t1) {
  const int b = blockIdx.y;
  const LoSample s = lo_load_sample(a, b);
  if (s.mode != OPP_LO_RUN) return;
  __shared__ LoParams s_prm;   // the body indexes K4 by thread: in LDS, not in registers (no scratch)
  if (threadIdx.x == 0) s_prm = s.prm;
  __syncthreads();
  const LoBuffers bf = lo_buffers(a.ws, a.L, b, s.first);
  lo_optimise_body(a.p2 + (size_t)2 * s.first, a.p3 + (size_t)3 * s.first, s_prm, skip_t1 >= 0 ? bf.ctl + 1 : nullptr, skip_t1, bf, blockIdx.x,
                   gridDim.x);
}

// one workgroup per sample.  bound_pass != 0: the walk over the first pass's candidates alone (mode 0), nothing for a sample
// that fails; else the outputs of every sample (mode 1, or 2 for fewer than 3 matches)
__global__ __launch_bounds__(256) void loransac_batch_final_kernel(LoBatch a, int bound_pass) {
  const int b = blockIdx.x;
  const LoSample s = lo_load_sample(a, b);
  if (bound_pass && s.mode != OPP_LO_RUN) return;
  __shared__ LoParams s_prm;   // as in loransac_batch_optimise_kernel
  if (threadIdx.x == 0) s_prm = s.prm;
  __syncthreads();
  const LoBuffers bf = lo_buffers(a.ws, a.L, b, s.first);
  lo_final_body(a.p2 + (size_t)2 * s.first, a.p3 + (size_t)3 * s.first, s_prm, bound_pass ? 0 : (s.mode == OPP_LO_RUN ? 1 : 2), bf,
                a.pose_out + (size_t)12 * b, a.mask + s.first, a.n_inl + b, a.ok + b, a.stop + b, OppLoRecord{});
}

}  // namespace

extern "C" size_t opp_pnp_loransac_batch_workspace_bytes(int iterations, int n_samples, int n_total) {
  return opp_lo_batch_layout(iterations, n_samples, n_total, nullptr);
}

extern "C" int opp_pnp_loransac_batch(const float* pts2d, const float* pts3d, const int* offsets, int n_samples, int n_total, const double* K4,
                                      const unsigned* seeds, double reproj_error_px, int iterations, double confidence, int min_trials,
                                      double min_inlier_ratio, double* pose_out, int* inlier_mask, int* n_inliers, int* ok, int* stop, void* ws,
                                      size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OPP_TRY(opp_pnp_check_batch("pnp_loransac_batch", n_samples, offsets, seeds, stop));
  OPP_TRY(opp_pnp_check_args("pnp_loransac_batch", pts2d, pts3d, n_total, K4, pose_out, inlier_mask, n_inliers, ok, ws, iterations,
                             reproj_error_px, min_trials >= 0 && min_inlier_ratio >= 0.0, confidence));
  OPP_CHECK_WS(ws_bytes >= opp_pnp_loransac_batch_workspace_bytes(iterations, n_samples, n_total), "pnp_loransac_batch: workspace too small");
  LoBatch a;
  a.p2 = pts2d;
  a.p3 = pts3d;
  a.offsets = offsets;
  a.K4 = K4;
  a.seeds = seeds;
  a.thr2 = reproj_error_px * reproj_error_px;
  a.conf = confidence;
  a.min_ratio = min_inlier_ratio;
  a.n_total = n_total;
  a.iters = iterations;
  a.min_trials = min_trials;
  a.ws = (char*)ws;
  opp_lo_batch_layout(iterations, n_samples, n_total, &a.L);
  a.pose_out = pose_out;
  a.mask = inlier_mask;
  a.n_inl = n_inliers;
  a.ok = ok;
  a.stop = stop;
  const int t1 = opp_lo_first_pass(min_trials, iterations);
  // first pass: the trials every run evaluates
  hipLaunchKernelGGL(loransac_batch_hypotheses_kernel, dim3(opp_cdiv(t1, 256), n_samples), dim3(256), 0, stream, a, 0, t1, 0);
  hipLaunchKernelGGL(loransac_batch_score_kernel, dim3(t1, n_samples), dim3(256), 0, stream, a, 0, t1, 0);
  hipLaunchKernelGGL(loransac_batch_candidates_kernel, dim3(n_samples), dim3(256), 0, stream, a, t1, -1);
  hipLaunchKernelGGL(loransac_batch_optimise_kernel, dim3(OPP_LO_GRID, n_samples), dim3(64), 0, stream, a, -1);
  if (t1 < iterations) {   // the trials up to each sample's bound after the first pass (read on the device; nothing runs past it)
    hipLaunchKernelGGL(loransac_batch_final_kernel, dim3(n_samples), dim3(256), 0, stream, a, 1);
    hipLaunchKernelGGL(loransac_batch_hypotheses_kernel, dim3(opp_cdiv(iterations - t1, 256), n_samples), dim3(256), 0, stream, a, t1,
                       iterations, 1);
    hipLaunchKernelGGL(loransac_batch_score_kernel, dim3(iterations - t1, n_samples), dim3(256), 0, stream, a, t1, iterations, 1);
    hipLaunchKernelGGL(loransac_batch_candidates_kernel, dim3(n_samples), dim3(256), 0, stream, a, iterations, t1);
    hipLaunchKernelGGL(loransac_batch_optimise_kernel, dim3(OPP_LO_GRID, n_samples), dim3(64), 0, stream, a, t1);
  }
  hipLaunchKernelGGL(loransac_batch_final_kernel, dim3(n_samples), dim3(256), 0, stream, a, 0);
  OPP_CHECK_LAUNCH("pnp_loransac_batch kernels");
  return OPP_OK;
}
