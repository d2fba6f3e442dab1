// PnP-RANSAC for a whole batch in one pass: the kernels of pnp.hip (their bodies, pnp_body.h) with the sample taken from
// blockIdx.y, so that B images cost one set of launches and no host sync instead of B serial, latency-bound single-workgroup
// tails (pnp_refine_kernel / pnp_epnp_final_kernel) with a device-to-host copy after each.
//
// The matches of all samples lie concatenated in sample order, delimited by a device array offsets [B+1]: the sizes n_b are
// known on the device only, so the table opp_pnp_ransac_ex reads on the host from n_points -- whether hypotheses are drawn,
// which minimal solver draws them, m, the mode of the final stage, the n < 4 failure -- is read per sample in the kernels
// (opp_pnp_mode, pnp_batch.h), and a workgroup whose sample does not use a kernel returns at once.  Each sample reads its own
// K4 and seed from device arrays and owns an `iterations`-sized slab of hyp / valid / score / score2; the EPnP refit's points
// of sample b start at 13 * offsets[b] doubles of one 13 * n_total array (opp_pnp_layout).  Offsets that do not describe a segment of
// [0, n_total] make an empty sample (opp_pnp_extent): nothing is read or written outside the caller's arrays.
//
//   grid (ceil(iters / 256), B)  pnp_batch_hypotheses_kernel       P3P hypotheses (solver 0; solver 1 when n == 4)
//   grid (iters, B) x 64         pnp_batch_epnp_hypotheses_kernel  EPnP hypotheses (solver 1, n >= 6)
//   grid (ceil(iters / 4), B)    pnp_batch_score_kernel
//   grid (B)                     pnp_batch_stop_kernel + pnp_batch_refine_kernel (solver 0) / pnp_batch_epnp_final_kernel (solver 1)
//
// Per sample the result is that of opp_pnp_ransac_ex on its slice, bit for bit (tests/test_pnp_batch_gpu.py).
#include "opp_common.h"
#include "pnp_args.h"
#include "pnp_batch.h"
#include "pnp_body.h"

namespace {

struct PnpBatch {
  const float* p2;
  const float* p3;
  const int* offsets;      // [B+1]
  const double* K4;        // [B][4] fx, fy, cx, cy
  const unsigned* seeds;   // [B]
  double thr2, scale, conf;
  int n_total, iters, solver, refine_iters;
  double* hyp;             // per-sample slabs, hyp_stride doubles / int_stride ints apart
  int* valid;
  int* score;
  int* score2;
  double* pts;             // [13 * n_total]
  size_t hyp_stride, int_stride;
  double* pose_out;        // [B][12]
  int* mask;               // [n_total]
  int* n_inl;              // [B]
  int* ok;                 // [B]
  int* stop;               // [B]
};

struct PnpSample {
  PnpParams prm;
  int first, mode, m;
};

__device__ __forceinline__ PnpSample pnp_load_sample(const PnpBatch& a, int b) {
  PnpSample s;
  opp_pnp_extent(a.offsets[b], a.offsets[b + 1], a.n_total, &s.first, &s.prm.n);
  for (int k = 0; k < 4; ++k) s.prm.K4[k] = a.K4[4 * b + k];
  s.prm.thr2 = a.thr2;
  s.prm.scale = a.scale;
  s.prm.iters = a.iters;
  s.prm.seed = a.seeds[b];
  s.mode = opp_pnp_mode(a.solver, s.prm.n, &s.m);
  return s;
}

// one thread per boundary (lower bound of b among the ids) and per id (the contract check); *bad is zeroed before the launch
__global__ __launch_bounds__(256) void pnp_offsets_kernel(const long long* __restrict__ m_bids, int n_total, int n_samples,
                                                          int* __restrict__ offsets, int* __restrict__ bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n_samples) offsets[i] = opp_pnp_offset(m_bids, n_total, i);
  if (i < n_total && opp_pnp_bid_bad(m_bids, i, n_samples)) *bad = 1;
}

__global__ __launch_bounds__(256) void pnp_batch_hypotheses_kernel(PnpBatch a) {
  const int b = blockIdx.y;
  const PnpSample s = pnp_load_sample(a, b);
  if (s.mode != OPP_PNP_P3P_RANSAC) return;
  pnp_hypotheses_body(a.p2 + (size_t)2 * s.first, a.p3 + (size_t)3 * s.first, s.prm, a.hyp + b * a.hyp_stride, a.valid + b * a.int_stride,
                      blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ __launch_bounds__(64) void pnp_batch_epnp_hypotheses_kernel(PnpBatch a) {
  const int b = blockIdx.y;
  const PnpSample s = pnp_load_sample(a, b);
  if (s.mode != OPP_PNP_EPNP_RANSAC) return;
  __shared__ PnpParams s_prm;   // the EPnP bodies index K4 by thread: in LDS, not in registers (no scratch)
  if (threadIdx.x == 0) s_prm = s.prm;
  __syncthreads();
  pnp_epnp_hypotheses_body(a.p2 + (size_t)2 * s.first, a.p3 + (size_t)3 * s.first, s_prm, a.hyp + b * a.hyp_stride,
                           a.valid + b * a.int_stride, nullptr, blockIdx.x);
}

__global__ __launch_bounds__(256) void pnp_batch_score_kernel(PnpBatch a) {
  const int b = blockIdx.y;
  const PnpSample s = pnp_load_sample(a, b);
  if (s.mode != OPP_PNP_P3P_RANSAC && s.mode != OPP_PNP_EPNP_RANSAC) return;
  pnp_score_body(a.p2 + (size_t)2 * s.first, a.p3 + (size_t)3 * s.first, s.prm, a.hyp + b * a.hyp_stride, a.valid + b * a.int_stride,
                 a.score + b * a.int_stride, blockIdx.x);
}

// solver 0: the stop index and the masked scores of every sample that drew hypotheses
__global__ __launch_bounds__(256) void pnp_batch_stop_kernel(PnpBatch a) {
  const int b = blockIdx.x;
  const PnpSample s = pnp_load_sample(a, b);
  if (s.mode != OPP_PNP_P3P_RANSAC) {
    if (threadIdx.x == 0) a.stop[b] = 0;
    return;
  }
  pnp_stop_body(a.score + b * a.int_stride, s.prm, s.m, a.conf, a.score2 + b * a.int_stride, a.stop + b);
}

// solver 0: one workgroup per sample; a sample without hypotheses refines over none of them and so fails (opp_pnp_ransac's n < 4)
__global__ __launch_bounds__(256) void pnp_batch_refine_kernel(PnpBatch a) {
  const int b = blockIdx.x;
  PnpSample s = pnp_load_sample(a, b);
  if (s.mode != OPP_PNP_P3P_RANSAC) s.prm.iters = 0;
  pnp_refine_body(a.p2 + (size_t)2 * s.first, a.p3 + (size_t)3 * s.first, s.prm, a.hyp + b * a.hyp_stride, a.score2 + b * a.int_stride,
                  a.refine_iters, a.pose_out + (size_t)12 * b, a.mask + s.first, a.n_inl + b, a.ok + b);
}

// solver 1: one workgroup per sample
__global__ __launch_bounds__(256) void pnp_batch_epnp_final_kernel(PnpBatch a) {
  const int b = blockIdx.x;
  const PnpSample s = pnp_load_sample(a, b);
  const int mode = opp_pnp_final_mode(s.mode);
  __shared__ PnpParams s_prm;   // as in pnp_batch_epnp_hypotheses_kernel
  if (threadIdx.x == 0) s_prm = s.prm;
  __syncthreads();
  pnp_epnp_final_body(a.p2 + (size_t)2 * s.first, a.p3 + (size_t)3 * s.first, s_prm, a.hyp + b * a.hyp_stride, a.score + b * a.int_stride,
                      mode, s.m, a.conf, a.pts + (size_t)13 * s.first, a.pose_out + (size_t)12 * b, a.mask + s.first, a.n_inl + b, a.ok + b,
                      a.stop + b);
}

}  // namespace

extern "C" size_t opp_pnp_batch_workspace_bytes(int iterations, int n_samples, int n_total) {
  return opp_pnp_layout(iterations, n_samples, n_total, nullptr);
}

extern "C" int opp_pnp_offsets(const long long* m_bids, int n_total, int n_samples, int* offsets, int* bad, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OPP_CHECK_ARG((n_total == 0 || m_bids) && n_total >= 0 && offsets && bad, "pnp_offsets: null argument");
  OPP_CHECK_ARG(n_samples >= 1 && n_samples <= 1024, "pnp_offsets: n_samples must be in [1, 1024]");
  if (hipMemsetAsync(bad, 0, sizeof(int), stream) != hipSuccess) {
    opp_set_error("pnp_offsets: clearing the flag failed");
    return OPP_ERR_LAUNCH;
  }
  const int threads = n_total > n_samples + 1 ? n_total : n_samples + 1;
  hipLaunchKernelGGL(pnp_offsets_kernel, dim3(opp_cdiv(threads, 256)), dim3(256), 0, stream, m_bids, n_total, n_samples, offsets, bad);
  OPP_CHECK_LAUNCH("pnp_offsets kernel");
  return OPP_OK;
}

extern "C" int opp_pnp_ransac_batch(const float* pts2d, const float* pts3d, const int* offsets, int n_samples, int n_total,
                                    const double* K4, const unsigned* seeds, double reproj_error_px, double scale, int iterations,
                                    int refine_iters, int solver, double confidence, double* pose_out, int* inlier_mask,
                                    int* n_inliers, int* ok, int* stop, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OPP_TRY(opp_pnp_check_batch("pnp_batch", n_samples, offsets, seeds, stop));
  OPP_TRY(opp_pnp_check_args("pnp_batch", pts2d, pts3d, n_total, K4, pose_out, inlier_mask, n_inliers, ok, ws, iterations, reproj_error_px,
                             scale > 0, confidence));
  OPP_TRY(opp_pnp_check_solver("pnp_batch", solver));
  OPP_CHECK_WS(ws_bytes >= opp_pnp_batch_workspace_bytes(iterations, n_samples, n_total), "pnp_batch: workspace too small");
  PnpBatch a;
  a.p2 = pts2d;
  a.p3 = pts3d;
  a.offsets = offsets;
  a.K4 = K4;
  a.seeds = seeds;
  a.thr2 = reproj_error_px * reproj_error_px;
  a.scale = scale;
  a.conf = confidence;
  a.n_total = n_total;
  a.iters = iterations;
  a.solver = solver;
  a.refine_iters = refine_iters;
  OppPnpLayout L;
  opp_pnp_layout(iterations, n_samples, n_total, &L);
  char* base = (char*)ws;
  a.hyp = (double*)(base + L.hyp);
  a.valid = (int*)(base + L.valid);
  a.score = (int*)(base + L.score);
  a.score2 = (int*)(base + L.score2);
  a.pts = (double*)(base + L.pts);
  a.hyp_stride = L.hyp_stride / sizeof(double);
  a.int_stride = L.int_stride / sizeof(int);
  a.pose_out = pose_out;
  a.mask = inlier_mask;
  a.n_inl = n_inliers;
  a.ok = ok;
  a.stop = stop;
  hipLaunchKernelGGL(pnp_batch_hypotheses_kernel, dim3(opp_cdiv(iterations, 256), n_samples), dim3(256), 0, stream, a);
  if (solver == 1) hipLaunchKernelGGL(pnp_batch_epnp_hypotheses_kernel, dim3(iterations, n_samples), dim3(64), 0, stream, a);
  hipLaunchKernelGGL(pnp_batch_score_kernel, dim3(opp_cdiv(iterations, 4), n_samples), dim3(256), 0, stream, a);
  if (solver == 0) {
    hipLaunchKernelGGL(pnp_batch_stop_kernel, dim3(n_samples), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(pnp_batch_refine_kernel, dim3(n_samples), dim3(256), 0, stream, a);
  } else {
    hipLaunchKernelGGL(pnp_batch_epnp_final_kernel, dim3(n_samples), dim3(256), 0, stream, a);
  }
  OPP_CHECK_LAUNCH("pnp_batch kernels");
  return OPP_OK;
}
