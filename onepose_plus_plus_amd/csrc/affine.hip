// Affine RANSAC on 2D-2D matches for a batch of views in one enqueue: the estimator half of the reference's first-frame detector
// (LocalFeatureObjectDetector.match_worker / detect_by_matching: cv2.estimateAffine2D per database view, the view's image corners
// mapped through the result, the box of the view with the most inliers).  No device-to-host copy, no host decision on a view's
// size, no atomics: the same inputs give the same bits.
//
// The matches of all views lie concatenated in view order, delimited by a device array offsets [V+1] (the convention of
// pnp_batch.hip; opp_pnp_extent turns anything that is no segment of [0, n_total] into an empty view).  Per view the result is
// that of OpenCV 4.x's RANSACPointSetRegistrator with modelPoints = 3 as we read it, evaluated in parallel: the stop index and the
// best hypothesis are those of the sequential loop over hypotheses 0, 1, ... (pnp_stop_body with m = 3).
//
//   grid (ceil(iters / 256), V)  affine_hypotheses_kernel  one thread per hypothesis: sample, collinearity test, closed-form model
//   grid (ceil(iters / 16), V)   affine_score_kernel       a workgroup scores 16 hypotheses of one view: their coefficients are
//                                                          wave-uniform (LDS), each match is loaded once per group, counts by ballot
//   grid (V)                     affine_stop_kernel        the sequential loop's stop index, scores masked past it
//   grid (V)                     affine_final_kernel       best hypothesis, inlier mask, centred least-squares refit, box
//   grid (1)                     affine_select_kernel      the view with the most inliers (the first on ties) and its box
//
// A workgroup whose view does not use a kernel returns at once.
#include "affine_batch.h"
#include "opp_common.h"
#include "pnp_body.h"

namespace {

constexpr int kScoreGroup = 16;   // hypotheses a scoring workgroup owns

struct AffineBatch {
  const float* p0;         // [n_total][2] source points (the database view)
  const float* p1;         // [n_total][2] destination points (the query frame)
  const int* offsets;      // [V+1]
  const unsigned* seeds;   // [V]
  const double* corners;   // [V][4][2]
  double thr2, conf;
  int n_total, n_views, iters, refine;
  int fb0, fb1, fb2, fb3;  // the fallback box
  double* hyp;             // per-view slabs, hyp_stride doubles / int_stride ints apart
  int* valid;
  int* score;
  int* score2;
  size_t hyp_stride, int_stride;
  double* affine_out;      // [V][6]
  int* mask;               // [n_total]
  int* n_inl;              // [V]
  int* ok;                 // [V]
  int* stop;               // [V]
  int* boxes;              // [V][4]
  int* best_view;          // [1]
  int* best_box;           // [4]
  int* samples_out;        // [V][iters][3] or null
  int* scores_out;         // [V][iters] or null
};

struct AffineView {
  int first, n, mode, hyps;
};

__device__ __forceinline__ AffineView affine_load_view(const AffineBatch& a, int v) {
  AffineView s;
  opp_pnp_extent(a.offsets[v], a.offsets[v + 1], a.n_total, &s.first, &s.n);
  s.mode = opp_affine_mode(s.n);
  s.hyps = opp_affine_hypotheses(s.mode, a.iters);
  return s;
}

__global__ __launch_bounds__(256) void affine_hypotheses_kernel(AffineBatch a) {
  const int v = blockIdx.y, h = blockIdx.x * blockDim.x + threadIdx.x;
  const AffineView s = affine_load_view(a, v);
  if (h >= a.iters) return;
  int i0 = -1, i1 = -1, i2 = -1;
  if (h < s.hyps) {
    if (s.mode == OPP_AFFINE_ONE) {
      i0 = 0, i1 = 1, i2 = 2;
    } else {
      int idx[3];
      draw_sample<3>(a.seeds[v], h, s.n, idx);
      i0 = idx[0], i1 = idx[1], i2 = idx[2];
    }
  }
  if (a.samples_out) {
    int* so = a.samples_out + ((size_t)v * a.iters + h) * 3;
    so[0] = i0, so[1] = i1, so[2] = i2;
  }
  if (h >= s.hyps) return;
  const float* p0 = a.p0 + (size_t)2 * s.first;
  const float* p1 = a.p1 + (size_t)2 * s.first;
  const double x0 = p0[2 * i0], y0 = p0[2 * i0 + 1], x1 = p0[2 * i1], y1 = p0[2 * i1 + 1], x2 = p0[2 * i2], y2 = p0[2 * i2 + 1];
  // a sample that repeats a match has two identical source points: collinear
  const bool good = !opp_affine_collinear(x0, y0, x1, y1, x2, y2);
  a.valid[v * a.int_stride + h] = good ? 1 : 0;
  if (!good) return;
  const double X0 = p1[2 * i0], Y0 = p1[2 * i0 + 1], X1 = p1[2 * i1], Y1 = p1[2 * i1 + 1], X2 = p1[2 * i2], Y2 = p1[2 * i2 + 1];
  double M[6];
  opp_affine_from3(x0, y0, x1, y1, x2, y2, X0, Y0, X1, Y1, X2, Y2, M);
  double* out = a.hyp + v * a.hyp_stride + (size_t)h * 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) out[k] = M[k];
}

__global__ __launch_bounds__(256) void affine_score_kernel(AffineBatch a) {
  __shared__ double s_M[kScoreGroup][6];
  __shared__ int s_valid[kScoreGroup];
  __shared__ int s_cnt[4][kScoreGroup];
  const int v = blockIdx.y, h0 = blockIdx.x * kScoreGroup, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const AffineView s = affine_load_view(a, v);
  if (h0 >= s.hyps) {   // hypotheses the view does not evaluate: recorded as "no model", nothing else to do
    if (a.scores_out && tid < kScoreGroup && h0 + tid < a.iters) a.scores_out[(size_t)v * a.iters + h0 + tid] = -1;
    return;
  }
  if (tid < kScoreGroup) {
    const int h = h0 + tid;
    const int ok = h < s.hyps ? a.valid[v * a.int_stride + h] : 0;
    s_valid[tid] = ok;
    const double* m = a.hyp + v * a.hyp_stride + (size_t)h * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) s_M[tid][k] = ok ? m[k] : 0.0;
  }
  __syncthreads();
  const float* p0 = a.p0 + (size_t)2 * s.first;
  const float* p1 = a.p1 + (size_t)2 * s.first;
  int cnt[kScoreGroup];
#pragma unroll
  for (int g = 0; g < kScoreGroup; ++g) cnt[g] = 0;
  for (int base = 0; base < s.n; base += 256) {   // every wave runs every trip: the ballots below see whole waves
    const int i = base + tid;
    const bool live = i < s.n;
    double x = 0.0, y = 0.0, X = 0.0, Y = 0.0;
    if (live) x = p0[2 * i], y = p0[2 * i + 1], X = p1[2 * i], Y = p1[2 * i + 1];
#pragma unroll
    for (int g = 0; g < kScoreGroup; ++g) {
      if (!s_valid[g]) continue;   // block-uniform
      const bool in = live && opp_affine_err2(s_M[g][0], s_M[g][1], s_M[g][2], s_M[g][3], s_M[g][4], s_M[g][5], x, y, X, Y) <= a.thr2;
      cnt[g] += __popcll(__ballot(in));   // NaN: not an inlier
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int g = 0; g < kScoreGroup; ++g) s_cnt[wave][g] = cnt[g];
  }
  __syncthreads();
  if (tid < kScoreGroup && h0 + tid < a.iters) {
    const int h = h0 + tid;
    const int sc = s_valid[tid] ? s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid] : -1;   // -1: never the best
    if (h < s.hyps) a.score[v * a.int_stride + h] = sc;
    if (a.scores_out) a.scores_out[(size_t)v * a.iters + h] = sc;
  }
}

__global__ __launch_bounds__(256) void affine_stop_kernel(AffineBatch a) {
  const int v = blockIdx.x;
  const AffineView s = affine_load_view(a, v);
  if (s.mode == OPP_AFFINE_FAIL) {
    if (threadIdx.x == 0) a.stop[v] = 0;
    return;
  }
  PnpParams prm = {};
  prm.n = s.n;
  prm.iters = s.hyps;
  pnp_stop_body(a.score + v * a.int_stride, prm, OPP_AFFINE_MODEL_POINTS, a.conf, a.score2 + v * a.int_stride, a.stop + v);
}

// the wave's part of a workgroup sum in a fixed order: butterfly within the wave -> s_red[slot][wave]; the caller adds the four
__device__ __forceinline__ void affine_block_sum(double x, double (*s_red)[4], int slot) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  if ((threadIdx.x & 63) == 0) s_red[slot][threadIdx.x >> 6] = x;
}

__device__ __forceinline__ void affine_fail(const AffineBatch& a, const AffineView& s, int v) {
  const int tid = threadIdx.x;
  if (tid < 6) a.affine_out[(size_t)6 * v + tid] = (tid == 0 || tid == 4) ? 1.0 : 0.0;
  for (int i = tid; i < s.n; i += 256) a.mask[s.first + i] = 0;
  if (tid == 0) {
    a.n_inl[v] = 0;
    a.ok[v] = 0;
    int* box = a.boxes + 4 * v;
    box[0] = a.fb0, box[1] = a.fb1, box[2] = a.fb2, box[3] = a.fb3;
  }
}

// one 256-thread workgroup per view: the best hypothesis before the stop index, its inliers (the ones returned), the
// least-squares refit on them in coordinates centred on their mean, the box of the mapped corners
__global__ __launch_bounds__(256) void affine_final_kernel(AffineBatch a) {
  __shared__ int s_best[256], s_idx[256];
  __shared__ double s_red[11][4];
  __shared__ double s_M[6], s_mean[4];
  __shared__ int s_cnt[4], s_nin, s_boxok, s_box[4];
  const int v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const AffineView s = affine_load_view(a, v);
  if (s.mode == OPP_AFFINE_FAIL) {
    affine_fail(a, s, v);
    return;
  }
  const int* score = a.score2 + v * a.int_stride;
  int bs = -1, bi = 0x7fffffff;
  for (int h = tid; h < s.hyps; h += 256)
    if (score[h] > bs) {
      bs = score[h];
      bi = h;
    }
  s_best[tid] = bs;
  s_idx[tid] = bi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      const int ob = s_best[tid + o], oi = s_idx[tid + o];
      if (ob > s_best[tid] || (ob == s_best[tid] && oi < s_idx[tid])) {
        s_best[tid] = ob;
        s_idx[tid] = oi;
      }
    }
    __syncthreads();
  }
  // the sequential loop takes a hypothesis only above max(best, 2) inliers: with at most 2 there is no model (OpenCV returns false)
  if (s_best[0] < OPP_AFFINE_MODEL_POINTS) {
    affine_fail(a, s, v);
    return;
  }
  if (tid < 6) s_M[tid] = a.hyp[v * a.hyp_stride + (size_t)s_idx[0] * 6 + tid];
  __syncthreads();
  const float* p0 = a.p0 + (size_t)2 * s.first;
  const float* p1 = a.p1 + (size_t)2 * s.first;
  int* mask = a.mask + s.first;
  const double m0 = s_M[0], m1 = s_M[1], m2 = s_M[2], m3 = s_M[3], m4 = s_M[4], m5 = s_M[5];
  int cnt = 0;
  double sx = 0.0, sy = 0.0, sX = 0.0, sY = 0.0;
  for (int i = tid; i < s.n; i += 256) {
    const double x = p0[2 * i], y = p0[2 * i + 1], X = p1[2 * i], Y = p1[2 * i + 1];
    const bool in = opp_affine_err2(m0, m1, m2, m3, m4, m5, x, y, X, Y) <= a.thr2;
    mask[i] = in ? 1 : 0;
    cnt += in ? 1 : 0;
    sx += in ? x : 0.0;
    sy += in ? y : 0.0;
    sX += in ? X : 0.0;
    sY += in ? Y : 0.0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) s_cnt[wave] = cnt;
  affine_block_sum(sx, s_red, 0);
  affine_block_sum(sy, s_red, 1);
  affine_block_sum(sX, s_red, 2);
  affine_block_sum(sY, s_red, 3);
  __syncthreads();
  if (tid == 0) s_nin = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
  if (tid < 4) s_mean[tid] = ((s_red[tid][0] + s_red[tid][1]) + (s_red[tid][2] + s_red[tid][3]));
  __syncthreads();
  const int nin = s_nin;
  if (a.refine && nin > OPP_AFFINE_MODEL_POINTS) {   // block-uniform
    const double mx = s_mean[0] / nin, my = s_mean[1] / nin, mX = s_mean[2] / nin, mY = s_mean[3] / nin;
    double Sxx = 0.0, Sxy = 0.0, Syy = 0.0, SxX = 0.0, SyX = 0.0, SxY = 0.0, SyY = 0.0;
    for (int i = tid; i < s.n; i += 256) {
      if (!mask[i]) continue;   // this thread's own store above
      const double x = (double)p0[2 * i] - mx, y = (double)p0[2 * i + 1] - my, X = (double)p1[2 * i] - mX, Y = (double)p1[2 * i + 1] - mY;
      Sxx += x * x;
      Sxy += x * y;
      Syy += y * y;
      SxX += x * X;
      SyX += y * X;
      SxY += x * Y;
      SyY += y * Y;
    }
    affine_block_sum(Sxx, s_red, 4);
    affine_block_sum(Sxy, s_red, 5);
    affine_block_sum(Syy, s_red, 6);
    affine_block_sum(SxX, s_red, 7);
    affine_block_sum(SyX, s_red, 8);
    affine_block_sum(SxY, s_red, 9);
    affine_block_sum(SyY, s_red, 10);
    __syncthreads();
    if (tid == 0) {
      double S[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) S[k] = (s_red[4 + k][0] + s_red[4 + k][1]) + (s_red[4 + k][2] + s_red[4 + k][3]);
      double M[6];
      if (opp_affine_refit(mx, my, mX, mY, S[0], S[1], S[2], S[3], S[4], S[5], S[6], M)) {   // a degenerate refit keeps the model
#pragma unroll
        for (int k = 0; k < 6; ++k) s_M[k] = M[k];
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    int box[4];
    const bool okb = opp_affine_box(s_M, a.corners + (size_t)8 * v, box);
    s_boxok = okb ? 1 : 0;
    if (okb) {
#pragma unroll
      for (int k = 0; k < 4; ++k) s_box[k] = box[k];
    }
  }
  __syncthreads();
  if (!s_boxok) {   // a corner that no int32 holds: the view fails, as box_from_pose does
    affine_fail(a, s, v);
    return;
  }
  if (tid < 6) a.affine_out[(size_t)6 * v + tid] = s_M[tid];
  if (tid < 4) a.boxes[4 * v + tid] = s_box[tid];
  if (tid == 0) {
    a.n_inl[v] = nin;
    a.ok[v] = 1;
  }
}

// one workgroup: the view with the most inliers among those that produced a model, the first one on ties (the reference sorts
// with Python's stable sort); none: -1 and the fallback box
__global__ __launch_bounds__(256) void affine_select_kernel(AffineBatch a) {
  __shared__ int s_best[256], s_idx[256];
  const int tid = threadIdx.x;
  int bs = -1, bi = 0x7fffffff;
  for (int v = tid; v < a.n_views; v += 256) {
    const int sc = a.ok[v] ? a.n_inl[v] : -1;
    if (sc > bs) {
      bs = sc;
      bi = v;
    }
  }
  s_best[tid] = bs;
  s_idx[tid] = bi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      const int ob = s_best[tid + o], oi = s_idx[tid + o];
      if (ob > s_best[tid] || (ob == s_best[tid] && oi < s_idx[tid])) {
        s_best[tid] = ob;
        s_idx[tid] = oi;
      }
    }
    __syncthreads();
  }
  const bool any = s_best[0] >= 0;
  if (tid == 0) a.best_view[0] = any ? s_idx[0] : -1;
  if (tid < 4) {
    const int fb = tid == 0 ? a.fb0 : (tid == 1 ? a.fb1 : (tid == 2 ? a.fb2 : a.fb3));
    a.best_box[tid] = any ? a.boxes[4 * s_idx[0] + tid] : fb;
  }
}

}  // namespace

extern "C" size_t opp_affine2d_batch_workspace_bytes(int iterations, int n_views, int n_total) {
  return opp_affine_layout(iterations, n_views, n_total, nullptr);
}

extern "C" int opp_affine2d_ransac_batch(const float* pts0, const float* pts1, const int* offsets, int n_views, int n_total,
                                         const unsigned* seeds, const double* corners, double thr_px, int iterations, double confidence,
                                         int refine, const int* fallback_box, double* affine_out, int* inlier_mask, int* n_inliers, int* ok,
                                         int* stop, int* boxes, int* best_view, int* best_box, int* samples_out, int* scores_out, void* ws,
                                         size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OPP_CHECK_ARG((n_total == 0 || (pts0 && pts1)) && n_total >= 0 && offsets && seeds && corners && fallback_box && affine_out && inlier_mask &&
                    n_inliers && ok && stop && boxes && best_view && best_box && ws,
                "affine2d_batch: null argument");
  OPP_CHECK_ARG(n_views >= 1 && n_views <= 1024, "affine2d_batch: n_views must be in [1, 1024]");
  OPP_CHECK_ARG(iterations > 0 && iterations <= (1 << 20) && thr_px > 0, "affine2d_batch: bad parameters");
  OPP_CHECK_ARG(confidence > 0.0, "affine2d_batch: confidence must be > 0 (>= 1: no early stop)");
  OppAffineLayout L;
  OPP_CHECK_WS(ws_bytes >= opp_affine_layout(iterations, n_views, n_total, &L), "affine2d_batch: workspace too small");
  // a match that no view's offsets cover is no inlier of anything: the whole mask is written
  if (n_total > 0 && hipMemsetAsync(inlier_mask, 0, (size_t)n_total * sizeof(int), stream) != hipSuccess) {
    opp_set_error("affine2d_batch: clearing the mask failed");
    return OPP_ERR_LAUNCH;
  }
  AffineBatch a;
  a.p0 = pts0;
  a.p1 = pts1;
  a.offsets = offsets;
  a.seeds = seeds;
  a.corners = corners;
  a.thr2 = thr_px * thr_px;
  a.conf = confidence;
  a.n_total = n_total;
  a.n_views = n_views;
  a.iters = iterations;
  a.refine = refine;
  a.fb0 = fallback_box[0], a.fb1 = fallback_box[1], a.fb2 = fallback_box[2], a.fb3 = fallback_box[3];
  char* base = (char*)ws;
  a.hyp = (double*)(base + L.hyp);
  a.valid = (int*)(base + L.valid);
  a.score = (int*)(base + L.score);
  a.score2 = (int*)(base + L.score2);
  a.hyp_stride = L.hyp_stride / sizeof(double);
  a.int_stride = L.int_stride / sizeof(int);
  a.affine_out = affine_out;
  a.mask = inlier_mask;
  a.n_inl = n_inliers;
  a.ok = ok;
  a.stop = stop;
  a.boxes = boxes;
  a.best_view = best_view;
  a.best_box = best_box;
  a.samples_out = samples_out;
  a.scores_out = scores_out;
  hipLaunchKernelGGL(affine_hypotheses_kernel, dim3(opp_cdiv(iterations, 256), n_views), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(affine_score_kernel, dim3(opp_cdiv(iterations, kScoreGroup), n_views), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(affine_stop_kernel, dim3(n_views), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(affine_final_kernel, dim3(n_views), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(affine_select_kernel, dim3(1), dim3(256), 0, stream, a);
  OPP_CHECK_LAUNCH("affine2d_batch kernels");
  return OPP_OK;
}
