// The bodies of the PnP-RANSAC kernels, shared by the single-sample kernels (pnp.hip) and the batched ones (pnp_batch.hip):
// each kernel of either file is a few lines that find their sample's pointers and PnpParams and call one of these, so a
// sample of a batch runs the arithmetic of the single call, in the same order.  Device only.
#pragma once
#include "pnp_math.h"
#include "pnp_sample.h"

namespace {

// hypothesis h: 4 distinct matches from the hash RNG, Grunert P3P on three (double), the 4th disambiguates
__device__ __forceinline__ void pnp_hypotheses_body(const float* __restrict__ p2, const float* __restrict__ p3, const PnpParams& prm,
                                                    double* __restrict__ hyp, int* __restrict__ valid, int h) {
  if (h >= prm.iters) return;
  int idx[4];
  draw_sample<4>(prm.seed, h, prm.n, idx);   // the sampler pnp_p3p_samples_kernel records
  double y[3][3], x[3][3];
  for (int k = 0; k < 3; ++k) {
    const double u = ((double)p2[2 * idx[k]] - prm.K4[2]) / prm.K4[0];
    const double v = ((double)p2[2 * idx[k] + 1] - prm.K4[3]) / prm.K4[1];
    const double inv = 1.0 / sqrt(u * u + v * v + 1.0);
    y[k][0] = u * inv;
    y[k][1] = v * inv;
    y[k][2] = inv;
    for (int c = 0; c < 3; ++c) x[k][c] = (double)p3[3 * idx[k] + c] * prm.scale;
  }
  OppPose sol[4];
  const int ns = opp_p3p_grunert(y, x, sol);
  const double X4[3] = {(double)p3[3 * idx[3]] * prm.scale, (double)p3[3 * idx[3] + 1] * prm.scale,
                        (double)p3[3 * idx[3] + 2] * prm.scale};
  const double uv4[2] = {(double)p2[2 * idx[3]], (double)p2[2 * idx[3] + 1]};
  int best = -1;
  double best_e = 1e300;
  for (int i = 0; i < ns; ++i) {
    const double e = opp_reproj_err2(sol[i], prm.K4, X4, uv4);
    if (e < best_e) {
      best_e = e;
      best = i;
    }
  }
  const bool ok = best >= 0 && best_e <= prm.thr2 * 4.0;   // the 4th match must roughly agree
  valid[h] = ok ? 1 : 0;
  if (ok) {
    for (int k = 0; k < 9; ++k) hyp[(size_t)h * 12 + k] = sol[best].R[k];
    for (int k = 0; k < 3; ++k) hyp[(size_t)h * 12 + 9 + k] = sol[best].t[k];
  }
}

// one wave per hypothesis counts reprojection inliers over all matches; bx: index of the 256-thread block among the sample's
__device__ __forceinline__ void pnp_score_body(const float* __restrict__ p2, const float* __restrict__ p3, const PnpParams& prm,
                                               const double* __restrict__ hyp, const int* __restrict__ valid, int* __restrict__ score,
                                               int bx) {
  const int lane = threadIdx.x & 63;
  const int h = bx * 4 + (threadIdx.x >> 6);
  if (h >= prm.iters) return;
  int cnt = 0;
  if (valid[h]) {
    OppPose P;
    for (int k = 0; k < 9; ++k) P.R[k] = hyp[(size_t)h * 12 + k];
    for (int k = 0; k < 3; ++k) P.t[k] = hyp[(size_t)h * 12 + 9 + k];
    for (int i = lane; i < prm.n; i += 64) {
      const double X[3] = {(double)p3[3 * i] * prm.scale, (double)p3[3 * i + 1] * prm.scale, (double)p3[3 * i + 2] * prm.scale};
      const double uv[2] = {(double)p2[2 * i], (double)p2[2 * i + 1]};
      cnt += opp_reproj_err2(P, prm.K4, X, uv) <= prm.thr2 ? 1 : 0;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) score[h] = valid[h] ? cnt : -1;   // -1: degenerate sample, never the best
}

// one 256-thread workgroup: best hypothesis, Gauss-Newton refinement on its inliers, final inlier mask
__device__ __forceinline__ void pnp_refine_body(const float* __restrict__ p2, const float* __restrict__ p3, const PnpParams& prm,
                                                const double* __restrict__ hyp, const int* __restrict__ score, int gn_iters,
                                                double* __restrict__ pose_out, int* __restrict__ mask, int* __restrict__ n_inl,
                                                int* __restrict__ ok_out) {
  __shared__ int s_best[256], s_idx[256];
  __shared__ double s_red[4][27];
  __shared__ OppPose s_pose;
  __shared__ int s_cnt[4];
  __shared__ int s_fail;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int bs = -1, bi = 0x7fffffff;
  for (int h = tid; h < prm.iters; h += 256)
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
  const int best_score = s_best[0], best_h = s_idx[0];
  if (tid == 0) {
    // fail only without any valid hypothesis (fewer than 4 matches, degenerate geometry): the reference's cv2.error
    // branch.  A best hypothesis with fewer than 4 inliers is still returned (state True, its few inliers), like
    // cv2.solvePnPRansac, which then reports success with an empty / tiny inlier set (metric_utils.py:194-196)
    s_fail = best_score < 0 ? 1 : 0;
    if (!s_fail) {
      for (int k = 0; k < 9; ++k) s_pose.R[k] = hyp[(size_t)best_h * 12 + k];
      for (int k = 0; k < 3; ++k) s_pose.t[k] = hyp[(size_t)best_h * 12 + 9 + k];
    }
  }
  __syncthreads();
  if (s_fail) {   // same failure convention as the reference's cv2.error branch: identity pose, no inliers
    if (tid < 12) pose_out[tid] = (tid == 0 || tid == 5 || tid == 10) ? 1.0 : 0.0;
    for (int i = tid; i < prm.n; i += 256) mask[i] = 0;
    if (tid == 0) {
      *n_inl = 0;
      *ok_out = 0;
    }
    return;
  }
  for (int it = 0; it <= gn_iters; ++it) {
    const OppPose P = s_pose;
    double acc[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
    int cnt = 0;
    const bool last = it == gn_iters;
    for (int i = tid; i < prm.n; i += 256) {
      const double X[3] = {(double)p3[3 * i] * prm.scale, (double)p3[3 * i + 1] * prm.scale, (double)p3[3 * i + 2] * prm.scale};
      const double uv[2] = {(double)p2[2 * i], (double)p2[2 * i + 1]};
      const bool in = opp_reproj_err2(P, prm.K4, X, uv) <= prm.thr2;
      cnt += in ? 1 : 0;
      if (last) {
        mask[i] = in ? 1 : 0;
      } else if (in) {
        double H[36], g[6];
#pragma unroll
        for (int k = 0; k < 36; ++k) H[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) g[k] = 0.0;
        opp_gn_accumulate(P, prm.K4, X, uv, H, g);
        int q = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
          for (int c = r; c < 6; ++c) acc[q++] += H[r * 6 + c];
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[21 + k] += g[k];
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) s_cnt[wave] = cnt;
    if (!last) {
#pragma unroll
      for (int k = 0; k < 27; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) s_red[wave][k] = v;
      }
    }
    __syncthreads();
    if (tid == 0) {
      const int total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
      if (last) {
        *n_inl = total;
        *ok_out = 1;
      } else if (total >= 4) {
        double H[36], g[6];
        int q = 0;
        for (int r = 0; r < 6; ++r)
          for (int c = r; c < 6; ++c) {
            const double v = s_red[0][q] + s_red[1][q] + s_red[2][q] + s_red[3][q];
            H[r * 6 + c] = v;
            H[c * 6 + r] = v;
            ++q;
          }
        for (int k = 0; k < 6; ++k) g[k] = s_red[0][21 + k] + s_red[1][21 + k] + s_red[2][21 + k] + s_red[3][21 + k];
        if (opp_solve6(H, g)) {
          OppPose N = s_pose;
          opp_rot_update(N.R, g);
          double E[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
          opp_rot_update(E, g);
          for (int r = 0; r < 3; ++r)
            N.t[r] = E[r * 3] * s_pose.t[0] + E[r * 3 + 1] * s_pose.t[1] + E[r * 3 + 2] * s_pose.t[2] + g[3 + r];
          s_pose = N;
        }
      }
    }
    __syncthreads();
  }
  // [R | t / scale] row-major 3x4 (the reference divides tvec by the scale again, metric_utils.py:192)
  if (tid < 12) {
    const int r = tid / 4, c = tid % 4;
    pose_out[tid] = c < 3 ? s_pose.R[r * 3 + c] : s_pose.t[r] / prm.scale;
  }
}

// one 64-thread workgroup (one wave) for hypothesis h: 5 distinct matches -> EPnP -> hyp[h] (R | t), valid[h]
__device__ __forceinline__ void pnp_epnp_hypotheses_body(const float* __restrict__ p2, const float* __restrict__ p3, const PnpParams& prm,
                                                         double* __restrict__ hyp, int* __restrict__ valid, int* __restrict__ samples,
                                                         int h) {
  __shared__ OppEpnpWs w;
  __shared__ double sX[15], suv[10], salph[20], spcs[15], sperr[5], sK[4];
  __shared__ int sidx[5], sdistinct;
  const int tid = threadIdx.x;
  if (tid == 0) {
    int idx[5];
    draw_sample<5>(prm.seed, h, prm.n, idx);
    bool distinct = true;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      sidx[k] = idx[k];
#pragma unroll
      for (int j = 0; j < k; ++j) distinct &= idx[j] != idx[k];
    }
    sdistinct = distinct ? 1 : 0;
    if (samples) {
#pragma unroll
      for (int k = 0; k < 5; ++k) samples[(size_t)h * 5 + k] = idx[k];
    }
  }
  if (tid < 4) sK[tid] = prm.K4[tid];
  __syncthreads();
  if (tid < 5) {
    const int i = sidx[tid];
    for (int c = 0; c < 3; ++c) sX[3 * tid + c] = (double)p3[3 * i + c] * prm.scale;
    suv[2 * tid] = (double)p2[2 * i];
    suv[2 * tid + 1] = (double)p2[2 * i + 1];
  }
  __syncthreads();
  opp_epnp_solve(sX, suv, 5, sK, &w, salph, spcs, sperr, tid, 64);
  const bool ok = w.best > 0 && sdistinct;
  if (tid < 12 && ok) hyp[(size_t)h * 12 + tid] = w.Rt[w.best][tid];
  if (tid == 0) valid[h] = ok ? 1 : 0;
}

// the sequential RANSAC loop over score[0, iters) (opp_ransac_stop), run by thread 0 over the 256ths of the range whose maximum
// exceeds the current threshold (no other hypothesis can become the best).  Every thread of the 256-thread block calls it.
// Also returns the lowest-index hypothesis of the highest score (-1 when no hypothesis produced a model).
__device__ __forceinline__ void ransac_scan(const int* __restrict__ score, int iters, int n, int m, double conf, int* s_cmax, int* stop,
                                            int* best, int* best_any) {
  const int tid = threadIdx.x;
  const int chunk = (iters + 255) / 256;
  int mx = -1;
  for (int i = tid * chunk; i < min(iters, (tid + 1) * chunk); ++i) mx = max(mx, score[i]);
  s_cmax[tid] = mx;
  __syncthreads();
  if (tid == 0) {
    int niters = iters, bc = 0, b = -1, gmax = -1;
    for (int c = 0; c < 256; ++c) gmax = max(gmax, s_cmax[c]);
    for (int c = 0; c < 256; ++c) {
      const int lo = c * chunk;
      if (lo >= niters) break;
      if (s_cmax[c] <= max(bc, m - 1)) continue;
      for (int i = lo; i < min((c + 1) * chunk, niters); ++i) {
        const int sc = score[i];
        if (sc > max(bc, m - 1)) {
          b = i;
          bc = sc;
          if (conf < 1.0) niters = opp_ransac_update_iters(conf, (double)(n - sc) / n, m, niters);
        }
      }
    }
    *stop = b < 0 ? iters : max(b + 1, niters);
    *best = b;
    int ba = -1;
    if (gmax >= 0)
      for (int c = 0; c < 256 && ba < 0; ++c)
        if (s_cmax[c] == gmax)
          for (int i = c * chunk; i < min(iters, (c + 1) * chunk); ++i)
            if (score[i] == gmax) {
              ba = i;
              break;
            }
    *best_any = ba;
  }
  __syncthreads();
}

// P3P with an adaptive stop: the stop index, and the scores with every hypothesis past it masked out (-1) for the refinement
__device__ __forceinline__ void pnp_stop_body(const int* __restrict__ score, const PnpParams& prm, int m, double conf,
                                              int* __restrict__ score_masked, int* __restrict__ stop_out) {
  __shared__ int s_cmax[256], s_stop, s_best, s_any;
  ransac_scan(score, prm.iters, prm.n, m, conf, s_cmax, &s_stop, &s_best, &s_any);
  for (int h = threadIdx.x; h < prm.iters; h += 256) score_masked[h] = h < s_stop ? score[h] : -1;
  if (threadIdx.x == 0 && stop_out) *stop_out = s_stop;
}

// one 256-thread workgroup, the end of the EPnP path.  mode 0: RANSAC, pose = best hypothesis (n == 4, P3P hypotheses);
// 1: RANSAC + EPnP refit on the best hypothesis's inliers; 2: one EPnP solve on all n points (n == 5); 3: failure (n < 4).
// pts: n * 13 doubles of workspace (inlier points, barycentric coordinates, camera points, errors).
__device__ __forceinline__ void pnp_epnp_final_body(const float* __restrict__ p2, const float* __restrict__ p3, const PnpParams& prm,
                                                    const double* __restrict__ hyp, const int* __restrict__ score, int mode, int m,
                                                    double conf, double* __restrict__ pts, double* __restrict__ pose_out,
                                                    int* __restrict__ mask, int* __restrict__ n_inl, int* __restrict__ ok_out,
                                                    int* __restrict__ stop_out) {
  __shared__ OppEpnpWs w;
  __shared__ int s_cmax[256], s_off[257];
  __shared__ int s_stop, s_best, s_any, s_fail, s_hyp, s_nin, s_refit;
  __shared__ double sK[4];
  __shared__ OppPose s_pose;
  const int tid = threadIdx.x, n = prm.n;
  if (tid < 4) sK[tid] = prm.K4[tid];
  if (mode <= 1) {
    ransac_scan(score, prm.iters, n, m, conf, s_cmax, &s_stop, &s_best, &s_any);
  } else if (tid == 0) {
    s_stop = 0;
    s_best = -1;
    s_any = -1;
  }
  if (tid == 0) {
    s_fail = mode == 3 || (mode <= 1 && s_any < 0);
    s_hyp = s_best >= 0 ? s_best : s_any;
    s_refit = mode == 2 || (mode == 1 && s_best >= 0);
    if (!s_fail && mode <= 1) {
      for (int k = 0; k < 9; ++k) s_pose.R[k] = hyp[(size_t)s_hyp * 12 + k];
      for (int k = 0; k < 3; ++k) s_pose.t[k] = hyp[(size_t)s_hyp * 12 + 9 + k];
    }
    if (stop_out) *stop_out = s_stop;
  }
  __syncthreads();
  if (s_fail) {   // the reference's cv2.error branch: identity pose, no inliers, state False
    if (tid < 12) pose_out[tid] = (tid == 0 || tid == 5 || tid == 10) ? 1.0 : 0.0;
    for (int i = tid; i < n; i += 256) mask[i] = 0;
    if (tid == 0) {
      *n_inl = 0;
      *ok_out = 0;
    }
    return;
  }
  // inliers of the chosen hypothesis (the scoring predicate), compacted in point order: thread t owns points [t*ch, (t+1)*ch)
  const int ch = (n + 255) / 256, lo = min(n, tid * ch), hi = min(n, lo + ch);
  const bool all = mode == 2, keep = all || s_best >= 0;   // no hypothesis reached m inliers: pose kept, inliers empty
  const OppPose P = s_pose;
  int cnt = 0;
  for (int i = lo; i < hi; ++i) {
    bool in = all;
    if (!all) {
      const double X[3] = {(double)p3[3 * i] * prm.scale, (double)p3[3 * i + 1] * prm.scale, (double)p3[3 * i + 2] * prm.scale};
      const double uv[2] = {(double)p2[2 * i], (double)p2[2 * i + 1]};
      in = keep && opp_reproj_err2(P, prm.K4, X, uv) <= prm.thr2;
    }
    mask[i] = in ? 1 : 0;
    cnt += in ? 1 : 0;
  }
  s_off[tid + 1] = cnt;
  __syncthreads();
  if (tid == 0) {
    s_off[0] = 0;
    for (int t = 0; t < 256; ++t) s_off[t + 1] += s_off[t];
    s_nin = s_off[256];
  }
  __syncthreads();
  if (s_refit) {
    const int nin = s_nin;
    double* X = pts;
    double* uv = X + (size_t)3 * nin;
    double* alph = uv + (size_t)2 * nin;
    double* pcs = alph + (size_t)4 * nin;
    double* perr = pcs + (size_t)3 * nin;
    int o = s_off[tid];
    for (int i = lo; i < hi; ++i)
      if (mask[i]) {
        for (int c = 0; c < 3; ++c) X[3 * o + c] = (double)p3[3 * i + c] * prm.scale;
        uv[2 * o] = (double)p2[2 * i];
        uv[2 * o + 1] = (double)p2[2 * i + 1];
        ++o;
      }
    __threadfence_block();
    __syncthreads();
    opp_epnp_solve(X, uv, nin, sK, &w, alph, pcs, perr, tid, 256);
    if (tid == 0) {
      if (w.best > 0) {
        for (int k = 0; k < 9; ++k) s_pose.R[k] = w.Rt[w.best][k];
        for (int k = 0; k < 3; ++k) s_pose.t[k] = w.Rt[w.best][9 + k];
      } else if (mode == 2) {
        s_fail = 1;
      }
    }
    __syncthreads();
    if (s_fail) {   // a degenerate 5-point input (OpenCV's solvePnP fails there)
      if (tid < 12) pose_out[tid] = (tid == 0 || tid == 5 || tid == 10) ? 1.0 : 0.0;
      for (int i = tid; i < n; i += 256) mask[i] = 0;
      if (tid == 0) {
        *n_inl = 0;
        *ok_out = 0;
      }
      return;
    }
  }
  if (tid < 12) {
    const int r = tid / 4, c = tid % 4;
    pose_out[tid] = c < 3 ? s_pose.R[r * 3 + c] : s_pose.t[r] / prm.scale;
  }
  if (tid == 0) {
    *n_inl = s_nin;
    *ok_out = 1;
  }
}

}  // namespace
