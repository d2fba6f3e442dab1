// The bodies of the LO-RANSAC kernels, shared by the single-sample kernels (pnp_lo.hip) and the batched ones
// (pnp_lo_batch.hip): each kernel of either file is a few lines that find their sample's pointers, LoParams and LoBuffers and
// call one of these, so a sample of a batch runs the arithmetic of the single call, in the same order -- lane l sums the points
// l, l + 64, ... and a butterfly follows; the candidate scan is chunked by lim * 4 / 256; inliers are compacted in point order.
// Every loop has a fixed bound, no workgroup waits on another, all arrays live in LDS or in the workspace.  Device only, but for
// lo_buffers, which the host of pnp_lo.hip calls too.
#pragma once
#include "pnp_lo_batch.h"
#include "pnp_math.h"
#include "pnp_sample.h"
#include "../../include/opp_hip.h"

namespace {

struct LoParams {
  double K4[4];      // fx, fy, cx, cy (fy = fx for the reference's SIMPLE_PINHOLE camera)
  double thr2;       // squared reprojection threshold (px^2)
  double conf;
  double min_ratio;  // minimal inlier ratio of a successful estimate
  int n, iters, min_trials;
  unsigned seed;
};

struct LoBuffers {
  double* hyp;        // [iters][4][12] R | t of every model
  int* nmod;          // [iters] models of the trial
  int* cnt;           // [iters][4] inlier count, -1 = no model
  double* sum;        // [iters][4] residual sum of the inliers
  int* cand_idx;      // [iters * 4] 4 * trial + model of the candidates, ascending
  int* cand_rc;       // raw support
  double* cand_rs;
  int* cand_lc;       // support after LO
  double* cand_ls;
  double* cand_pose;  // [iters * 4][12] pose after LO
  int* cand_taken;
  int* ctl;           // [0] number of candidates, [1] bound on the trials after the first pass
  double* lo_pts;     // [OPP_LO_GRID][13 n]
  double* fin_pts;    // [21 n]
};

// sample b's buffers in a workspace laid out by opp_lo_batch_layout: its slabs, and the regions of the point arrays that follow
// its first match.  The single call is sample 0 of a batch of one
__host__ __device__ __forceinline__ LoBuffers lo_buffers(char* ws, const OppLoBatchLayout& L, int b, int first) {
  const size_t sb = (size_t)b;
  LoBuffers r;
  r.hyp = (double*)(ws + L.hyp + sb * L.pose_stride);
  r.nmod = (int*)(ws + L.nmod + sb * L.i1_stride);
  r.cnt = (int*)(ws + L.cnt + sb * L.i4_stride);
  r.sum = (double*)(ws + L.sum + sb * L.d4_stride);
  r.cand_idx = (int*)(ws + L.cand_idx + sb * L.i4_stride);
  r.cand_rc = (int*)(ws + L.cand_rc + sb * L.i4_stride);
  r.cand_rs = (double*)(ws + L.cand_rs + sb * L.d4_stride);
  r.cand_lc = (int*)(ws + L.cand_lc + sb * L.i4_stride);
  r.cand_ls = (double*)(ws + L.cand_ls + sb * L.d4_stride);
  r.cand_pose = (double*)(ws + L.cand_pose + sb * L.pose_stride);
  r.cand_taken = (int*)(ws + L.cand_taken + sb * L.i4_stride);
  r.ctl = (int*)(ws + L.ctl + sb * L.ctl_stride);
  r.lo_pts = (double*)(ws + L.lo_pts) + (size_t)OPP_LO_GRID * OPP_LO_PTS_ROW * (size_t)first;
  r.fin_pts = (double*)(ws + L.fin_pts) + (size_t)OPP_LO_FIN_ROW * (size_t)first;
  return r;
}

__device__ __forceinline__ void lo_load_pose(const double* src, OppPose& P) {
#pragma unroll
  for (int k = 0; k < 9; ++k) P.R[k] = src[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) P.t[k] = src[9 + k];
}

// support of pose P over all matches, by one wave; every lane returns the same (count, sum)
__device__ __forceinline__ void lo_wave_support(const OppPose& P, const LoParams& prm, const float* __restrict__ p2,
                                                const float* __restrict__ p3, int lane, int* cnt_out, double* sum_out) {
  int cnt = 0;
  double sum = 0.0;
  for (int i = lane; i < prm.n; i += 64) {
    const double X[3] = {(double)p3[3 * i], (double)p3[3 * i + 1], (double)p3[3 * i + 2]};
    const double uv[2] = {(double)p2[2 * i], (double)p2[2 * i + 1]};
    const double e = opp_reproj_err2(P, prm.K4, X, uv);
    if (e <= prm.thr2) {
      cnt += 1;
      sum += e;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    sum += __shfl_xor(sum, o, 64);
  }
  *cnt_out = cnt;
  *sum_out = sum;
}

// trial t = t0 + tx of [t0, min(t1, *bound)): 3 matches -> P3P -> hyp[t][0..ns), nmod[t]; tx: index of the thread among the
// sample's
__device__ __forceinline__ void lo_hypotheses_body(const float* __restrict__ p2, const float* __restrict__ p3, const LoParams& prm, int t0,
                                                   int t1, const int* __restrict__ bound, double* __restrict__ hyp, int* __restrict__ nmod,
                                                   int* __restrict__ samples, int tx) {
  const int t = t0 + tx;
  int lim = t1;
  if (bound) lim = min(lim, *bound);
  if (t >= lim) return;
  int idx[3];
  draw_sample<3>(prm.seed, t, prm.n, idx);
  if (samples) {
#pragma unroll
    for (int k = 0; k < 3; ++k) samples[(size_t)t * 3 + k] = idx[k];
  }
  const bool distinct = idx[0] != idx[1] && idx[0] != idx[2] && idx[1] != idx[2];
  double y[3][3], x[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double u = ((double)p2[2 * idx[k]] - prm.K4[2]) / prm.K4[0];
    const double v = ((double)p2[2 * idx[k] + 1] - prm.K4[3]) / prm.K4[1];
    const double inv = 1.0 / sqrt(u * u + v * v + 1.0);
    y[k][0] = u * inv;
    y[k][1] = v * inv;
    y[k][2] = inv;
#pragma unroll
    for (int c = 0; c < 3; ++c) x[k][c] = (double)p3[3 * idx[k] + c];
  }
  // the solver writes its poses straight into hyp[t] (an OppPose is the 12 doubles R | t)
  nmod[t] = distinct ? opp_p3p_grunert(y, x, reinterpret_cast<OppPose*>(hyp + (size_t)t * 48)) : 0;
}

// one 256-thread workgroup per trial t = t0 + bx, one wave per model
__device__ __forceinline__ void lo_score_body(const float* __restrict__ p2, const float* __restrict__ p3, const LoParams& prm, int t0, int t1,
                                              const int* __restrict__ bound, const double* __restrict__ hyp, const int* __restrict__ nmod,
                                              int* __restrict__ cnt, double* __restrict__ sum, const OppLoRecord& rec, int bx) {
  const int lane = threadIdx.x & 63, m = threadIdx.x >> 6;
  const int t = t0 + bx;
  int lim = t1;
  if (bound) lim = min(lim, *bound);
  if (t >= lim) return;
  const size_t e = (size_t)t * 4 + m;
  int c = -1;
  double s = 0.0;
  const bool have = m < nmod[t];
  if (have) {
    OppPose P;
    lo_load_pose(hyp + e * 12, P);
    lo_wave_support(P, prm, p2, p3, lane, &c, &s);
    if (rec.models && lane < 12) rec.models[e * 12 + lane] = hyp[e * 12 + lane];
  }
  if (lane == 0) {
    cnt[e] = c;
    sum[e] = s;
    if (rec.counts) rec.counts[e] = c;
    if (rec.sums) rec.sums[e] = s;
  }
}

// one 256-thread workgroup: the models of trials [0, min(t1, *bound)) whose support beats that of every earlier model, in order.
// skip_t1 >= 0: the second pass, nothing to do when the bound did not pass the first pass's trials.
__device__ __forceinline__ void lo_candidates_body(int t1, const int* __restrict__ bound, int skip_t1, const LoBuffers& b) {
  __shared__ int s_c[256], s_off[257];
  __shared__ double s_s[256];
  const int tid = threadIdx.x;
  int lim = t1;
  if (bound) lim = min(lim, *bound);
  if (skip_t1 >= 0 && *bound <= skip_t1) return;
  const int total = lim * 4, chunk = (total + 255) / 256;
  const int lo = min(total, tid * chunk), hi = min(total, lo + chunk);
  int bc = 0;
  double bs = OPP_LO_NOSUM;
  for (int e = lo; e < hi; ++e) {
    const int c = b.cnt[e];
    const double s = b.sum[e];
    if (c >= 0 && opp_support_better(c, s, bc, bs)) {
      bc = c;
      bs = s;
    }
  }
  s_c[tid] = bc;
  s_s[tid] = bs;
  __syncthreads();
  if (tid == 0) {   // exclusive prefix: the best support before each chunk
    int rc = 0;
    double rs = OPP_LO_NOSUM;
    for (int k = 0; k < 256; ++k) {
      const int c = s_c[k];
      const double s = s_s[k];
      s_c[k] = rc;
      s_s[k] = rs;
      if (opp_support_better(c, s, rc, rs)) {
        rc = c;
        rs = s;
      }
    }
  }
  __syncthreads();
  const int pc = s_c[tid];
  const double ps = s_s[tid];
  bc = pc;
  bs = ps;
  int k = 0;
  for (int e = lo; e < hi; ++e) {
    const int c = b.cnt[e];
    const double s = b.sum[e];
    if (c >= 0 && opp_support_better(c, s, bc, bs)) {
      bc = c;
      bs = s;
      ++k;
    }
  }
  s_off[tid + 1] = k;
  __syncthreads();
  if (tid == 0) {
    s_off[0] = 0;
    for (int q = 0; q < 256; ++q) s_off[q + 1] += s_off[q];
    b.ctl[0] = s_off[256];
  }
  __syncthreads();
  bc = pc;
  bs = ps;
  int o = s_off[tid];
  for (int e = lo; e < hi; ++e) {
    const int c = b.cnt[e];
    const double s = b.sum[e];
    if (c >= 0 && opp_support_better(c, s, bc, bs)) {
      bc = c;
      bs = s;
      b.cand_idx[o] = e;
      b.cand_rc[o] = c;
      b.cand_rs[o] = s;
      ++o;
    }
  }
}

// local optimisation of every candidate: one wave per workgroup, workgroup g of the sample's ng takes the candidates g, g + ng, ...
__device__ __forceinline__ void lo_optimise_body(const float* __restrict__ p2, const float* __restrict__ p3, const LoParams& prm,
                                                 const int* __restrict__ bound, int skip_t1, const LoBuffers& b, int g, int ng) {
  __shared__ OppEpnpWs w;
  __shared__ double sK[4], s_pose[12];
  const int tid = threadIdx.x, n = prm.n;
  if (skip_t1 >= 0 && *bound <= skip_t1) return;
  const int ncand = b.ctl[0];
  double* X = b.lo_pts + (size_t)g * 13 * n;
  double* uv = X + (size_t)3 * n;
  double* alph = uv + (size_t)2 * n;
  double* pcs = alph + (size_t)4 * n;
  double* perr = pcs + (size_t)3 * n;
  if (tid < 4) sK[tid] = prm.K4[tid];
  for (int c = g; c < ncand; c += ng) {
    const size_t e = (size_t)b.cand_idx[c];
    int bc = b.cand_rc[c];
    double bs = b.cand_rs[c];
    __syncthreads();
    if (tid < 12) s_pose[tid] = b.hyp[e * 12 + tid];
    __syncthreads();
    if (bc > OPP_LO_MIN_INLIERS) {
      for (int round = 0; round < OPP_LO_ROUNDS; ++round) {
        const int prev = bc;
        OppPose P;
        lo_load_pose(s_pose, P);
        int nin = 0;   // inliers of the best model so far, compacted in point order
        for (int base = 0; base < n; base += 64) {
          const int i = base + tid;
          bool in = false;
          double Xi[3] = {0.0, 0.0, 0.0}, ui[2] = {0.0, 0.0};
          if (i < n) {
            Xi[0] = (double)p3[3 * i];
            Xi[1] = (double)p3[3 * i + 1];
            Xi[2] = (double)p3[3 * i + 2];
            ui[0] = (double)p2[2 * i];
            ui[1] = (double)p2[2 * i + 1];
            in = opp_reproj_err2(P, prm.K4, Xi, ui) <= prm.thr2;
          }
          const unsigned long long bal = __ballot(in);
          const int pos = nin + __popcll(bal & ((1ull << tid) - 1ull));
          if (in) {
            X[3 * pos] = Xi[0];
            X[3 * pos + 1] = Xi[1];
            X[3 * pos + 2] = Xi[2];
            uv[2 * pos] = ui[0];
            uv[2 * pos + 1] = ui[1];
          }
          nin += __popcll(bal);
        }
        __threadfence_block();
        __syncthreads();
        if (nin <= OPP_LO_MIN_INLIERS) break;
        opp_epnp_solve(X, uv, nin, sK, &w, alph, pcs, perr, tid, 64);
        const int cand = w.best;
        if (cand == 0) break;
        OppPose Q;
        lo_load_pose(w.Rt[cand], Q);
        int c2;
        double s2;
        lo_wave_support(Q, prm, p2, p3, tid, &c2, &s2);
        const bool better = opp_support_better(c2, s2, bc, bs);
        __syncthreads();
        if (better) {
          bc = c2;
          bs = s2;
          if (tid < 12) s_pose[tid] = w.Rt[cand][tid];
        }
        __syncthreads();
        if (bc <= prev) break;
      }
    }
    if (tid == 0) {
      b.cand_lc[c] = bc;
      b.cand_ls[c] = bs;
    }
    if (tid < 12) b.cand_pose[(size_t)c * 12 + tid] = s_pose[tid];
  }
}

// one 256-thread workgroup.  mode 0: the walk over the first pass's candidates -> ctl[1] = bound on the trials; 1: the walk, the
// inlier mask, the refinement and the outputs; 2: fewer than 3 matches (the failure outputs).
__device__ __forceinline__ void lo_final_body(const float* __restrict__ p2, const float* __restrict__ p3, const LoParams& prm, int mode,
                                              const LoBuffers& b, double* __restrict__ pose_out, int* __restrict__ mask,
                                              int* __restrict__ n_inl, int* __restrict__ ok_out, int* __restrict__ stop_out,
                                              const OppLoRecord& rec) {
  __shared__ OppLmWs w;
  __shared__ int s_off[257];
  __shared__ int s_best, s_stop, s_fail, s_nin, s_ncand;
  __shared__ double sK[4];
  const int tid = threadIdx.x, n = prm.n;
  if (tid < 4) sK[tid] = prm.K4[tid];
  if (tid == 0) {
    const int ncand = mode == 2 ? 0 : b.ctl[0];
    int best = -1;
    s_stop = mode == 2 ? 0 : opp_lo_resolve(b.cand_idx, b.cand_rc, b.cand_rs, b.cand_lc, b.cand_ls, ncand, n, prm.conf, prm.min_trials,
                                            prm.iters, &best, b.cand_taken);
    s_best = best;
    s_ncand = ncand;
    s_fail = best < 0 || b.cand_lc[best] <= 0 || (double)b.cand_lc[best] < prm.min_ratio * (double)n;
    if (mode == 0) b.ctl[1] = s_stop;
  }
  __syncthreads();
  if (mode == 0) return;
  const int ncand = s_ncand, best = s_best;
  if (tid == 0) {
    if (stop_out) *stop_out = s_stop;
    if (rec.n_cand) *rec.n_cand = ncand;
  }
  for (int c = tid; c < ncand; c += 256) {
    if (rec.cand_idx) rec.cand_idx[c] = b.cand_idx[c];
    if (rec.cand_cnt) rec.cand_cnt[c] = b.cand_lc[c];
    if (rec.cand_sum) rec.cand_sum[c] = b.cand_ls[c];
    if (rec.cand_taken) rec.cand_taken[c] = b.cand_taken[c];
  }
  if (s_fail) {   // the reference's failure convention: identity pose, no inliers, state False
    if (tid < 12) {
      const double v = (tid == 0 || tid == 5 || tid == 10) ? 1.0 : 0.0;
      pose_out[tid] = v;
      if (rec.ransac_pose) rec.ransac_pose[tid] = v;
    }
    for (int i = tid; i < n; i += 256) mask[i] = 0;
    if (tid == 0) {
      *n_inl = 0;
      *ok_out = 0;
      if (rec.lm_iters) *rec.lm_iters = 0;
    }
    return;
  }
  if (tid == 0) lo_load_pose(b.cand_pose + (size_t)best * 12, w.P);
  __syncthreads();
  if (tid < 12 && rec.ransac_pose) rec.ransac_pose[tid] = (tid % 4) < 3 ? w.P.R[(tid / 4) * 3 + tid % 4] : w.P.t[tid / 4];
  // the RANSAC inliers of the best model (the ones returned), compacted in point order: thread t owns [t * ch, (t + 1) * ch)
  const int ch = (n + 255) / 256, lo = min(n, tid * ch), hi = min(n, lo + ch);
  const OppPose P = w.P;
  int cnt = 0;
  for (int i = lo; i < hi; ++i) {
    const double Xi[3] = {(double)p3[3 * i], (double)p3[3 * i + 1], (double)p3[3 * i + 2]};
    const double ui[2] = {(double)p2[2 * i], (double)p2[2 * i + 1]};
    const bool in = opp_reproj_err2(P, prm.K4, Xi, ui) <= prm.thr2;
    mask[i] = in ? 1 : 0;
    cnt += in ? 1 : 0;
  }
  s_off[tid + 1] = cnt;
  __syncthreads();
  if (tid == 0) {
    s_off[0] = 0;
    for (int q = 0; q < 256; ++q) s_off[q + 1] += s_off[q];
    s_nin = s_off[256];
  }
  __syncthreads();
  const int nin = s_nin;
  double* X = b.fin_pts;
  double* uv = X + (size_t)3 * n;
  double* rows = uv + (size_t)2 * n;
  int o = s_off[tid];
  for (int i = lo; i < hi; ++i)
    if (mask[i]) {
      for (int c = 0; c < 3; ++c) X[3 * o + c] = (double)p3[3 * i + c];
      uv[2 * o] = (double)p2[2 * i];
      uv[2 * o + 1] = (double)p2[2 * i + 1];
      ++o;
    }
  __threadfence_block();
  __syncthreads();
  opp_lm_refine(X, uv, nin, sK, &w, rows, tid, 256);
  if (tid < 12) pose_out[tid] = (tid % 4) < 3 ? w.P.R[(tid / 4) * 3 + tid % 4] : w.P.t[tid / 4];
  if (tid == 0) {
    *n_inl = nin;
    *ok_out = 1;
    if (rec.lm_iters) *rec.lm_iters = w.iters;
  }
}

}  // namespace
