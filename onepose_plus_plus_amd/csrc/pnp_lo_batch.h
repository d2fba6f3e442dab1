// The pure logic of LO-RANSAC, written once for the device and the host (compiled with g++: tests/test_loransac_batch_cpu.py):
// what a sample of n matches runs -- opp_pnp_loransac (pnp_lo.hip) asks on the host, the batched kernels (pnp_lo_batch.hip) per
// sample --, the trials of the first pass, and the layout of the one workspace that holds every sample's buffers (B = 1: the
// single call's).
#pragma once
#include <stddef.h>

#include "pnp_batch.h"   // OPP_BHD, opp_ws_align, opp_pnp_extent
#include "pnp_math.h"    // OPP_LM_ROW

#define OPP_LO_GRID 32                     // LO workgroups per sample, each with its own OPP_LO_PTS_ROW * n doubles
#define OPP_LO_PTS_ROW 13                  // doubles per match and LO workgroup: X[3], uv[2], alphas[4], pcs[3], err
#define OPP_LO_FIN_ROW (5 + OPP_LM_ROW)    // doubles per match of the final stage: X[3], uv[2] and a row of the refinement

// what a sample runs
enum OppLoMode {
  OPP_LO_FAIL = 0,   // n < 3: pycolmap reports failure (identity pose, no inliers, ok 0, stop 0): the final kernel's mode 2 alone
  OPP_LO_RUN = 1     // every stage
};

OPP_BHD int opp_lo_mode(int n) { return n < 3 ? OPP_LO_FAIL : OPP_LO_RUN; }

// the trials every run evaluates, [0, t1): the first pass.  t1 == iterations: there is no second pass
OPP_BHD int opp_lo_first_pass(int min_trials, int iterations) {
  return min_trials < iterations ? (min_trials > 0 ? min_trials : 1) : iterations;
}

// byte offsets into the workspace.  The arrays that scale with the trials are per-sample slabs: sample b's starts at
// <array> + b * <stride>.  The point arrays follow the matches: sample b's LO region starts OPP_LO_GRID * OPP_LO_PTS_ROW *
// offsets[b] doubles into lo_pts, its final-stage region OPP_LO_FIN_ROW * offsets[b] doubles into fin_pts.
struct OppLoBatchLayout {
  size_t hyp, nmod, cnt, sum, cand_idx, cand_rc, cand_rs, cand_lc, cand_ls, cand_pose, cand_taken, ctl, lo_pts, fin_pts;
  size_t pose_stride;   // hyp, cand_pose: [iterations][4][12] doubles
  size_t i1_stride;     // nmod: [iterations] ints
  size_t i4_stride;     // cnt, cand_idx, cand_rc, cand_lc, cand_taken: [iterations * 4] ints
  size_t d4_stride;     // sum, cand_rs, cand_ls: [iterations * 4] doubles
  size_t ctl_stride;    // ctl: [0] number of candidates, [1] bound on the trials after the first pass
  size_t bytes;
};

OPP_BHD size_t opp_lo_batch_layout(int iterations, int n_samples, int n_total, OppLoBatchLayout* L) {
  const size_t I = (size_t)(iterations < 1 ? 1 : iterations), B = (size_t)(n_samples < 1 ? 1 : n_samples);
  const size_t n = (size_t)(n_total < 1 ? 1 : n_total);
  OppLoBatchLayout l;
  l.pose_stride = opp_ws_align(I * 48 * sizeof(double));
  l.i1_stride = opp_ws_align(I * sizeof(int));
  l.i4_stride = opp_ws_align(I * 4 * sizeof(int));
  l.d4_stride = opp_ws_align(I * 4 * sizeof(double));
  l.ctl_stride = 64;
  size_t off = 0;
  l.hyp = off, off += B * l.pose_stride;
  l.nmod = off, off += B * l.i1_stride;
  l.cnt = off, off += B * l.i4_stride;
  l.sum = off, off += B * l.d4_stride;
  l.cand_idx = off, off += B * l.i4_stride;
  l.cand_rc = off, off += B * l.i4_stride;
  l.cand_rs = off, off += B * l.d4_stride;
  l.cand_lc = off, off += B * l.i4_stride;
  l.cand_ls = off, off += B * l.d4_stride;
  l.cand_pose = off, off += B * l.pose_stride;
  l.cand_taken = off, off += B * l.i4_stride;
  l.ctl = off, off += opp_ws_align(B * l.ctl_stride);
  l.lo_pts = off, off += opp_ws_align((size_t)OPP_LO_GRID * OPP_LO_PTS_ROW * n * sizeof(double));
  l.fin_pts = off, off += opp_ws_align((size_t)OPP_LO_FIN_ROW * n * sizeof(double));
  l.bytes = off;
  if (L) *L = l;
  return off;
}
