// The pure logic of the P3P / EPnP PnP-RANSAC, written once for the device and the host (compiled with g++:
// tests/test_pnp_batch_cpu.py): what a sample of n matches runs under a solver -- the one table opp_pnp_ransac_ex reads on the
// host from n_points and the batched kernels (pnp_batch.hip) read per sample --, the layout of the workspace of the single
// calls (pnp.hip, B = 1) and of the batch, and the sample boundaries from the matcher's batch ids.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define OPP_BHD __host__ __device__ inline
#else
#define OPP_BHD inline
#endif

// what a sample runs
enum OppPnpMode {
  OPP_PNP_FAIL = 0,         // n < 4: the reference's cv2.error branch (identity pose, no inliers, state False)
  OPP_PNP_P3P_RANSAC = 1,   // P3P hypotheses on 4-match samples (solver 0; solver 1 with exactly 4 matches, OpenCV's switch)
  OPP_PNP_EPNP_ONE = 2,     // solver 1, exactly 5 matches: one EPnP solve on all of them, no sampling
  OPP_PNP_EPNP_RANSAC = 3   // solver 1, n >= 6: EPnP hypotheses on 5-match samples
};

// solver 0 = P3P, 1 = EPnP.  *m = the model's minimal sample (a new best needs more than max(best, m - 1) inliers)
OPP_BHD int opp_pnp_mode(int solver, int n, int* m) {
  *m = (solver == 1 && n != 4) ? 5 : 4;
  if (n < 4) return OPP_PNP_FAIL;
  if (solver == 0 || n == 4) return OPP_PNP_P3P_RANSAC;
  return n == 5 ? OPP_PNP_EPNP_ONE : OPP_PNP_EPNP_RANSAC;
}

// the mode number of solver 1's final stage (pnp_epnp_final_body) for what opp_pnp_mode returned
OPP_BHD int opp_pnp_final_mode(int mode) {
  return mode == OPP_PNP_FAIL ? 3 : (mode == OPP_PNP_P3P_RANSAC ? 0 : (mode == OPP_PNP_EPNP_ONE ? 2 : 1));
}

OPP_BHD size_t opp_ws_align(size_t x) { return (x + 255) / 256 * 256; }

// byte offsets into the workspace: hyp | valid | score | score2 | pts.  The first four are per-sample slabs, sample b's at
// <array> + b * <stride>; the EPnP refit's points follow the matches, sample b's 13 * offsets[b] doubles into pts.
// opp_pnp_ransac needs hyp | valid | score alone, the bytes before score2 (at B = 1).
struct OppPnpLayout {
  size_t hyp, valid, score, score2, pts;
  size_t hyp_stride;   // hyp: [iterations][12] doubles, R | t
  size_t int_stride;   // valid, score, score2: [iterations] ints
  size_t bytes;
};

OPP_BHD size_t opp_pnp_layout(int iterations, int n_samples, int n_total, OppPnpLayout* L) {
  const size_t I = (size_t)(iterations < 1 ? 1 : iterations), B = (size_t)(n_samples < 1 ? 1 : n_samples);
  const size_t n = (size_t)(n_total < 1 ? 1 : n_total);
  OppPnpLayout l;
  l.hyp_stride = opp_ws_align(I * 12 * sizeof(double));
  l.int_stride = opp_ws_align(I * sizeof(int));
  size_t off = 0;
  l.hyp = off, off += B * l.hyp_stride;
  l.valid = off, off += B * l.int_stride;
  l.score = off, off += B * l.int_stride;
  l.score2 = off, off += B * l.int_stride;
  l.pts = off, off += opp_ws_align(n * 13 * sizeof(double));
  l.bytes = off + 1024;
  if (L) *L = l;
  return l.bytes;
}

// first index i in [0, n) with ids[i] >= key (n when there is none); ids non-decreasing
OPP_BHD int opp_lower_bound_i64(const long long* ids, int n, long long key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (ids[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// offsets[b] = where sample b starts among n_total ids sorted by sample; b in [0, n_samples]
OPP_BHD int opp_pnp_offset(const long long* ids, int n_total, int b) { return opp_lower_bound_i64(ids, n_total, (long long)b); }

// ids[i] breaks the contract: outside [0, n_samples) or below its predecessor
OPP_BHD bool opp_pnp_bid_bad(const long long* ids, int i, int n_samples) {
  return ids[i] < 0 || ids[i] >= (long long)n_samples || (i > 0 && ids[i] < ids[i - 1]);
}

// a sample's extent from offsets that nothing has validated: anything outside [0, n_total] or reversed counts as empty
OPP_BHD void opp_pnp_extent(int o0, int o1, int n_total, int* first, int* n) {
  const bool ok = o0 >= 0 && o1 >= o0 && o1 <= n_total;
  *first = ok ? o0 : 0;
  *n = ok ? o1 - o0 : 0;
}
