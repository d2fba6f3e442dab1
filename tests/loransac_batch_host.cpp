// Host build of the batched LO-RANSAC's pure logic (onepose_plus_plus_amd/csrc/pnp_lo_batch.h) for CPU unit tests.
#include "../onepose_plus_plus_amd/csrc/pnp_lo_batch.h"

extern "C" {
int t_lo_mode(int n) { return opp_lo_mode(n); }

int t_lo_first_pass(int min_trials, int iterations) { return opp_lo_first_pass(min_trials, iterations); }

// the layout as 21 numbers: the 14 array offsets, the 5 strides, the total, and what opp_lo_batch_layout returns
void t_lo_layout(int iterations, int n_samples, int n_total, unsigned long long* out) {
  OppLoBatchLayout L;
  const size_t bytes = opp_lo_batch_layout(iterations, n_samples, n_total, &L);
  const size_t v[21] = {L.hyp,       L.nmod,       L.cnt,        L.sum,         L.cand_idx,  L.cand_rc,  L.cand_rs,
                        L.cand_lc,   L.cand_ls,    L.cand_pose,  L.cand_taken,  L.ctl,       L.lo_pts,   L.fin_pts,
                        L.pose_stride, L.i1_stride, L.i4_stride, L.d4_stride,   L.ctl_stride, L.bytes,   bytes};
  for (int k = 0; k < 21; ++k) out[k] = v[k];
}

// sample b's regions of the two point arrays, in bytes from the start of the workspace, as the kernels compute them from
// unvalidated offsets: {lo_pts begin, end, fin_pts begin, end}
void t_lo_point_regions(int iterations, int n_samples, int n_total, int o0, int o1, unsigned long long* out) {
  OppLoBatchLayout L;
  opp_lo_batch_layout(iterations, n_samples, n_total, &L);
  int first, n;
  opp_pnp_extent(o0, o1, n_total, &first, &n);
  const size_t lo_row = (size_t)OPP_LO_GRID * OPP_LO_PTS_ROW * sizeof(double), fin_row = (size_t)OPP_LO_FIN_ROW * sizeof(double);
  out[0] = L.lo_pts + lo_row * first;
  out[1] = out[0] + lo_row * n;
  out[2] = L.fin_pts + fin_row * first;
  out[3] = out[2] + fin_row * n;
}
}
