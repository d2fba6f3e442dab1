// Host build of the batched PnP-RANSAC's pure logic (onepose_plus_plus_amd/csrc/pnp_batch.h) for CPU unit tests.
#include "../onepose_plus_plus_amd/csrc/pnp_batch.h"

extern "C" {
// what pnp_offsets_kernel computes, thread by thread: offsets [n_samples + 1] and the flag
void t_offsets(const long long* ids, int n_total, int n_samples, int* offsets, int* bad) {
  *bad = 0;
  for (int b = 0; b <= n_samples; ++b) offsets[b] = opp_pnp_offset(ids, n_total, b);
  for (int i = 0; i < n_total; ++i)
    if (opp_pnp_bid_bad(ids, i, n_samples)) *bad = 1;
}

int t_mode(int solver, int n, int* m) { return opp_pnp_mode(solver, n, m); }

// the mode number opp_pnp_ransac_ex and pnp_batch_epnp_final_kernel hand to the final stage
int t_final_mode(int solver, int n) {
  int m;
  return opp_pnp_final_mode(opp_pnp_mode(solver, n, &m));
}

// the layout as 9 numbers: the 5 array offsets, the 2 strides, the total, and what opp_pnp_layout returns
void t_pnp_layout(int iterations, int n_samples, int n_total, unsigned long long* out) {
  OppPnpLayout L;
  const size_t bytes = opp_pnp_layout(iterations, n_samples, n_total, &L);
  const size_t v[9] = {L.hyp, L.valid, L.score, L.score2, L.pts, L.hyp_stride, L.int_stride, L.bytes, bytes};
  for (int k = 0; k < 9; ++k) out[k] = v[k];
}

void t_extent(int o0, int o1, int n_total, int* first, int* n) { opp_pnp_extent(o0, o1, n_total, first, n); }
}
