// The argument checks of the five PnP entry points (pnp.hip, pnp_batch.hip, pnp_lo.hip, pnp_lo_batch.hip), written once.  `what`
// is the entry's prefix in the messages.  Host only.
#pragma once
#include "opp_common.h"

// what every entry checks.  No matches at all (an empty tensor has no address) is allowed: it is the entry's failure result.
// others_ok: the entry's conditions on the parameters it alone has (scale; min_trials and min_inlier_ratio)
static inline int opp_pnp_check_args(const char* what, const float* pts2d, const float* pts3d, int n, const double* K4, const double* pose_out,
                                     const int* inlier_mask, const int* n_inliers, const int* ok, const void* ws, int iterations,
                                     double reproj_error_px, bool others_ok, double confidence) {
  OPP_CHECK_ARG((n == 0 || (pts2d && pts3d)) && n >= 0 && K4 && pose_out && inlier_mask && n_inliers && ok && ws, "%s: null argument", what);
  OPP_CHECK_ARG(iterations > 0 && iterations <= (1 << 20) && reproj_error_px > 0 && others_ok, "%s: bad parameters", what);
  OPP_CHECK_ARG(confidence > 0.0, "%s: confidence must be > 0 (>= 1: no early stop)", what);
  return OPP_OK;
}

// what the two batch entries add: the number of samples and the per-sample arrays
static inline int opp_pnp_check_batch(const char* what, int n_samples, const int* offsets, const unsigned* seeds, const int* stop) {
  OPP_CHECK_ARG(offsets && seeds && stop, "%s: null argument", what);
  OPP_CHECK_ARG(n_samples >= 1 && n_samples <= 1024, "%s: n_samples must be in [1, 1024]", what);
  return OPP_OK;
}

static inline int opp_pnp_check_solver(const char* what, int solver) {
  OPP_CHECK_ARG(solver == 0 || solver == 1, "%s: solver must be 0 (P3P) or 1 (EPnP)", what);
  return OPP_OK;
}
