// The counter-based hash sampler and the parameter block of the PnP-RANSAC kernels (pnp.hip, pnp_lo.hip).
#pragma once

namespace {

__device__ __forceinline__ unsigned hash32(unsigned x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

struct PnpParams {
  double K4[4];   // fx, fy, cx, cy
  double thr2;    // squared reprojection threshold (px^2)
  double scale;   // world-point scale (reference: configs["point_cloud_rescale"])
  int n, iters;
  unsigned seed;
};

// the sampling of pnp_hypotheses_kernel, drawing K distinct indices
template <int K>
__device__ __forceinline__ void draw_sample(unsigned seed, int h, int n, int* idx) {
  unsigned s = hash32(seed ^ (0x9e3779b9u * (unsigned)(h + 1)));
#pragma unroll
  for (int k = 0; k < K; ++k) {
    for (int tries = 0; tries < 64; ++tries) {
      s = hash32(s + 0x632be5abu);
      const int c = (int)(s % (unsigned)n);
      bool dup = false;
#pragma unroll
      for (int j = 0; j < k; ++j) dup |= idx[j] == c;
      idx[k] = c;
      if (!dup) break;
    }
  }
}

}  // namespace
