// A training sample's per-sample tensors, made on the device from the small annotation arrays: what the training branch of
// OnePosePlusDataset.read_anno (src/datasets/OnePosePlus_dataset.py:341-437) does on the host before build_assignmatrix.
//
//   homography_warp_kernel   kornia 0.4.1 `homography_warp` of a batch of fp32 images (restated; kornia is not pinned here):
//                            destination grid linspace(-1, 1, w) x linspace(-1, 1, h) -> transform_points (scale 1 / z where
//                            |z| > 1e-8, else 1) -> F.grid_sample(bilinear, zeros, align_corners).  The coordinate chain runs in
//                            double and is rounded to fp32 once, at the source pixel position: with the identity matrix and
//                            align_corners the position of pixel j is then exactly j (a fp32 chain gives j - 1 ulp for some j
//                            and blends a neighbour in), so the image comes back bit for bit.  The four taps and their weights
//                            are fp32 as in grid_sample.  One thread per destination pixel, 1 MB in and 1 MB out per 512 x 512
//                            image: HBM-bound byte work, nothing to tune.
//   project_pairs_kernel     K (R X + t), x / (z + 1e-6), optionally the pixel-space homography with the division by its third
//                            row (:352-391), in double from the fp32 inputs, one fp32 rounding at the store.
//   select_pairs_kernel      the discrete half (:393-433), exact: out-of-bounds filter on the unrounded points (warped samples
//                            only), round(p / cell) * cell half-to-even in fp32, invalid filter on the rounded points, one survivor per
//                            rounded cell (smallest pair index: np.unique's return_index; -0.0 and 0.0 are one cell), survivors in
//                            np.unique(axis=0) order (x, then y), write-back into the per-2D-keypoint arrays with last-write-wins.
//                            One workgroup: a per-cell atomicMin table laid out [x][y], whose ordered compaction IS the
//                            lexicographic order, and a per-2D-keypoint atomicMax table for the write-back.
#include <limits.h>
#include <math.h>

#include "../../include/opp_hip.h"
#include "opp_common.h"

namespace {

__global__ __launch_bounds__(256) void homography_warp_kernel(const float* __restrict__ src, int h, int w, int stride, long long batch_stride,
                                                              const float* __restrict__ mats, int align_corners, float* __restrict__ dst) {
  const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
  const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int b = blockIdx.z;
  if (dx >= w || dy >= h) return;
  const float* __restrict__ m = mats + 9 * (size_t)b;
  // create_meshgrid(normalized_coordinates=True): -1 at pixel 0, +1 at pixel n - 1
  const double gx = (double)(2 * dx - (w - 1)) / (double)(w - 1), gy = (double)(2 * dy - (h - 1)) / (double)(h - 1);
  const double px = (double)m[0] * gx + (double)m[1] * gy + (double)m[2];
  const double py = (double)m[3] * gx + (double)m[4] * gy + (double)m[5];
  const double pz = (double)m[6] * gx + (double)m[7] * gy + (double)m[8];
  const double scale = fabs(pz) > 1e-8 ? 1.0 / pz : 1.0;        // convert_points_from_homogeneous
  const double sx = px * scale, sy = py * scale;
  // grid_sampler_unnormalize
  const float ix = (float)(align_corners ? (sx + 1.0) * 0.5 * (double)(w - 1) : ((sx + 1.0) * (double)w - 1.0) * 0.5);
  const float iy = (float)(align_corners ? (sy + 1.0) * 0.5 * (double)(h - 1) : ((sy + 1.0) * (double)h - 1.0) * 0.5);
  float out = 0.f;
  // every tap of a position outside (-1, n) is padding; the test also keeps NaN / inf away from the integer conversion
  if (ix > -1.f && ix < (float)w && iy > -1.f && iy < (float)h) {
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float tx = ix - fx0, ty = iy - fy0, ux = (fx0 + 1.f) - ix, uy = (fy0 + 1.f) - iy;
    const float* __restrict__ img = src + (size_t)b * (size_t)batch_stride;
    const bool xl = x0 >= 0, xr = x0 + 1 < w, yt = y0 >= 0, yb = y0 + 1 < h;
    const float nw = (xl && yt) ? img[(size_t)y0 * stride + x0] : 0.f;
    const float ne = (xr && yt) ? img[(size_t)y0 * stride + x0 + 1] : 0.f;
    const float sw = (xl && yb) ? img[(size_t)(y0 + 1) * stride + x0] : 0.f;
    const float se = (xr && yb) ? img[(size_t)(y0 + 1) * stride + x0 + 1] : 0.f;
    out = nw * (ux * uy) + ne * (tx * uy) + sw * (ux * ty) + se * (tx * ty);
  }
  dst[((size_t)b * h + dy) * w + dx] = out;
}

struct ProjMats {
  float Rt[12];
  float K[9];
  float H[9];
  int warp;
};

__global__ __launch_bounds__(256) void project_pairs_kernel(const float* __restrict__ kp3d, int n3d, const long long* __restrict__ assign, int k,
                                                            ProjMats mm, float* __restrict__ proj, int* __restrict__ status) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= k) return;
  long long i = assign[(size_t)k + t];
  if (i < 0) i += n3d;                                           // torch indexing wraps a negative index once
  float ox = nanf(""), oy = ox;
  if (i < 0 || i >= n3d) {
    if (status) atomicOr(status, 1);                             // keypoints3d[assign_matrix[1]] raises IndexError upstream
  } else {
    const double X = kp3d[3 * i], Y = kp3d[3 * i + 1], Z = kp3d[3 * i + 2];
    const float* R = mm.Rt;
    const double cx = (double)R[0] * X + (double)R[1] * Y + (double)R[2] * Z + (double)R[3];
    const double cy = (double)R[4] * X + (double)R[5] * Y + (double)R[6] * Z + (double)R[7];
    const double cz = (double)R[8] * X + (double)R[9] * Y + (double)R[10] * Z + (double)R[11];
    const float* K = mm.K;
    const double qx = (double)K[0] * cx + (double)K[1] * cy + (double)K[2] * cz;
    const double qy = (double)K[3] * cx + (double)K[4] * cy + (double)K[5] * cz;
    const double qz = (double)K[6] * cx + (double)K[7] * cy + (double)K[8] * cz;
    double u = qx / (qz + 1e-6), v = qy / (qz + 1e-6);           // (:354)
    if (mm.warp) {
      const float* H = mm.H;
      const double wx = (double)H[0] * u + (double)H[1] * v + (double)H[2];
      const double wy = (double)H[3] * u + (double)H[4] * v + (double)H[5];
      const double wz = (double)H[6] * u + (double)H[7] * v + (double)H[8];
      u = wx / wz;                                               // "NOTE: Important! [:, 2] is not all 1!"  (:388-390)
      v = wy / wz;
    }
    ox = (float)u;
    oy = (float)v;
  }
  proj[2 * (size_t)t] = ox;
  proj[2 * (size_t)t + 1] = oy;
}

constexpr int kSelThreads = 256;

// One workgroup.  cells [ncx][ncy] and owner [n2d] are global scratch, both written here before they are read.
__global__ __launch_bounds__(kSelThreads) void select_pairs_kernel(const float* __restrict__ proj, const long long* __restrict__ assign, int k, int h, int w,
                                                                   float cell, int ncx, int ncy, int warped, int n2d, int* __restrict__ cells,
                                                                   int* __restrict__ owner, long long* __restrict__ assign_out, int* __restrict__ n_out,
                                                                   float* __restrict__ kp_coarse, float* __restrict__ kp_fine, int* __restrict__ status) {
  __shared__ int counts[kSelThreads];
  __shared__ int offsets[kSelThreads + 1];
  const int tid = threadIdx.x;
  const int ncells = ncx * ncy;
  for (int c = tid; c < ncells; c += kSelThreads) cells[c] = INT_MAX;
  for (int q = tid; q < n2d; q += kSelThreads) owner[q] = -1;
  __syncthreads();
  const float xmax = (float)(w - 1), ymax = (float)(h - 1);
  // the two filters and the first occurrence of every rounded cell
  for (int t = tid; t < k; t += kSelThreads) {
    const float px = proj[2 * (size_t)t], py = proj[2 * (size_t)t + 1];
    if (!(fabsf(px) < INFINITY && fabsf(py) < INFINITY)) {       // NaN / inf pass upstream's comparisons and fail in build_assignmatrix
      if (status) atomicOr(status, 1);
      continue;
    }
    if (warped && (px < 0.f || px > xmax || py < 0.f || py > ymax)) continue;       // out_of_boundry_mask  (:393-400)
    const float rx = rintf(px / cell) * cell, ry = rintf(py / cell) * cell;          // (:411-415), half to even
    if (rx < 0.f || rx > xmax || ry < 0.f || ry > ymax) continue;                    // invalid  (:416-424)
    const int c = (int)(rx / cell) * ncy + (int)(ry / cell);                         // -0.0 lands in cell 0
    atomicMin(&cells[c], t);
  }
  __syncthreads();
  // ordered compaction of the occupied cells: x-major = np.unique(axis=0)'s lexicographic (x, y)
  const int per = (ncells + kSelThreads - 1) / kSelThreads;
  const int c0 = min(tid * per, ncells), c1 = min(c0 + per, ncells);
  int cnt = 0;
  for (int c = c0; c < c1; ++c) cnt += cells[c] != INT_MAX;
  counts[tid] = cnt;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < kSelThreads; ++i) {
      offsets[i] = run;
      run += counts[i];
    }
    offsets[kSelThreads] = run;
    *n_out = run;
  }
  __syncthreads();
  const int total = offsets[kSelThreads];
  int rank = offsets[tid];
  for (int c = c0; c < c1; ++c) {
    const int t = cells[c];
    if (t == INT_MAX) continue;
    long long q = assign[t];
    assign_out[rank] = q;
    assign_out[(size_t)k + rank] = assign[(size_t)k + t];
    if (q < 0) q += n2d;
    if (q < 0 || q >= n2d) {
      if (status) atomicOr(status, 1);                           // keypoints2d_coarse[assign_matrix[0]] = ... raises upstream
    } else {
      atomicMax(&owner[q], rank);                                // index_put on the CPU keeps the last of repeated indices
    }
    ++rank;
  }
  // columns past k' hold a pair that opp_build_assignmatrix drops without a status bit (3D index >= any shape3d)
  for (int r = total + tid; r < k; r += kSelThreads) {
    assign_out[r] = 0;
    assign_out[(size_t)k + r] = LLONG_MAX;
  }
  __syncthreads();
  rank = offsets[tid];
  for (int c = c0; c < c1; ++c) {
    const int t = cells[c];
    if (t == INT_MAX) continue;
    long long q = assign[t];
    if (q < 0) q += n2d;
    if (q >= 0 && q < n2d && owner[q] == rank) {
      const float px = proj[2 * (size_t)t], py = proj[2 * (size_t)t + 1];
      kp_coarse[2 * q] = rintf(px / cell) * cell;
      kp_coarse[2 * q + 1] = rintf(py / cell) * cell;
      kp_fine[2 * q] = px;
      kp_fine[2 * q + 1] = py;
    }
    ++rank;
  }
}

}  // namespace

extern "C" int opp_homography_warp(const float* src, int B, int h, int w, int src_stride, long long src_batch_stride, const float* src_homo_dst,
                                   int align_corners, float* dst, void* stream) {
  OPP_CHECK_ARG(src && src_homo_dst && dst, "homography_warp: null argument");
  OPP_CHECK_ARG(B > 0 && B <= 65535, "homography_warp: batch of %d images", B);
  OPP_CHECK_ARG(h >= 2 && w >= 2, "homography_warp: image %dx%d (the normalised grid needs at least 2 pixels a side)", h, w);
  OPP_CHECK_ARG(src_stride >= w && (B == 1 || src_batch_stride >= (long long)(h - 1) * src_stride + w), "homography_warp: source stride %d < width %d, or images overlap",
                src_stride, w);
  hipLaunchKernelGGL(homography_warp_kernel, dim3(opp_cdiv(w, 64), opp_cdiv(h, 4), B), dim3(256), 0, (hipStream_t)stream, src, h, w, src_stride,
                     src_batch_stride, src_homo_dst, align_corners ? 1 : 0, dst);
  OPP_CHECK_LAUNCH("homography_warp_kernel");
  return OPP_OK;
}

extern "C" int opp_project_pairs(const float* keypoints3d, int n3d, const long long* assign, int k, const float* pose_Rt, const float* K,
                                 const float* homography_px, float* mkpts_proj, int* status, void* stream) {
  OPP_CHECK_ARG(k >= 0 && n3d >= 0 && pose_Rt && K, "project_pairs: bad argument");
  if (k == 0) return OPP_OK;
  OPP_CHECK_ARG(keypoints3d && assign && mkpts_proj, "project_pairs: null pair data");
  ProjMats mm;
  for (int i = 0; i < 12; ++i) mm.Rt[i] = pose_Rt[i];
  for (int i = 0; i < 9; ++i) mm.K[i] = K[i];
  for (int i = 0; i < 9; ++i) mm.H[i] = homography_px ? homography_px[i] : 0.f;
  mm.warp = homography_px ? 1 : 0;
  hipLaunchKernelGGL(project_pairs_kernel, dim3(opp_cdiv(k, 256)), dim3(256), 0, (hipStream_t)stream, keypoints3d, n3d, assign, k, mm, mkpts_proj, status);
  OPP_CHECK_LAUNCH("project_pairs_kernel");
  return OPP_OK;
}

extern "C" int opp_select_pairs(const float* mkpts_proj, const long long* assign, int k, int h, int w, int cell, int warped, int n2d, float* kp2d_coarse,
                                float* kp2d_fine, long long* assign_out, int* n_out, int* scratch, int* status, void* stream) {
  OPP_CHECK_ARG(k >= 0 && n2d >= 0 && cell > 0 && h >= cell && w >= cell, "select_pairs: bad sizes (k %d, n2d %d, image %dx%d, cell %d)", k, n2d, h, w, cell);
  OPP_CHECK_ARG(h % cell == 0 && w % cell == 0, "select_pairs: image %dx%d is not a multiple of the coarse cell %d", h, w, cell);
  OPP_CHECK_ARG(n_out && scratch && (n2d == 0 || (kp2d_coarse && kp2d_fine)), "select_pairs: null argument");
  OPP_CHECK_ARG(k == 0 || (mkpts_proj && assign && assign_out), "select_pairs: null pair data");
  const int ncx = w / cell + 1, ncy = h / cell + 1;
  OPP_CHECK_ARG((long long)ncx * ncy + n2d < INT_MAX, "select_pairs: cell grid too large");
  hipLaunchKernelGGL(select_pairs_kernel, dim3(1), dim3(kSelThreads), 0, (hipStream_t)stream, mkpts_proj, assign, k, h, w, (float)cell, ncx, ncy,
                     warped ? 1 : 0, n2d, scratch, scratch + ncx * ncy, assign_out, n_out, kp2d_coarse, kp2d_fine, status);
  OPP_CHECK_LAUNCH("select_pairs_kernel");
  return OPP_OK;
}
