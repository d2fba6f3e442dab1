// Pose-error metrics on the GPU: the scoring half of the reference's `compute_query_pose_errors`
// (src/utils/metric_utils.py:207-292) for B poses of one model in one enqueue --
//   query_pose_error   (:91-118)  rotation error in degrees, translation error in cm
//   add_metric         (:55-87)   ADD  = mean_i |(Rp v_i + tp) - (Rg v_i + tg)|
//                                 ADD-S = mean_i min_j |(Rg v_i + tg) - (Rp v_j + tp)|   (cKDTree(model_pred).query(model_target))
//   projection_2d_error (:31-53)  mean_i |pi(K, Rp, tp, v_i) - pi(K, Rg, tg, v_i)|, pi divides by z without a guard
// Everything is fp64 on the vector ALU, as the reference's numpy is (fp32 vertices times fp64 poses promote to fp64); the vertices
// convert to double exactly on load.  At most three launches, no host synchronisation, no atomics, every sum in a fixed order:
//
//   (a) point sweep   grid (P / 256, B): one thread per vertex computes its ADD distance and its 2D distance; the block sums of both
//                     (LDS tree) go to the workspace
//   (b) ADD-S sweep   grid (P / 256 target tiles, P / 1024 predicted chunks, B), only when a `syn` array is given: the block transforms
//                     its <= 1024 predicted points into LDS as doubles (24 KB), every thread keeps one transformed target point in
//                     registers and walks the chunk through same-address (broadcast) LDS reads; the minimum of the squared distance per
//                     (pose, chunk, target) goes to the workspace.  Blocks of a pose with syn = 0 or valid = 0 return at once
//   (c) finalise      one workgroup per pose: minimum over the chunks in chunk order, sqrt, tree sum, the means, the 3x3 and
//                     translation metrics, the 4 outputs.  A pose with valid = 0 gets +inf four times and no point work
//
// Tails (P % 256, P % 1024, P < 64) are index guards.  No kernel uses private-segment memory: the poses live in registers through
// constant indices only.
#include "opp_common.h"
#include <math.h>
#include "../../include/opp_hip.h"

namespace {

constexpr int kTile = 256;      // threads per workgroup = vertices per tile
constexpr int kChunk = 1024;    // predicted points of one ADD-S block (3 doubles each in LDS)
constexpr int kMaxPoints = 1 << 24;
constexpr int kMaxPoses = 65535;

struct Rt {
  double r[9], t[3];
};

__device__ __forceinline__ Rt load_pose(const double* p) {   // [12] row-major 3x4 R | t
  Rt o;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) o.r[3 * i + j] = p[4 * i + j];
    o.t[i] = p[4 * i + 3];
  }
  return o;
}

__device__ __forceinline__ void transform(const Rt& P, double x, double y, double z, double& ox, double& oy, double& oz) {
  ox = P.r[0] * x + P.r[1] * y + P.r[2] * z + P.t[0];
  oy = P.r[3] * x + P.r[4] * y + P.r[5] * z + P.t[1];
  oz = P.r[6] * x + P.r[7] * y + P.r[8] * z + P.t[2];
}

// sum of one value per thread of a 256-thread workgroup in a fixed order; the total is returned to every thread
__device__ __forceinline__ double block_sum(double v, double* red, int tid) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = kTile / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ bool flag(const unsigned char* a, int b, bool dflt) { return a ? a[b] != 0 : dflt; }

__global__ __launch_bounds__(kTile) void pose_metrics_points_kernel(const float* __restrict__ pts, int P, const double* __restrict__ pose_pred,
                                                                    const double* __restrict__ pose_gt, const double* __restrict__ Kmat,
                                                                    const unsigned char* __restrict__ valid, double* __restrict__ part_add,
                                                                    double* __restrict__ part_2d) {
  __shared__ double red[kTile];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (!flag(valid, b, true)) return;
  const Rt Pp = load_pose(pose_pred + 12 * (size_t)b), Pg = load_pose(pose_gt + 12 * (size_t)b);
  const int i = blockIdx.x * kTile + tid;
  double d_add = 0.0, d_2d = 0.0;
  if (i < P) {
    const double x = (double)pts[3 * (size_t)i], y = (double)pts[3 * (size_t)i + 1], z = (double)pts[3 * (size_t)i + 2];
    double px, py, pz, gx, gy, gz;
    transform(Pp, x, y, z, px, py, pz);
    transform(Pg, x, y, z, gx, gy, gz);
    const double ax = px - gx, ay = py - gy, az = pz - gz;
    d_add = sqrt(ax * ax + ay * ay + az * az);
    if (Kmat) {
      const double* k = Kmat + 9 * (size_t)b;
      const double k0 = k[0], k1 = k[1], k2 = k[2], k3 = k[3], k4 = k[4], k5 = k[5], k6 = k[6], k7 = k[7], k8 = k[8];
      const double pw = k6 * px + k7 * py + k8 * pz, gw = k6 * gx + k7 * gy + k8 * gz;
      const double du = (k0 * px + k1 * py + k2 * pz) / pw - (k0 * gx + k1 * gy + k2 * gz) / gw;
      const double dv = (k3 * px + k4 * py + k5 * pz) / pw - (k3 * gx + k4 * gy + k5 * gz) / gw;
      d_2d = sqrt(du * du + dv * dv);
    }
  }
  const size_t slot = (size_t)b * gridDim.x + blockIdx.x;
  const double s_add = block_sum(d_add, red, tid);
  if (tid == 0) part_add[slot] = s_add;
  if (Kmat) {
    const double s_2d = block_sum(d_2d, red, tid);
    if (tid == 0) part_2d[slot] = s_2d;
  }
}

__global__ __launch_bounds__(kTile) void pose_metrics_adds_kernel(const float* __restrict__ pts, int P, const double* __restrict__ pose_pred,
                                                                  const double* __restrict__ pose_gt, const unsigned char* __restrict__ syn,
                                                                  const unsigned char* __restrict__ valid, double* __restrict__ mins) {
  __shared__ double pred[3 * kChunk];
  const int b = blockIdx.z, chunk = blockIdx.y, tid = threadIdx.x;
  if (!flag(syn, b, false) || !flag(valid, b, true)) return;
  const int j0 = chunk * kChunk;
  const int nc = (P - j0) < kChunk ? (P - j0) : kChunk;
  {
    const Rt Pp = load_pose(pose_pred + 12 * (size_t)b);
    for (int j = tid; j < nc; j += kTile) {
      const size_t g = 3 * (size_t)(j0 + j);
      double ox, oy, oz;
      transform(Pp, (double)pts[g], (double)pts[g + 1], (double)pts[g + 2], ox, oy, oz);
      pred[3 * j] = ox;
      pred[3 * j + 1] = oy;
      pred[3 * j + 2] = oz;
    }
  }
  const int i = blockIdx.x * kTile + tid;
  const int ic = i < P ? i : P - 1;        // a tail thread walks the chunk on the last vertex and writes nothing
  double gx, gy, gz;
  {
    const Rt Pg = load_pose(pose_gt + 12 * (size_t)b);
    const size_t g = 3 * (size_t)ic;
    transform(Pg, (double)pts[g], (double)pts[g + 1], (double)pts[g + 2], gx, gy, gz);
  }
  __syncthreads();
  double best = INFINITY;
#pragma unroll 8
  for (int j = 0; j < nc; ++j) {
    const double dx = gx - pred[3 * j], dy = gy - pred[3 * j + 1], dz = gz - pred[3 * j + 2];
    const double d = dx * dx + dy * dy + dz * dz;
    best = d < best ? d : best;     // a NaN distance (non-finite pose) is skipped; numpy's min / cKDTree would propagate it
  }
  if (i < P) mins[((size_t)b * gridDim.y + chunk) * (size_t)P + i] = best;
}

__global__ __launch_bounds__(kTile) void pose_metrics_final_kernel(int P, int tiles, int chunks, const double* __restrict__ pose_pred,
                                                                   const double* __restrict__ pose_gt, int have_K,
                                                                   const unsigned char* __restrict__ syn, const unsigned char* __restrict__ valid,
                                                                   double t_to_cm, const double* __restrict__ part_add,
                                                                   const double* __restrict__ part_2d, const double* __restrict__ mins,
                                                                   double* __restrict__ out) {
  __shared__ double red[kTile];
  const int b = blockIdx.x, tid = threadIdx.x;
  double* o = out + 4 * (size_t)b;
  if (!flag(valid, b, true)) {
    if (tid < 4) o[tid] = INFINITY;
    return;
  }
  double acc = 0.0;
  if (flag(syn, b, false)) {
    for (int i = tid; i < P; i += kTile) {
      const double* m = mins + (size_t)b * chunks * (size_t)P + i;
      double best = m[0];
      for (int c = 1; c < chunks; ++c) {
        const double v = m[(size_t)c * P];
        best = v < best ? v : best;
      }
      acc += sqrt(best);
    }
  } else {
    for (int t = tid; t < tiles; t += kTile) acc += part_add[(size_t)b * tiles + t];
  }
  const double sum_dist = block_sum(acc, red, tid);
  double sum_2d = 0.0;
  if (have_K) {
    acc = 0.0;
    for (int t = tid; t < tiles; t += kTile) acc += part_2d[(size_t)b * tiles + t];
    sum_2d = block_sum(acc, red, tid);
  }
  if (tid == 0) {
    const Rt Pp = load_pose(pose_pred + 12 * (size_t)b), Pg = load_pose(pose_gt + 12 * (size_t)b);
    double tr = 0.0;       // trace(Rp Rg^T), row by row as the matrix product forms its diagonal
#pragma unroll
    for (int r = 0; r < 3; ++r) tr += Pp.r[3 * r] * Pg.r[3 * r] + Pp.r[3 * r + 1] * Pg.r[3 * r + 1] + Pp.r[3 * r + 2] * Pg.r[3 * r + 2];
    tr = tr <= 3.0 ? tr : 3.0;       // the reference's only clamp (:116); below -1 acos gives NaN there too
    const double dx = Pp.t[0] - Pg.t[0], dy = Pp.t[1] - Pg.t[1], dz = Pp.t[2] - Pg.t[2];
    const double qnan = __builtin_nan("");
    o[0] = acos((tr - 1.0) / 2.0) * (180.0 / 3.14159265358979323846);
    o[1] = sqrt(dx * dx + dy * dy + dz * dz) * t_to_cm;
    o[2] = P > 0 ? sum_dist / (double)P : qnan;
    o[3] = (P > 0 && have_K) ? sum_2d / (double)P : qnan;
  }
}

struct Layout {
  int tiles, chunks;
  size_t part_add, part_2d, mins, total;   // byte offsets
};

Layout layout(int n_poses, int n_points) {
  Layout l;
  const size_t B = (size_t)(n_poses < 1 ? 1 : n_poses), P = (size_t)(n_points < 0 ? 0 : n_points);
  l.tiles = (int)((P + kTile - 1) / kTile);
  l.chunks = (int)((P + kChunk - 1) / kChunk);
  size_t off = 0;
  l.part_add = off;
  off += opp_align(B * (size_t)(l.tiles < 1 ? 1 : l.tiles) * sizeof(double));
  l.part_2d = off;
  off += opp_align(B * (size_t)(l.tiles < 1 ? 1 : l.tiles) * sizeof(double));
  l.mins = off;
  // reserved whether or not a `syn` array is given (the size query has no such argument): B * chunks * P doubles, about
  // 25 MB at P = 20000, B = 8; never written or read without `syn`
  off += opp_align(B * (size_t)l.chunks * P * sizeof(double));
  l.total = off;
  return l;
}

}  // namespace

extern "C" size_t opp_pose_metrics_workspace_bytes(int n_poses, int n_points) { return layout(n_poses, n_points).total; }

extern "C" int opp_pose_metrics(const float* model_pts, int n_points, const double* pose_pred, const double* pose_gt, const double* K,
                                const unsigned char* syn, const unsigned char* valid, int n_poses, double t_to_cm, double* out, void* ws,
                                size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OPP_CHECK_ARG(n_poses >= 0 && n_poses <= kMaxPoses, "pose_metrics: n_poses must be in [0, %d], got %d", kMaxPoses, n_poses);
  OPP_CHECK_ARG(n_points >= 0 && n_points <= kMaxPoints, "pose_metrics: n_points must be in [0, %d], got %d", kMaxPoints, n_points);
  if (n_poses == 0) return OPP_OK;
  OPP_CHECK_ARG(pose_pred && pose_gt && out && ws && (n_points == 0 || model_pts), "pose_metrics: null argument");
  const Layout l = layout(n_poses, n_points);
  if (ws_bytes < l.total) {
    opp_set_error("pose_metrics: workspace too small (%zu bytes given, %zu needed for %d poses of %d points)", ws_bytes, l.total, n_poses,
                  n_points);
    return OPP_ERR_WORKSPACE;
  }
  double* part_add = (double*)((char*)ws + l.part_add);
  double* part_2d = (double*)((char*)ws + l.part_2d);
  double* mins = (double*)((char*)ws + l.mins);
  if (n_points > 0) {
    hipLaunchKernelGGL(pose_metrics_points_kernel, dim3(l.tiles, n_poses), dim3(kTile), 0, stream, model_pts, n_points, pose_pred, pose_gt, K,
                       valid, part_add, part_2d);
    if (syn)
      hipLaunchKernelGGL(pose_metrics_adds_kernel, dim3(l.tiles, l.chunks, n_poses), dim3(kTile), 0, stream, model_pts, n_points, pose_pred,
                         pose_gt, syn, valid, mins);
  }
  hipLaunchKernelGGL(pose_metrics_final_kernel, dim3(n_poses), dim3(kTile), 0, stream, n_points, l.tiles, l.chunks, pose_pred, pose_gt,
                     K ? 1 : 0, syn, valid, t_to_cm, part_add, part_2d, mins, out);
  OPP_CHECK_LAUNCH("pose_metrics kernels");
  return OPP_OK;
}
