// SfM point-cloud post-processing between COLMAP's points3D and the descriptor bank:
// the box mask of filter_bbox and the close-point merge of filter_points.merge, float64 end to end.
//
// Reference: src/sfm_utils/postprocess/filter_points.py  filter_bbox :172-234 (inner filter_), merge :265-297
//   merge builds squareform(pdist(xyzs)) -- a dense float64 n x n matrix -- and walks its rows in Python.  Here the same
//   clusters come from a tiled all-pairs search that keeps only the pairs below the threshold (CSR), a deterministic
//   selection over that list, and a per-cluster emit; nothing of size n x n is allocated.
//
// This file is compiled with -ffp-contract=off (build.SOURCE_FLAGS): the squared distance ((dx dx + dy dy) + dz dz) and the box
// dot products round after every operation, like the float64 numpy restatement they are tested against bit for bit.
//
// The distance test.  The reference decides sqrt(d2) < thr.  IEEE sqrt is correctly rounded and therefore monotone, so there is
// one double t2 with  sqrt(d2) < thr  <=>  d2 < t2: the smallest double whose square root is >= thr.  The host finds it (a few
// nextafter steps around thr * thr); the kernels compare d2 against it and never take a square root.
#include <cmath>

#include "../../include/opp_hip.h"
#include "opp_internal.h"

namespace {

constexpr int PC_MAX_POINTS = 1 << 20;
constexpr int PC_ROWS = 64;          // rows per workgroup of the pair search: one wave, a lane per row
constexpr int PC_TILE = 256;         // columns staged in LDS per sweep step (3 x 2 KB)
constexpr int PC_SELECT_THREADS = 1024;
enum : unsigned char { PC_UNDECIDED = 0, PC_SELECTED = 1, PC_REJECTED = 2 };

struct PcBox {
  double o[3];        // corner 4
  double v[3][3];     // v45, v40, v47
  double vv[3];       // v . v
};

__global__ __launch_bounds__(256) void pc_box_mask_kernel(const double* __restrict__ xyz, int n, PcBox b, unsigned char* __restrict__ mask) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double px = xyz[3 * (size_t)i] - b.o[0], py = xyz[3 * (size_t)i + 1] - b.o[1], pz = xyz[3 * (size_t)i + 2] - b.o[2];
  bool in = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double m = (px * b.v[a][0] + py * b.v[a][1]) + pz * b.v[a][2];
    in = in && (0.0 < m) && (m < b.vv[a]);          // strict on both faces; a NaN fails both
  }
  mask[i] = in ? 1 : 0;
}

// One lane per row j, the columns swept in ascending index through an LDS tile every lane reads at the same address (broadcast).
// FILL = false: counts[j] = |N(j)|.  FILL = true: the same sweep writes the column indices of row j to nbr[offsets[j] ...]; a lane
// writes its own row only and in sweep order, so the list is ascending and does not depend on scheduling (no claimed slots).
template <bool FILL>
__global__ __launch_bounds__(PC_ROWS) void pc_neighbor_kernel(const double* __restrict__ xyz, int n, double t2, int* __restrict__ counts,
                                                              const long long* __restrict__ offsets, long long pairs,
                                                              int* __restrict__ nbr) {
  __shared__ double sx[PC_TILE], sy[PC_TILE], sz[PC_TILE];
  const int row = blockIdx.x * PC_ROWS + threadIdx.x;
  const bool live = row < n;
  const size_t r = live ? row : n - 1;
  const double x = xyz[3 * r], y = xyz[3 * r + 1], z = xyz[3 * r + 2];
  long long pos = 0, end = 0;
  if (FILL && live) {
    pos = offsets[row];
    end = offsets[row + 1];
    if (end > pairs) end = pairs;
  }
  int cnt = 0;
  for (int c0 = 0; c0 < n; c0 += PC_TILE) {
    __syncthreads();
    for (int t = threadIdx.x; t < PC_TILE; t += PC_ROWS) {
      const int c = c0 + t;
      if (c < n) {
        sx[t] = xyz[3 * (size_t)c];
        sy[t] = xyz[3 * (size_t)c + 1];
        sz[t] = xyz[3 * (size_t)c + 2];
      }
    }
    __syncthreads();
    const int m = n - c0 < PC_TILE ? n - c0 : PC_TILE;
    for (int t = 0; t < m; ++t) {
      const double dx = x - sx[t], dy = y - sy[t], dz = z - sz[t];
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      if (d2 < t2) {
        if (FILL) {
          if (pos >= 0 && pos < end) nbr[pos] = c0 + t;
          ++pos;
        } else {
          ++cnt;
        }
      }
    }
  }
  if (!FILL && live) counts[row] = cnt;
}

// The reference walks j = 0 .. n-1 and takes row j iff no member of N(j) is in N(i) of an earlier taken i, i.e. iff no earlier
// taken i has N(i) and N(j) in common: the lexicographically first independent set of that conflict relation.  Rounds: an
// undecided j looks at every i < j in N(m), m in N(j) (N is symmetric, so these are exactly the earlier rows in conflict with j) --
// any selected -> rejected; all rejected (or none) -> selected; else it waits.  Every decision is the sequential walk's decision,
// whatever the round it is taken in, and the lowest undecided index decides in every round, so n rounds bound the loop.
// ONE workgroup: the rounds are separated by __syncthreads(), there is no barrier across workgroups.  A round reads `cur` and
// writes every entry of `nxt`, so no thread reads a byte another one writes in the same round.
__global__ __launch_bounds__(PC_SELECT_THREADS) void pc_select_kernel(const long long* __restrict__ offsets, const int* __restrict__ nbr, int n,
                                                                       unsigned char* state_a, unsigned char* state_b, int* __restrict__ sel,
                                                                       int* __restrict__ selcnt, int* __restrict__ status) {
  unsigned char* cur = state_a;
  unsigned char* nxt = state_b;
  for (int j = threadIdx.x; j < n; j += PC_SELECT_THREADS) cur[j] = PC_UNDECIDED;
  __syncthreads();
  int left = 1;
  for (int round = 0; round < n && left; ++round) {       // hard trip bound: n rounds
    int mine = 0;
    for (int j = threadIdx.x; j < n; j += PC_SELECT_THREADS) {
      unsigned char s = cur[j];
      if (s == PC_UNDECIDED) {
        bool any_sel = false, any_und = false;
        const long long a1 = offsets[j + 1];
        for (long long a = offsets[j]; a < a1 && !any_sel; ++a) {
          const int m = nbr[a];
          if ((unsigned)m >= (unsigned)n) continue;
          const long long b1 = offsets[m + 1];
          for (long long b = offsets[m]; b < b1; ++b) {
            const int i = nbr[b];
            if (i >= j || i < 0) break;                    // ascending lists: nothing earlier than j follows
            const unsigned char si = cur[i];
            if (si == PC_SELECTED) {
              any_sel = true;
              break;
            }
            any_und = any_und || si == PC_UNDECIDED;
          }
        }
        s = any_sel ? PC_REJECTED : (any_und ? PC_UNDECIDED : PC_SELECTED);
        mine |= s == PC_UNDECIDED;
      }
      nxt[j] = s;
    }
    left = __syncthreads_or(mine);
    unsigned char* t = cur;
    cur = nxt;
    nxt = t;
  }
  for (int j = threadIdx.x; j < n; j += PC_SELECT_THREADS) {
    const bool taken = cur[j] == PC_SELECTED;
    sel[j] = taken ? 1 : 0;
    selcnt[j] = taken ? (int)(offsets[j + 1] - offsets[j]) : 0;
  }
  if (threadIdx.x == 0) *status = left ? 1 : 0;           // 1: the bound was hit with rows still undecided
}

// rank / mem_end: inclusive prefix sums of sel / selcnt.  Selected row j is cluster rank[j] - 1 (ascending j) and owns the member
// span that ends at mem_end[j].  Mean: the members' coordinates added one after the other in ascending position, one division --
// numpy's axis-0 mean of xyzs[mask].
__global__ __launch_bounds__(256) void pc_emit_kernel(const double* __restrict__ xyz, const long long* __restrict__ ids, int n,
                                                       const long long* __restrict__ offsets, const int* __restrict__ nbr,
                                                       const int* __restrict__ sel, const long long* __restrict__ rank,
                                                       const long long* __restrict__ mem_end, long long n_clusters, long long n_members,
                                                       double* __restrict__ ret_points, long long* __restrict__ cl_offsets,
                                                       long long* __restrict__ members) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n || !sel[j]) return;
  const long long c = rank[j] - 1, e = mem_end[j];
  const long long a0 = offsets[j], k = offsets[j + 1] - a0;
  if (c < 0 || c >= n_clusters || k <= 0 || e - k < 0 || e > n_members) return;
  cl_offsets[c] = e - k;
  if (c == n_clusters - 1) cl_offsets[n_clusters] = e;
  const int i0 = nbr[a0];
  if ((unsigned)i0 >= (unsigned)n) return;
  double sx = xyz[3 * (size_t)i0], sy = xyz[3 * (size_t)i0 + 1], sz = xyz[3 * (size_t)i0 + 2];
  members[e - k] = ids[i0];
  for (long long t = 1; t < k; ++t) {
    const int i = nbr[a0 + t];
    if ((unsigned)i >= (unsigned)n) return;
    sx += xyz[3 * (size_t)i];
    sy += xyz[3 * (size_t)i + 1];
    sz += xyz[3 * (size_t)i + 2];
    members[e - k + t] = ids[i];
  }
  const double kd = (double)k;
  ret_points[3 * c] = sx / kd;
  ret_points[3 * c + 1] = sy / kd;
  ret_points[3 * c + 2] = sz / kd;
}

size_t pc_align(size_t b) { return (b + 255) / 256 * 256; }

// workspace: neighbour lists [pairs] int32 | state a [n] | state b [n]
struct PcWorkspace {
  int* nbr;
  unsigned char* state_a;
  unsigned char* state_b;
};

int pc_workspace(int n, long long pairs, void* ws, size_t ws_bytes, PcWorkspace* out) {
  OPP_CHECK_ARG(n > 0 && n <= PC_MAX_POINTS, "pointcloud: n = %d outside 1 .. 2^20", n);
  OPP_CHECK_ARG(pairs >= n && pairs <= (long long)n * n, "pointcloud: %lld pairs for %d points (every point is its own neighbour)", pairs, n);
  if (!ws || ws_bytes < opp_pc_workspace_bytes(n, pairs)) {
    opp_set_error("pointcloud: workspace of %zu bytes, %zu needed", ws_bytes, opp_pc_workspace_bytes(n, pairs));
    return OPP_ERR_WORKSPACE;
  }
  char* p = (char*)ws;
  out->nbr = (int*)p;
  p += pc_align((size_t)pairs * sizeof(int));
  out->state_a = (unsigned char*)p;
  p += pc_align((size_t)n);
  out->state_b = (unsigned char*)p;
  return OPP_OK;
}

// smallest double t2 with sqrt(t2) >= thr, so that  sqrt(d2) < thr  <=>  d2 < t2
int pc_threshold(double thr, double* t2_out) {
  OPP_CHECK_ARG(std::isfinite(thr) && thr > 0.0, "pointcloud: the distance threshold must be finite and positive");
  OPP_CHECK_ARG(thr >= 1e-150 && thr <= 1e150, "pointcloud: distance threshold %g outside 1e-150 .. 1e150", thr);
  double t2 = thr * thr;
  int steps = 0;
  while (std::sqrt(t2) >= thr && steps++ < 16) t2 = std::nextafter(t2, 0.0);
  while (std::sqrt(t2) < thr && steps++ < 32) t2 = std::nextafter(t2, HUGE_VAL);
  OPP_CHECK_ARG(std::sqrt(t2) >= thr && std::sqrt(std::nextafter(t2, 0.0)) < thr, "pointcloud: no squared bound found for threshold %g", thr);
  *t2_out = t2;
  return OPP_OK;
}

}  // namespace

extern "C" size_t opp_pc_workspace_bytes(int n, long long pairs) {
  if (n <= 0 || n > PC_MAX_POINTS || pairs < 0 || pairs > (long long)n * n) return 0;
  return pc_align((size_t)pairs * sizeof(int)) + 2 * pc_align((size_t)n);
}

extern "C" int opp_pc_box_mask(const double* xyz, int n, const double* corners, unsigned char* mask, void* stream) {
  OPP_CHECK_ARG(n >= 0 && n <= PC_MAX_POINTS, "pc_box_mask: n = %d outside 0 .. 2^20", n);
  OPP_CHECK_ARG(corners, "pc_box_mask: corners missing");
  for (int i = 0; i < 24; ++i) OPP_CHECK_ARG(std::isfinite(corners[i]), "pc_box_mask: box corner %d is not finite", i / 3);
  if (n == 0) return OPP_OK;
  OPP_CHECK_ARG(xyz && mask, "pc_box_mask: bad argument");
  PcBox b;
  const int other[3] = {5, 0, 7};
  for (int a = 0; a < 3; ++a) {
    b.o[a] = corners[3 * 4 + a];
    for (int d = 0; d < 3; ++d) b.v[a][d] = corners[3 * other[a] + d] - corners[3 * 4 + d];
    b.vv[a] = (b.v[a][0] * b.v[a][0] + b.v[a][1] * b.v[a][1]) + b.v[a][2] * b.v[a][2];
  }
  hipLaunchKernelGGL(pc_box_mask_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, xyz, n, b, mask);
  OPP_CHECK_LAUNCH("pc_box_mask_kernel");
  return OPP_OK;
}

extern "C" int opp_pc_neighbor_count(const double* xyz, int n, double thr, int* counts, void* stream) {
  OPP_CHECK_ARG(n > 0 && n <= PC_MAX_POINTS, "pc_neighbor_count: n = %d outside 1 .. 2^20", n);
  OPP_CHECK_ARG(xyz && counts, "pc_neighbor_count: bad argument");
  double t2;
  OPP_TRY(pc_threshold(thr, &t2));
  hipLaunchKernelGGL(pc_neighbor_kernel<false>, dim3((n + PC_ROWS - 1) / PC_ROWS), dim3(PC_ROWS), 0, (hipStream_t)stream, xyz, n, t2, counts,
                     (const long long*)nullptr, 0LL, (int*)nullptr);
  OPP_CHECK_LAUNCH("pc_neighbor_kernel<count>");
  return OPP_OK;
}

extern "C" int opp_pc_neighbor_fill(const double* xyz, int n, double thr, const long long* offsets, long long pairs, void* ws, size_t ws_bytes,
                                    void* stream) {
  OPP_CHECK_ARG(xyz && offsets, "pc_neighbor_fill: bad argument");
  double t2;
  OPP_TRY(pc_threshold(thr, &t2));
  PcWorkspace w;
  OPP_TRY(pc_workspace(n, pairs, ws, ws_bytes, &w));
  hipLaunchKernelGGL(pc_neighbor_kernel<true>, dim3((n + PC_ROWS - 1) / PC_ROWS), dim3(PC_ROWS), 0, (hipStream_t)stream, xyz, n, t2, (int*)nullptr,
                     offsets, pairs, w.nbr);
  OPP_CHECK_LAUNCH("pc_neighbor_kernel<fill>");
  return OPP_OK;
}

extern "C" int opp_pc_select(const long long* offsets, int n, long long pairs, int* sel, int* selcnt, int* status, void* ws, size_t ws_bytes,
                             void* stream) {
  OPP_CHECK_ARG(offsets && sel && selcnt && status, "pc_select: bad argument");
  PcWorkspace w;
  OPP_TRY(pc_workspace(n, pairs, ws, ws_bytes, &w));
  hipLaunchKernelGGL(pc_select_kernel, dim3(1), dim3(PC_SELECT_THREADS), 0, (hipStream_t)stream, offsets, w.nbr, n, w.state_a, w.state_b, sel,
                     selcnt, status);
  OPP_CHECK_LAUNCH("pc_select_kernel");
  return OPP_OK;
}

extern "C" int opp_pc_emit(const double* xyz, const long long* ids, int n, long long pairs, const long long* offsets, const int* sel,
                           const long long* rank, const long long* mem_end, long long n_clusters, long long n_members, double* ret_points,
                           long long* cl_offsets, long long* members, void* ws, size_t ws_bytes, void* stream) {
  OPP_CHECK_ARG(xyz && ids && offsets && sel && rank && mem_end && ret_points && cl_offsets && members, "pc_emit: bad argument");
  OPP_CHECK_ARG(n_clusters >= 1 && n_clusters <= n && n_members >= n_clusters && n_members <= pairs, "pc_emit: %lld clusters with %lld members",
                n_clusters, n_members);
  PcWorkspace w;
  OPP_TRY(pc_workspace(n, pairs, ws, ws_bytes, &w));
  hipLaunchKernelGGL(pc_emit_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, xyz, ids, n, offsets, w.nbr, sel, rank, mem_end,
                     n_clusters, n_members, ret_points, cl_offsets, members);
  OPP_CHECK_LAUNCH("pc_emit_kernel");
  return OPP_OK;
}
