// Kernels of the 2D-2D matcher (LoFTR, onepose_plus_plus_amd/loftr.py) that the 2D-3D path has no counterpart for:
//   - the window gather of the fine level from TWO 1/2-resolution maps (FinePreprocess of LoFTR: F.unfold(kernel W, stride 4, padding W / 2)
//     of both maps, indexed by the coarse cells of the matches),
//   - LinearAttention of ONE stream of a segment against the K | V of a source stream of the same segment, for segments of up to 81 + 81
//     tokens at d_model 128 / 8 heads (the fine level at W = 9): KV and Ksum never leave the workgroup,
//   - the expectation head of fine.hip for windows of more than 64 cells.
// Reference: src/KeypointFreeSfM/loftr_for_sfm/loftr.py:16-128 (the LoFTR submodule it imports is absent: published LoFTR, parity unpinned);
// the attention arithmetic is loftr_module/linear_attention.py:29-61.
#include "opp_common.h"
#include "opp_internal.h"

namespace {

constexpr int kSegMaxLen = 81;    // tokens per stream and segment: W = 9
constexpr int kSegTile = 16;      // source rows staged per step

// win [2][M][WW][C]: stream 0 = windows of map 0 around i_ids, stream 1 = windows of map 1 around j_ids.  grid (M, 2).
__global__ __launch_bounds__(128) void window_gather2_kernel(const float* __restrict__ feat0, int Hf0, int Wf0, const float* __restrict__ feat1, int Hf1,
                                                             int Wf1, const long long* __restrict__ i_ids, const long long* __restrict__ j_ids, int M,
                                                             int w0c, int w1c, int stride, int Wwin, int C, float* __restrict__ win) {
  const int m = blockIdx.x, which = blockIdx.y;
  const float* feat = which ? feat1 : feat0;
  const int Hf = which ? Hf1 : Hf0, Wf = which ? Wf1 : Wf0, wc = which ? w1c : w0c;
  const int cell = (int)(which ? j_ids[m] : i_ids[m]);
  const int gy = cell / wc, gx = cell - gy * wc;
  const int cy = gy * stride - Wwin / 2, cx = gx * stride - Wwin / 2;
  const int WW = Wwin * Wwin, c4n = C >> 2;
  float* dst = win + ((size_t)which * M + m) * WW * C;
  for (int e = threadIdx.x; e < WW * c4n; e += blockDim.x) {
    const int r = e / c4n, c = (e - r * c4n) * 4;
    const int ky = r / Wwin, kx = r - ky * Wwin;
    const int y = cy + ky, x = cx + kx;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((unsigned)y < (unsigned)Hf && (unsigned)x < (unsigned)Wf) v = *reinterpret_cast<const float4*>(feat + ((size_t)y * Wf + x) * C + c);
    *reinterpret_cast<float4*>(dst + (size_t)r * C + c) = v;
  }
}

// One workgroup per segment.  q: phi(Q) rows of the QUERY stream's first token, k / v: phi(K) / V / S_src columns of the SOURCE stream's first
// token (row stride ld floats each; segment g starts len_q / len_src rows further).  out [n_seg * len_q][ldo]:
//   out[l][h * D + e] = (sum_d q[l][h D + d] KV[h][d][e]) / (sum_d q[l][h D + d] Ksum[h][d] + eps) * len_src,  KV[h][d][e] = sum_s k[s][h D + d] v[s][h D + e]
// (linear_attention.py:55-59), the source rows summed in ascending order: the same bits from run to run.
// LDS: one tile of K | V rows (16 KB); KV lives in registers of the thread that owns its column, Ksum goes through 512 B of LDS.
template <int D, int C>
__global__ __launch_bounds__(2 * C) void linattn_seg_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int ld,
                                                            int len_q, int len_src, float* __restrict__ out, int ldo, float eps) {
  static_assert(D == 16 && C == 128, "thread mapping below: 8 heads of 16, 256 threads");
  __shared__ float ksh[kSegTile][C];
  __shared__ float vsh[kSegTile][C];
  __shared__ float kv_sh[C * D];      // [h][d][e]
  __shared__ float ks_sh[C];
  const int tid = threadIdx.x, seg = blockIdx.x;
  const float* kseg = k + (size_t)seg * len_src * ld;
  const float* vseg = v + (size_t)seg * len_src * ld;
  // reduction: thread = (head h, row d of the head's D x D block, half of its columns)
  const int h = tid >> 5, d = (tid & 31) >> 1, e0 = (tid & 1) * 8;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  float ksum = 0.f;
  for (int s0 = 0; s0 < len_src; s0 += kSegTile) {
    const int rows = len_src - s0 < kSegTile ? len_src - s0 : kSegTile;
    __syncthreads();
    for (int e = tid; e < rows * (C / 4) * 2; e += 2 * C) {   // rows x (32 float4 of K + 32 float4 of V)
      const int r = e / (C / 2), c4 = e - r * (C / 2);
      const bool isv = c4 >= C / 4;
      const int c = (isv ? c4 - C / 4 : c4) * 4;
      const float4 val = *reinterpret_cast<const float4*>((isv ? vseg : kseg) + (size_t)(s0 + r) * ld + c);
      *reinterpret_cast<float4*>(isv ? &vsh[r][c] : &ksh[r][c]) = val;
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      const float kd = ksh[r][h * D + d];
      const float4 va = *reinterpret_cast<const float4*>(&vsh[r][h * D + e0]);
      const float4 vb = *reinterpret_cast<const float4*>(&vsh[r][h * D + e0 + 4]);
      acc[0] = fmaf(kd, va.x, acc[0]);
      acc[1] = fmaf(kd, va.y, acc[1]);
      acc[2] = fmaf(kd, va.z, acc[2]);
      acc[3] = fmaf(kd, va.w, acc[3]);
      acc[4] = fmaf(kd, vb.x, acc[4]);
      acc[5] = fmaf(kd, vb.y, acc[5]);
      acc[6] = fmaf(kd, vb.z, acc[6]);
      acc[7] = fmaf(kd, vb.w, acc[7]);
      ksum += kd;
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) kv_sh[(h * D + d) * D + e0 + i] = acc[i];
  if (e0 == 0) ks_sh[h * D + d] = ksum;
  __syncthreads();
  // apply: thread = output column c = hq * D + e of rows l = tid / C, + 2, ...; its KV column and the head's Ksum in registers
  const int c = tid & (C - 1), hq = c / D, e = c - hq * D;
  float kvc[D], ksc[D];
#pragma unroll
  for (int dd = 0; dd < D; ++dd) {
    kvc[dd] = kv_sh[(hq * D + dd) * D + e];
    ksc[dd] = ks_sh[hq * D + dd];
  }
  const float src = (float)len_src;
  for (int l = tid / C; l < len_q; l += 2) {
    const float* qr = q + ((size_t)seg * len_q + l) * ld + hq * D;
    float o = 0.f, z = 0.f;
#pragma unroll
    for (int d4 = 0; d4 < D; d4 += 4) {
      const float4 q4 = *reinterpret_cast<const float4*>(qr + d4);
      o = fmaf(q4.x, kvc[d4], o);
      o = fmaf(q4.y, kvc[d4 + 1], o);
      o = fmaf(q4.z, kvc[d4 + 2], o);
      o = fmaf(q4.w, kvc[d4 + 3], o);
      z = fmaf(q4.x, ksc[d4], z);
      z = fmaf(q4.y, ksc[d4 + 1], z);
      z = fmaf(q4.z, ksc[d4 + 2], z);
      z = fmaf(q4.w, ksc[d4 + 3], z);
    }
    out[((size_t)seg * len_q + l) * ldo + c] = o * (1.f / (z + eps)) * src;
  }
}

// fine_head_kernel of fine.hip for windows of 65 .. 128 cells: one wave per match, cells `lane` and `lane + 64` per lane
__global__ __launch_bounds__(256) void fine_head_wide_kernel(const float* __restrict__ f3, size_t ld3, const float* __restrict__ win, int ldw, int M, int Wwin,
                                                             int C, float temp, const float* __restrict__ mkpts_c, float base_scale,
                                                             const float* __restrict__ qscale, float* __restrict__ expec, float* __restrict__ mkpts_f) {
  const int lane = threadIdx.x & 63;
  const int m_raw = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool live = m_raw < M;              // waves past the end redo the last match and store nothing
  const int m = live ? m_raw : M - 1;
  const int WW = Wwin * Wwin;
  __shared__ float sim_sh[4][128];
  const int wv = threadIdx.x >> 6, grp = lane >> 4, sub = lane & 15;
  for (int r0 = 0; r0 < WW; r0 += 4) {
    const int r = r0 + grp;
    float acc = 0.f;
    if (r < WW) {
      const float* w = win + ((size_t)m * WW + r) * ldw;
      const float* f = f3 + (size_t)m * ld3;
      for (int c = sub * 4; c < C; c += 64) {
        const float4 w4 = *reinterpret_cast<const float4*>(w + c);
        const float4 f4 = *reinterpret_cast<const float4*>(f + c);
        acc = fmaf(f4.x, w4.x, acc);
        acc = fmaf(f4.y, w4.y, acc);
        acc = fmaf(f4.z, w4.z, acc);
        acc = fmaf(f4.w, w4.w, acc);
      }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (sub == 0 && r < WW) sim_sh[wv][r] = acc;
  }
  __syncthreads();
  float sim[2], p[2];
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int r = lane + 64 * t;
    sim[t] = r < WW ? temp * sim_sh[wv][r] : -INFINITY;
    mx = fmaxf(mx, sim[t]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float tot = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    p[t] = lane + 64 * t < WW ? expf(sim[t] - mx) : 0.f;
    tot += p[t];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
  float ex = 0.f, ey = 0.f, exx = 0.f, eyy = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int r = lane + 64 * t;
    if (r < WW) {
      const int ky = r / Wwin, kx = r - ky * Wwin;
      // normalised grid: (k / (W-1) - 0.5) * 2, x fastest
      const float gx = ((float)kx / (float)(Wwin - 1) - 0.5f) * 2.f;
      const float gy = ((float)ky / (float)(Wwin - 1) - 0.5f) * 2.f;
      const float pr = p[t] / tot;
      ex += gx * pr;
      ey += gy * pr;
      exx += gx * gx * pr;
      eyy += gy * gy * pr;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ex += __shfl_xor(ex, o, 64);
    ey += __shfl_xor(ey, o, 64);
    exx += __shfl_xor(exx, o, 64);
    eyy += __shfl_xor(eyy, o, 64);
  }
  if (lane == 0 && live) {
    const float vx = fmaxf(exx - ex * ex, 1e-10f);
    const float vy = fmaxf(eyy - ey * ey, 1e-10f);
    expec[3 * m + 0] = ex;
    expec[3 * m + 1] = ey;
    expec[3 * m + 2] = sqrtf(vx) + sqrtf(vy);
    const float half_w = (float)(Wwin / 2);
    const float qsx = qscale ? base_scale * qscale[1] : base_scale;
    const float qsy = qscale ? base_scale * qscale[0] : base_scale;
    mkpts_f[2 * m + 0] = mkpts_c[2 * m + 0] + (ex * half_w) * qsx;
    mkpts_f[2 * m + 1] = mkpts_c[2 * m + 1] + (ey * half_w) * qsy;
  }
}

}  // namespace

int opp_window_gather2(const float* feat0, int Hf0, int Wf0, const float* feat1, int Hf1, int Wf1, const long long* i_ids, const long long* j_ids, int M,
                       int w0c, int w1c, int stride, int Wwin, int C, float* win, hipStream_t stream) {
  if (M <= 0) return OPP_OK;
  OPP_CHECK_ARG(C % 4 == 0 && w0c > 0 && w1c > 0 && stride > 0 && Wwin > 0, "window_gather2: bad shape");
  hipLaunchKernelGGL(window_gather2_kernel, dim3(M, 2), dim3(128), 0, stream, feat0, Hf0, Wf0, feat1, Hf1, Wf1, i_ids, j_ids, M, w0c, w1c, stride, Wwin, C,
                     win);
  OPP_CHECK_LAUNCH("window_gather2_kernel");
  return OPP_OK;
}

bool opp_linattn_seg_ok(int len_q, int len_src, int C, int D) {
  return C == 128 && D == 16 && len_q > 0 && len_src > 0 && len_q <= kSegMaxLen && len_src <= kSegMaxLen;
}

int opp_linattn_seg(const float* q, const float* k, const float* v, int ld, int n_seg, int len_q, int len_src, float* out, int ldo, int C, int D, float eps,
                    hipStream_t stream) {
  if (n_seg <= 0) return OPP_OK;
  OPP_CHECK_ARG(opp_linattn_seg_ok(len_q, len_src, C, D) && ld % 4 == 0, "linattn_seg: unsupported shape");
  hipLaunchKernelGGL((linattn_seg_kernel<16, 128>), dim3(n_seg), dim3(256), 0, stream, q, k, v, ld, len_q, len_src, out, ldo, eps);
  OPP_CHECK_LAUNCH("linattn_seg_kernel");
  return OPP_OK;
}

int opp_fine_head_wide(const float* f3, size_t ld3, const float* win, int ldw, int M, int Wwin, int C, float temp, const float* mkpts_c, float base_scale,
                       const float* qscale, float* expec, float* mkpts_f, hipStream_t stream) {
  if (M <= 0) return OPP_OK;
  OPP_CHECK_ARG(Wwin >= 2 && Wwin * Wwin <= 128 && C % 4 == 0 && ldw % 4 == 0 && ld3 % 4 == 0, "fine head: window %d / channels %d unsupported", Wwin, C);
  hipLaunchKernelGGL(fine_head_wide_kernel, dim3(opp_cdiv(M, 4)), dim3(256), 0, stream, f3, ld3, win, ldw, M, Wwin, C, temp, mkpts_c, base_scale, qscale, expec,
                     mkpts_f);
  OPP_CHECK_LAUNCH("fine_head_wide_kernel");
  return OPP_OK;
}
