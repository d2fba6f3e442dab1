// FullAttention (softmax scaled dot-product attention) of both token streams of one encoder layer, for gfx950.
//
// Reference:
//   FullAttention.forward     src/models/OnePosePlus/loftr_module/linear_attention.py:64-95
//   selected by               src/models/OnePosePlus/loftr_module/transformer.py:32-40 (any `attention` other than "linear")
//
// Per head h (D = C / nhead columns of each third of qkv):  out = softmax(Q K^T / sqrt(D)) V over the source tokens.  No feature map,
// no V / S, no dropout (use_dropout = False is hard-wired upstream).  Masked forwards are refused by the callers (model.py): upstream
// indexes a None q_mask in every cross layer (quirk of FullAttention with x_mask = None, source_mask = query_mask).
//
// Layout: qkv [n_seg * (len0 + len1)][3 C] = the plain projections Q | K | V; stream 0 = rows [0, n_seg len0) as [n_seg][len0], stream 1
// behind it as [n_seg][len1].  msg [same rows][C] fp32.  cross = 0: each stream attends to itself within its segment; cross = 1: to the
// other stream's segment.
//
// Two kernels, chosen by shape (opp_full_attention_run):
//   full_attn_flash_kernel  D = 32 (the coarse level: C = 256, 8 heads).  Flash style: one workgroup of 4 waves per (64-query block,
//       head, segment), both streams' query blocks in one launch; 64-key K / V tiles staged through LDS, double-buffered; online softmax
//       with the running max and sum in fp32 and the O accumulators in registers; exp2 with log2(e) / sqrt(D) folded into the logit scale;
//       one normalisation at the end.  Each wave owns 16 query rows and computes S^T = K Q^T, so a lane holds the logits of ONE query
//       (its column) for 16 keys of a tile, and O^T = V^T P^T, so its O column belongs to that same query: the row max / sum need two
//       lane swaps per tile and the rescale of O is lane-local.
//         bf16x3 (gemm_precision 3): Q, K, V and P carried exactly as hi + mid + lo bf16 (the split of gemm_mfma.hip), six
//           v_mfma_f32_16x16x32_bf16 per product (include/opp_hip.h, gemm_precision); Q split once per block, K and V once per tile as they
//           are staged, P in registers after the exponential; the row sum is formed from the fp32 P.
//         fp32 (gemm_precision 0): v_mfma_f32_16x16x4_f32 on the raw fp32 operands.
//   full_attn_small_kernel  any D in {16, 32} (the fine level: M segments of 25 window cells + 1 point, C = 128, D = 16): exact fp32 on the
//       vector ALU, one thread per (query row, head), the segment's K / V in LDS when they fit.  Self-attention over one token returns V
//       exactly (p = exp2(0) = 1, sum = 1).
#include "enc_frag.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kFaRows = 64;   // query rows per workgroup (16 per wave)
constexpr int kFaKeys = 64;   // keys per K / V tile
constexpr int kFaD = 32;      // head dim of the flash kernel
// bf16x3 LDS images of one tile: K [key][hi x32 | mid x32 | lo x32] (+16 B pad), V^T [part][d][64 keys in MFMA k order] (+16 B pad)
constexpr int kKRowB = 3 * kFaD * 2 + 16;
constexpr int kVRowB = kFaKeys * 2 + 16;
constexpr int kKTileB3 = kFaKeys * kKRowB;
constexpr int kVTileB3 = 3 * kFaD * kVRowB;
// fp32 LDS images: K [key][36], V [key][36] (36: the 16 rows x 4 k of an operand read hit 64 distinct banks)
constexpr int kF32Row = 36;
constexpr int kTileB3 = kKTileB3 + kVTileB3;
constexpr int kTileF32 = 2 * kFaKeys * kF32Row * 4;
constexpr float kLog2e = 1.4426950408889634f;

// rows of stream `st`, segment `seg`: first global row and length
struct FaStream {
  int row0, len;
};
__device__ __forceinline__ FaStream fa_stream(int st, int seg, int n_seg, int len0, int len1) {
  return st == 0 ? FaStream{seg * len0, len0} : FaStream{n_seg * len0 + seg * len1, len1};
}

template <int PREC>
__global__ __launch_bounds__(256) void full_attn_flash_kernel(const float* __restrict__ qkv, int n_seg, int len0, int len1, int C, int cross,
                                                              int nb0, float scale, float* __restrict__ msg) {
  constexpr bool B3 = PREC == OPP_PREC_BF16X3;
  __shared__ __attribute__((aligned(16))) char lds[2 * (B3 ? kTileB3 : kTileF32)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, grp = lane >> 4;
  const int h = blockIdx.y, seg = blockIdx.z;
  const int qst = (int)blockIdx.x < nb0 ? 0 : 1;
  const int qb = qst == 0 ? blockIdx.x : blockIdx.x - nb0;
  const FaStream qs = fa_stream(qst, seg, n_seg, len0, len1);
  const FaStream ks = fa_stream(cross ? 1 - qst : qst, seg, n_seg, len0, len1);
  const size_t ld = 3 * (size_t)C;
  const int hc = h * kFaD;

  // ---- this lane's query (row q0 + col of the wave's 16) as the B operand of S^T = K Q^T
  const int qrow = qb * kFaRows + wave * 16 + col;
  const bool qvalid = qrow < qs.len;
  const float* qp = qkv + (size_t)(qs.row0 + (qvalid ? qrow : 0)) * ld + hc;
  u32x4 qf3[3];   // bf16x3: d = 8 grp + j
  float qf[8];    // fp32: d = 4 i + grp
  if constexpr (B3) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 a = *reinterpret_cast<const float4*>(qp + 8 * grp), b = *reinterpret_cast<const float4*>(qp + 8 * grp + 4);
    split8(qvalid ? a : z, qvalid ? b : z, qf3[0], qf3[1], qf3[2]);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float v = qp[4 * i + grp];
      qf[i] = qvalid ? v : 0.f;
    }
  }

  // ---- staging of one K / V tile: global -> registers (issued early), registers -> LDS (after the tile's compute).  Rows past the end of
  // the segment load row 0 of the segment (always in bounds) and are replaced by zeros as VALUES (a select of pointers to a local zero
  // puts that zero in scratch)
  // K: thread = (key tid >> 2, 8 d from 8 (tid & 3)); V (bf16x3): thread = (d tid & 31, positions 8 (tid >> 5) .. +7); V (fp32): as K
  const int sk_key = tid >> 2, sk_d = 8 * (tid & 3);
  const int sv_d = tid & 31, sv_pb = tid >> 5;
  float4 rk0, rk1, rv0, rv1;
  float rv[8];
  auto load_tile = [&](int t) {
    const int kb = t * kFaKeys;
    const bool kv = kb + sk_key < ks.len;
    const float* kp = qkv + (size_t)(ks.row0 + (kv ? kb + sk_key : 0)) * ld + C + hc + sk_d;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 k0 = *reinterpret_cast<const float4*>(kp), k1 = *reinterpret_cast<const float4*>(kp + 4);
    rk0 = kv ? k0 : z;
    rk1 = kv ? k1 : z;
    if constexpr (B3) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int key = kb + 32 * (sv_pb >> 2) + 4 * (sv_pb & 3) + (j & 3) + 16 * (j >> 2);
        const float v = qkv[(size_t)(ks.row0 + (key < ks.len ? key : 0)) * ld + 2 * C + hc + sv_d];
        rv[j] = key < ks.len ? v : 0.f;
      }
    } else {
      const float4 v0 = *reinterpret_cast<const float4*>(kp + C), v1 = *reinterpret_cast<const float4*>(kp + C + 4);
      rv0 = kv ? v0 : z;
      rv1 = kv ? v1 : z;
    }
  };
  auto store_tile = [&](int buf) {
    char* base = lds + buf * (B3 ? kTileB3 : kTileF32);
    if constexpr (B3) {
      u32x4 hi, mid, lo;
      split8(rk0, rk1, hi, mid, lo);
      char* kd = base + sk_key * kKRowB + sk_d * 2;
      *reinterpret_cast<u32x4*>(kd) = hi;
      *reinterpret_cast<u32x4*>(kd + 64) = mid;
      *reinterpret_cast<u32x4*>(kd + 128) = lo;
      split8(make_float4(rv[0], rv[1], rv[2], rv[3]), make_float4(rv[4], rv[5], rv[6], rv[7]), hi, mid, lo);
      char* vd = base + kKTileB3 + sv_d * kVRowB + sv_pb * 16;
      *reinterpret_cast<u32x4*>(vd) = hi;
      *reinterpret_cast<u32x4*>(vd + kFaD * kVRowB) = mid;
      *reinterpret_cast<u32x4*>(vd + 2 * kFaD * kVRowB) = lo;
    } else {
      float* kd = reinterpret_cast<float*>(base) + sk_key * kF32Row + sk_d;
      *reinterpret_cast<float4*>(kd) = rk0;
      *reinterpret_cast<float4*>(kd + 4) = rk1;
      float* vd = kd + kFaKeys * kF32Row;
      *reinterpret_cast<float4*>(vd) = rv0;
      *reinterpret_cast<float4*>(vd + 4) = rv1;
    }
  };

  // ---- online softmax state of this lane's query (partial sum over this lane group's keys; max shared by the 4 groups)
  float m = -INFINITY, l = 0.f;
  f32x4 o[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};   // O^T[d = 16 db + 4 grp + r][query]
  constexpr int PA[6] = {2, 0, 1, 1, 0, 0};   // part of the first operand per product (0 hi, 1 mid, 2 lo), smallest terms first
  constexpr int PB[6] = {0, 2, 1, 0, 1, 0};

  const int ntiles = (ks.len + kFaKeys - 1) / kFaKeys;
  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) load_tile(t + 1);
    const char* base = lds + (t & 1) * (B3 ? kTileB3 : kTileF32);
    // S^T = K Q^T: 4 blocks of 16 keys; s[kb][r] = logit of key 16 kb + 4 grp + r
    f32x4 s[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      s[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (B3) {
        const char* kr = base + (16 * kb + col) * kKRowB + 16 * grp;
        const u32x4 kf[3] = {*reinterpret_cast<const u32x4*>(kr), *reinterpret_cast<const u32x4*>(kr + 64),
                             *reinterpret_cast<const u32x4*>(kr + 128)};
#pragma unroll
        for (int pr = 0; pr < 6; ++pr)
          s[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kf[PA[pr]]), __builtin_bit_cast(bf16x8, qf3[PB[pr]]),
                                                          s[kb], 0, 0, 0);
      } else {
        const float* kr = reinterpret_cast<const float*>(base) + (16 * kb + col) * kF32Row + grp;
#pragma unroll
        for (int i = 0; i < 8; ++i) s[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[4 * i], qf[i], s[kb], 0, 0, 0);
      }
    }
    // scaled logits, keys past the end of the source segment -> -inf (before the max)
    const int kbase = t * kFaKeys + 4 * grp;
    float tmax = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = kbase + 16 * kb + r < ks.len ? s[kb][r] * scale : -INFINITY;
        s[kb][r] = v;
        tmax = fmaxf(tmax, v);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float mn = fmaxf(m, tmax);          // finite: every tile holds at least one key of the segment
    const float alpha = exp2f(m - mn);        // 0 on the first tile
    m = mn;
    float psum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = exp2f(s[kb][r] - mn);
        s[kb][r] = p;
        psum += p;
      }
    l = l * alpha + psum;
#pragma unroll
    for (int db = 0; db < 2; ++db) o[db] *= alpha;
    // O^T += V^T P^T
    if constexpr (B3) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        u32x4 pf[3];   // element j = P of key 32 c + 16 (j >> 2) + 4 grp + (j & 3) = s[2 c + (j >> 2)][j & 3]
        split8(make_float4(s[2 * c][0], s[2 * c][1], s[2 * c][2], s[2 * c][3]),
               make_float4(s[2 * c + 1][0], s[2 * c + 1][1], s[2 * c + 1][2], s[2 * c + 1][3]), pf[0], pf[1], pf[2]);
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const char* vr = base + kKTileB3 + (16 * db + col) * kVRowB + (32 * c + 8 * grp) * 2;
          const u32x4 vf[3] = {*reinterpret_cast<const u32x4*>(vr), *reinterpret_cast<const u32x4*>(vr + kFaD * kVRowB),
                               *reinterpret_cast<const u32x4*>(vr + 2 * kFaD * kVRowB)};
#pragma unroll
          for (int pr = 0; pr < 6; ++pr)
            o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vf[PA[pr]]), __builtin_bit_cast(bf16x8, pf[PB[pr]]),
                                                            o[db], 0, 0, 0);
        }
      }
    } else {
      const float* vb = reinterpret_cast<const float*>(base) + kFaKeys * kF32Row;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float* vr = vb + (16 * kb + 4 * grp + r) * kF32Row + col;
#pragma unroll
          for (int db = 0; db < 2; ++db) o[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[16 * db], s[kb][r], o[db], 0, 0, 0);
        }
    }
    if (t + 1 < ntiles) store_tile((t + 1) & 1);
    __syncthreads();
  }
  // normalise once: the row sum over the 4 lane groups
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (!qvalid) return;
  const float inv = 1.f / l;
  float* op = msg + (size_t)(qs.row0 + qrow) * C + hc + 4 * grp;
#pragma unroll
  for (int db = 0; db < 2; ++db)
    *reinterpret_cast<float4*>(op + 16 * db) = make_float4(o[db][0] * inv, o[db][1] * inv, o[db][2] * inv, o[db][3] * inv);
}

// ---- small shapes / any D in {16, 32}: one thread per (query row, head), exact fp32 on the vector ALU ------------------------------------
// grid (n_seg, ceil((len0 + len1) * nhead / 256)).  LDS_KV: the segment's K and V of both streams ((len0 + len1) x 2 C floats) are
// staged once per workgroup; otherwise read through the caches.
template <int D, bool LDS_KV>
__global__ __launch_bounds__(256) void full_attn_small_kernel(const float* __restrict__ qkv, int n_seg, int len0, int len1, int C, int cross,
                                                              float scale, float* __restrict__ msg) {
  extern __shared__ __attribute__((aligned(16))) float kvs[];   // [len0 + len1][2 C]: K | V, stream 0 rows first
  const int seg = blockIdx.x, nhead = C / D;
  const size_t ld = 3 * (size_t)C;
  const FaStream s0 = fa_stream(0, seg, n_seg, len0, len1), s1 = fa_stream(1, seg, n_seg, len0, len1);
  if constexpr (LDS_KV) {
    const int rows = len0 + len1, n4 = 2 * C / 4;
    for (int i = threadIdx.x; i < rows * n4; i += blockDim.x) {
      const int r = i / n4, c = 4 * (i - r * n4);
      const int grow = r < len0 ? s0.row0 + r : s1.row0 + r - len0;
      *reinterpret_cast<float4*>(kvs + (size_t)r * 2 * C + c) = *reinterpret_cast<const float4*>(qkv + (size_t)grow * ld + C + c);
    }
    __syncthreads();
  }
  const int item = blockIdx.y * blockDim.x + threadIdx.x;
  if (item >= (len0 + len1) * nhead) return;
  const int qi = item / nhead, h = item - qi * nhead;
  const int qst = qi < len0 ? 0 : 1;
  const FaStream qs = qst == 0 ? s0 : s1;
  const FaStream ks = (cross ? 1 - qst : qst) == 0 ? s0 : s1;
  const int klocal0 = (cross ? 1 - qst : qst) == 0 ? 0 : len0;   // first LDS row of the key stream
  const float* qp = qkv + (size_t)(qs.row0 + (qst == 0 ? qi : qi - len0)) * ld + h * D;
  float q[D], acc[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    q[d] = qp[d] * scale;   // log2(e) / sqrt(D) folded into Q: the logits come out in exp2 units
    acc[d] = 0.f;
  }
  float m = -INFINITY, l = 0.f;
  for (int k = 0; k < ks.len; ++k) {
    const float* kp = LDS_KV ? kvs + (size_t)(klocal0 + k) * 2 * C + h * D : qkv + (size_t)(ks.row0 + k) * ld + C + h * D;
    const float* vp = kp + C;   // V follows K by C columns in both layouts
    float sv = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) sv = fmaf(q[d], kp[d], sv);
    const float mn = fmaxf(m, sv);
    const float alpha = exp2f(m - mn);
    const float p = exp2f(sv - mn);
    m = mn;
    l = l * alpha + p;
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] = fmaf(p, vp[d], acc[d] * alpha);
  }
  const float inv = 1.f / l;
  float* op = msg + (size_t)(qs.row0 + (qst == 0 ? qi : qi - len0)) * C + h * D;
#pragma unroll
  for (int d = 0; d < D; ++d) op[d] = acc[d] * inv;
}

template <int D>
int launch_small(const float* qkv, int n_seg, int len0, int len1, int C, int cross, float scale, float* msg, hipStream_t stream) {
  const size_t lds = (size_t)(len0 + len1) * 2 * C * sizeof(float);
  const dim3 grid(n_seg, opp_cdiv((len0 + len1) * (C / D), 256));
  if (lds <= 32768 && C % 4 == 0 && (reinterpret_cast<uintptr_t>(qkv) & 15) == 0) {
    hipLaunchKernelGGL((full_attn_small_kernel<D, true>), grid, dim3(256), lds, stream, qkv, n_seg, len0, len1, C, cross, scale, msg);
    OPP_CHECK_LAUNCH("full_attn_small_kernel");
  } else {
    hipLaunchKernelGGL((full_attn_small_kernel<D, false>), grid, dim3(256), 0, stream, qkv, n_seg, len0, len1, C, cross, scale, msg);
    OPP_CHECK_LAUNCH("full_attn_small_kernel");
  }
  return OPP_OK;
}

}  // namespace

// the flash kernel takes D = 32 with 16-byte aligned rows once a stream is longer than one 32-key block; everything else (the fine level,
// D = 16, tiny streams) runs on the small kernel
int opp_full_attention_run(const float* qkv, int n_seg, int len0, int len1, int C, int nhead, int cross, int prec, float* msg,
                           hipStream_t stream) {
  OPP_CHECK_ARG(qkv && msg && n_seg > 0 && len0 > 0 && len1 > 0 && nhead > 0 && C % nhead == 0, "full_attention: bad shape");
  const int D = C / nhead;
  OPP_CHECK_ARG(D == 16 || D == 32, "full_attention: head dim %d unsupported (16 or 32)", D);
  OPP_CHECK_ARG(prec == OPP_PREC_FP32 || prec == OPP_PREC_BF16X3, "full_attention: arithmetic must be fp32 or bf16x3");
  OPP_CHECK_ARG((long long)n_seg * (len0 + len1) < (1ll << 31) / 3 / C, "full_attention: too many rows");
  const float scale = kLog2e / sqrtf((float)D);
  const bool flash = D == kFaD && (len0 > 32 || len1 > 32) && n_seg <= 65535 && C % 4 == 0 && (reinterpret_cast<uintptr_t>(qkv) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(msg) & 15) == 0;
  if (!flash) return D == 16 ? launch_small<16>(qkv, n_seg, len0, len1, C, cross, scale, msg, stream)
                             : launch_small<32>(qkv, n_seg, len0, len1, C, cross, scale, msg, stream);
  const int nb0 = opp_cdiv(len0, kFaRows), nb1 = opp_cdiv(len1, kFaRows);
  const dim3 grid(nb0 + nb1, nhead, n_seg);
  if (prec == OPP_PREC_BF16X3) {
    hipLaunchKernelGGL((full_attn_flash_kernel<OPP_PREC_BF16X3>), grid, dim3(256), 0, stream, qkv, n_seg, len0, len1, C, cross, nb0, scale, msg);
    OPP_CHECK_LAUNCH("full_attn_flash_kernel");
  } else {
    hipLaunchKernelGGL((full_attn_flash_kernel<OPP_PREC_FP32>), grid, dim3(256), 0, stream, qkv, n_seg, len0, len1, C, cross, nb0, scale, msg);
    OPP_CHECK_LAUNCH("full_attn_flash_kernel");
  }
  return OPP_OK;
}
