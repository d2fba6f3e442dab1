// FullAttention of the training step: forward that also returns the softmax statistics, and its backward, for gfx950.
//
// Reference:
//   FullAttention.forward     src/models/OnePosePlus/loftr_module/linear_attention.py:64-95 (no mask, use_dropout = False: transformer.py:37)
//
// Operands as HipLinearAttention's: q [B][L][H][D], k, v [B][S][H][D] fp32 contiguous.  Per head: out = softmax(q k^T / sqrt(D)) v.
// The forward also writes lse [B][H][L] = log2 sum_s exp(logit_s) in BASE 2 (row maximum + log2 of the row sum of the exp2 logits;
// x ln 2 = the natural log-sum-exp); the backward rebuilds the probabilities from it tile by tile, P = exp2(logit2 - lse), so nothing
// of size L x S exists anywhere:
//     delta_l = sum_d dO_ld O_ld,   dP = dO V^T,   dS = P o (dP - delta),   dV = P^T dO,   dK = dS^T Q / sqrt(D),   dQ = dS K / sqrt(D)
//
// Two kernel families, chosen by shape as csrc/full_attention.hip does:
//   fat_tile_kernel<PREC, MODE>   D = 32 and a stream longer than 32 rows (the coarse level).  ONE body serves the forward and the two
//       backward kernels: a workgroup of 4 waves owns 64 rows of the "own" stream (16 per wave, one row per lane column) and walks the
//       "tile" stream in 64-row tiles staged through LDS; every product has the tile rows as the MFMA's A operand and the lane's own row
//       (or the values just computed for it) as the B operand, exactly the swapped orientation of the inference kernel, so that all
//       per-row state (running max / sum, lse, delta, the accumulators) is lane-local and the accumulator of one product is the B operand
//       of the next without leaving its registers:
//         MODE_FWD   own = queries (Q),      tiles = keys (K, V):    S^T = K Q^T, online softmax, O^T += V^T P^T              -> out, lse
//         MODE_DQ    own = queries (Q, dO),  tiles = keys (K, V):    S^T = K Q^T, dP^T = V dO^T,  dQ^T += K^T dS^T             -> dQ
//         MODE_DKV   own = keys (K, V),      tiles = queries (Q, dO): S = Q K^T,  dP = dO V^T,    dK^T += Q^T dS, dV^T += dO^T P -> dK, dV
//       2 + 3 + 4 MFMA products: 7 in the backward against 2 in the forward.  No atomics: every output row has one owner.
//         bf16x3 (precision 3): operands exact hi + mid + lo bf16 (enc_frag.h split8), six v_mfma_f32_16x16x32_bf16 per product; a tile is
//           staged row-major [row][hi x32 | mid x32 | lo x32] for the products that reduce over d, and transposed [part][d][64 rows in MFMA
//           k order] for those that reduce over the tile's rows (the V^T image of the inference kernel).
//         fp32 (precision 0): v_mfma_f32_16x16x4_f32 on the raw operands; one row-major [row][36] image serves both kinds of product.
//       Global loads of tile t + 1 are issued before the MFMAs of tile t.  fp32 double-buffers the LDS images; bf16x3 keeps ONE buffer
//       (54 KB for MODE_DKV: two would leave one workgroup per CU) and pays a second barrier per tile.
//       Rows past a stream's end load row 0 of the sample (in bounds) and are zeroed as values; their probabilities are forced to 0.
//   fat_small_*                   both streams <= 64 rows and (L + S) D <= 2048 (the fine level: 25 + 1 tokens, D = 16; D = 32 up to 32 + 32):
//       one workgroup per (sample, head), q / k / v / dO of the head in LDS, exact fp32 on the vector ALU in both arithmetics.  One token
//       attending to itself gives p = exp2(0) = 1 exactly, hence dv = dO and dq = dk = 0.
#include "enc_frag.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kRows = 64;    // own rows per workgroup (16 per wave)
constexpr int kTile = 64;    // rows per staged tile
constexpr int kD = 32;       // head dim of the tile kernels
constexpr int kRowB = 3 * kD * 2 + 16;        // bf16x3 row-major image: [row][hi x32 | mid x32 | lo x32] + 16 B pad
constexpr int kTrB = kTile * 2 + 16;          // bf16x3 transposed image: [part][d][64 rows in MFMA k order] + 16 B pad
constexpr int kRowImg = kTile * kRowB;        // 13312
constexpr int kTrImg = 3 * kD * kTrB;         // 13824
constexpr int kF32Row = 36;
constexpr int kF32Img = kTile * kF32Row * 4;  // 9216
constexpr float kLog2e = 1.4426950408889634f;

enum { MODE_FWD = 0, MODE_DQ = 1, MODE_DKV = 2 };

// which LDS images a mode needs of the tile's first (T1: K or Q) and second (T2: V or dO) tensor
template <int MODE> struct Imgs {
  static constexpr bool r1 = true;                 // S reduces over d
  static constexpr bool t1 = MODE != MODE_FWD;     // dQ / dK reduce over the tile rows of T1
  static constexpr bool r2 = MODE != MODE_FWD;     // dP reduces over d
  static constexpr bool t2 = MODE != MODE_DQ;      // O / dV reduce over the tile rows of T2
};

template <int PREC, int MODE> struct Lds {
  static constexpr bool B3 = PREC == OPP_PREC_BF16X3;
  using I = Imgs<MODE>;
  static constexpr int oR1 = 0;
  static constexpr int oT1 = oR1 + (I::r1 ? kRowImg : 0);
  static constexpr int oR2 = oT1 + (I::t1 ? kTrImg : 0);
  static constexpr int oT2 = oR2 + (I::r2 ? kRowImg : 0);
  static constexpr int endB3 = oT2 + (I::t2 ? kTrImg : 0);
  static constexpr int oStat = B3 ? endB3 : 2 * kF32Img;           // lse | delta of the tile's rows (MODE_DKV)
  static constexpr int buf = oStat + (MODE == MODE_DKV ? 2 * kTile * 4 : 0);
  static constexpr int nbuf = B3 ? 1 : 2;
};

// v, or zeros when !c -- component by component: a select between two float4 OBJECTS becomes a select of their addresses (scratch)
__device__ __forceinline__ float4 sel4(bool c, const float4 v) { return make_float4(c ? v.x : 0.f, c ? v.y : 0.f, c ? v.z : 0.f, c ? v.w : 0.f); }

// own / tile: first row ((b * len) * H + h) * D is folded into the pointers; row stride ld = H * D floats
template <int PREC, int MODE>
__global__ __launch_bounds__(256) void fat_tile_kernel(const float* __restrict__ own1, const float* __restrict__ own2,
                                                       const float* __restrict__ til1, const float* __restrict__ til2,
                                                       const float* __restrict__ lse_in, const float* __restrict__ delta_in, int own_len,
                                                       int til_len, int H, float scale2, float out_scale, float* __restrict__ out1,
                                                       float* __restrict__ out2, float* __restrict__ lse_out) {
  constexpr bool B3 = PREC == OPP_PREC_BF16X3;
  using I = Imgs<MODE>;
  using LD = Lds<PREC, MODE>;
  __shared__ __attribute__((aligned(16))) char lds[LD::nbuf * LD::buf];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, grp = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  const size_t ld = (size_t)H * kD;
  const size_t own_base = ((size_t)b * own_len * H + h) * kD, til_base = ((size_t)b * til_len * H + h) * kD;
  // lse / delta are [B][H][L] over the QUERIES: the own rows of MODE_DQ, the tile rows of MODE_DKV
  const size_t stat_base = ((size_t)b * H + h) * (size_t)(MODE == MODE_DKV ? til_len : own_len);

  // ---- this lane's own row (orow) as the B operand of the products that reduce over d
  const int orow = blockIdx.x * kRows + wave * 16 + col;
  const bool ovalid = orow < own_len;
  const size_t ooff = own_base + (size_t)(ovalid ? orow : 0) * ld;
  u32x4 a3[3], b3[3];   // bf16x3: d = 8 grp + j
  float af[8], bf[8];   // fp32: d = 4 i + grp
  {
    if constexpr (B3) {
      const float4 x0 = *reinterpret_cast<const float4*>(own1 + ooff + 8 * grp), x1 = *reinterpret_cast<const float4*>(own1 + ooff + 8 * grp + 4);
      split8(sel4(ovalid, x0), sel4(ovalid, x1), a3[0], a3[1], a3[2]);
      if constexpr (MODE != MODE_FWD) {
        const float4 y0 = *reinterpret_cast<const float4*>(own2 + ooff + 8 * grp), y1 = *reinterpret_cast<const float4*>(own2 + ooff + 8 * grp + 4);
        split8(sel4(ovalid, y0), sel4(ovalid, y1), b3[0], b3[1], b3[2]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float x = own1[ooff + 4 * i + grp];
        af[i] = ovalid ? x : 0.f;
        if constexpr (MODE != MODE_FWD) {
          const float y = own2[ooff + 4 * i + grp];
          bf[i] = ovalid ? y : 0.f;
        }
      }
    }
  }
  float own_lse = 0.f, own_delta = 0.f;
  if constexpr (MODE == MODE_DQ) {
    const float l0 = lse_in[stat_base + (ovalid ? orow : 0)], d0 = delta_in[stat_base + (ovalid ? orow : 0)];
    own_lse = ovalid ? l0 : 0.f;
    own_delta = ovalid ? d0 : 0.f;
  }

  // ---- staging of one tile: global -> registers (issued before the tile's MFMAs), registers -> LDS afterwards.  Rows past the end load
  // row 0 of the sample and become zeros as VALUES.  Row-major images: thread = (row tid >> 2, 8 d from 8 (tid & 3)); transposed images
  // (bf16x3): thread = (d tid & 31, k positions 8 (tid >> 5) .. + 7, i.e. rows 32 (pb >> 2) + 4 (pb & 3) + (j & 3) + 16 (j >> 2))
  const int s_row = tid >> 2, s_d = 8 * (tid & 3);
  const int s_td = tid & 31, s_pb = tid >> 5;
  float4 r1a, r1b, r2a, r2b;
  float t1[8], t2[8];
  float st_l = 0.f, st_d = 0.f;
  auto load_tile = [&](int t) __attribute__((always_inline)) {
    const int tb = t * kTile;
    const bool rv = tb + s_row < til_len;
    const size_t roff = til_base + (size_t)(rv ? tb + s_row : 0) * ld + s_d;
    {
      const float4 x0 = *reinterpret_cast<const float4*>(til1 + roff), x1 = *reinterpret_cast<const float4*>(til1 + roff + 4);
      r1a = sel4(rv, x0);
      r1b = sel4(rv, x1);
    }
    if constexpr (I::r2 || !B3) {
      const float4 y0 = *reinterpret_cast<const float4*>(til2 + roff), y1 = *reinterpret_cast<const float4*>(til2 + roff + 4);
      r2a = sel4(rv, y0);
      r2b = sel4(rv, y1);
    }
    if constexpr (B3 && (I::t1 || I::t2)) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int row = tb + 32 * (s_pb >> 2) + 4 * (s_pb & 3) + (j & 3) + 16 * (j >> 2);
        const size_t off = til_base + (size_t)(row < til_len ? row : 0) * ld + s_td;
        if constexpr (I::t1) {
          const float x = til1[off];
          t1[j] = row < til_len ? x : 0.f;
        }
        if constexpr (I::t2) {
          const float y = til2[off];
          t2[j] = row < til_len ? y : 0.f;
        }
      }
    }
    if constexpr (MODE == MODE_DKV) {
      if (tid < kTile) {
        const bool sv = tb + tid < til_len;
        const float l0 = lse_in[stat_base + (sv ? tb + tid : 0)], d0 = delta_in[stat_base + (sv ? tb + tid : 0)];
        st_l = sv ? l0 : 0.f;
        st_d = sv ? d0 : 0.f;
      }
    }
  };
  auto store_tile = [&](int buf) __attribute__((always_inline)) {
    char* base = lds + buf * LD::buf;
    if constexpr (B3) {
      u32x4 hi, mid, lo;
      {
        split8(r1a, r1b, hi, mid, lo);
        char* p = base + LD::oR1 + s_row * kRowB + s_d * 2;
        *reinterpret_cast<u32x4*>(p) = hi;
        *reinterpret_cast<u32x4*>(p + 64) = mid;
        *reinterpret_cast<u32x4*>(p + 128) = lo;
      }
      if constexpr (I::r2) {
        split8(r2a, r2b, hi, mid, lo);
        char* p = base + LD::oR2 + s_row * kRowB + s_d * 2;
        *reinterpret_cast<u32x4*>(p) = hi;
        *reinterpret_cast<u32x4*>(p + 64) = mid;
        *reinterpret_cast<u32x4*>(p + 128) = lo;
      }
      if constexpr (I::t1) {
        split8(make_float4(t1[0], t1[1], t1[2], t1[3]), make_float4(t1[4], t1[5], t1[6], t1[7]), hi, mid, lo);
        char* p = base + LD::oT1 + s_td * kTrB + s_pb * 16;
        *reinterpret_cast<u32x4*>(p) = hi;
        *reinterpret_cast<u32x4*>(p + kD * kTrB) = mid;
        *reinterpret_cast<u32x4*>(p + 2 * kD * kTrB) = lo;
      }
      if constexpr (I::t2) {
        split8(make_float4(t2[0], t2[1], t2[2], t2[3]), make_float4(t2[4], t2[5], t2[6], t2[7]), hi, mid, lo);
        char* p = base + LD::oT2 + s_td * kTrB + s_pb * 16;
        *reinterpret_cast<u32x4*>(p) = hi;
        *reinterpret_cast<u32x4*>(p + kD * kTrB) = mid;
        *reinterpret_cast<u32x4*>(p + 2 * kD * kTrB) = lo;
      }
    } else {
      float* p = reinterpret_cast<float*>(base) + s_row * kF32Row + s_d;
      *reinterpret_cast<float4*>(p) = r1a;
      *reinterpret_cast<float4*>(p + 4) = r1b;
      float* p2 = p + kTile * kF32Row;
      *reinterpret_cast<float4*>(p2) = r2a;
      *reinterpret_cast<float4*>(p2 + 4) = r2b;
    }
    if constexpr (MODE == MODE_DKV) {
      if (tid < kTile) {
        float* sp = reinterpret_cast<float*>(base + LD::oStat);
        sp[tid] = st_l;
        sp[kTile + tid] = st_d;
      }
    }
  };

  constexpr int PA[6] = {2, 0, 1, 1, 0, 0};   // part of the first operand per product (0 hi, 1 mid, 2 lo), smallest terms first
  constexpr int PB[6] = {0, 2, 1, 0, 1, 0};
  // C^T[tile row 16 rb + 4 grp + r][own col] = sum_d tile[row][d] own[d]: A from a row-major image, B from the own-row registers
  auto prod_rows = [&](const char* base, int img_off, int f32_img, const u32x4* o3, const float* of, f32x4* c) __attribute__((always_inline)) {
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
      c[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (B3) {
        const char* ar = base + img_off + (16 * rb + col) * kRowB + 16 * grp;
        const u32x4 av[3] = {*reinterpret_cast<const u32x4*>(ar), *reinterpret_cast<const u32x4*>(ar + 64),
                             *reinterpret_cast<const u32x4*>(ar + 128)};
#pragma unroll
        for (int pr = 0; pr < 6; ++pr)
          c[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av[PA[pr]]), __builtin_bit_cast(bf16x8, o3[PB[pr]]), c[rb],
                                                          0, 0, 0);
      } else {
        const float* ar = reinterpret_cast<const float*>(base) + f32_img * kTile * kF32Row + (16 * rb + col) * kF32Row + grp;
#pragma unroll
        for (int i = 0; i < 8; ++i) c[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[4 * i], of[i], c[rb], 0, 0, 0);
      }
    }
  };
  // acc^T[d = 16 db + 4 grp + r][own col] += sum_rows tile[row][d] w[row][own col]: A from a transposed image, B = w in registers
  // (w[rb][r] belongs to tile row 16 rb + 4 grp + r: the layout prod_rows leaves)
  auto acc_cols = [&](const char* base, int img_off, int f32_img, const f32x4* w, f32x4* acc) __attribute__((always_inline)) {
    if constexpr (B3) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        u32x4 wf[3];   // element j = w of tile row 32 c + 16 (j >> 2) + 4 grp + (j & 3) = w[2 c + (j >> 2)][j & 3]
        split8(make_float4(w[2 * c][0], w[2 * c][1], w[2 * c][2], w[2 * c][3]),
               make_float4(w[2 * c + 1][0], w[2 * c + 1][1], w[2 * c + 1][2], w[2 * c + 1][3]), wf[0], wf[1], wf[2]);
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const char* ar = base + img_off + (16 * db + col) * kTrB + (32 * c + 8 * grp) * 2;
          const u32x4 av[3] = {*reinterpret_cast<const u32x4*>(ar), *reinterpret_cast<const u32x4*>(ar + kD * kTrB),
                               *reinterpret_cast<const u32x4*>(ar + 2 * kD * kTrB)};
#pragma unroll
          for (int pr = 0; pr < 6; ++pr)
            acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av[PA[pr]]), __builtin_bit_cast(bf16x8, wf[PB[pr]]),
                                                              acc[db], 0, 0, 0);
        }
      }
    } else {
      const float* ab = reinterpret_cast<const float*>(base) + f32_img * kTile * kF32Row;
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float* ar = ab + (16 * rb + 4 * grp + r) * kF32Row + col;
#pragma unroll
          for (int db = 0; db < 2; ++db) acc[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[16 * db], w[rb][r], acc[db], 0, 0, 0);
        }
    }
  };

  float m = -INFINITY, l = 0.f;                                                  // MODE_FWD: online softmax state of this lane's query
  f32x4 acc1[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};                  // O^T / dQ^T / dK^T [d = 16 db + 4 grp + r][own col]
  f32x4 acc2[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};                  // dV^T (MODE_DKV)

  const int ntiles = (til_len + kTile - 1) / kTile;
  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) load_tile(t + 1);
    const char* base = lds + (LD::nbuf == 2 ? (t & 1) : 0) * LD::buf;
    f32x4 s[4];
    prod_rows(base, LD::oR1, 0, a3, af, s);
    const int rbase = t * kTile + 4 * grp;
    if constexpr (MODE == MODE_FWD) {
      // scaled logits, keys past the end -> -inf (before the max)
      float tmax = -INFINITY;
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = rbase + 16 * rb + r < til_len ? s[rb][r] * scale2 : -INFINITY;
          s[rb][r] = v;
          tmax = fmaxf(tmax, v);
        }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
      const float mn = fmaxf(m, tmax);          // finite: every tile holds at least one key
      const float alpha = exp2f(m - mn);        // 0 on the first tile
      m = mn;
      float psum = 0.f;
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = exp2f(s[rb][r] - mn);
          s[rb][r] = p;
          psum += p;
        }
      l = l * alpha + psum;
#pragma unroll
      for (int db = 0; db < 2; ++db) acc1[db] *= alpha;
      acc_cols(base, LD::oT2, 1, s, acc1);
    } else {
      f32x4 dp[4];
      prod_rows(base, LD::oR2, 1, b3, bf, dp);
      const float* stat = reinterpret_cast<const float*>(base + LD::oStat);
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int tr = 16 * rb + 4 * grp + r;
          const float lse = MODE == MODE_DKV ? stat[tr] : own_lse;
          const float del = MODE == MODE_DKV ? stat[kTile + tr] : own_delta;
          // rows of the tile past the end of its stream: probability 0 (their operands are zeros, lse 0)
          const float p = rbase + 16 * rb + r < til_len ? exp2f(s[rb][r] * scale2 - lse) : 0.f;
          s[rb][r] = p;
          dp[rb][r] = p * (dp[rb][r] - del);
        }
      acc_cols(base, LD::oT1, 0, dp, acc1);
      if constexpr (MODE == MODE_DKV) acc_cols(base, LD::oT2, 1, s, acc2);
    }
    if (t + 1 < ntiles) {
      if constexpr (LD::nbuf == 1) __syncthreads();   // one buffer: every wave is done reading tile t
      store_tile(LD::nbuf == 2 ? (t + 1) & 1 : 0);
    }
    __syncthreads();
  }

  if constexpr (MODE == MODE_FWD) {
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
  }
  if (!ovalid) return;
  float mul = out_scale;
  if constexpr (MODE == MODE_FWD) {
    mul = 1.f / l;
    if (grp == 0) lse_out[stat_base + orow] = m + log2f(l);
  }
  float* op = out1 + own_base + (size_t)orow * ld + 4 * grp;
#pragma unroll
  for (int db = 0; db < 2; ++db)
    *reinterpret_cast<float4*>(op + 16 * db) = make_float4(acc1[db][0] * mul, acc1[db][1] * mul, acc1[db][2] * mul, acc1[db][3] * mul);
  if constexpr (MODE == MODE_DKV) {
    float* vp = out2 + own_base + (size_t)orow * ld + 4 * grp;
#pragma unroll
    for (int db = 0; db < 2; ++db) *reinterpret_cast<float4*>(vp + 16 * db) = make_float4(acc2[db][0], acc2[db][1], acc2[db][2], acc2[db][3]);
  }
}

// delta [B][H][L] = sum_d dO O: one thread per (b, l, h)
template <int D>
__global__ __launch_bounds__(256) void fat_delta_kernel(const float* __restrict__ go, const float* __restrict__ out, int L, int H, size_t n,
                                                        float* __restrict__ delta) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // (b * L + l) * H + h
  if (i >= n) return;
  const float4* g4 = reinterpret_cast<const float4*>(go + i * D);
  const float4* o4 = reinterpret_cast<const float4*>(out + i * D);
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < D / 4; ++j) {
    const float4 g = g4[j], o = o4[j];
    acc = fmaf(g.x, o.x, acc);
    acc = fmaf(g.y, o.y, acc);
    acc = fmaf(g.z, o.z, acc);
    acc = fmaf(g.w, o.w, acc);
  }
  const int h = (int)(i % H);
  const size_t bl = i / H;
  const int lq = (int)(bl % L);
  const size_t b = bl / L;
  delta[(b * H + h) * L + lq] = acc;
}

// ---- short streams: one workgroup per (sample, head), exact fp32 on the vector ALU ---------------------------------------------------
constexpr int kSmallRows = 64;       // longest stream
constexpr int kSmallElems = 2048;    // (L + S) * D at most: q | dO and k | v of one head in LDS

// stage rows [len][D] of head h of sample b into LDS (row stride D)
template <int D>
__device__ __forceinline__ void small_stage(const float* __restrict__ src, int b, int len, int H, int h, float* dst) {
  const float* base = src + ((size_t)b * len * H + h) * D;
  for (int i = threadIdx.x; i < len * (D / 4); i += blockDim.x) {
    const int r = i / (D / 4), c = 4 * (i - r * (D / 4));
    *reinterpret_cast<float4*>(dst + r * D + c) = *reinterpret_cast<const float4*>(base + (size_t)r * H * D + c);
  }
}

// logit in exp2 units, the fma chain of full_attn_small_kernel (log2(e) / sqrt(D) folded into q)
template <int D>
__device__ __forceinline__ float small_logit(const float* q, const float* k, float scale2) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < D; ++d) s = fmaf(q[d] * scale2, k[d], s);
  return s;
}

template <int D>
__global__ __launch_bounds__(128) void fat_small_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                            int L, int S, int H, float scale2, float* __restrict__ out, float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) float sm[2 * kSmallElems];   // q [L][D] | k [S][D] | v [S][D]
  const int b = blockIdx.x, h = blockIdx.y;
  float* qs = sm;
  float* ks = qs + L * D;
  float* vs = ks + S * D;
  small_stage<D>(q, b, L, H, h, qs);
  small_stage<D>(k, b, S, H, h, ks);
  small_stage<D>(v, b, S, H, h, vs);
  __syncthreads();
  const int i = threadIdx.x;
  if (i >= L) return;
  float acc[D];
#pragma unroll
  for (int d = 0; d < D; ++d) acc[d] = 0.f;
  float m = -INFINITY, l = 0.f;
  for (int j = 0; j < S; ++j) {
    const float sv = small_logit<D>(qs + i * D, ks + j * D, scale2);
    const float mn = fmaxf(m, sv);
    const float alpha = exp2f(m - mn);
    const float p = exp2f(sv - mn);
    m = mn;
    l = l * alpha + p;
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] = fmaf(p, vs[j * D + d], acc[d] * alpha);
  }
  const float inv = 1.f / l;
  float* op = out + (((size_t)b * L + i) * H + h) * D;
#pragma unroll
  for (int d = 0; d < D; ++d) op[d] = acc[d] * inv;
  lse[((size_t)b * H + h) * L + i] = m + log2f(l);
}

template <int D>
__global__ __launch_bounds__(256) void fat_small_bwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                            const float* __restrict__ lse, const float* __restrict__ go, int L, int S, int H,
                                                            float scale2, float out_scale, float* __restrict__ gq, float* __restrict__ gk,
                                                            float* __restrict__ gv) {
  __shared__ __attribute__((aligned(16))) float sm[2 * kSmallElems + 2 * kSmallRows * kSmallRows];
  const int b = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
  float* qs = sm;                       // [L][D]
  float* gs = qs + L * D;               // dO [L][D]
  float* ks = gs + L * D;               // [S][D]
  float* vs = ks + S * D;               // [S][D]
  float* P = sm + 2 * kSmallElems;      // [L][S]: logits, then probabilities
  float* dS = P + kSmallRows * kSmallRows;   // [L][S]: dP, then dS
  small_stage<D>(q, b, L, H, h, qs);
  small_stage<D>(go, b, L, H, h, gs);
  small_stage<D>(k, b, S, H, h, ks);
  small_stage<D>(v, b, S, H, h, vs);
  __syncthreads();
  for (int e = tid; e < L * S; e += blockDim.x) {
    const int i = e / S, j = e - i * S;
    P[e] = small_logit<D>(qs + i * D, ks + j * D, scale2);
    float dp = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) dp = fmaf(gs[i * D + d], vs[j * D + d], dp);
    dS[e] = dp;
  }
  __syncthreads();
  // one thread per query row: p = exp2(logit - lse), delta = sum_j p dP (= dO . O), dS = p (dP - delta)
  if (tid < L) {
    const float ls = lse[((size_t)b * H + h) * L + tid];
    float delta = 0.f;
    for (int j = 0; j < S; ++j) {
      const float p = exp2f(P[tid * S + j] - ls);
      P[tid * S + j] = p;
      delta = fmaf(p, dS[tid * S + j], delta);
    }
    for (int j = 0; j < S; ++j) dS[tid * S + j] = P[tid * S + j] * (dS[tid * S + j] - delta);
  }
  __syncthreads();
  for (int e = tid; e < L * D; e += blockDim.x) {
    const int i = e / D, d = e - i * D;
    float a = 0.f;
    for (int j = 0; j < S; ++j) a = fmaf(dS[i * S + j], ks[j * D + d], a);
    gq[(((size_t)b * L + i) * H + h) * D + d] = a * out_scale;
  }
  for (int e = tid; e < S * D; e += blockDim.x) {
    const int j = e / D, d = e - j * D;
    float ak = 0.f, av = 0.f;
    for (int i = 0; i < L; ++i) {
      ak = fmaf(dS[i * S + j], qs[i * D + d], ak);
      av = fmaf(P[i * S + j], gs[i * D + d], av);
    }
    const size_t o = (((size_t)b * S + j) * H + h) * D + d;
    gk[o] = ak * out_scale;
    gv[o] = av;
  }
}

enum { FAM_NONE = 0, FAM_TILE = 1, FAM_SMALL = 2 };

int family(int B, int L, int S, int H, int D) {
  if (B <= 0 || L <= 0 || S <= 0 || H <= 0 || H > 65535 || B > 65535 || (D != 16 && D != 32)) return FAM_NONE;
  if ((long long)B * H * D * (L > S ? L : S) >= (1ll << 31)) return FAM_NONE;
  if (D == kD && (L > 32 || S > 32)) return FAM_TILE;
  if (L <= kSmallRows && S <= kSmallRows && (L + S) * D <= kSmallElems) return FAM_SMALL;
  return FAM_NONE;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int PREC, int MODE>
int launch_tile(const float* own1, const float* own2, const float* til1, const float* til2, const float* lse, const float* delta, int B, int own_len,
                int til_len, int H, float scale2, float out_scale, float* out1, float* out2, float* lse_out, hipStream_t stream) {
  const dim3 grid(opp_cdiv(own_len, kRows), H, B);
  hipLaunchKernelGGL((fat_tile_kernel<PREC, MODE>), grid, dim3(256), 0, stream, own1, own2, til1, til2, lse, delta, own_len, til_len, H, scale2,
                     out_scale, out1, out2, lse_out);
  OPP_CHECK_LAUNCH("fat_tile_kernel");
  return OPP_OK;
}

int check(const char* what, int B, int L, int S, int H, int D, int prec, int* fam) {
  OPP_CHECK_ARG(B > 0 && L > 0 && S > 0 && H > 0, "%s: bad shape", what);
  *fam = (prec == OPP_PREC_FP32 || prec == OPP_PREC_BF16X3) ? family(B, L, S, H, D) : FAM_NONE;
  if (*fam == FAM_NONE) {
    opp_set_error("%s: B %d, L %d, S %d, nhead %d, D %d, arithmetic %d is not supported (D 32, or D 16 with both streams <= 64 rows; "
                  "B <= 65535; fp32 or bf16x3)", what, B, L, S, H, D, prec);
    return OPP_ERR_UNSUPPORTED;
  }
  return OPP_OK;
}

}  // namespace

size_t opp_fullattn_train_ws_bytes(int B, int L, int S, int H, int D) {
  if (family(B, L, S, H, D) == FAM_NONE) return 0;
  return opp_align((size_t)B * H * L * sizeof(float)) + 256;   // delta
}

int opp_fullattn_train_fwd(const float* q, const float* k, const float* v, int B, int L, int S, int H, int D, int prec, float* out, float* lse,
                           hipStream_t stream) {
  int fam;
  OPP_TRY(check("full_attention_train_forward", B, L, S, H, D, prec, &fam));
  OPP_CHECK_ARG(q && k && v && out && lse, "full_attention_train_forward: null argument");
  OPP_CHECK_ARG(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out), "full_attention_train_forward: operands must be 16-byte aligned");
  const float scale2 = kLog2e / sqrtf((float)D);
  if (fam == FAM_SMALL) {
    const dim3 grid(B, H);
    if (D == 16) hipLaunchKernelGGL((fat_small_fwd_kernel<16>), grid, dim3(128), 0, stream, q, k, v, L, S, H, scale2, out, lse);
    else hipLaunchKernelGGL((fat_small_fwd_kernel<32>), grid, dim3(128), 0, stream, q, k, v, L, S, H, scale2, out, lse);
    OPP_CHECK_LAUNCH("fat_small_fwd_kernel");
    return OPP_OK;
  }
  if (prec == OPP_PREC_BF16X3)
    return launch_tile<OPP_PREC_BF16X3, MODE_FWD>(q, nullptr, k, v, nullptr, nullptr, B, L, S, H, scale2, 1.f, out, nullptr, lse, stream);
  return launch_tile<OPP_PREC_FP32, MODE_FWD>(q, nullptr, k, v, nullptr, nullptr, B, L, S, H, scale2, 1.f, out, nullptr, lse, stream);
}

int opp_fullattn_train_bwd(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* go, int B, int L,
                           int S, int H, int D, int prec, float* gq, float* gk, float* gv, void* ws, size_t ws_bytes, hipStream_t stream) {
  int fam;
  OPP_TRY(check("full_attention_train_backward", B, L, S, H, D, prec, &fam));
  OPP_CHECK_ARG(q && k && v && out && lse && go && gq && gk && gv, "full_attention_train_backward: null argument");
  OPP_CHECK_ARG(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) && aligned16(go) && aligned16(gq) && aligned16(gk) && aligned16(gv),
                "full_attention_train_backward: operands must be 16-byte aligned");
  const float scale2 = kLog2e / sqrtf((float)D), sc = 1.f / sqrtf((float)D);
  // asked of every supported shape, as the size query reports it (the vector kernels of the short streams leave it untouched)
  if (!ws || ws_bytes < opp_fullattn_train_ws_bytes(B, L, S, H, D) || !aligned16(ws)) {
    opp_set_error("full_attention_train_backward: workspace too small");
    return OPP_ERR_WORKSPACE;
  }
  if (fam == FAM_SMALL) {
    const dim3 grid(B, H);
    if (D == 16) hipLaunchKernelGGL((fat_small_bwd_kernel<16>), grid, dim3(256), 0, stream, q, k, v, lse, go, L, S, H, scale2, sc, gq, gk, gv);
    else hipLaunchKernelGGL((fat_small_bwd_kernel<32>), grid, dim3(256), 0, stream, q, k, v, lse, go, L, S, H, scale2, sc, gq, gk, gv);
    OPP_CHECK_LAUNCH("fat_small_bwd_kernel");
    return OPP_OK;
  }
  float* delta = reinterpret_cast<float*>(ws);
  const size_t n = (size_t)B * L * H;
  hipLaunchKernelGGL((fat_delta_kernel<kD>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, go, out, L, H, n, delta);
  OPP_CHECK_LAUNCH("fat_delta_kernel");
  if (prec == OPP_PREC_BF16X3) {
    OPP_TRY((launch_tile<OPP_PREC_BF16X3, MODE_DKV>(k, v, q, go, lse, delta, B, S, L, H, scale2, sc, gk, gv, nullptr, stream)));
    return launch_tile<OPP_PREC_BF16X3, MODE_DQ>(q, go, k, v, lse, delta, B, L, S, H, scale2, sc, gq, nullptr, nullptr, stream);
  }
  OPP_TRY((launch_tile<OPP_PREC_FP32, MODE_DKV>(k, v, q, go, lse, delta, B, S, L, H, scale2, sc, gk, gv, nullptr, stream)));
  return launch_tile<OPP_PREC_FP32, MODE_DQ>(q, go, k, v, lse, delta, B, L, S, H, scale2, sc, gq, nullptr, nullptr, stream);
}
