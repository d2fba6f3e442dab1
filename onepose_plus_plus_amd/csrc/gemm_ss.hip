// "split-split" GEMM for gfx950: BOTH operands arrive pre-split in memory in the bf16x3 form
// (x = hi + mid + lo bf16 exactly; every 8 consecutive k = 48 B [hi x8 | mid x8 | lo x8], opp_pack_b3), so the K loop has no
// conversion arithmetic, no VGPR staging and no LDS stores: the operand tiles go global -> LDS with
// buffer_load_dwordx4 ... lds (LDS-DMA).
//
// Structure (MI355X-first): a workgroup is FOUR waves (one per SIMD) on a 128 x 128 tile, 64 x 64 per wave; a stage is one
// k16-step (96 B per tile row) in an LDS slot of 24 KB.  Per stage and wave: 24 MFMAs (six bf16 products per 32 x 32 x 16
// block, fp32 accumulate, the accumulation sequence of opp_gemm_kernel<bf16x3>), 12 ds_read_b128 of fragments, 6 LDS-DMA
// instructions issued between the MFMAs, ONE raw s_barrier with explicit vmcnt / lgkmcnt counts (a __syncthreads() would
// drain the DMA queue).
//
// LDS image: a tile row of one stage is 96 B = 6 pieces of 16 B (2 k-groups x {hi, mid, lo}).  LDS-DMA writes lane-linearly
// (wave-uniform base + lane * 16), so the image is plain row-major [row][6 pieces], no padding; the bank-conflict-free
// fragment reads come from a rotation applied on the SOURCE side: position pos of row r holds global piece
// (pos + 3 * ((r >> 3) & 1)) mod 6.  The 16 rows of a ds_read_b128 lane group then fall on 16 distinct 4-bank groups
// ((6 r + pos) mod 16 runs over the 8 even residues for the rows with bit 3 clear and the 8 odd ones for the others).
//
// First user: the coarse score matrix and its dual softmax (utils/coarse_matching.py:99-115, :145-172) in TWO SWEEPS of the
// same GEMM instead of GEMM + in-place softmax passes over the materialised N x L matrix:
//   sweep 1 (OPP_SS_STATS): the score tile lives only in the accumulators; its (max, sum exp) per tile row and tile column
//                           leave as partials (merged by the small kernels of coarse_match.hip);
//   sweep 2 (OPP_SS_CONF):  the tile is recomputed (bit-identical: same instruction sequence), turned into
//                           conf = softmax_col * softmax_row with the merged statistics and written ONCE; the maxima the
//                           mutual-nearest-neighbour test needs leave as per-tile partials.
// or in one sweep (OPP_SS_STATS_STORE): the statistics and the score tile itself; conf is then formed in place by conf_reg_kernel.
// The kernel's M dimension is the IMAGE CELL and its N dimension (MFMA lanes) the 3D POINT: a lane then holds four
// consecutive cells of one point per accumulator quad, i.e. 16 contiguous bytes of conf[point][cell].
// HBM traffic of the whole stage: one 82 MB write (N = 5000, L = 4096) instead of write + read + write (246 MB).
//
// Organisation: the pieces every kernel is made of -- tile order, tile setup (LDS-DMA source offsets), DMA item, fragment reads,
// the 24-MFMA product block, scaling / masking, column statistics, staged stores, the half-staged statistics epilogue -- are
// stated once as force-inlined functions (ss_*); the three kernels behind them say only what differs: how many LDS slots, which
// slot a stage lands in, what is issued behind which MFMA, and what happens between two tiles.
#include <stdlib.h>

#include <type_traits>

#include "opp_internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr unsigned kOob = 0x80000000u;
constexpr int BM = 128, BN = 128, WM = 2, WN = 2, NT = 256, TM = 2, TN = 2;
constexpr int ROWB = 96;                              // bytes per tile row and stage (one k16-step)
constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, SLOT = A_BYTES + B_BYTES, NS = 3;
constexpr int A_LD = BM * 6 / NT, B_LD = BN * 6 / NT; // LDS-DMA instructions per wave and stage
constexpr int LPS = A_LD + B_LD;
constexpr int TS = BM + 4;                            // row stride (floats) of a tile staged through LDS as T[col][row]
constexpr int HC = BN / 2;                            // columns per staged half (half-staged epilogue)
constexpr int MISC = 4096;                            // statistics scratch of the half-staged epilogue: never aliases the slots
static_assert(HC * TS * 4 <= 2 * SLOT, "a staged half tile must fit two operand slots");

// x / d for a loop-invariant divisor d with rd = RN(1 / d): q = RN(x rd), then one exact-remainder correction -- the
// correctly rounded quotient (Markstein), three FMAs instead of the ten-instruction IEEE division sequence
__device__ __forceinline__ float div_invariant(float x, float d, float rd) {
  const float q = x * rd;
  const float rem = fmaf(-q, d, x);
  return fmaf(rem, rd, q);
}
// v_max via inline asm: fmaxf() costs an extra canonicalising v_max per operand here
__device__ __forceinline__ float vmax(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// ---- tile order ---------------------------------------------------------------------------------------------------------------------
// XCD-aware (workgroup b runs on XCD b % 8; speed only -- every output is indexed by tile coordinates): an XCD gets a contiguous range
// of a linear order that walks STRIPS of RS row panels column by column (row fastest).  The ~64 tiles an XCD has in flight then cover
// RS row panels x 8 column panels = 16 operand panels of 192 KB (3 MB of its 4 MB L2), every column panel is fetched once per strip and
// XCD instead of once per row panel (row-major order: each XCD streamed all 40 column panels four times at 4096 x 5000).
// ss_xcd_first: where the range of XCD b % 8 begins when `count` items are dealt to the eight XCDs
__device__ __forceinline__ int ss_xcd_first(int b, int count) {
  const int q = count >> 3, r = count & 7, xcd = b & 7;
  return xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
}
// the tile of this workgroup in a one-tile-per-workgroup grid
__device__ __forceinline__ int ss_tile_lin() { return ss_xcd_first(blockIdx.x, gridDim.x) + (blockIdx.x >> 3); }
__device__ __forceinline__ void ss_strip_tile(int tile_lin, int tiles_m, int tiles_n, int& tile_m, int& tile_n) {
  constexpr int RS = 8;
  const int strip = tile_lin / (RS * tiles_n);
  const int within = tile_lin - strip * (RS * tiles_n);
  const int strip_rows = min(RS, tiles_m - strip * RS);
  tile_n = within / strip_rows;
  tile_m = strip * RS + (within - tile_n * strip_rows);
}

// ---- a thread's place in the tile: wave (wm, wn) owns 64 x 64, lane = (column l31, row group half) of each 32 x 32 block --------------
struct SsCoord {
  int wave, wm, wn, half, l31;
  __device__ __forceinline__ int row_of(int i, int r) const { return wm * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half; }   // tile row of acc[i][.][r]
  __device__ __forceinline__ int quad_row(int i, int q4) const { return wm * TM * 32 + i * 32 + 8 * q4 + 4 * half; }                                 // first of the four rows of quad q4
  __device__ __forceinline__ int col_of(int j) const { return wn * TN * 32 + j * 32 + l31; }                                       // tile column of acc[.][j][.]
};
__device__ __forceinline__ SsCoord ss_coord(int wave, int tid) {
  SsCoord c;
  c.wave = wave;
  c.wm = c.wave / WN;
  c.wn = c.wave % WN;
  c.half = (tid >> 5) & 1;
  c.l31 = tid & 31;
  return c;
}

// ---- tile setup: LDS-DMA instruction n of a tile covers linear pieces [64 n, 64 n + 64) of the [rows][6] image --------------------------
struct SsTile {
  unsigned a_voff[A_LD], b_voff[B_LD];
  int soffA0, soffB0, m0, n0, tile_m, tile_n;
};
// source offset of piece P of an operand tile (the rotation of the header); rows past the operand's end read nothing
__device__ __forceinline__ unsigned ss_src_voff(int P, int row0, int rows, int ld) {
  const int row = P / 6, pos = P - row * 6;
  const int q = (pos + 3 * ((row >> 3) & 1)) % 6;
  return row0 + row < rows ? (unsigned)(row * ld + q * 16) : kOob;
}
__device__ __forceinline__ SsTile ss_tile_setup(const OppGemmSS& g, int tile_m, int tile_n, int wave, int lane) {
  SsTile t;
  t.tile_m = tile_m;
  t.tile_n = tile_n;
  t.m0 = tile_m * BM;
  t.n0 = tile_n * BN;
#pragma unroll
  for (int i = 0; i < A_LD; ++i) t.a_voff[i] = ss_src_voff((wave * A_LD + i) * 64 + lane, t.m0, g.M, g.lda);
#pragma unroll
  for (int i = 0; i < B_LD; ++i) t.b_voff[i] = ss_src_voff((wave * B_LD + i) * 64 + lane, t.n0, g.N, g.ldb);
  t.soffA0 = t.m0 * g.lda;
  t.soffB0 = t.n0 * g.ldb;
  return t;
}
// item k of stage s (k < LPS) into the slot at slot_base: one buffer_load_dwordx4 ... lds.  live = false (stages past the end of K): a
// zero-sized buffer (one s_cselect on the wave-uniform descriptor), the instruction still counts in vmcnt, so the loops have no branches
__device__ __forceinline__ void ss_dma_item(const OppGemmSS& g, const SsTile& t, char* slot_base, int s, int k, bool live, int wave) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  if (k < A_LD) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.A), 0, live ? g.a_bytes : 0, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(slot_base + (wave * A_LD + k) * 1024), 16, (int)t.a_voff[k], t.soffA0 + s * ROWB, 0, 0);
  } else {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.B), 0, live ? g.b_bytes : 0, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(slot_base + A_BYTES + (wave * B_LD + (k - A_LD)) * 1024), 16, (int)t.b_voff[k - A_LD],
                                             t.soffB0 + s * ROWB, 0, 0);
  }
}
__device__ __forceinline__ void ss_dma_stage(const OppGemmSS& g, const SsTile& t, char* slot_base, int s, bool live, int wave) {
#pragma unroll
  for (int k = 0; k < LPS; ++k) ss_dma_item(g, t, slot_base, s, k, live, wave);
}

// ---- fragments: lane (row l31, k-group = half) reads parts hi / mid / lo = global pieces 3 half + p ------------------------------------
struct SsFragAddr {
  int foff[3], a_row, b_row;
};
__device__ __forceinline__ SsFragAddr ss_frag_addr(const SsCoord& c) {
  SsFragAddr f;
  const int b3 = (c.l31 >> 3) & 1;
#pragma unroll
  for (int p = 0; p < 3; ++p) f.foff[p] = 16 * ((3 * c.half + p + 3 * b3) % 6);
  f.a_row = (c.wm * TM * 32 + c.l31) * ROWB;
  f.b_row = A_BYTES + (c.wn * TN * 32 + c.l31) * ROWB;
  return f;
}
__device__ __forceinline__ void ss_read_frags(const char* base, const SsFragAddr& f, u32x4 (&fa)[TM][3], u32x4 (&fb)[TN][3]) {
#pragma unroll
  for (int p = 0; p < 3; ++p) {
#pragma unroll
    for (int i = 0; i < TM; ++i) fa[i][p] = *reinterpret_cast<const u32x4*>(base + f.a_row + i * 32 * ROWB + f.foff[p]);
#pragma unroll
    for (int j = 0; j < TN; ++j) fb[j][p] = *reinterpret_cast<const u32x4*>(base + f.b_row + j * 32 * ROWB + f.foff[p]);
  }
}
__device__ __forceinline__ void ss_zero(f32x16 (&acc)[TM][TN]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}
// the 24 MFMAs of one stage -- THE accumulation sequence: every bit-identity claim of the matcher rests on it.  after(n) runs behind MFMA n
template <class F>
__device__ __forceinline__ void ss_products(const u32x4 (&fa)[TM][3], const u32x4 (&fb)[TN][3], f32x16 (&acc)[TM][TN], F after) {
  constexpr int PA[6] = {2, 0, 1, 1, 0, 0};   // A part of product pr (0 hi, 1 mid, 2 lo), smallest terms first
  constexpr int PB[6] = {0, 2, 1, 0, 1, 0};
  int n = 0;
#pragma unroll
  for (int pr = 0; pr < 6; ++pr)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[i][PA[pr]]), __builtin_bit_cast(bf16x8, fb[j][PB[pr]]),
                                                             acc[i][j], 0, 0, 0);
        after(n);
        ++n;
      }
}
// ---- epilogue pieces ------------------------------------------------------------------------------------------------------------------
// v = acc * out_mul / out_div, the reference's order of operations (feature scaling, then the temperature division); masked image cells:
// sim += -1e9 (coarse_matching.py:108-114); cells = kernel rows
__device__ __forceinline__ void ss_scale_and_mask(const OppGemmSS& g, f32x16 (&acc)[TM][TN], int m0, const SsCoord& c) {
  if ((g.out_mul != 1.f) || (g.out_div != 1.f)) {
    const float rd = 1.0f / g.out_div;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = div_invariant(acc[i][j][r] * g.out_mul, g.out_div, rd);
  }
  if (g.row_mask != nullptr) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float mk = g.row_mask[min(m0 + c.row_of(i, r), g.M - 1)];      // (rows past M are never used)
        const float add = mk == 0.f ? -1e9f : 0.f;
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j][r] += add;
      }
  }
}
// max / sum exp(v - cmx) of column block j over this wave's 64 rows, from the accumulators (both wave halves hold the result).  Every partial
// is a fixed-order function of the column's values only, so duplicated columns get bit-equal statistics wherever they sit
template <bool FULL>
__device__ __forceinline__ float ss_col_max(const f32x16 (&acc)[TM][TN], const SsCoord& c, int nrows, int j) {
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) m = vmax(m, (FULL || c.row_of(i, r) < nrows) ? acc[i][j][r] : -INFINITY);
  return vmax(m, __shfl_xor(m, 32, 64));
}
template <bool FULL>
__device__ __forceinline__ float ss_col_sumexp(const f32x16 (&acc)[TM][TN], const SsCoord& c, int nrows, int j, float cmx) {
  float sm = 0.f;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) sm += (FULL || c.row_of(i, r) < nrows) ? __expf(acc[i][j][r] - cmx) : 0.f;
  return sm + __shfl_xor(sm, 32, 64);
}
// column maxima of the tile from the per-wave-row partials red[WM][BN], and their way out
__device__ __forceinline__ void ss_col_max_merge(const SsCoord& c, const float* red, float (&cmx)[TN]) {
#pragma unroll
  for (int j = 0; j < TN; ++j) cmx[j] = vmax(red[c.col_of(j)], red[BN + c.col_of(j)]);
}
__device__ __forceinline__ void ss_put_col_max(const OppGemmSS& g, const SsTile& t, const SsCoord& c, int ncols, const float (&cmx)[TN]) {
  if (c.wm == 0 && c.half == 0) {
#pragma unroll
    for (int j = 0; j < TN; ++j)
      if (c.col_of(j) < ncols) g.stat_colmax[(size_t)t.tile_m * g.N + t.n0 + c.col_of(j)] = cmx[j];
  }
}
// the accumulators -> T[col][row] (a lane's accumulator quad = four consecutive rows of one column = one ds_write_b128); col0: tile column
// of this wave's first column minus the first staged column
__device__ __forceinline__ void ss_stage_acc(float* T, const f32x16 (&acc)[TM][TN], const SsCoord& c, int col0) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int col = col0 + j * 32 + c.l31, row = c.quad_row(i, q4);
        *reinterpret_cast<float4*>(T + col * TS + row) = make_float4(acc[i][j][4 * q4], acc[i][j][4 * q4 + 1], acc[i][j][4 * q4 + 2], acc[i][j][4 * q4 + 3]);
      }
}
// COLS staged columns (tile columns first_col ...) leave: lane = 16 bytes of a row of out[col][row], fully coalesced (a wave writes two
// 512-byte rows per instruction); needs 16-byte aligned output rows (g.vec_store).  (Scalars by reference, like the captures of a closure: the
// loop is then simplified in its caller's context, not on its own -- by value the three-resident kernel spills 28 bytes instead of 12)
template <bool FULL, int COLS>
__device__ __forceinline__ void ss_store_staged(const OppGemmSS& g, const SsTile& t, const float* const& T, const int& first_col, const int& tid,
                                                const int& nrows, const int& ncols) {
#pragma unroll
  for (int it = 0; it < COLS * (BM / 4) / NT; ++it) {
    const int u = tid + it * NT;
    const int col = u / (BM / 4), r4 = (u - col * (BM / 4)) * 4;
    const int gc = first_col + col;
    if (FULL || (gc < ncols && r4 + 3 < nrows)) {
      *reinterpret_cast<float4*>(g.C + (size_t)(t.n0 + gc) * g.ldc + t.m0 + r4) = *reinterpret_cast<const float4*>(T + col * TS + r4);
    } else if (gc < ncols) {
      for (int e = 0; e < 4; ++e)
        if (r4 + e < nrows) g.C[(size_t)(t.n0 + gc) * g.ldc + t.m0 + r4 + e] = T[col * TS + r4 + e];
    }
  }
}
// the whole staged tile leaves, by whichever stores the output's alignment allows
template <bool FULL>
__device__ __forceinline__ void ss_store_tile(const OppGemmSS& g, const SsTile& t, const float* T, int tid, int nrows, int ncols) {
  if (g.vec_store) {
    ss_store_staged<FULL, BN>(g, t, T, 0, tid, nrows, ncols);
  } else {
    for (int u = tid; u < BN * BM; u += NT) {
      const int col = u / BM, r = u - col * BM;
      if (col < ncols && r < nrows) g.C[(size_t)(t.n0 + col) * g.ldc + t.m0 + r] = T[col * TS + r];
    }
  }
}
__device__ __forceinline__ bool ss_tile_extent(const OppGemmSS& g, const SsTile& t, int& nrows, int& ncols) {
  nrows = min(BM, g.M - t.m0);
  ncols = min(BN, g.N - t.n0);
  return nrows == BM && ncols == BN;      // wave-uniform: interior tiles skip every validity select
}

// Statistics + score tile with HALF of the tile staged at a time (persistent and three-resident kernels): 33 KB of LDS at the slots' start
// instead of 66, the statistics scratch (4 KB at `misc`) never aliases the slots.  The per-row statistics (max, sum exp) of the two halves are
// merged online in the registers of the thread that owns the row (fixed order: a function of the row's values only -- duplicated rows get
// bit-equal statistics).  after_slots_dead() runs once every operand slot is dead, after_halves() once the staged halves are consumed.
// te / e: the thread index and its coordinates, re-derived by the caller from an opaque copy (see the call sites).
// Returns the epilogue as a closure over the caller's variables, to be called with std::true_type for an interior tile: everything is
// taken by reference and must outlive the call.  (As a plain function of values it is simplified before it meets its kernel; at the 168
// registers of the three-resident kernel that moved the spills from 12 bytes to 16-28 in every form tried.)
// (guard of the closure below: an argument that is a temporary would dangle)
template <class... A, std::enable_if_t<(... || std::is_rvalue_reference_v<A&&>), int> = 0>
void ss_half_staged_stats(A&&...) = delete;
template <class F1, class F2>
__device__ __forceinline__ auto ss_half_staged_stats(const OppGemmSS& g, const SsTile& t, char* const& smem, char* const& misc, const int& te, const SsCoord& e,
                                                     const int& nrows, const int& ncols, const int& tiles_n, const f32x16 (&acc)[TM][TN],
                                                     const F1& after_slots_dead, const F2& after_halves) {
  return [&](auto full_c) {
    constexpr bool FULL = decltype(full_c)::value;
    float* T = reinterpret_cast<float*>(smem);                                  // [HC][TS]
    float* red_cmax = reinterpret_cast<float*>(misc);                           // [WM][BN]
    float* red_csum = red_cmax + WM * BN;                                       // [WM][BN]
    float* red_rm = red_csum + WM * BN;                                         // [2][BM]
    float* red_rs = red_rm + 2 * BM;                                            // [2][BM]
    constexpr int CPS = HC / 2;
    const int e_rrow = te & (BM - 1), e_rsub = te >> 7;                         // row pass: thread = (row, half of the staged columns)
    const int m0 = t.m0, n0 = t.n0;
    float cmx[TN], csm[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const float m = ss_col_max<FULL>(acc, e, nrows, j);
      if (e.half == 0) red_cmax[e.wm * BN + e.col_of(j)] = m;
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                 // the zero-sized tail DMAs and the last fragment reads
    __syncthreads();                                                             // every slot is dead; the column maxima are visible
    after_slots_dead();
    ss_col_max_merge(e, red_cmax, cmx);
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      csm[j] = ss_col_sumexp<FULL>(acc, e, nrows, j, cmx[j]);
      if (e.half == 0) red_csum[e.wm * BN + e.col_of(j)] = csm[j];
    }
    ss_put_col_max(g, t, e, ncols, cmx);
    // rows: the tile is staged 64 columns at a time; the thread (row, 32 columns) keeps a running (max, sum exp) of its row
    float RM = -INFINITY, RSUM = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (e.wn == h) ss_stage_acc(T, acc, e, 0);
      __syncthreads();
      {
        const int c0 = e_rsub * CPS;
        float rv[CPS];
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < CPS; ++c) {
          rv[c] = T[(c0 + c) * TS + e_rrow];
          m = vmax(m, (FULL || h * HC + c0 + c < ncols) ? rv[c] : -INFINITY);
        }
        float sacc = 0.f;
#pragma unroll
        for (int c = 0; c < CPS; ++c) sacc += (FULL || h * HC + c0 + c < ncols) ? __expf(rv[c] - m) : 0.f;
        // online merge, fixed order (half 0 then half 1): exp(-inf - finite) = 0 covers the empty side
        const float M2 = vmax(RM, m);
        if (FULL || M2 > -INFINITY) RSUM = RSUM * __expf(RM - M2) + sacc * __expf(m - M2);
        RM = M2;
      }
      ss_store_staged<FULL, HC>(g, t, T, h * HC, te, nrows, ncols);             // (the launcher takes these kernels for 16-byte aligned outputs only)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __syncthreads();                                                           // the staged half is consumed
    }
    after_halves();
    red_rm[e_rsub * BM + e_rrow] = RM;
    red_rs[e_rsub * BM + e_rrow] = RSUM;
    __syncthreads();
    if (te < BM) {
      if (te < nrows) {
        const float ma = red_rm[te], mb = red_rm[BM + te];
        const float M2 = vmax(ma, mb);
        const size_t o = (size_t)(m0 + te) * tiles_n + t.tile_n;
        g.stat_rowmax[o] = M2;
        g.stat_rowsum[o] = red_rs[te] * __expf(ma - M2) + red_rs[BM + te] * __expf(mb - M2);
      }
    } else if (te - BM < ncols) {
      const int u = te - BM;
      g.stat_colsum[(size_t)t.tile_m * g.N + n0 + u] = red_csum[u] + red_csum[BN + u];
    }
  };
}

#ifdef OPP_TUNING
// tuning builds: 4 shader-clock stamps per wave (start, K loop entered, K loop left, now) in block `index` of g.dbg_ts; with `placement`
// wave 1 reports where the workgroup ran instead of its start stamp
__device__ __forceinline__ void ss_write_stamps(const OppGemmSS& g, size_t index, int wave, int lane, bool placement, unsigned long long ts0,
                                                unsigned long long ts1, unsigned long long ts2) {
  if (g.dbg_ts != nullptr && lane == 0) {
    unsigned long long* o = g.dbg_ts + (index * 4 + wave) * 4;
    unsigned hw = 0, xcc = 0;
    if (placement) {
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    }
    o[0] = placement && wave == 1 ? (((unsigned long long)xcc << 32) | hw) : ts0;
    o[1] = ts1;
    o[2] = ts2;
    o[3] = __builtin_readcyclecounter();
  }
}
#endif

// ---- whole-tile epilogues of the two-resident kernel: the tile is staged once as T[col][row] (66 KB of the 72 KB, small cross-wave scratch
// behind it); the per-column quantities are in-register reductions over the lane's own 64 values, the per-row ones a loop over the columns
// with lane = row (consecutive LDS addresses), and nothing needs a cross-lane butterfly -------------------------------------------------------
constexpr int CPP = BN / 2;                                 // row pass: thread = (row, half of the columns)

// (max, sum exp(v - max)) of the tile per row (over its columns, two parts against their common maximum) and per column (over its rows);
// STORE: the score tile itself leaves as well
template <bool STORE, bool FULL>
__device__ __forceinline__ void ss_whole_tile_stats(const OppGemmSS& g, const SsTile& t, float* T, int tid, const SsCoord& c, int nrows, int ncols,
                                                    int tiles_n, const f32x16 (&acc)[TM][TN]) {
  float* red_r = T + BN * TS;           // [2][BM]
  float* red_c = red_r + 2 * BM;        // [WM][BN]
  const int rrow = tid & (BM - 1), rpart = tid >> 7;
  ss_stage_acc(T, acc, c, c.wn * TN * 32);
  float cmx[TN], csm[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const float m = ss_col_max<FULL>(acc, c, nrows, j);
    if (c.half == 0) red_c[c.wm * BN + c.col_of(j)] = m;
  }
  __syncthreads();
  // rows, from the staged tile: max over this part's columns
  const int c0 = rpart * CPP, c1 = FULL ? c0 + CPP : min(c0 + CPP, ncols);
  float rv[CPP];
  float rm = -INFINITY;
#pragma unroll
  for (int cc = 0; cc < CPP; ++cc) {
    rv[cc] = T[(c0 + cc) * TS + rrow];
    rm = vmax(rm, (FULL || c0 + cc < c1) ? rv[cc] : -INFINITY);
  }
  red_r[rpart * BM + rrow] = rm;
  ss_col_max_merge(c, red_c, cmx);
  __syncthreads();
  rm = vmax(red_r[rrow], red_r[BM + rrow]);
  float rs = 0.f;
#pragma unroll
  for (int cc = 0; cc < CPP; ++cc) rs += (FULL || c0 + cc < c1) ? __expf(rv[cc] - rm) : 0.f;
#pragma unroll
  for (int j = 0; j < TN; ++j) csm[j] = ss_col_sumexp<FULL>(acc, c, nrows, j, cmx[j]);
  if constexpr (STORE) ss_store_tile<FULL>(g, t, T, tid, nrows, ncols);   // (single-sweep matcher: conf is formed in place by conf_reg_kernel)
  __syncthreads();                       // red_r / red_c maxima consumed
  red_r[rpart * BM + rrow] = rs;
  if (c.half == 0) {
#pragma unroll
    for (int j = 0; j < TN; ++j) red_c[c.wm * BN + c.col_of(j)] = csm[j];
  }
  ss_put_col_max(g, t, c, ncols, cmx);
  __syncthreads();
  if (tid < BM) {
    if (tid < nrows) {
      const size_t o = (size_t)(t.m0 + tid) * tiles_n + t.tile_n;
      g.stat_rowmax[o] = rm;
      g.stat_rowsum[o] = red_r[tid] + red_r[BM + tid];
    }
  } else if (tid - BM < ncols) {
    const int u = tid - BM;
    g.stat_colsum[(size_t)t.tile_m * g.N + t.n0 + u] = red_c[u] + red_c[BN + u];
  }
}

// conf tile from the merged statistics, staged as T[col][row] = conf[point][cell] row-major.  Per column (point): best confidence / first
// row (cell) holding it / how many rows hold it; per row (cell): max over the columns
template <bool FULL>
__device__ __forceinline__ void ss_conf_tile(const OppGemmSS& g, const SsTile& t, float* T, int tid, const SsCoord& c, int nrows, int ncols, int tiles_n,
                                             const f32x16 (&acc_in)[TM][TN]) {
  f32x16 acc[TM][TN];                                 // scores in, confidences out: a copy of its own (in the caller's registers: 480 more moves)
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = acc_in[i][j];
  float* s_rm = T + BN * TS;                          // [BM] row statistic: max
  float* s_rr = s_rm + BM;                            // [BM] row statistic: 1 / sum (v_rcp, as conf_value() of coarse_match.hip)
  float* p_best = s_rm + 2 * BM;                      // [WM][BN]
  int* p_arg = reinterpret_cast<int*>(p_best + WM * BN);
  int* p_ties = p_arg + WM * BN;
  unsigned* red_r = reinterpret_cast<unsigned*>(p_ties + WM * BN);   // [2][BM]
  const int rrow = tid & (BM - 1), rpart = tid >> 7;
  const int m0 = t.m0, n0 = t.n0;
  if (tid < BM) {
    const bool ok = tid < nrows;
    s_rm[tid] = ok ? g.rstat_max[m0 + tid] : 0.f;
    s_rr[tid] = ok ? __frcp_rn(g.rstat_sum[m0 + tid]) : 0.f;
  }
  float cm[TN], crs[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + c.col_of(j);
    const bool ok = col < g.N;
    cm[j] = ok ? g.cstat_max[col] : 0.f;
    crs[j] = ok ? 1.0f / g.cstat_sum[col] : 0.f;
  }
  __syncthreads();
  float best[TN];
  int arg[TN], ties[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    best[j] = -1.f;
    arg[j] = 0x7fffffff;
    ties[j] = 0;
  }
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int lr0 = c.quad_row(i, q4);       // 4 consecutive tile rows: r = 4 q4 + e
      const float4 rm4 = *reinterpret_cast<const float4*>(s_rm + lr0);
      const float4 rr4 = *reinterpret_cast<const float4*>(s_rr + lr0);
      const float rm[4] = {rm4.x, rm4.y, rm4.z, rm4.w}, rr[4] = {rr4.x, rr4.y, rr4.z, rr4.w};
#pragma unroll
      for (int j = 0; j < TN; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          // exp((v - cellmax) + (v - pointmax)) * (1 / cellsum * 1 / pointsum): conf_value() of coarse_match.hip
          const float cf = __expf((acc[i][j][4 * q4 + e] - rm[e]) + (acc[i][j][4 * q4 + e] - cm[j])) * (rr[e] * crs[j]);
          acc[i][j][4 * q4 + e] = cf;
          if (FULL || lr0 + e < nrows) {     // (invalid columns are never written out)
            if (cf > best[j]) {
              best[j] = cf;
              arg[j] = lr0 + e;
              ties[j] = 1;
            } else if (cf == best[j]) {
              ++ties[j];
            }
          }
        }
      }
    }
  ss_stage_acc(T, acc, c, c.wn * TN * 32);
  // the other wave half holds the interleaved rows (4 half + 0..3 of every 8): combine, lowest row wins a tie
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const float ob = __shfl_xor(best[j], 32, 64);
    const int oa = __shfl_xor(arg[j], 32, 64), ot = __shfl_xor(ties[j], 32, 64);
    if (ob > best[j]) {
      best[j] = ob;
      arg[j] = oa;
      ties[j] = ot;
    } else if (ob == best[j]) {
      ties[j] += ot;
      arg[j] = min(arg[j], oa);
    }
    if (c.half == 0) {
      const int u = c.wm * BN + c.col_of(j);
      p_best[u] = best[j];
      p_arg[u] = arg[j];
      p_ties[u] = ties[j];
    }
  }
  __syncthreads();
  // rows (cells): max over this part's columns; confidences are >= +0, so the unsigned max of the bit patterns is the max
  {
    const int c0 = rpart * CPP, c1 = FULL ? c0 + CPP : min(c0 + CPP, ncols);
    const unsigned* Tu = reinterpret_cast<const unsigned*>(T);
    unsigned m = 0u;
#pragma unroll
    for (int cc = 0; cc < CPP; ++cc) {
      const unsigned v = Tu[(c0 + cc) * TS + rrow];
      m = max(m, (FULL || c0 + cc < c1) ? v : 0u);
    }
    red_r[rpart * BM + rrow] = m;
  }
  ss_store_tile<FULL>(g, t, T, tid, nrows, ncols);
  __syncthreads();
  if (tid < BN) {
    if (tid < ncols) {      // wave rows 0 / 1 in ascending row order: ties keep the lowest row
      float b = p_best[tid];
      int a = p_arg[tid], n = p_ties[tid];
      const float ob = p_best[BN + tid];
      if (ob > b) {
        b = ob;
        a = p_arg[BN + tid];
        n = p_ties[BN + tid];
      } else if (ob == b) {
        n += p_ties[BN + tid];
      }
      const size_t o = (size_t)t.tile_m * g.N + n0 + tid;
      g.part_best[o] = b;
      g.part_arg[o] = m0 + a;
      g.part_ties[o] = n;
    }
  } else if (tid - BN < nrows) {
    const int u = tid - BN;
    g.part_rowmax[(size_t)(m0 + u) * tiles_n + t.tile_n] = __uint_as_float(max(red_r[u], red_r[BM + u]));
  }
}

// ---- two residents per CU: one tile per workgroup, three LDS slots = 72 KB.  While one workgroup is in its prologue / epilogue (global
// latency, VALU-heavy statistics, stores) the other's MFMAs own the matrix pipes -- the overlap a single 8-wave workgroup per CU cannot have.
// Stage s lives in slot s % 3; the fragments of stage s + 1 are read and stage s + 3 is fetched under the MFMAs of stage s ---------------------
template <int MODE>
__global__ __launch_bounds__(NT, 2) void gemm_ss_kernel(const OppGemmSS g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
#ifdef OPP_TUNING
  const unsigned long long ts0 = __builtin_readcyclecounter();
  unsigned long long ts1 = 0, ts2 = 0;
#endif
  const int tid = threadIdx.x, lane = tid & 63;
  const SsCoord c = ss_coord(__builtin_amdgcn_readfirstlane(tid >> 6), tid);
  const int tiles_n = (g.N + BN - 1) / BN, tiles_m = (g.M + BM - 1) / BM;
  int tile_m, tile_n;
  ss_strip_tile(ss_tile_lin(), tiles_m, tiles_n, tile_m, tile_n);
  const SsTile t = ss_tile_setup(g, tile_m, tile_n, c.wave, lane);
  const SsFragAddr fr = ss_frag_addr(c);
  u32x4 fa[2][TM][3], fb[2][TN][3];
  f32x16 acc[TM][TN];
  ss_zero(acc);
  const int ns = g.K / 16;     // stages (even: K % 32 == 0)

  // one stage: barrier (stage s + 1 landed everywhere, slot s % 3 free), 24 MFMAs of stage s; behind the first two the fragment reads of
  // stage s + 1 (past the last stage: a dead slot, never used), then the six DMA instructions of stage s + 3 into slot s % 3, one per four MFMAs
  auto stage = [&](int s, auto set_c) {
    constexpr int set = decltype(set_c)::value;
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LPS) : "memory");     // stage s + 1 landed; s + 2 may be in flight
    __builtin_amdgcn_s_barrier();
    const int slot = s % NS;
    const bool live = s + 3 < ns;
    ss_products(fa[set], fb[set], acc, [&](int n) __attribute__((always_inline)) {
      if (n == 1) {
        __builtin_amdgcn_sched_barrier(0);
        ss_read_frags(smem + ((s + 1) % NS) * SLOT, fr, fa[set ^ 1], fb[set ^ 1]);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (n % 4 == 3 && n / 4 < LPS) {
        ss_dma_item(g, t, smem + slot * SLOT, s + 3, n / 4, live, c.wave);
        __builtin_amdgcn_sched_barrier(0);
      }
    });
    __builtin_amdgcn_sched_barrier(0);
  };

  // prologue: three stages in flight, the first one awaited
#pragma unroll
  for (int s = 0; s < NS; ++s) ss_dma_stage(g, t, smem + s * SLOT, s, s < ns, c.wave);
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPS) : "memory");
  __builtin_amdgcn_s_barrier();
  ss_read_frags(smem, fr, fa[0], fb[0]);
#ifdef OPP_TUNING
  ts1 = __builtin_readcyclecounter();
#endif
  for (int s = 0; s < ns; s += 2) {
    stage(s, std::integral_constant<int, 0>{});
    stage(s + 1, std::integral_constant<int, 1>{});
  }
#ifdef OPP_TUNING
  ts2 = __builtin_readcyclecounter();
#endif

  ss_scale_and_mask(g, acc, t.m0, c);
  int nrows, ncols;
  const bool full = ss_tile_extent(g, t, nrows, ncols);
  float* T = reinterpret_cast<float*>(smem);         // the (dead) operand slots
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // the zero-sized tail DMAs and the last fragment reads
  __syncthreads();
  if constexpr (MODE == OPP_SS_CONF) {
    if (full) ss_conf_tile<true>(g, t, T, tid, c, nrows, ncols, tiles_n, acc);
    else ss_conf_tile<false>(g, t, T, tid, c, nrows, ncols, tiles_n, acc);
  } else {
    constexpr bool STORE = MODE == OPP_SS_STATS_STORE;
    if (full) ss_whole_tile_stats<STORE, true>(g, t, T, tid, c, nrows, ncols, tiles_n, acc);
    else ss_whole_tile_stats<STORE, false>(g, t, T, tid, c, nrows, ncols, tiles_n, acc);
  }
#ifdef OPP_TUNING
  ss_write_stamps(g, blockIdx.x, c.wave, lane, false, ts0, ts1, ts2);
#endif
}

// ---- persistent single-sweep kernel (OPP_SS_PERSIST=1): statistics + score matrix ------------------------------------------------------------
// What changes against gemm_ss_kernel<OPP_SS_STATS_STORE> is what a workgroup does BETWEEN K loops.  Measured on the one-tile-per-workgroup
// kernel (tools/gemm_ss_probe.py, 4096 x 5000 x 256): prologue 7.1 k cycles (every workgroup of a generation asks for its first 72 KB at once),
// K loop 23.7 k, epilogue 9 k, and 1280 tiles on 512 resident workgroups = 2.5 generations of which the last runs alone.  Here 2 workgroups per
// CU stay resident and walk a static tile list (XCD x: its contiguous range of the strip order, workgroup idx of the XCD takes tiles idx,
// idx + 64, idx + 128):
//   * the first k16-stage of the NEXT tile is fetched under the half-staged epilogue of the current one, which leaves the third operand slot
//     free for that stage: stage s of a tile lives in slot (s + 2) % 3;
//   * the second resident of a CU (the upper half of an XCD's workgroups: they are dispatched after every CU has its first) starts
//     `g.delay` x 64 cycles late, so that one workgroup's K loop runs under the other's epilogue from the first tile on, and takes the
//     shorter tile list (2 of the CU's 5 tiles at 4096 x 5000).
// LDS: 3 slots of 24 KB + 4 KB of statistics scratch = 76 KB, two workgroups per CU.
constexpr size_t PT_LDS = (size_t)NS * SLOT + MISC;

__global__ __launch_bounds__(NT, 2) void gemm_ss_persist_kernel(const OppGemmSS g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const SsCoord c = ss_coord(__builtin_amdgcn_readfirstlane(tid >> 6), tid);
  const int tiles_n = (g.N + BN - 1) / BN, tiles_m = (g.M + BM - 1) / BM;
  const int ntiles = tiles_m * tiles_n;
  // static tile list: the XCD owns a contiguous range of the strip order
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  const int wgs_x = ((int)gridDim.x + 7 - xcd) >> 3;             // workgroups of this launch on the XCD
  const int t_first = ss_xcd_first(blockIdx.x, ntiles), t_count = (ntiles >> 3) + (xcd < (ntiles & 7) ? 1 : 0);
  if (idx >= t_count) return;
  // the second resident of a CU starts late (see above); wave-uniform
  if (g.delay > 0 && 2 * idx >= wgs_x)
    for (int i = 0; i < g.delay; i += 1024) __builtin_amdgcn_s_sleep(16);     // s_sleep n = about 64 n cycles

  auto setup = [&](int local) {
    int tile_m, tile_n;
    ss_strip_tile(t_first + local, tiles_m, tiles_n, tile_m, tile_n);
    return ss_tile_setup(g, tile_m, tile_n, c.wave, lane);
  };
  auto slot = [&](int s) { return smem + ((s + 2) % NS) * SLOT; };            // the epilogue keeps slot 2 free for stage 0 of the next tile
  const SsFragAddr fr = ss_frag_addr(c);
  u32x4 fa[2][TM][3], fb[2][TN][3];
  f32x16 acc[TM][TN];
  const int ns = g.K / 16;
  SsTile cur = setup(idx);

  // the two-resident stage, with every slot shifted by two.  (The hook is written out here and there on purpose: as one function taking the
  // slots, it put six more VALU instructions per two stages beside the MFMAs of the two-resident kernel, 32 against 26)
  auto stage = [&](int s, auto set_c) {
    constexpr int set = decltype(set_c)::value;
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LPS) : "memory");     // stage s + 1 landed; s + 2 may be in flight
    __builtin_amdgcn_s_barrier();
    const bool live = s + 3 < ns;
    ss_products(fa[set], fb[set], acc, [&](int n) __attribute__((always_inline)) {
      if (n == 1) {
        __builtin_amdgcn_sched_barrier(0);
        ss_read_frags(slot(s + 1), fr, fa[set ^ 1], fb[set ^ 1]);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (n % 4 == 3 && n / 4 < LPS) {
        ss_dma_item(g, cur, slot(s + 3), s + 3, n / 4, live, c.wave);
        __builtin_amdgcn_sched_barrier(0);
      }
    });
    __builtin_amdgcn_sched_barrier(0);
  };

  // prologue of the first tile: three stages in flight
#pragma unroll
  for (int s = 0; s < NS; ++s) ss_dma_stage(g, cur, slot(s), s, s < ns, c.wave);

  for (int local = idx;;) {
#ifdef OPP_TUNING
    const unsigned long long ts0 = __builtin_readcyclecounter();
#endif
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPS) : "memory");            // stage 0 landed (and everything older: the last tile's stores)
    __builtin_amdgcn_s_barrier();
    ss_read_frags(slot(0), fr, fa[0], fb[0]);
    ss_zero(acc);
#ifdef OPP_TUNING
    const unsigned long long ts1 = __builtin_readcyclecounter();
#endif
    for (int s = 0; s < ns; s += 2) {
      stage(s, std::integral_constant<int, 0>{});
      stage(s + 1, std::integral_constant<int, 1>{});
    }
#ifdef OPP_TUNING
    const unsigned long long ts2 = __builtin_readcyclecounter();
#endif
    // epilogue (thread coordinates re-derived from an opaque copy of the thread index: hoisted out of the tile loop, the epilogue's address
    // arithmetic would stay live across the K loop -- 120 spilled registers in the first build)
    int te = tid;
    asm volatile("" : "+v"(te));
    const SsCoord e = ss_coord(__builtin_amdgcn_readfirstlane(te >> 6), te);
    ss_scale_and_mask(g, acc, cur.m0, e);
    int nrows, ncols;
    const bool full = ss_tile_extent(g, cur, nrows, ncols);
    const int next_local = local + wgs_x;
    const bool has_next = next_local < t_count;
    SsTile nxt = cur;
    auto prefetch_first = [&]() __attribute__((always_inline)) {               // stage 0 of the next tile -> slot 2, under this epilogue
      if (has_next) {
        nxt = setup(next_local);
        ss_dma_stage(g, nxt, slot(0), 0, true, c.wave);
      }
    };
    auto prefetch_rest = [&]() __attribute__((always_inline)) {                // stages 1, 2 of the next tile -> slots 0, 1
      if (has_next) {
#pragma unroll
        for (int s = 1; s < NS; ++s) ss_dma_stage(g, nxt, slot(s), s, s < ns, c.wave);
      }
    };
    char* const lds = smem, * const misc = smem + NS * SLOT;
    auto epilogue = ss_half_staged_stats(g, cur, lds, misc, te, e, nrows, ncols, tiles_n, acc, prefetch_first, prefetch_rest);
    if (full) epilogue(std::true_type{});
    else epilogue(std::false_type{});
#ifdef OPP_TUNING
    ss_write_stamps(g, (size_t)(t_first + local), c.wave, lane, true, ts0, ts1, ts2);
#endif
    if (!has_next) break;
    cur = nxt;
    local = next_local;
  }
}

// ---- three residents per CU (the default): statistics + score matrix ------------------------------------------------------------------------
// The timeline of the two-resident kernel (profiles/r06_ss_timeline.txt) says a tile is 12.3 k cycles of MFMAs inside 43 k: 6.3 k of prologue
// latency, 12.4 k of epilogue, and a K loop that runs at half rate whenever the CU's other resident is in its own.  Staggering, static tile
// lists and wave priorities did not change that; what does is a THIRD resident: with three workgroups per CU one of them is in its K loop far
// more often, and the critical path of a CU's five tiles is two tiles long instead of three.  What it costs: LDS for TWO k16-stages instead of
// three (2 x 24 KB + 4 KB of statistics scratch = 52 KB, three workgroups = 156 KB) and <= 168 registers:
//   * ONE operand fragment set, read right behind the stage barrier (the other residents' MFMAs run under that LDS latency);
//   * ONE stage of LDS-DMA in flight: stage s + 1 goes into the slot stage s - 1 was read from, issued one piece per R3_DMA_EVERY MFMAs of
//     stage s (every wave read its stage s - 1 fragments before the barrier that opens stage s), and is awaited with vmcnt(0) at the next barrier;
//   * the half-staged epilogue, so the row statistics are the persistent kernel's.
// One tile per workgroup in the XCD-aware strip order.  (Static tile lists -- 2 + 2 + 1 tiles per CU on 768 resident workgroups -- were
// measured as well: a tile costs 60 k cycles with three residents, the two-tile critical path is as long as before, matcher 143 vs 143 us;
// the dynamic grid lets whichever workgroup slot frees first take the next tile: -4 us, profiles/r06_ss_res3_ab.txt.)
constexpr int R3_NS = 2;
#ifndef R3_DMA_EVERY
#define R3_DMA_EVERY 4         // one DMA piece behind every R3_DMA_EVERY-th MFMA of a stage (6 pieces, 24 MFMAs); 1 / 2 / 3 measured the same (134-138 us)
#endif
constexpr size_t R3_LDS = (size_t)R3_NS * SLOT + MISC;

__global__ __launch_bounds__(NT, 3) void gemm_ss_res3_kernel(const OppGemmSS g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
#ifdef OPP_TUNING
  const unsigned long long ts0 = __builtin_readcyclecounter();
  unsigned long long ts1 = 0, ts2 = 0;
#endif
  const int tid = threadIdx.x, lane = tid & 63;
  const SsCoord c = ss_coord(__builtin_amdgcn_readfirstlane(tid >> 6), tid);
  const int tiles_n = (g.N + BN - 1) / BN, tiles_m = (g.M + BM - 1) / BM;
  const int tile_lin = ss_tile_lin();
  int tile_m, tile_n;
  ss_strip_tile(tile_lin, tiles_m, tiles_n, tile_m, tile_n);
  const SsTile t = ss_tile_setup(g, tile_m, tile_n, c.wave, lane);
  const SsFragAddr fr = ss_frag_addr(c);
  u32x4 fa[TM][3], fb[TN][3];
  f32x16 acc[TM][TN];
  ss_zero(acc);
  const int ns = g.K / 16;

  // one stage: my pieces of stage s landed (vmcnt(0): nothing else is in flight) -> barrier (stage s is complete and visible, and every wave has
  // read its fragments of stage s - 1) -> fragments of stage s -> 24 MFMAs with the six pieces of stage s + 1 behind them
  auto stage = [&](int s) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    ss_read_frags(smem + (s & 1) * SLOT, fr, fa, fb);
    __builtin_amdgcn_sched_barrier(0);
    const bool live = s + 1 < ns;
    ss_products(fa, fb, acc, [&](int n) __attribute__((always_inline)) {
      if (n % R3_DMA_EVERY == R3_DMA_EVERY - 1 && n / R3_DMA_EVERY < LPS) {
        ss_dma_item(g, t, smem + ((s + 1) & 1) * SLOT, s + 1, n / R3_DMA_EVERY, live, c.wave);
        __builtin_amdgcn_sched_barrier(0);
      }
    });
    __builtin_amdgcn_sched_barrier(0);
  };

  ss_dma_stage(g, t, smem, 0, true, c.wave);
#ifdef OPP_TUNING
  ts1 = __builtin_readcyclecounter();
#endif
  for (int s = 0; s < ns; ++s) stage(s);
#ifdef OPP_TUNING
  ts2 = __builtin_readcyclecounter();
#endif

  // epilogue (thread coordinates re-derived from an opaque copy of the thread index: otherwise the epilogue's address arithmetic stays live
  // across the K loop and spills)
  int te = tid;
  asm volatile("" : "+v"(te));
  const SsCoord e = ss_coord(__builtin_amdgcn_readfirstlane(te >> 6), te);
  ss_scale_and_mask(g, acc, t.m0, e);
  int nrows, ncols;
  const bool full = ss_tile_extent(g, t, nrows, ncols);
  auto nothing = []() {};
  char* const lds = smem, * const misc = smem + R3_NS * SLOT;
  auto epilogue = ss_half_staged_stats(g, t, lds, misc, te, e, nrows, ncols, tiles_n, acc, nothing, nothing);
  if (full) epilogue(std::true_type{});
  else epilogue(std::false_type{});
#ifdef OPP_TUNING
  ss_write_stamps(g, (size_t)tile_lin, c.wave, lane, false, ts0, ts1, ts2);
#endif
}

#ifdef OPP_TUNING
unsigned long long* g_ss_dbg_ts = nullptr;
int g_ss_dbg_mode = 0;
#endif

constexpr int kPersistDelay = 12288;      // cycles the second resident of a CU starts late (about half a tile); OPP_SS_DELAY overrides

// compute units of the current device (cached per device: a process may drive several GPUs)
int opp_cu_count() {
  static int cached[64] = {0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64) dev = 0;
  if (!cached[dev]) {
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    cached[dev] = cus > 0 ? cus : 256;
  }
  return cached[dev];
}

template <void (*KERNEL)(const OppGemmSS)>
int launch_kernel(size_t lds, int grid, int symbol, const char* name, const OppGemmSS& g, hipStream_t stream) {
  static OppLdsOnce lds_once;            // per kernel and device (opp_common.h)
  opp_lds_opt_in(reinterpret_cast<const void*>(KERNEL), lds, lds_once);
  OppProfScope prof(symbol, stream, 2.0 * (double)g.M * (double)g.N * (double)g.K);
  hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(NT), lds, stream, g);
  OPP_CHECK_LAUNCH(name);
  return OPP_OK;
}

}  // namespace

void opp_gemm_ss_debug_timestamps(void* buf, int mode) {
#ifdef OPP_TUNING
  g_ss_dbg_ts = static_cast<unsigned long long*>(buf);
  g_ss_dbg_mode = mode;
#else
  (void)buf;
  (void)mode;
#endif
}
int opp_gemm_ss_tile_rows() { return BM; }
int opp_gemm_ss_tile_cols() { return BN; }

int opp_gemm_ss(const OppGemmSS& g_in, hipStream_t stream) {
  OppGemmSS g = g_in;
  OPP_CHECK_ARG(g.A && g.B && g.M > 0 && g.N > 0 && g.K > 0 && g.K % 32 == 0, "gemm_ss: bad operands / K %% 32 (M %d N %d K %d)", g.M, g.N, g.K);
  OPP_CHECK_ARG(g.lda % 16 == 0 && g.ldb % 16 == 0 && g.lda >= g.K * 6 && g.ldb >= g.K * 6, "gemm_ss: operand row strides are bytes, >= 6 K, 16-byte multiples");
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  OPP_CHECK_ARG(al16(g.A) && al16(g.B), "gemm_ss: operands must be 16-byte aligned");
  OPP_CHECK_ARG((size_t)g.M * g.lda < (1ull << 31) && (size_t)g.N * g.ldb < (1ull << 31), "gemm_ss: operand too large for buffer addressing");
  g.a_bytes = (int)((size_t)g.M * g.lda);
  g.b_bytes = (int)((size_t)g.N * g.ldb);
#ifdef OPP_TUNING
  g.dbg_ts = (g_ss_dbg_mode == 0 || g_ss_dbg_mode == g.mode) ? g_ss_dbg_ts : nullptr;
#endif
  constexpr size_t lds2 = (size_t)NS * SLOT;
  const int tiles = opp_cdiv(g.M, BM) * opp_cdiv(g.N, BN);
  if (g.mode == OPP_SS_STATS) {
    OPP_CHECK_ARG(g.stat_rowmax && g.stat_rowsum && g.stat_colmax && g.stat_colsum, "gemm_ss: statistics outputs missing");
    return launch_kernel<gemm_ss_kernel<OPP_SS_STATS>>(lds2, tiles, OPP_PROF_SCORE_SWEEP1, "gemm_ss_kernel", g, stream);
  }
  if (g.mode == OPP_SS_STATS_STORE) {
    OPP_CHECK_ARG(g.stat_rowmax && g.stat_rowsum && g.stat_colmax && g.stat_colsum && g.C && g.ldc >= g.M, "gemm_ss: statistics / score outputs missing");
    OPP_CHECK_ARG((size_t)g.N * (size_t)g.ldc < (1ull << 31), "gemm_ss: output too large for 32-bit indexing");
    g.vec_store = (al16(g.C) && g.ldc % 4 == 0) ? 1 : 0;
    // persistent kernel (two resident workgroups per CU walk static tile lists): OPP_SS_PERSIST=1.  Measured r06 (profiles/r06_ss_persistent_ab.txt,
    // r06_ss_timeline.txt): the prologue disappears (6.3 k -> 0.4 k cycles per tile) but the tile costs the same 42-43 k cycles -- the K loops of the
    // two residents overlap 46-56 % of the time and slow each other down exactly as in the one-tile kernel -- so the matcher is 140 us either way
    // and the default stays the one-tile kernel.  (Static wave priorities for the K loops -- a loop outranks the partner's epilogue, the second
    // resident's loop outranks the first's -- were tried on top, profiles/r06_ss_prio_ab.txt: 142-148 us, no better; removed.)
    static const int persist_env = getenv("OPP_SS_PERSIST") ? atoi(getenv("OPP_SS_PERSIST")) : 0;
    static const int delay_env = getenv("OPP_SS_DELAY") ? atoi(getenv("OPP_SS_DELAY")) : kPersistDelay;
    // default since r06: three resident workgroups per CU (gemm_ss_res3_kernel; OPP_SS_RES3=0 selects the two-resident one-tile kernel).  Measured
    // (profiles/r06_ss_res3_ab.txt): matcher 138.3 -> 135.7 us, matrix pipe busy 0.383 -> 0.401 inside the forward, forward +0.6 % with one
    // forward in flight, unchanged with four
    const char* res3_s = getenv("OPP_SS_RES3");            // (read per call: the tests switch it inside one process)
    const int res3_env = res3_s ? atoi(res3_s) : 1;
    if (res3_env && !persist_env && g.vec_store)
      return launch_kernel<gemm_ss_res3_kernel>(R3_LDS, tiles, OPP_PROF_SCORE_SS, "gemm_ss_res3_kernel", g, stream);
    if (persist_env && tiles > 8 && g.vec_store) {
      const int slots = 2 * opp_cu_count();
      g.delay = tiles > slots ? delay_env : 0;         // (one tile per workgroup: nothing to de-phase)
      return launch_kernel<gemm_ss_persist_kernel>(PT_LDS, tiles < slots ? tiles : slots, OPP_PROF_SCORE_SS, "gemm_ss_persist_kernel", g, stream);
    }
    return launch_kernel<gemm_ss_kernel<OPP_SS_STATS_STORE>>(lds2, tiles, OPP_PROF_SCORE_SS, "gemm_ss_kernel", g, stream);
  }
  if (g.mode == OPP_SS_CONF) {
    OPP_CHECK_ARG(g.C && g.ldc >= g.M && g.rstat_max && g.rstat_sum && g.cstat_max && g.cstat_sum && g.part_best && g.part_arg && g.part_ties &&
                      g.part_rowmax, "gemm_ss: confidence sweep arguments missing");
    OPP_CHECK_ARG((size_t)g.N * (size_t)g.ldc < (1ull << 31), "gemm_ss: output too large for 32-bit indexing");
    g.vec_store = (al16(g.C) && g.ldc % 4 == 0) ? 1 : 0;
    return launch_kernel<gemm_ss_kernel<OPP_SS_CONF>>(lds2, tiles, OPP_PROF_SCORE_SWEEP2, "gemm_ss_kernel", g, stream);
  }
  opp_set_error("gemm_ss: unknown mode %d", g.mode);
  return OPP_ERR_INVALID;
}

#ifdef OPP_TUNING
// tuning builds only: the statistics sweep on caller-given split operands of any K (loop-efficiency probe, tools/gemm_ss_probe.py)
extern "C" int opp_debug_gemm_ss_stats(const void* A, const void* B, int M, int N, int K, float* stats, void* stream) {
  OppGemmSS g;
  g.A = A;
  g.B = B;
  g.lda = K * 6;
  g.ldb = K * 6;
  g.M = M;
  g.N = N;
  g.K = K;
  g.mode = OPP_SS_STATS;
  const size_t tn = opp_cdiv(N, BN), tm = opp_cdiv(M, BM);
  g.stat_rowmax = stats;
  g.stat_rowsum = g.stat_rowmax + (size_t)M * tn;
  g.stat_colmax = g.stat_rowsum + (size_t)M * tn;
  g.stat_colsum = g.stat_colmax + tm * (size_t)N;
  return opp_gemm_ss(g, (hipStream_t)stream);
}
#endif
