// Float64 Gram C = A^T B on gfx950: the dense contraction of the polynomial-ridge fit (G = P^T [P | Y] with
// P = [1 | monomials of the standardised inputs], contraction over pixels) on v_mfma_f64_16x16x4_f64, with a fixed-order
// reduction of the pixel chunks.  Two kernels: the LDS-panel form (the fast path, single and batched) and the register-operand
// form behind it (rows that cannot be loaded by DMA, or a plan that does not fit), and the reduction that joins their chunks.
// Needs nothing from the ridge path but hsr_common.h.
#include <mutex>

#include "hsr_common.h"

namespace hsr {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// gram: C (na x nb) = A^T B over n rows, float64 MFMA 16x16x4, one wave per 16x16 tile and row chunk
// ------------------------------------------------------------------------------------------------
// A (n, lda), B (n, ldb) row-major float64 with na, nb multiples of 16 inside lda/ldb.  Grid:
// (tiles_i * tiles_j, chunks).  v_mfma_f64_16x16x4_f64: lane l supplies A[i = l&15][k = l>>4] and
// B[k = l>>4][j = l&15]; D[row = (l>>4) + 4*reg][col = l&15] (the f64 map, NOT the f32 one).
// One wave = a 48 x 48 output block (R x R = 3 x 3 MFMA tiles): three A and three B operands per k-step feed
// nine MFMAs.  The kernel is bound by operand traffic from L2, not by the matrix pipe (the 2 x 2 version:
// one operand load per MFMA, 50 % MFMA busy), so the lever is operands per MFMA: 0.67 here.  With `sym`
// (B's first tiles_i tile columns are A itself, the Gram of the fit) blocks strictly below the diagonal
// are skipped and mirrored by the reduction: 15 of the 36 symmetric blocks at 288 features.
constexpr int kGramR = 3;

__device__ __forceinline__ bool gram_block_skipped(int bi, int bj, int sym) { return sym && bj < bi; }

__global__ __launch_bounds__(256) void gram_f64_kernel(const double* __restrict__ A, int64_t lda, int tiles_i,
                                                       const double* __restrict__ B, int64_t ldb, int tiles_j,
                                                       int64_t n, int64_t rows_per_chunk, int sym,
                                                       double* __restrict__ partials) {
  constexpr int R = kGramR;
  __shared__ double red[R * R][256];   // cross-wave reduction of the block's output tiles (18 KB)
  const int nbj = (tiles_j + R - 1) / R;
  const int bi = blockIdx.x / nbj, bj = blockIdx.x % nbj;
  if (gram_block_skipped(bi, bj, sym)) return;
  const int ti0 = bi * R, tj0 = bj * R;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, kk = lane >> 4;
  // the chunk's rows are dealt to the 4 waves in quarters (whole k-steps); their sums are combined in wave
  // order below, so the result does not depend on timing
  const int64_t c0 = (int64_t)blockIdx.y * rows_per_chunk;
  const int64_t quarter = ((rows_per_chunk / 4) + 3) / 4 * 4;
  const int64_t r0 = c0 + wave * quarter;
  int64_t cend = c0 + rows_per_chunk;
  if (cend > n) cend = n;
  int64_t r1 = wave == 3 ? cend : r0 + quarter;
  if (r1 > cend) r1 = cend;
  f64x4 acc[R][R];
#pragma unroll
  for (int x = 0; x < R; ++x)
#pragma unroll
    for (int y = 0; y < R; ++y) acc[x][y] = f64x4{0.0, 0.0, 0.0, 0.0};
  const double* ap = A + ti0 * 16 + col;
  const double* bp = B + tj0 * 16 + col;
  int ao[R], bo[R];   // tiles past the edge alias the first one (loaded, multiplied, never stored)
#pragma unroll
  for (int x = 0; x < R; ++x) {
    ao[x] = ti0 + x < tiles_i ? 16 * x : 0;
    bo[x] = tj0 + x < tiles_j ? 16 * x : 0;
  }
  constexpr int KU = 4;   // k-steps per operand batch (24 loads); two batches alternate: one in flight, one in the MFMAs
  auto load = [&](double (&av)[KU][R], double (&bv)[KU][R], int64_t r) {
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int64_t rr = r + 4 * u + kk;
      const bool ok = rr < r1;                    // ragged tail / past the end: zeros
      const int64_t rc = ok ? rr : c0;            // clamped address, value masked below
#pragma unroll
      for (int x = 0; x < R; ++x) {
        const double va = ap[rc * lda + ao[x]], vb = bp[rc * ldb + bo[x]];
        av[u][x] = ok ? va : 0.0;
        bv[u][x] = ok ? vb : 0.0;
      }
    }
  };
  auto mma = [&](const double (&av)[KU][R], const double (&bv)[KU][R]) {
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int x = 0; x < R; ++x)
#pragma unroll
        for (int y = 0; y < R; ++y)
          acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][x], bv[u][y], acc[x][y], 0, 0, 0);
  };
  if (r0 < r1) {
    double a0[KU][R], b0[KU][R], a1[KU][R], b1[KU][R];
    load(a0, b0, r0);
    for (int64_t r = r0; r < r1; r += 8 * KU) {
      load(a1, b1, r + 4 * KU);
      mma(a0, b0);
      load(a0, b0, r + 8 * KU);
      if (r + 4 * KU < r1) mma(a1, b1);
    }
  }
  // ordered cross-wave sum: wave 0 stores, waves 1..3 add in turn
#pragma unroll 1
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int x = 0; x < R; ++x)
#pragma unroll
        for (int y = 0; y < R; ++y)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            double* p = &red[x * R + y][(kk + 4 * g) * 16 + col];
            *p = w == 0 ? acc[x][y][g] : *p + acc[x][y][g];
          }
    }
    __syncthreads();
  }
  const int ntiles = tiles_i * tiles_j;
  for (int q = 0; q < R * R; ++q) {
    const int x = q / R, y = q % R;
    if (ti0 + x >= tiles_i || tj0 + y >= tiles_j) continue;
    const int tile = (ti0 + x) * tiles_j + (tj0 + y);
    partials[((size_t)blockIdx.y * ntiles + tile) * 256 + threadIdx.x] = red[q][threadIdx.x];
  }
}

// LDS-panel form of the Gram kernel (the fast path).  Measured on the way here: f64 MFMA does not overlap with
// the wave's own VALU work (a variant that built the feature panels on chip, 2 v_mul_f64 per operand, ran the
// MFMAs at exactly MFMA time + VALU time), and the register-operand kernel above stalls on its 24 global loads
// per batch.  So the operands take the one route that costs no VALU and no VGPRs: global_load_lds_dwordx4
// (scalar row base + one constant per-lane offset) straight into two 8-row x 96-column panels (A and B) per
// batch, ring-buffered, and conflict-free ds_read_b64 from there.  A workgroup (4 waves = 2 x 2 blocks of 3 x 3
// MFMA tiles) owns a 96 x 96 output block over a chunk of rows; blocks below the diagonal of the symmetric part
// are not launched.
//
// r03 (rocprofv3 PMC on the r02 kernel: matrix pipe busy 58 %, and 9 launched 96 x 96 blocks for 207 useful tiles
// of 324 at 288 features + 32 targets):
//  * a last column strip of <= 32 columns (the 32 targets of the notebook) is no longer a ragged 96-wide block
//    with two thirds of its MFMAs on padding: it is a NARROW block, 96 x 32, 3 x 1 tiles per wave, over chunks
//    5/2 as long (a third of the MFMAs per row, but the same DMA / barrier / address work: measured 0.72 us against
//    1.80 us per batch), so that every workgroup takes the same time (9 -> 7.2 block equivalents at T = 32);
//  * the DMA address is a scalar (global_load_lds with an SGPR base), one exec region covers a wave's four DMAs,
//    and only batches at the ragged end of the last chunk take the row-checked path;
//  * ONE workgroup of kGramGroups x 4 waves per CU instead of two of 4 waves: the groups take the batches of the
//    chunk in turn (group g: batches g, g + G, ...), each with its own panel ring, and their accumulators are added
//    in group order through LDS at the end.  Three waves per SIMD instead of two, in lockstep - with independent
//    workgroups (3 x 4 waves per CU, also measured) the oldest workgroup of a CU wins the matrix pipe, finishes at
//    86 us and leaves the youngest alone until 139 us - and a third of the partial sums: every workgroup writes
//    72 KB and the reduction reads them again (55 MB each way with 768 workgroups, 18 MB with 256);
//  * software pipeline over the barrier: the operands of batch b + 1 are read from LDS while the MFMAs of batch b
//    run, and after the barrier every wave first issues MFMAs and only then its ~60 scalar / DMA / LDS
//    instructions (4 240 -> 3 750 shader cycles per batch of 3 x 18 MFMAs = 3 456).
//  * the diagonal blocks of the symmetric part are a third kind (gram_diag_block below): upper tiles only.
//  What is left: the shader clock runs at 2.10 GHz under this kernel (s_memtime against s_memrealtime), not 2.4.
constexpr int kGpCols = 96;          // panel width = 6 MFMA tiles
constexpr int kGpNarrow = 32;        // widest last strip that becomes a narrow block
constexpr int kGpRows = 8;           // rows per batch = 2 k-steps
constexpr int kGpBufs = 4;           // panel ring: batch b lives in slot b % kGpBufs, the DMA runs kGpBufs - 1 batches ahead
constexpr int kGpAhead = kGpBufs - 1;
constexpr int kGpStride = 208;       // doubles per LDS row = [A 96 | B 96 | 16 spare]: 1664 B = 128 B mod 256 B -> kk rows 0/1 and 2/3 on disjoint banks
constexpr int kGpDmaPerWave = 2 * kGpRows / 4;   // panel rows each wave moves per batch (waves 0, 1: A; waves 2, 3: B)
constexpr int kGramGroups = 3;                   // 4-wave groups per workgroup
constexpr int kGramWgs = 1;                      // workgroups per CU
constexpr int kGramSlots = 256 * kGramWgs;       // resident workgroups of this kernel on the chip
constexpr int kGramThreads = 256 * kGramGroups;
constexpr int kGpRingDoubles = kGpBufs * kGpRows * kGpStride;       // one group's panel ring (4 slots: 53 248 B; three groups: 159 744 B)
constexpr int kGpDumpDoubles = 4 * 9 * 4 * 64;                      // one group's accumulators (72 KB)
constexpr int kGramLdsDoubles = (kGramGroups == 1 || kGramGroups * kGpRingDoubles > kGpDumpDoubles)
                                    ? kGramGroups * kGpRingDoubles : kGpDumpDoubles;
constexpr int kGpMaxBlocks = 64;

struct GramCore {                     // scalars only: handed to the block routine by value (a struct with a dynamically
  const double* A;                    // indexed array would be copied to scratch, and everything read from it would count
  const double* B;                    // as divergent)
  int64_t lda, ldb, n;
  int64_t rows_wide, rows_narrow;    // rows per chunk of a 96-wide / a narrow block
  int32_t na, nb, tiles_i, tiles_j;
  int32_t nwide, nnarrow;            // launched blocks of either kind (wide ones first in `blocks`, then diagonal, then narrow)
  int32_t chunks_wide, chunks_narrow;
  int32_t ndiag, chunks_diag;        // diagonal blocks of the symmetric part (upper tiles only)
  int64_t rows_diag;
  int32_t narrow_col, narrow_width;  // first column and width of the narrow strip of B
  int32_t total, per_xcd;            // workgroups with work; ceil(total / 8)
  double* partials;                  // [chunk][tile][256]
  int64_t pair_a, pair_p;            // batched form: element strides of A (== B) and of the partials between pairs (blockIdx.y)
#ifdef HSR_GRAM_STAMPS
  unsigned long long* stamps;        // [workgroup][8] s_memrealtime at the phase boundaries (diagnostic builds only)
#endif
};
#ifdef HSR_GRAM_STAMPS
__device__ __forceinline__ unsigned long long gram_realtime() {   // 100 MHz
  unsigned long long t;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
static unsigned long long* g_gram_stamps = nullptr;
extern "C" void hsr_dbg_gram_stamps(unsigned long long* dev) { g_gram_stamps = dev; }
#define GRAM_STAMP(i)                                                                                   \
  do {                                                                                                  \
    if (a.stamps && threadIdx.x == 0) a.stamps[(size_t)blockIdx.x * 8 + (i)] = gram_realtime();           \
  } while (0)
#else
#define GRAM_STAMP(i) \
  do {                \
  } while (0)
#endif
struct GramLdsArgs {
  GramCore c;
  uint8_t blocks[kGpMaxBlocks][2];   // (bi, bj) in 96-column units; bj is ignored for narrow blocks
};

__device__ __forceinline__ void glds16_s(uint32_t voff, const void* sbase, uint32_t lds_base) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_base)
               : "memory");
}

__device__ __forceinline__ const double* uniform_ptr(const double* p) {   // a wave-uniform pointer, provably in SGPRs
  const uint64_t v = (uint64_t)(uintptr_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (const double*)(uintptr_t)(((uint64_t)hi << 32) | lo);
}

template <int RY>
__device__ __forceinline__ void gram_block(const GramCore a, double* pan_base, int acol0, int bcol0, int bw,
                                           int64_t c0, int64_t cend, int chunk) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);        // wave inside its group
  const int grp = __builtin_amdgcn_readfirstlane(tid >> 8);
  constexpr int G = kGramGroups;
  const int col = lane & 15, kk = lane >> 4;
  const int wx = wave >> 1, wy = wave & 1;
  // the chunk's batches are dealt to the groups in turn; all groups run the same number of local batches (a batch
  // past the end of the chunk is zero-filled), so that every wave meets the same barriers
  const int nbatch_all = (int)((cend - c0 + kGpRows - 1) / kGpRows);
  const int nbatch = (nbatch_all + G - 1) / G;              // local batches per group
  const int nfull = (int)((cend - c0) / kGpRows) / G;       // local batches whose rows all exist in every group
  pan_base += grp * kGpRingDoubles;                         // this group's ring
  typedef double Slot[kGpRows][kGpStride];
  Slot* pan = reinterpret_cast<Slot*>(pan_base);            // [slot][row][A cols | B cols]
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)(pan_base);

  // 16 panel rows per batch (8 of A, 8 of B), 4 per wave; a row is up to 96 doubles = 48 lanes x 16 bytes.  Lanes whose
  // columns lie past the block or the matrix stay off: their LDS words only feed tiles that are never stored.
  const int p = wave >> 1;                 // which panel this wave fills
  const int pr0 = (wave & 1) * kGpDmaPerWave;
  const int mcol0 = p ? bcol0 : acol0;
  const bool on = p ? (2 * lane < bw && mcol0 + 2 * lane < a.nb) : (lane < 48 && mcol0 + 2 * lane < a.na);
  const int64_t ld = p ? a.ldb : a.lda;
  const double* mbase = uniform_ptr((p ? a.B : a.A) + mcol0);
  const uint32_t voff = (uint32_t)lane * 16u;
  auto issue_full = [&](int b) {           // every row of batch b exists
    const int slot = b % kGpBufs;
    const double* src = mbase + (c0 + (int64_t)(b * G + grp) * kGpRows + pr0) * ld;
    const uint32_t dst = lds0 + (uint32_t)(((slot * kGpRows + pr0) * kGpStride + p * kGpCols) * 8);
    if (on) {
#pragma unroll
      for (int i = 0; i < kGpDmaPerWave; ++i) glds16_s(voff, src + i * ld, dst + (uint32_t)(i * kGpStride * 8));
    }
  };
  auto issue_any = [&](int b) {            // rows past the chunk are zero-filled by hand
    const int slot = b % kGpBufs;
#pragma unroll
    for (int i = 0; i < kGpDmaPerWave; ++i) {
      const int64_t row = c0 + (int64_t)(b * G + grp) * kGpRows + pr0 + i;
      const uint32_t dst = lds0 + (uint32_t)(((slot * kGpRows + pr0 + i) * kGpStride + p * kGpCols) * 8);
      if (row < cend) {
        if (on) glds16_s(voff, mbase + row * ld, dst);
      } else if (lane < 48) {
        pan[slot][pr0 + i][p * kGpCols + 2 * lane] = 0.0;
        pan[slot][pr0 + i][p * kGpCols + 2 * lane + 1] = 0.0;
      }
    }
  };

  constexpr int R = 3, KU = kGpRows / 4;
  f64x4 acc[R][RY];
#pragma unroll
  for (int x = 0; x < R; ++x)
#pragma unroll
    for (int y = 0; y < RY; ++y) acc[x][y] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int asub = wx * 48;
  const int bsub = kGpCols + (RY == 3 ? wy * 48 : wy * 16);     // this wave's first B column inside the row
  struct Ops {
    double a[KU][R], b[KU][RY];
  };
  auto fetch = [&](Ops& o, int b) {        // the operands of local batch b: LDS -> registers
    const double (*ps)[kGpStride] = pan[b % kGpBufs];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
#pragma unroll
      for (int x = 0; x < R; ++x) o.a[u][x] = ps[4 * u + kk][asub + 16 * x + col];
#pragma unroll
      for (int y = 0; y < RY; ++y) o.b[u][y] = ps[4 * u + kk][bsub + 16 * y + col];
    }
  };
  auto mma_row = [&](const Ops& o, int u, int x) {
#pragma unroll
    for (int y = 0; y < RY; ++y)
      acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a[u][x], o.b[u][y], acc[x][y], 0, 0, 0);
  };
  // One local batch.  On entry the panels of batches <= b + 1 have landed (for every wave of the workgroup) and `cur`
  // holds the operands of batch b.  The DMA of batch b + 3 goes to the slot of batch b - 1, whose LDS reads were issued
  // during step b - 2 and had completed before the barrier that ended it.  The operands of batch b + 1 are read while
  // the MFMAs of batch b run, so that no wave starts a batch by waiting for LDS behind the barrier; the step ends when
  // the panel of batch b + 2 has landed (the 4 DMAs of batch b + 3 may stay in flight).
  // The three waves of a SIMD leave the barrier together: each first feeds the matrix pipe (RY MFMAs whose operands are
  // in registers) and only then runs its ~60 scalar / DMA / LDS instructions, in the shadow of those MFMAs - with the
  // address work first the pipe stood idle for ~800 of the 4 240 cycles of a batch.
  auto step = [&](Ops& cur, Ops& nxt, int b) {
    const bool steady = b + kGpAhead < nfull;
    mma_row(cur, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (steady) issue_full(b + kGpAhead);
    else if (b + kGpAhead < nbatch) issue_any(b + kGpAhead);
    if (b + 1 < nbatch) fetch(nxt, b + 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int x = 0; x < R; ++x)
        if (u || x) mma_row(cur, u, x);
    if (steady) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kGpDmaPerWave) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  };

  GRAM_STAMP(0);
  for (int b = 0; b < kGpAhead && b < nbatch; ++b) issue_any(b);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  GRAM_STAMP(1);
#ifdef HSR_GRAM_STAMPS
  if (a.stamps && threadIdx.x == 0) a.stamps[(size_t)blockIdx.x * 8 + 6] = __builtin_readcyclecounter();   // s_memtime: shader clock
#endif
  {
    Ops o0, o1;
    fetch(o0, 0);
#pragma unroll 1
    for (int b = 0; b < nbatch; b += 2) {
      step(o0, o1, b);
      if (b + 1 < nbatch) step(o1, o0, b + 1);
    }
  }

#ifdef HSR_GRAM_STAMPS
  if (a.stamps && threadIdx.x == 0) a.stamps[(size_t)blockIdx.x * 8 + 7] = __builtin_readcyclecounter();
#endif
  GRAM_STAMP(2);
  // the groups' sums, added in group order through LDS (the rings are free: the loop ended in a barrier)
  if (G > 1) {
    double* dump = pan_base - grp * kGpRingDoubles + (wave * 9 * 4) * 64 + lane;
#pragma unroll 1
    for (int g = 1; g < G; ++g) {
      if (grp == g) {
#pragma unroll
        for (int x = 0; x < R; ++x)
#pragma unroll
          for (int y = 0; y < RY; ++y)
#pragma unroll
            for (int r = 0; r < 4; ++r) dump[((x * RY + y) * 4 + r) * 64] = acc[x][y][r];
      }
      __syncthreads();
      if (grp == 0) {
#pragma unroll
        for (int x = 0; x < R; ++x)
#pragma unroll
          for (int y = 0; y < RY; ++y)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[x][y][r] += dump[((x * RY + y) * 4 + r) * 64];
      }
      __syncthreads();
    }
    if (grp != 0) return;
  }
  GRAM_STAMP(3);

  const int ntiles = a.tiles_i * a.tiles_j;
#pragma unroll
  for (int x = 0; x < R; ++x) {
#pragma unroll
    for (int y = 0; y < RY; ++y) {
      const int ti = acol0 / 16 + wx * 3 + x, tjl = RY == 3 ? wy * 3 + y : wy;
      const int tj = bcol0 / 16 + tjl;
      if (ti >= a.tiles_i || tj >= a.tiles_j || 16 * tjl >= bw) continue;
      double* out = a.partials + ((size_t)chunk * ntiles + (size_t)ti * a.tiles_j + tj) * 256;
#pragma unroll
      for (int g = 0; g < 4; ++g) out[(kk + 4 * g) * 16 + col] = acc[x][y][g];
    }
  }
#ifdef HSR_GRAM_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  GRAM_STAMP(4);
  if (a.stamps && threadIdx.x == 0) a.stamps[(size_t)blockIdx.x * 8 + 5] = (unsigned long long)(RY * 1000000 + nbatch);
#endif
}

// Diagonal 96 x 96 block of the symmetric part (A's panel against itself): only its 21 upper tiles are needed - the reduction
// mirrors every tile below the diagonal - so the four waves of a group do not take a 3 x 3 quadrant each (36 tiles, one
// quadrant wasted, two half wasted) but a share of the upper triangle:
//     role 0: (0,0) (0,1) (0,2) (0,3) (0,4) (0,5)        role 1: (1,1) (1,2) (1,3) (1,4) (1,5)
//     role 2: (2,2) (2,3) (2,4) (2,5) (5,5)              role 3: (3,3) (3,4) (3,5) (4,4) (4,5)
// (at most two distinct A operands and six B operands per k-step), role = (wave + group) mod 4 so that every SIMD carries
// 15-16 MFMAs per k-step from its three waves instead of 27.  One panel per batch (2 rows per wave), both operands read
// from it.  Everything else - rings, split of the batches over the groups, software pipeline, combine - as gram_block.
constexpr int kGdTiles = 6;
struct GramDiagRole { int8_t n, arow[2], sel[kGdTiles], tj[kGdTiles]; };
constexpr GramDiagRole kGdRoles[4] = {{6, {0, 0}, {0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5}},
                                      {5, {1, 1}, {0, 0, 0, 0, 0, 0}, {1, 2, 3, 4, 5, 5}},
                                      {5, {2, 5}, {0, 0, 0, 0, 1, 1}, {2, 3, 4, 5, 5, 5}},
                                      {5, {3, 4}, {0, 0, 0, 1, 1, 1}, {3, 4, 5, 4, 5, 5}}};
constexpr int kGdDmaPerWave = kGpRows / 4;       // 8 panel rows per batch over 4 waves

template <int ROLE>
__device__ __forceinline__ void gram_diag_run(const GramCore a, double* pan_base, int acol0, int64_t c0, int64_t cend, int chunk,
                                              int wave, int grp) {
  constexpr GramDiagRole role = kGdRoles[ROLE];
  const int lane = threadIdx.x & 63;
  constexpr int G = kGramGroups;
  const int col = lane & 15, kk = lane >> 4;
  const int nbatch_all = (int)((cend - c0 + kGpRows - 1) / kGpRows);
  const int nbatch = (nbatch_all + G - 1) / G;
  const int nfull = (int)((cend - c0) / kGpRows) / G;
  double* ring = pan_base + grp * kGpRingDoubles;
  typedef double Slot[kGpRows][kGpStride];
  Slot* pan = reinterpret_cast<Slot*>(ring);
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)(ring);
  const int pr0 = wave * kGdDmaPerWave;
  const bool on = lane < 48 && acol0 + 2 * lane < a.nb;    // (A and B are the same matrix here: the columns of a ragged last block
  const double* mbase = uniform_ptr(a.A + acol0);          //  that lie past na are B's, and tiles in them are stored, too)
  const uint32_t voff = (uint32_t)lane * 16u;
  auto issue_full = [&](int b) {
    const int slot = b % kGpBufs;
    const double* src = mbase + (c0 + (int64_t)(b * G + grp) * kGpRows + pr0) * a.lda;
    const uint32_t dst = lds0 + (uint32_t)((slot * kGpRows + pr0) * kGpStride * 8);
    if (on) {
#pragma unroll
      for (int i = 0; i < kGdDmaPerWave; ++i) glds16_s(voff, src + i * a.lda, dst + (uint32_t)(i * kGpStride * 8));
    }
  };
  auto issue_any = [&](int b) {
    const int slot = b % kGpBufs;
#pragma unroll
    for (int i = 0; i < kGdDmaPerWave; ++i) {
      const int64_t row = c0 + (int64_t)(b * G + grp) * kGpRows + pr0 + i;
      const uint32_t dst = lds0 + (uint32_t)((slot * kGpRows + pr0 + i) * kGpStride * 8);
      if (row < cend) {
        if (on) glds16_s(voff, mbase + row * a.lda, dst);
      } else if (lane < 48) {
        pan[slot][pr0 + i][2 * lane] = 0.0;
        pan[slot][pr0 + i][2 * lane + 1] = 0.0;
      }
    }
  };
  constexpr int KU = kGpRows / 4;
  f64x4 acc[kGdTiles];
#pragma unroll
  for (int k = 0; k < kGdTiles; ++k) acc[k] = f64x4{0.0, 0.0, 0.0, 0.0};
  struct Ops {
    double a[KU][2], b[KU][kGdTiles];
  };
  auto fetch = [&](Ops& o, int b) {
    const double (*ps)[kGpStride] = pan[b % kGpBufs];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      o.a[u][0] = ps[4 * u + kk][16 * role.arow[0] + col];
      if (role.arow[1] != role.arow[0]) o.a[u][1] = ps[4 * u + kk][16 * role.arow[1] + col];
#pragma unroll
      for (int k = 0; k < role.n; ++k)
        if (k == 0 || role.tj[k] != role.tj[k - 1]) o.b[u][k] = ps[4 * u + kk][16 * role.tj[k] + col];
    }
  };
  auto mma_one = [&](const Ops& o, int u, int k) {
    // (a B operand shared by two consecutive tiles of the table - (2,5) (5,5) - was fetched once, for the first of them)
    const int kb = (k > 0 && role.tj[k] == role.tj[k - 1]) ? k - 1 : k;
    acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a[u][role.sel[k]], o.b[u][kb], acc[k], 0, 0, 0);
  };
  auto step = [&](Ops& cur, Ops& nxt, int b) {
    const bool steady = b + kGpAhead < nfull;
    mma_one(cur, 0, 0);
    mma_one(cur, 0, 1);
    __builtin_amdgcn_sched_barrier(0);
    if (steady) issue_full(b + kGpAhead);
    else if (b + kGpAhead < nbatch) issue_any(b + kGpAhead);
    if (b + 1 < nbatch) fetch(nxt, b + 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int k = 0; k < role.n; ++k)
        if (u || k > 1) mma_one(cur, u, k);
    if (steady) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kGdDmaPerWave) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  };
  GRAM_STAMP(0);
  for (int b = 0; b < kGpAhead && b < nbatch; ++b) issue_any(b);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  GRAM_STAMP(1);
#ifdef HSR_GRAM_STAMPS
  if (a.stamps && threadIdx.x == 0) a.stamps[(size_t)blockIdx.x * 8 + 6] = __builtin_readcyclecounter();
#endif
  {
    Ops o0, o1;
    fetch(o0, 0);
#pragma unroll 1
    for (int b = 0; b < nbatch; b += 2) {
      step(o0, o1, b);
      if (b + 1 < nbatch) step(o1, o0, b + 1);
    }
  }
#ifdef HSR_GRAM_STAMPS
  if (a.stamps && threadIdx.x == 0) a.stamps[(size_t)blockIdx.x * 8 + 7] = __builtin_readcyclecounter();
#endif
  GRAM_STAMP(2);
  // the groups' sums, added in group order through LDS; a role sits in a different wave in every group, so the dump is
  // indexed by role
  if (G > 1) {
    double* dump = pan_base + (ROLE * kGdTiles * 4) * 64 + lane;
#pragma unroll 1
    for (int g = 1; g < G; ++g) {
      if (grp == g) {
#pragma unroll
        for (int k = 0; k < role.n; ++k)
#pragma unroll
          for (int r = 0; r < 4; ++r) dump[(k * 4 + r) * 64] = acc[k][r];
      }
      __syncthreads();
      if (grp == 0) {
#pragma unroll
        for (int k = 0; k < role.n; ++k)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[k][r] += dump[(k * 4 + r) * 64];
      }
      __syncthreads();
    }
    if (grp != 0) return;
  }
  GRAM_STAMP(3);
  const int ntiles = a.tiles_i * a.tiles_j;
#pragma unroll
  for (int k = 0; k < role.n; ++k) {
    const int ti = acol0 / 16 + role.arow[role.sel[k]], tj = acol0 / 16 + role.tj[k];
    if (ti >= a.tiles_i || tj >= a.tiles_j) continue;
    double* out = a.partials + ((size_t)chunk * ntiles + (size_t)ti * a.tiles_j + tj) * 256;
#pragma unroll
    for (int g = 0; g < 4; ++g) out[(kk + 4 * g) * 16 + col] = acc[k][g];
  }
#ifdef HSR_GRAM_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  GRAM_STAMP(4);
  if (a.stamps && threadIdx.x == 0) a.stamps[(size_t)blockIdx.x * 8 + 5] = (unsigned long long)(2 * 1000000 + nbatch);   // kind 2 = diagonal
#endif
}

__device__ __forceinline__ void gram_diag_block(const GramCore a, double* pan_base, int acol0, int64_t c0, int64_t cend, int chunk) {
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);
  const int grp = __builtin_amdgcn_readfirstlane(tid >> 8);
  switch ((wave + grp) & 3) {      // wave-uniform; every role runs the same sequence of barriers
    case 0: gram_diag_run<0>(a, pan_base, acol0, c0, cend, chunk, wave, grp); break;
    case 1: gram_diag_run<1>(a, pan_base, acol0, c0, cend, chunk, wave, grp); break;
    case 2: gram_diag_run<2>(a, pan_base, acol0, c0, cend, chunk, wave, grp); break;
    default: gram_diag_run<3>(a, pan_base, acol0, c0, cend, chunk, wave, grp); break;
  }
}

// Workgroup id -> (block, chunk): consecutive ids are the blocks of one chunk of rows, and the eight XCDs take
// contiguous runs of ids (hardware deals workgroup w to XCD w % 8), so that the workgroups that read the same rows
// of A sit behind the same L2.
__global__ __launch_bounds__(kGramThreads, kGramWgs) void gram_f64_lds_kernel(const GramLdsArgs args) {
  extern __shared__ __attribute__((aligned(16))) double pan[];   // kGramLdsDoubles
  GramCore a = args.c;
  a.A += blockIdx.y * a.pair_a;                   // pair of a batched launch (0 otherwise); the grid's x extent is a multiple
  a.B += blockIdx.y * a.pair_a;                   // of 8, so the XCD of workgroup (x, y) is x % 8 as in a single launch
  a.partials += blockIdx.y * a.pair_p;
  const int id = (int)(blockIdx.x % 8) * a.per_xcd + (int)(blockIdx.x / 8);
  if (id >= a.total) return;
  const int wide_ids = a.nwide * a.chunks_wide;
  if (id < wide_ids) {
    const int k = id % a.nwide, chunk = id / a.nwide;
    const int64_t c0 = (int64_t)chunk * a.rows_wide;
    int64_t cend = c0 + a.rows_wide;
    if (cend > a.n) cend = a.n;
    gram_block<3>(a, pan, args.blocks[k][0] * kGpCols, args.blocks[k][1] * kGpCols, kGpCols, c0, cend, chunk);
  } else if (id < wide_ids + a.ndiag * a.chunks_diag) {
    const int k = a.nwide + (id - wide_ids) % a.ndiag, chunk = (id - wide_ids) / a.ndiag;
    const int64_t c0 = (int64_t)chunk * a.rows_diag;
    int64_t cend = c0 + a.rows_diag;
    if (cend > a.n) cend = a.n;
    gram_diag_block(a, pan, args.blocks[k][0] * kGpCols, c0, cend, chunk);
  } else {
    const int nid = id - wide_ids - a.ndiag * a.chunks_diag;
    const int k = a.nwide + a.ndiag + nid % a.nnarrow, chunk = nid / a.nnarrow;
    const int64_t c0 = (int64_t)chunk * a.rows_narrow;
    int64_t cend = c0 + a.rows_narrow;
    if (cend > a.n) cend = a.n;
    gram_block<1>(a, pan, args.blocks[k][0] * kGpCols, a.narrow_col, a.narrow_width, c0, cend, chunk);
  }
}

// chunks summed in index order -> C[(ti*16 + r) * ldc + tj*16 + c]; with `sym` every tile below the diagonal is the transpose
// of its mirror tile (whole skipped blocks, and the lower tiles of diagonal blocks).  Tiles from column tile `narrow_tj` on
// have `chunks_narrow` chunks, tiles of diagonal blocks (edge `blk` tiles) `chunks_diag` when that is > 0.
__global__ __launch_bounds__(256) void gram_reduce_kernel(const double* __restrict__ partials, int ntiles, int chunks,
                                                          int tiles_j, int sym, int blk, int narrow_tj,
                                                          int chunks_narrow, int chunks_diag, double* __restrict__ C, int64_t ldc,
                                                          int64_t pair_p, int64_t pair_c) {
  const int tile = blockIdx.x, e = threadIdx.x;
  partials += blockIdx.y * pair_p;                 // pair of a batched launch (0 otherwise)
  C += blockIdx.y * pair_c;
  const int ti = tile / tiles_j, tj = tile % tiles_j;
  const bool mirror = sym && tj < ti;
  const int si = mirror ? tj : ti, sj = mirror ? ti : tj;           // the tile that was computed
  const int src_tile = si * tiles_j + sj;
  const int src_e = mirror ? (e & 15) * 16 + (e >> 4) : e;
  const int nc = sj >= narrow_tj ? chunks_narrow : (sym && chunks_diag > 0 && si / blk == sj / blk) ? chunks_diag : chunks;
  const double* p = partials + (size_t)src_tile * 256 + src_e;
  const size_t step = (size_t)ntiles * 256;
  double s = 0.0;
  int c = 0;
  for (; c + 8 <= nc; c += 8) {          // eight loads in flight, the sum stays in chunk order
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = p[(size_t)(c + i) * step];
#pragma unroll
    for (int i = 0; i < 8; ++i) s += v[i];
  }
  for (; c < nc; ++c) s += p[(size_t)c * step];
  C[(size_t)(ti * 16 + (e >> 4)) * ldc + tj * 16 + (e & 15)] = s;
}

}  // namespace hsr

using namespace hsr;

// Decomposition of the LDS-panel kernel.  Blocks: every 96 x 96 block of the result above the diagonal of the
// symmetric part (wide), the diagonal blocks of the symmetric part (upper tiles only), plus - when B ends in a strip
// of <= 32 columns - one narrow block per 96 rows of A.  Chunks: rows per chunk as small as fills the resident
// workgroup slots in ONE round (257 workgroups take as long as 512), scaled per kind for equal time; <= 256 chunks,
// as the work buffer is sized for.
static bool gram_lds_plan(int na, int nb, int sym, int64_t n, GramLdsArgs* g) {
  const int nbi = (na + kGpCols - 1) / kGpCols;
  const int rem = nb % kGpCols;
  const bool strip = rem > 0 && rem <= kGpNarrow;
  const int nbj = strip ? nb / kGpCols : (nb + kGpCols - 1) / kGpCols;
  int k = 0;
  auto put = [&](int bi, int bj) {
    if (k < kGpMaxBlocks) {
      g->blocks[k][0] = (uint8_t)bi;
      g->blocks[k][1] = (uint8_t)bj;
    }
    ++k;
  };
  for (int bi = 0; bi < nbi; ++bi)                 // wide: every launched block that is not a diagonal block of the symmetric part
    for (int bj = 0; bj < nbj; ++bj)
      if (!(sym && bj <= bi)) put(bi, bj);
  g->c.nwide = k;
  for (int bi = 0; sym && bi < nbi && bi < nbj; ++bi) put(bi, bi);
  g->c.ndiag = k - g->c.nwide;
  for (int bi = 0; strip && bi < nbi; ++bi) put(bi, nbj);
  g->c.nnarrow = strip ? nbi : 0;
  if (k > kGpMaxBlocks) return false;
  g->c.narrow_col = strip ? nbj * kGpCols : nb;
  g->c.narrow_width = strip ? rem : 0;
  // Rows per chunk by kind, for equal time per workgroup (measured per 8-row batch: wide 1.80 us, narrow 0.72 us - a third of the
  // MFMAs but the same DMA / barrier / address work -, diagonal 1.08 us: 16 of 27 MFMAs per SIMD and k-step):
  // narrow 5/2 and diagonal 5/3 of the rows of a wide block; rows in multiples of 48 keep all three whole batches.
  auto narrow_rows = [](int64_t rows) { return rows / 2 * 5; };
  auto diag_rows = [](int64_t rows) { return rows / 3 * 5; };
  auto count = [&](int64_t rows, int64_t* cw, int64_t* cd, int64_t* cn) {
    *cw = g->c.nwide ? (n + rows - 1) / rows : 0;
    *cd = g->c.ndiag ? (n + diag_rows(rows) - 1) / diag_rows(rows) : 0;
    *cn = g->c.nnarrow ? (n + narrow_rows(rows) - 1) / narrow_rows(rows) : 0;
    return g->c.nwide * *cw + g->c.ndiag * *cd + g->c.nnarrow * *cn;
  };
  // start from the even split and grow until the count fits
  int64_t rows = (int64_t)((double)n * (g->c.nwide + g->c.ndiag * 0.6 + g->c.nnarrow / 2.5) / kGramSlots);
  rows = (rows + 47) / 48 * 48;
  const int64_t floor_rows = g->c.nwide ? 240 : (g->c.ndiag ? 144 : 96);   // >= 240 rows per chunk whatever the kind
  if (rows < floor_rows) rows = floor_rows;
  int64_t cw = 0, cd = 0, cn = 0;
  while (count(rows, &cw, &cd, &cn) > kGramSlots || cw > 256 || cd > 256 || cn > 256) rows += 48;
  g->c.rows_wide = rows;
  g->c.rows_diag = diag_rows(rows);
  g->c.rows_narrow = narrow_rows(rows);
  g->c.chunks_wide = (int32_t)cw;
  g->c.chunks_diag = (int32_t)cd;
  g->c.chunks_narrow = (int32_t)cn;
  g->c.total = (int32_t)(g->c.nwide * cw + g->c.ndiag * cd + g->c.nnarrow * cn);
  g->c.per_xcd = (g->c.total + 7) / 8;
  return true;
}

static int64_t gram_reg_chunks(int64_t n, int64_t* rows_out) {
  int64_t chunks = (n + 1023) / 1024;
  if (chunks > 256) chunks = 256;
  int64_t rows = (n + chunks - 1) / chunks;
  rows = (rows + 15) / 16 * 16;                    // whole k-steps inside every wave's quarter of a chunk
  chunks = (n + rows - 1) / rows;
  if (rows_out) *rows_out = rows;
  return chunks;
}

extern "C" size_t hsr_gram_work_bytes(int32_t na, int32_t nb, int64_t n) {
  if (na < 16 || nb < 16 || n < 1) return 0;
  // both kernels use at most 256 chunks; size for the larger count so that either path can run
  GramLdsArgs g{};
  int64_t c1 = gram_reg_chunks(n, nullptr), c2 = 0;
  if (gram_lds_plan(na, nb, nb >= na, n, &g)) {
    c2 = g.c.chunks_wide > g.c.chunks_narrow ? g.c.chunks_wide : g.c.chunks_narrow;
    if (g.c.chunks_diag > c2) c2 = g.c.chunks_diag;
  }
  GramLdsArgs g0{};                                   // the same matrices as two different pointers: no symmetric skip
  if (gram_lds_plan(na, nb, 0, n, &g0) && g0.c.chunks_wide > c2) c2 = g0.c.chunks_wide;
  const int64_t chunks = c1 > c2 ? c1 : c2;
  return (size_t)chunks * (na / 16) * (nb / 16) * 256 * sizeof(double);
}

// The LDS-panel Gram of `npairs` problems of one shape (A == B for the batched form): the pairs are the grid's y extent, with
// per-pair element strides of A, of the partials and of C.  False when the panels cannot be loaded by DMA or the plan does not fit.
static bool launch_gram_lds(const double* a_dev, int64_t lda, int32_t na, const double* b_dev, int64_t ldb, int32_t nb, int64_t n,
                            int sym, double* work_dev, double* c_dev, int64_t ldc, int64_t pair_a, int64_t pair_p,
                            int64_t pair_c, int32_t npairs, hipStream_t s, int* instance) {
  const bool dma_ok = (lda % 2 == 0) && (ldb % 2 == 0) && (((uintptr_t)a_dev | (uintptr_t)b_dev) & 15) == 0 &&
                      (npairs == 1 || pair_a % 2 == 0);
  GramLdsArgs g{};
  if (!dma_ok || !gram_lds_plan(na, nb, sym, n, &g)) return false;
  g.c.A = a_dev;
  g.c.B = b_dev;
  g.c.lda = lda;
  g.c.ldb = ldb;
  g.c.n = n;
  g.c.na = na;
  g.c.nb = nb;
  g.c.tiles_i = na / 16;
  g.c.tiles_j = nb / 16;
  g.c.partials = work_dev;
  g.c.pair_a = pair_a;
  g.c.pair_p = pair_p;
#ifdef HSR_GRAM_STAMPS
  g.c.stamps = g_gram_stamps;
#endif
  static std::once_flag lds_once;
  constexpr size_t lds_bytes = (size_t)kGramLdsDoubles * sizeof(double);
  std::call_once(lds_once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gram_f64_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_bytes);
  });
  const int ti = na / 16, tj = nb / 16;
  *instance = kK4GramLds + ((g.c.nwide ? 1 : 0) | (g.c.ndiag ? 2 : 0) | (g.c.nnarrow ? 4 : 0)) - 1;   // a plan has at least one block
  hipLaunchKernelGGL(gram_f64_lds_kernel, dim3(8 * (unsigned)g.c.per_xcd, (unsigned)npairs), dim3(kGramThreads), lds_bytes, s, g);
  hipLaunchKernelGGL(gram_reduce_kernel, dim3(ti * tj, (unsigned)npairs), dim3(256), 0, s, work_dev, ti * tj, g.c.chunks_wide, tj,
                     sym, kGpCols / 16, g.c.narrow_col / 16, g.c.chunks_narrow, g.c.chunks_diag, c_dev, ldc, pair_p, pair_c);
  return true;
}

extern "C" int hsr_gram_f64(const double* a_dev, int64_t lda, int32_t na, const double* b_dev, int64_t ldb,
                            int32_t nb, int64_t n, double* work_dev, double* c_dev, int64_t ldc,
                            hsr_stream_t stream) {
  HSR_REQUIRE(a_dev && b_dev && work_dev && c_dev && n > 0, HSR_ERR_INVALID, "hsr_gram_f64: bad argument");
  HSR_REQUIRE(na >= 16 && nb >= 16 && na % 16 == 0 && nb % 16 == 0 && lda >= na && ldb >= nb && ldc >= nb,
              HSR_ERR_INVALID, "hsr_gram_f64: na=%d nb=%d must be multiples of 16 inside the leading dimensions", na, nb);
  const int ti = na / 16, tj = nb / 16;
  // Gram of one matrix with itself (the fit: A == B, same leading dimension): the first na columns of the
  // result are symmetric, compute the upper block triangle only
  const int sym = (a_dev == b_dev && lda == ldb && nb >= na) ? 1 : 0;
  hipStream_t s = (hipStream_t)stream;
  int lds_instance = -1;
  if (launch_gram_lds(a_dev, lda, na, b_dev, ldb, nb, n, sym, work_dev, c_dev, ldc, 0, 0, 0, 1, s, &lds_instance))
    return launched(kLaunchK4, "gram_f64_lds_kernel launch", lds_instance, kK4GramReduce);
  int64_t rows = 0;
  const int64_t chunks = gram_reg_chunks(n, &rows);
  constexpr int R = hsr::kGramR;
  hipLaunchKernelGGL(gram_f64_kernel, dim3(((ti + R - 1) / R) * ((tj + R - 1) / R), (unsigned)chunks), dim3(256), 0, s,
                     a_dev, lda, ti, b_dev, ldb, tj, n, rows, sym, work_dev);
  hipLaunchKernelGGL(gram_reduce_kernel, dim3(ti * tj), dim3(256), 0, s, work_dev, ti * tj, (int)chunks, tj, sym, R, tj,
                     (int)chunks, 0, c_dev, ldc, (int64_t)0, (int64_t)0);
  return launched(kLaunchK4, "gram_f64_kernel launch", kK4GramReg + (sym ? 0 : 1), kK4GramReduce);
}

extern "C" int hsr_gram_f64_batched(const double* a_dev, int64_t lda, int32_t na, int32_t nb, int64_t n, int64_t pair_a,
                                    double* work_dev, int64_t pair_work, double* c_dev, int64_t ldc, int64_t pair_c,
                                    int32_t npairs, hsr_stream_t stream) {
  HSR_REQUIRE(a_dev && work_dev && c_dev && n > 0 && npairs >= 1 && npairs <= 65535, HSR_ERR_INVALID,
              "hsr_gram_f64_batched: bad argument");
  HSR_REQUIRE(na >= 16 && nb >= na && na % 16 == 0 && nb % 16 == 0 && lda >= nb && ldc >= nb, HSR_ERR_INVALID,
              "hsr_gram_f64_batched: na=%d nb=%d must be multiples of 16 inside the leading dimensions", na, nb);
  HSR_REQUIRE(npairs == 1 || (pair_a >= n * lda && pair_c >= (int64_t)na * ldc &&
                              (size_t)pair_work * sizeof(double) >= hsr_gram_work_bytes(na, nb, n)),
              HSR_ERR_INVALID, "hsr_gram_f64_batched: pair strides overlap");
  // every pair takes the plan of a single launch of its shape: its chunks, and so its bits, do not depend on the batch
  int lds_instance = -1;
  HSR_REQUIRE(launch_gram_lds(a_dev, lda, na, a_dev, lda, nb, n, 1, work_dev, c_dev, ldc, pair_a, pair_work, pair_c, npairs,
                              (hipStream_t)stream, &lds_instance),
              HSR_ERR_UNSUPPORTED, "hsr_gram_f64_batched: needs 16-byte aligned rows of an even leading dimension");
  return launched(kLaunchK4, "gram_f64_lds_kernel (batched) launch", lds_instance, kK4GramReduce);
}
