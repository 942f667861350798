// K4 (variant a9): multivariate polynomial-ridge fusion S2 (n_in bands) -> EMIT (T bands) on gfx950.
//
// Reference: legacy_notebooks/Spectral_matching.ipynb - Pipeline(StandardScaler, PolynomialFeatures(3,
// include_bias=False), Ridge(alpha=1)) fitted on logit(EMIT) at 60 m (raw lines 475-490) and applied at
// 10 m by predict_cube_logit (raw lines 192-213) through sigmoid(clip(z, +-50)).
// This file holds the monomial table, everything around the fit's Gram (hsr_gram.hip) and Cholesky (hsr_chol.hip), and the predict:
//   fit      expand P = [1 | 285 monomials of the standardised inputs] (float64), StandardScaler statistics, assembly of the
//            ridge system from the Gram, model read-out;
//   predict  out[T][pixels] = W^T Phi^T with the 285 features of each 64-pixel tile expanded ON CHIP into
//            LDS (never written to HBM: 1.2 GB per Mpixel otherwise), v_mfma_f32_32x32x2_f32 (exact
//            float32 fma chain), epilogue intercept + clip + sigmoid, coalesced band-major stores.
// Feature order = sklearn's: degree-major, combinations_with_replacement (x0..x9, x0^2, x0x1, ..., x9^3).
#include <vector>

#include "hsr_common.h"
#include "hsr_tree_dev.h"

namespace hsr {

constexpr int kMaxIn = 16;        // input bands
constexpr int kMaxFeat = 1024;    // monomials (10 inputs, degree 3 -> 285)

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct FeatTable {                // monomial f = z[a] * z[b] * z[c]; index n_in means the constant 1
  uint8_t idx[kMaxFeat][3];
};
static FeatTable g_table_host;
static int g_table_nin = -1, g_table_deg = -1, g_table_nfeat = 0;
static uint8_t* g_table_dev = nullptr;   // [nfeat][4] bytes (a, b, c, pad) - allocated once, outside launches

static int build_table(int n_in, int degree) {
  int f = 0;
  for (int d = 1; d <= degree; ++d) {
    int c[3] = {0, 0, 0};   // non-decreasing index tuple of length d
    while (true) {
      if (f >= kMaxFeat) return -1;
      for (int k = 0; k < 3; ++k) g_table_host.idx[f][k] = (uint8_t)(k < d ? c[k] : n_in);
      ++f;
      int pos = d - 1;
      while (pos >= 0 && c[pos] == n_in - 1) --pos;
      if (pos < 0) break;
      const int v = c[pos] + 1;
      for (int k = pos; k < d; ++k) c[k] = v;
    }
  }
  return f;
}

// ------------------------------------------------------------------------------------------------
// expand: X (N, n_in) float32 rows -> P (N, ldp) float64 = [1 | monomials of (x - mean)/scale | 0 pad]
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void expand_f64_kernel(const float* __restrict__ x, int64_t x_rs, int64_t x_cs,
                                                         const double* __restrict__ mean,
                                                         const double* __restrict__ scale, int64_t n, int n_in,
                                                         int nfeat, const uint8_t* __restrict__ table,
                                                         double* __restrict__ P, int64_t ldp, int ncols) {
  __shared__ double z[32][kMaxIn + 1];
  const int rows_per_block = 32;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  for (int i = threadIdx.x; i < rows_per_block * (n_in + 1); i += 256) {
    const int r = i / (n_in + 1), c = i % (n_in + 1);
    double v = 1.0;
    if (c < n_in && r0 + r < n) v = ((double)x[(r0 + r) * x_rs + c * x_cs] - mean[c]) / scale[c];
    z[r][c] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < rows_per_block * ncols; i += 256) {
    const int r = i / ncols, c = i % ncols;
    if (r0 + r >= n) continue;
    double v = 0.0;
    if (c == 0) v = 1.0;
    else if (c <= nfeat) {
      const uint8_t* t = table + (size_t)(c - 1) * 4;
      v = z[r][t[0]] * z[r][t[1]] * z[r][t[2]];
    }
    P[(r0 + r) * ldp + c] = v;
  }
}

// Masked, batched form for tile pairs (hsr_pair_expand_f64): the inputs of a pair are band-major planes (x: n_in planes, y: T
// planes of npix), the row of pixel r is [1 | monomials | 0 pad | logit(y) | 0 pad] when mask[r] is set, and ALL zero (the
// constant column included) otherwise - so that the Gram over all npix rows is the Gram over the training pixels, with G[0][0]
// their count.  The monomials are expand_f64_kernel's (same z, same product order); logit(clip(y, eps, 1 - eps)) in float64 from
// the float32 reflectance.  blockIdx.y is the pair.
struct PairExpandArgs {
  const float* x;
  const double* mean;
  const double* scale;
  const float* y;
  const uint8_t* mask;
  double* Q;
  int64_t pair_x, pair_ms, pair_y, pair_m, pair_q;
  int64_t npix, ldq;
  int32_t n_in, nfeat, T, na;
  double eps;
  const uint8_t* table;
};

__global__ __launch_bounds__(256) void pair_expand_f64_kernel(const PairExpandArgs a) {
  __shared__ double z[32][kMaxIn + 1];
  __shared__ int ok[32];
  const int64_t pr = blockIdx.y;
  const float* x = a.x + pr * a.pair_x;
  const double* mean = a.mean + pr * a.pair_ms;
  const double* scale = a.scale + pr * a.pair_ms;
  const float* y = a.y + pr * a.pair_y;
  const uint8_t* mask = a.mask + pr * a.pair_m;
  double* Q = a.Q + pr * a.pair_q;
  const int64_t n = a.npix;
  const int n_in = a.n_in;
  const int64_t r0 = (int64_t)blockIdx.x * 32;
  for (int i = threadIdx.x; i < 32 * (n_in + 1); i += 256) {
    const int r = i / (n_in + 1), c = i % (n_in + 1);
    double v = 1.0;
    if (c < n_in && r0 + r < n) v = ((double)x[c * n + r0 + r] - mean[c]) / scale[c];
    z[r][c] = v;
  }
  if (threadIdx.x < 32) ok[threadIdx.x] = r0 + threadIdx.x < n && mask[r0 + threadIdx.x] != 0;
  __syncthreads();
  const int ncols = (int)a.ldq;
  for (int i = threadIdx.x; i < 32 * ncols; i += 256) {
    const int r = i / ncols, c = i % ncols;
    if (r0 + r >= n) continue;
    double v = 0.0;
    if (ok[r]) {
      if (c == 0) {
        v = 1.0;
      } else if (c <= a.nfeat) {
        const uint8_t* t = a.table + (size_t)(c - 1) * 4;
        v = z[r][t[0]] * z[r][t[1]] * z[r][t[2]];
      } else if (c >= a.na && c < a.na + a.T) {
        double u = (double)y[(int64_t)(c - a.na) * n + r0 + r];
        u = u < a.eps ? a.eps : (u > 1.0 - a.eps ? 1.0 - a.eps : u);
        v = log(u / (1.0 - u));
      }
    }
    Q[(r0 + r) * a.ldq + c] = v;
  }
}

// ------------------------------------------------------------------------------------------------
// predict: out[t][p] = act( sum_f W[f][t] * phi_f(z_p) + b[t] ),  fused expand + f32 MFMA + epilogue
// ------------------------------------------------------------------------------------------------
struct PredArgs {
  const float* x;      // inputs: element (pixel p, band c) at x[p * x_ps + c * x_cs]
  int64_t x_ps, x_cs;
  const float* mean;   // [n_in]
  const float* inv;    // [n_in] 1/scale
  int64_t npix;
  int32_t n_in, nfeat, kpad;   // kpad = nfeat rounded up to even
  const uint8_t* table;        // [nfeat][4]
  const float* W;              // (kpad, ldw) float32, rows >= nfeat are zero
  int64_t ldw;
  const float* bias;           // [T]
  int32_t T, ttiles;           // ttiles = ceil(T / 32)
  int32_t act;                 // 1: sigmoid(clip(z, +-50)); 0: raw
  int32_t nan_bad;             // 1: a pixel with a non-finite (or nodata) input comes out NaN in every target
  int32_t use_nodata;
  float nodata;
  float* out;                  // (T, out_stride)
  int64_t out_stride;
  int64_t pair_x, pair_mi, pair_w, pair_b, pair_out;   // batched form: element strides between the pairs (blockIdx.z)
};

// The operands of this workgroup's pair: a batched launch has one pair per grid z index and every workgroup stays on its pair,
// so W is staged once per workgroup as in a single launch (z = 0, strides 0).
__device__ __forceinline__ PredArgs pred_pair(PredArgs a) {
  const int64_t z = blockIdx.z;
  a.x += z * a.pair_x;
  a.mean += z * a.pair_mi;
  a.inv += z * a.pair_mi;
  a.W += z * a.pair_w;
  a.bias += z * a.pair_b;
  a.out += z * a.pair_out;
  return a;
}

// predict_cube_logit's rule for unusable pixels (Spectral_matching.ipynb raw lines 197-203): any input non-finite, or
// close to the nodata value in torch.isclose's sense (|x - nd| <= 1e-8 + 1e-5 |nd|, equal infinities close, NaN never).
// Epilogue of the predict103 kernels.  r03 (rocprofv3 PMC: matrix pipe busy 57 % of the SIMD cycles, 88 k wave-cycles per
// tile of which 55 k are MFMA): the first version loaded the bias of each of a lane's 16 x TT targets inside the tile loop,
// every load in its own exec-masked block behind `trg < T` with its own s_waitcnt - ~0.5 k cycles of exposed latency each,
// 24 k per tile - and evaluated 1 / (1 + e) as an IEEE division (10 instructions).  The targets of a lane do not depend on
// the tile, so the bias values are loaded ONCE before the tile loop and the accumulators start from them; the sigmoid uses
// v_rcp_f32 (1 ulp; the bar is 1e-4 in reflectance); only the store stays behind `trg < T`.
__device__ __forceinline__ float predict_activation(float v, int act) {
  if (act) {
    v = v < -50.0f ? -50.0f : (v > 50.0f ? 50.0f : v);   // NaN falls through, like np.clip
    v = __builtin_amdgcn_rcpf(1.0f + __expf(-v));
  }
  return v;
}

__device__ __forceinline__ bool pred_bad_input(float x, int use_nodata, float nd) {
  const bool nonfinite = (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
  const bool close = use_nodata && (x == nd || fabsf(x - nd) <= 1e-8f + 1e-5f * fabsf(nd));
  return nonfinite || close;
}

constexpr int kPredPix = 64;      // pixels per workgroup tile
constexpr int kPredThreads = 256;

template <int TT>   // number of 32-wide target tiles held by a wave (accumulators: TT * 16 VGPRs)
__global__ __launch_bounds__(kPredThreads) void predict_kernel(const PredArgs args) {
  const PredArgs a = pred_pair(args);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int ldphi = a.kpad + 1;                      // odd row stride -> conflict-free column walks
  float* phi = reinterpret_cast<float*>(smem);       // [64][ldphi]
  float* zt = phi + kPredPix * ldphi;                // [64][n_in + 1]
  uint32_t* badl = reinterpret_cast<uint32_t*>(zt + kPredPix * (a.n_in + 1));   // [64]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nz = a.n_in + 1;
  for (int64_t tile = blockIdx.x; tile * kPredPix < a.npix; tile += gridDim.x) {
    const int64_t p0 = tile * kPredPix;
    // standardised inputs (+ the constant 1 at index n_in); non-finite inputs propagate to NaN outputs
    for (int i = t; i < kPredPix * nz; i += kPredThreads) {
      const int p = i / nz, c = i % nz;
      float v = 1.0f;
      if (c < a.n_in) v = (p0 + p < a.npix) ? (a.x[(p0 + p) * a.x_ps + c * a.x_cs] - a.mean[c]) * a.inv[c] : 0.0f;
      zt[p * nz + c] = v;
    }
    if (t < kPredPix) {
      uint32_t bad = 0u;
      if (a.nan_bad && p0 + t < a.npix)
        for (int c = 0; c < a.n_in; ++c) bad |= pred_bad_input(a.x[(p0 + t) * a.x_ps + c * a.x_cs], a.use_nodata, a.nodata) ? 1u : 0u;
      badl[t] = bad;
    }
    __syncthreads();
    for (int i = t; i < kPredPix * a.kpad; i += kPredThreads) {
      const int f = i / kPredPix, p = i % kPredPix;       // consecutive threads -> consecutive pixels
      float v = 0.0f;
      if (f < a.nfeat) {
        const uint8_t* tb = a.table + (size_t)f * 4;
        v = zt[p * nz + tb[0]] * zt[p * nz + tb[1]] * zt[p * nz + tb[2]];
      }
      phi[p * ldphi + f] = v;
    }
    __syncthreads();
    // wave w: pixel half (w & 1) * 32, target tiles (w >> 1), (w >> 1) + 2, ...
    const int ph = (wave & 1) * 32;
    const int j = lane & 31, kh = lane >> 5;
    for (int tt0 = wave >> 1; tt0 < a.ttiles; tt0 += 2 * TT) {
      f32x16 acc[TT];
#pragma unroll
      for (int q = 0; q < TT; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.0f;
      const float* brow = phi + (ph + j) * ldphi + kh;   // B[k][pixel j] = phi[pixel][k]
      for (int k = 0; k < a.kpad; k += 2) {
        const float bv = brow[k];
#pragma unroll
        for (int q = 0; q < TT; ++q) {
          const int tt = tt0 + 2 * q;
          const int tcol = tt * 32 + j;                  // A[i = target][k] = W[k][target]
          const float av = (tt < a.ttiles && tcol < a.T) ? a.W[(size_t)(k + kh) * a.ldw + tcol] : 0.0f;
          acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[q], 0, 0, 0);
        }
      }
      // D[row = target, col = pixel]: row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), col = lane & 31
#pragma unroll
      for (int q = 0; q < TT; ++q) {
        const int tt = tt0 + 2 * q;
        if (tt >= a.ttiles) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int trg = tt * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
          const int64_t p = p0 + ph + j;
          if (trg < a.T && p < a.npix) {
            float v = predict_activation(acc[q][r] + a.bias[trg], a.act);
            if (badl[ph + j]) v = __uint_as_float(0x7fc00000u);
            a.out[(size_t)trg * a.out_stride + p] = v;
          }
        }
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// predict, specialised for the notebook's shape (10 inputs, degree 3 -> 285 monomials): MFMA-bound
// ------------------------------------------------------------------------------------------------
// The generic kernel above stages a 64 x 286 feature tile in LDS (73 KB -> one workgroup per CU) and fetches
// W from global memory per MFMA: 10-12 % of the f32 matrix peak.  In the kernels below every lane keeps the 10
// standardised inputs of its pixel in registers, the monomials are generated by fully unrolled code from
// compile-time tables, and W is staged in LDS once per workgroup for the whole launch:
//   T <= 16            predict103_x16_kernel       (16-target tiles, v_mfma_f32_16x16x4_f32)
//   17 <= T <= 32      predict103_slice_kernel<1>  (one 32-target slice)
//   33 <= T <= 512     predict103_slice_kernel<2 / 3>  (slices of 64 or 96 targets, blockIdx.y)
// Larger T take the generic kernel.  Targets sit on the M axis so each accumulator register holds consecutive
// pixels of one target: coalesced band-major stores.
struct Tab103 {
  uint8_t v[286][3];
};
constexpr Tab103 make_tab103() {
  Tab103 t{};
  int f = 0;
  for (int d = 1; d <= 3; ++d) {
    int c[3] = {0, 0, 0};
    while (true) {
      for (int k = 0; k < 3; ++k) t.v[f][k] = (uint8_t)(k < d ? c[k] : 10);
      ++f;
      int pos = d - 1;
      while (pos >= 0 && c[pos] == 9) --pos;
      if (pos < 0) break;
      const int nv = c[pos] + 1;
      for (int k = pos; k < d; ++k) c[k] = nv;
    }
  }
  t.v[285][0] = t.v[285][1] = t.v[285][2] = 10;   // padding monomial (its W row is zero)
  return t;
}
constexpr Tab103 kTab103 = make_tab103();
// (r04, measured and dropped: two accumulator tiles per wave for T <= 32 - even / odd steps, added at the end - so that a wave always
// has an independent MFMA to issue: 0.2039 vs 0.2054 ms per Mpixel.  The chain's latency is not what idles the matrix pipe.)
// the 10 inputs of one pixel.  Pixel-major rows (x_cs == 1, the (N, 10) arrays of predict()) with an even pitch and an 8-byte
// aligned base are read as five float2 instead of ten scalars: a wave's 32 pixels then touch their 40-byte rows once per 8 bytes
__device__ __forceinline__ void pred_load10(const PredArgs& a, int64_t pc, float (&x)[10]) {
  if (a.x_cs == 1 && (a.x_ps & 1) == 0 && (((uintptr_t)a.x) & 7) == 0) {       // launch-uniform
    const float2* r = reinterpret_cast<const float2*>(a.x + pc * a.x_ps);
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      const float2 v = r[c];
      x[2 * c] = v.x;
      x[2 * c + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int c = 0; c < 10; ++c) x[c] = a.x[pc * a.x_ps + c * a.x_cs];
  }
}

// pred_load10's predicate on the host, for the launch record (the suffix " x2" / " scalar" of hsr_k4_last_launch): keep the two alike
static bool pred_x2_arm(const float* x, int64_t x_ps, int64_t x_cs) {
  return x_cs == 1 && (x_ps & 1) == 0 && (((uintptr_t)x) & 7) == 0;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
// ---- the K axis in ORBIT order (r04) ------------------------------------------------------------------------------------------
// An MFMA's K index is spread over lane groups (two for v_mfma_f32_32x32x2_f32, four for v_mfma_f32_16x16x4_f32), so the lane
// groups of one instruction need DIFFERENT monomials - compile-time index triples - of their pixel.  Rounds 1-3 formed both
// products in every lane and picked one (v_cndmask): ~5 VALU per step, and the measurements of r04 say the SIMD does not hide
// VALU work under its own MFMAs (T <= 32: 64 % matrix-pipe busy with 20 cycles of VALU per 64-cycle MFMA; a 16-target variant with
// 20 VALU per 64 cycles of MFMA ran SLOWER than the 32-target kernel).  The order of the K axis is free (a sum): the 286 index
// multisets {a <= b <= c} over the 11 symbols (10 inputs + the constant 1) are grouped into orbits of a symbol permutation sigma
// of order G = number of lane groups; step s takes one orbit, and lane group g evaluates the orbit's REPRESENTATIVE on its own copy
// of the inputs, permuted once per tile (Z_g[m] = z[sigma^g(m)]): Z[a] Z[b] Z[c] in group g is the monomial sigma^g(a, b, c).  One code
// path, ~1.3 v_mul per step, no pick.  Members an orbit repeats (short orbits) meet a zero row of W; the staging loop gathers W's
// rows in orbit order.   G = 2: sigma = (0 1)(2 3)(4 5)(6 7)(8 9): 146 steps for 143.   G = 4: sigma = (0 1 2 3)(4 5 6 7): 82 for 71.5.
template <int G>
constexpr int perm_sym(int m, int g) {
  if (G == 2) return (m < 10 && (g & 1)) ? (m ^ 1) : m;
  return m < 4 ? (m + g) & 3 : (m < 8 ? 4 + ((m - 4 + g) & 3) : m);
}
template <int G>
struct Orbits103 {
  uint8_t rep[160][3];     // representative triple of step s (symbols 0 .. 10; 10 = the constant 1)
  int16_t src[160][G];     // feature row of W that lane group g's member of the orbit multiplies, -1: none (a repeat, or 1 * 1 * 1)
  int steps;
};
template <int G>
constexpr Orbits103<G> make_orbits103() {
  Orbits103<G> o{};
  bool seen[11][11][11] = {};
  int n = 0;
  for (int a = 0; a <= 10; ++a)
    for (int b = a; b <= 10; ++b)
      for (int c = b; c <= 10; ++c) {
        if (seen[a][b][c]) continue;
        o.rep[n][0] = (uint8_t)a; o.rep[n][1] = (uint8_t)b; o.rep[n][2] = (uint8_t)c;
        for (int g = 0; g < G; ++g) {
          int t0 = perm_sym<G>(a, g), t1 = perm_sym<G>(b, g), t2 = perm_sym<G>(c, g);
          if (t0 > t1) { const int x = t0; t0 = t1; t1 = x; }
          if (t1 > t2) { const int x = t1; t1 = t2; t2 = x; }
          if (t0 > t1) { const int x = t0; t0 = t1; t1 = x; }
          int row = -1;
          if (!seen[t0][t1][t2]) {
            seen[t0][t1][t2] = true;
            for (int f = 0; f < 285; ++f)      // kTab103 lists a monomial's indices in ascending order, padded with 10
              if (kTab103.v[f][0] == t0 && kTab103.v[f][1] == t1 && kTab103.v[f][2] == t2) row = f;
          }
          o.src[n][g] = (int16_t)row;
        }
        ++n;
      }
  o.steps = n;
  return o;
}
constexpr Orbits103<4> kOrb103 = make_orbits103<4>();
constexpr Orbits103<2> kOrb2 = make_orbits103<2>();
static_assert(kOrb103.steps == 82, "orbits of (0 1 2 3)(4 5 6 7) on the 286 index multisets");
static_assert(kOrb2.steps == 146, "orbits of (0 1)(2 3)(4 5)(6 7)(8 9) on the 286 index multisets");
constexpr int kStepsOrb = kOrb103.steps, kStepsOrb2 = kOrb2.steps;
static int16_t* g_orb_rows_dev = nullptr;              // kOrb103.src then kOrb2.src on the device (uploaded by hsr_polyfeat_prepare, not on a launch path)

// the slice kernels' MFMA chain over the orbit-ordered K axis (G = 2): Z is the lane half's permuted copy of the inputs
template <int TT>
__device__ __forceinline__ void mfma_steps_orb2(const float (&Z)[11], int kh, const float* __restrict__ wl, int ldwl, int j, f32x16 (&acc)[TT]) {
  float wc[TT], wn[TT];
  const float* wr = wl + kh * ldwl + j;              // A[i = target][k] = staged row 2 s + kh
#pragma unroll
  for (int q = 0; q < TT; ++q) wc[q] = wr[q * 32];
#pragma unroll
  for (int s = 0; s < kStepsOrb2; ++s) {
    const float bv = Z[kOrb2.rep[s][0]] * Z[kOrb2.rep[s][1]] * Z[kOrb2.rep[s][2]];      // B[k = 2 s + kh][pixel j]
    if (s + 1 < kStepsOrb2) {
#pragma unroll
      for (int q = 0; q < TT; ++q) wn[q] = wr[(size_t)2 * (s + 1) * ldwl + q * 32];
    }
#pragma unroll
    for (int q = 0; q < TT; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[q], bv, acc[q], 0, 0, 0);
#pragma unroll
    for (int q = 0; q < TT; ++q) wc[q] = wn[q];
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Many targets (T > 96, e.g. EMIT's 285 bands): the chunked kernel of rounds 1-2 re-staged the whole 329 KB of W through
// LDS for every 128-pixel tile, with nine barriers per tile, and sat at 39 % of the f32-MFMA peak against 50 % for T <= 32
// where W was resident.  W does not fit one LDS, but a SLICE of 96 targets does (286 x 96 x 4 = 110 KB): blockIdx.y picks the
// slice, the slice is staged once per workgroup and stays for the whole launch, and the workgroup (12 waves = 3 per
// SIMD, each wave its own 32 pixels) walks the pixel tiles with no staging and no barrier in the loop.  The monomials
// of a pixel are recomputed once per slice (2-4 v_mul per MFMA step of 3 x 64 cycles: free) and its 10 inputs re-read
// (40 B per slice: nothing).  3 accumulator tiles per wave instead of 9.
// r03: (a) 8 -> 12 waves on the one 96-target slice a CU holds (3 per SIMD, 168 VGPRs, no spill; 16 waves = 128 VGPRs spill):
// 1.675 -> 1.603 ms at T = 285 on one box; (b) the kernel is a template on the slice width, and it also serves 33 <= T <= 96 with
// ONE slice: the chunked kernel (nine barriers and a re-staged W per 128-pixel tile) took 0.83-0.87 ms
// per Mpixel for 65-96 targets, the 96-wide slice kernel 0.51-0.52 ms; (c) slices are as narrow as the target count allows
// (T = 97: two slices of 64 instead of two of 96).  64-target slices run 16 waves (4 per SIMD) on their 73 KB of W.
// Wave priorities of the slice and 16-target kernels (r04, after they paid in the uint16 K1): level of a wave during its MFMA chain /
// outside it (inputs, standardisation, activation, stores).  A/B on one box, ms per Mpixel at T = 16 / 32 / 96 / 285
// (profiles/r04_k4_ridge.md): none 0.129 / 0.203 / 0.528 / 1.523; REST 1 (shipped): 0.123 / 0.198 / 0.520 / 1.491; REST 3: the same;
// CHAIN 3 or 1: no change; STAGGER (the four waves of a SIMD at four different levels during the chain, so that they drift apart and
// one wave's epilogue meets another's chain - either guess of the wave -> SIMD mapping): T = 32 unchanged at 0.200-0.205.
// Shipped: level 1 from the start of the tile loop, 0 during each MFMA chain, back to 1 after it.
constexpr int slice_waves(int tt) { return tt == 3 ? 12 : 16; }      // one workgroup per CU
template <int TT>
__global__ __launch_bounds__(64 * slice_waves(TT), (slice_waves(TT) + 3) / 4) void predict103_slice_kernel(const PredArgs args, const int16_t* __restrict__ src_rows) {
  const PredArgs a = pred_pair(args);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* wl = reinterpret_cast<float*>(smem);       // [2 * kStepsOrb2][Tp]: W's rows in orbit order (kOrb2)
  constexpr int Tp = TT * 32;
  constexpr int kSliceThreads = 64 * slice_waves(TT);      // waves per workgroup = waves per CU (one workgroup per CU)
  constexpr int kSlicePix = 32 * slice_waves(TT);          // pixels per tile: 32 per wave
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int j = lane & 31, kh = lane >> 5;
  const int t0 = blockIdx.y * Tp;                   // first target of this workgroup's slice
  for (int i = t; i < 2 * kStepsOrb2 * Tp; i += kSliceThreads) {
    const int r = i / Tp, c = i % Tp;
    const int f = src_rows[r];
    wl[i] = (f >= 0 && t0 + c < a.T) ? a.W[(size_t)f * a.ldw + t0 + c] : 0.0f;
  }
  __syncthreads();
  float bv[TT][16];                                    // bias of this lane's targets: tile-invariant
#pragma unroll
  for (int q = 0; q < TT; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int trg = t0 + q * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
      bv[q][r] = trg < a.T ? a.bias[trg] : 0.0f;
    }
  float xn[10];                                        // inputs of the next tile, loaded under this tile's MFMA chain
  auto load_inputs = [&](int64_t tile_) {
    const int64_t p_ = tile_ * kSlicePix + wave * 32 + j;
    const int64_t pc_ = p_ < a.npix ? p_ : a.npix - 1;
    pred_load10(a, pc_, xn);
  };
  if ((int64_t)blockIdx.x * kSlicePix < a.npix) load_inputs(blockIdx.x);
  __builtin_amdgcn_s_setprio(1);
  for (int64_t tile = blockIdx.x; tile * kSlicePix < a.npix; tile += gridDim.x) {
    const int64_t p = tile * kSlicePix + wave * 32 + j;
    float z[11];
    bool bad = false;
#pragma unroll
    for (int c = 0; c < 10; ++c) {
      const float xr = xn[c];
      bad = bad || pred_bad_input(xr, a.use_nodata, a.nodata);
      z[c] = (xr - a.mean[c]) * a.inv[c];
    }
    bad = bad && a.nan_bad != 0;
    z[10] = 1.0f;
#pragma unroll
    for (int c = 0; c < 10; c += 2) {                   // the lane half's copy: kh = 1 swaps the inputs pairwise (sigma of kOrb2)
      const float lo = z[c], hi = z[c + 1];
      z[c] = kh ? hi : lo;
      z[c + 1] = kh ? lo : hi;
    }
    if ((tile + gridDim.x) * kSlicePix < a.npix) load_inputs(tile + gridDim.x);
    f32x16 acc[TT];
#pragma unroll
    for (int q = 0; q < TT; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[q][r] = bv[q][r];
    __builtin_amdgcn_s_setprio(0);
    mfma_steps_orb2<TT>(z, kh, wl, Tp, j, acc);
    __builtin_amdgcn_s_setprio(1);
    if (p < a.npix) {
      // keep the epilogue's addressing inside the tile loop: hoisted out of it (LICM) the 64-bit offsets of
      // all 16*TT accumulator rows cost up to 288 VGPRs and spilled the accumulators
      int64_t ostride = a.out_stride;
      int tmax = a.T;
      asm volatile("" : "+s"(ostride), "+s"(tmax));
      float* orow = a.out + (size_t)(t0 + 4 * kh) * ostride + p;
#pragma unroll
      for (int q = 0; q < TT; ++q) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int tu = q * 32 + (r & 3) + 8 * (r >> 2);
          const int trg = t0 + tu + 4 * kh;
          float v = predict_activation(acc[q][r], a.act);
          if (bad) v = __uint_as_float(0x7fc00000u);
          if (trg < tmax) orow[(size_t)tu * ostride] = v;
        }
      }
    }
  }
}

// Few targets (r04).  v_mfma_f32_32x32x2_f32 puts 32 targets on the M axis, so T = 16 cost what T = 32 costs (r03: 0.189 ms per
// Mpixel for both).  v_mfma_f32_16x16x4_f32 has the same rate (16 x 16 x 4 x 2 flop in 32 cycles) with 16 targets per tile; a wave
// holds one tile of 16 targets x two sets of 16 pixels.
//   A[i = target][k] = W[k][target]: lane (i = lane & 15, g = lane >> 4) reads row 4 s + g of the staged W (64 consecutive LDS words);
//   B[k][j = pixel]:  lane (j, g) must supply "monomial 4 s + g" of ITS pixel - four DIFFERENT compile-time index triples in the four
//     lane groups of one instruction.  Two versions that pick per lane were measured and dropped: a ?: chain over the four products
//     (hipcc wraps every pick in exec-masked branches: 0.173 ms) and bit-mask picks (20 VALU per step against 64 cycles of matrix
//     pipe, and the SIMD does not hide them: 0.201 ms).  What is built: the ORDER of the K axis is free (a sum), so the 286 index
//     multisets {a <= b <= c} over the 11 symbols (10 inputs + the constant) are grouped into orbits of the symbol permutation
//     sigma = (0 1 2 3)(4 5 6 7); step s takes one orbit: lane group g computes the orbit's representative on ITS OWN copy of the
//     inputs, permuted once per tile (Z_g[m] = z[sigma^g(m)]): Z[a] Z[b] Z[c] in group g IS the monomial sigma^g(a, b, c).  One code
//     path, two v_mul per step and pixel set, no pick.  82 orbits (66 of four, 6 of two, 10 fixed) instead of 286 / 4 = 71.5 steps:
//     the repeated members of short orbits meet a zero row of W.  The staging loop gathers W's rows in orbit order.
//   D[i][j]: lane (j, g) holds targets 4 g + r, r = 0 .. 3, of pixel j: 64-byte store segments per target.
// One 16-wave workgroup per CU, W staged once.  (Three such tiles for 33 <= T <= 48 were measured too: 82 x 6 MFMAs of 32 cycles are
// no better than the 64-target slice's 143 x 2 of 64; those T keep the slice kernel.)
constexpr int kX16Waves = 12, kX16Wgs = 2;     // 2 x 12 waves per CU = 6 per SIMD at <= 80 VGPRs (r04: 16 x 1: 0.132 ms per Mpixel)
__global__ __launch_bounds__(64 * kX16Waves, kX16Wgs) void predict103_x16_kernel(const PredArgs args, const int16_t* __restrict__ src_rows) {
  const PredArgs a = pred_pair(args);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* wl = reinterpret_cast<float*>(smem);          // [4 * kStepsOrb][16]
  constexpr int kPix = 32 * kX16Waves;                 // pixels per workgroup tile: 32 per wave
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int i = lane & 15, g = lane >> 4;
  for (int e = t; e < 4 * kStepsOrb * 16; e += 64 * kX16Waves) {
    const int r = e >> 4, c = e & 15;
    const int f = src_rows[r];
    wl[e] = (f >= 0 && c < a.T) ? a.W[(size_t)f * a.ldw + c] : 0.0f;
  }
  __syncthreads();
  float bias[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bias[r] = 4 * g + r < a.T ? a.bias[4 * g + r] : 0.0f;
  float xn[2][10];
  auto load_inputs = [&](int64_t tile_) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t p_ = tile_ * kPix + wave * 32 + h * 16 + i;
      pred_load10(a, p_ < a.npix ? p_ : a.npix - 1, xn[h]);
    }
  };
  if ((int64_t)blockIdx.x * kPix < a.npix) load_inputs(blockIdx.x);
  __builtin_amdgcn_s_setprio(1);
  for (int64_t tile = blockIdx.x; tile * kPix < a.npix; tile += gridDim.x) {
    float Z[2][11];                                    // this lane group's permuted copy of the standardised inputs
    bool bad[2] = {false, false};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float z[8];
#pragma unroll
      for (int c = 0; c < 10; ++c) {
        const float xr = xn[h][c];
        bad[h] = bad[h] || pred_bad_input(xr, a.use_nodata, a.nodata);
        const float zc = (xr - a.mean[c]) * a.inv[c];
        if (c < 8) z[c] = zc; else Z[h][c] = zc;
      }
      bad[h] = bad[h] && a.nan_bad != 0;
      Z[h][10] = 1.0f;
#pragma unroll
      for (int m = 0; m < 8; ++m) {                    // Z[m] = z[sigma^g(m)]: a rotation inside each block of four
        const int b4 = m & 4, r4 = m & 3;
        const float v0 = z[b4 + r4], v1 = z[b4 + ((r4 + 1) & 3)], v2 = z[b4 + ((r4 + 2) & 3)], v3 = z[b4 + ((r4 + 3) & 3)];
        Z[h][m] = g == 0 ? v0 : (g == 1 ? v1 : (g == 2 ? v2 : v3));
      }
    }
    if ((tile + gridDim.x) * kPix < a.npix) load_inputs(tile + gridDim.x);
    f32x4 acc[2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[h][r] = bias[r];
    const float* wr = wl + g * 16 + i;
    float wc = wr[0], wn = 0.0f;
    __builtin_amdgcn_s_setprio(0);
#pragma unroll
    for (int s = 0; s < kStepsOrb; ++s) {
      const float b0 = Z[0][kOrb103.rep[s][0]] * Z[0][kOrb103.rep[s][1]] * Z[0][kOrb103.rep[s][2]];
      const float b1 = Z[1][kOrb103.rep[s][0]] * Z[1][kOrb103.rep[s][1]] * Z[1][kOrb103.rep[s][2]];
      if (s + 1 < kStepsOrb) wn = wr[(s + 1) * 64];
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc, b0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc, b1, acc[1], 0, 0, 0);
      wc = wn;
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_s_setprio(1);
    int64_t ostride = a.out_stride;
    int tmax = a.T;
    asm volatile("" : "+s"(ostride), "+s"(tmax));      // keep the addressing inside the loop (see predict103_slice_kernel)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t p = tile * kPix + wave * 32 + h * 16 + i;
      if (p < a.npix) {
        float* orow = a.out + (size_t)(4 * g) * ostride + p;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = predict_activation(acc[h][r], a.act);
          if (bad[h]) v = __uint_as_float(0x7fc00000u);
          if (4 * g + r < tmax) orow[(size_t)r * ostride] = v;
        }
      }
    }
  }
}

static size_t predict_generic_lds(int kpad, int n_in) {
  return ((size_t)kPredPix * (kpad + 1) + (size_t)kPredPix * (n_in + 1) + kPredPix) * sizeof(float);
}

// The predict kernel of a shape, the one rule behind launch_predict and hsr_polyfeat_predict_kernel: 10 inputs at degree 3 with
// the orbit rows on the device and T <= 512 take the MFMA kernels above (0 x16 for T <= 16, else slice<per> with per = the
// 32-target tiles of a slice: 1 .. 3); every other shape takes the generic predict_kernel<1 / 2 / 4> (4 .. 6, by the target
// tiles a wave pair covers), or none (-1) when its feature tile does not fit in LDS.
static int predict_slot(int n_in, int nfeat, int degree, int T, bool orb_rows) {
  const int tt = (T + 31) / 32;
  if (degree == 3 && n_in == 10 && nfeat == 285 && orb_rows && tt <= 16) {
    if (T <= 16) return 0;
    const int slices = (tt + 2) / 3;
    return (tt + slices - 1) / slices;
  }
  if (predict_generic_lds((nfeat + 1) & ~1, n_in) > 150 * 1024) return -1;
  const int per_wave = (tt + 1) / 2;                    // target tiles a wave pair must cover
  return 4 + (per_wave <= 1 ? 0 : (per_wave <= 2 ? 1 : 2));
}

// Picks the predict kernel (predict_slot), its grid and its LDS for the shape in PredArgs, and launches it.
typedef void (*PredOrbKernel)(PredArgs, const int16_t*);
typedef void (*PredGenericKernel)(PredArgs);
static int launch_predict(const PredArgs& a, int degree, hipStream_t s, int npairs = 1) {
  static thread_local size_t configured[7] = {};     // per kernel: x16, slice<1 / 2 / 3>, predict_kernel<1 / 2 / 4>
  PredOrbKernel orb = nullptr;
  PredGenericKernel generic = nullptr;
  const void* kern;
  const char* what;
  int gx, slices = 1, threads, instance;
  size_t lds;
  const int16_t* rows = nullptr;
  const int tt = a.ttiles;
  const int slot = predict_slot(a.n_in, a.nfeat, degree, a.T, g_orb_rows_dev != nullptr);
  if (slot >= 0 && slot <= 3) {
    int waves, wgs_per_cu = 1;
    if (slot == 0) {                                    // 16-target tiles (v_mfma_f32_16x16x4_f32)
      orb = predict103_x16_kernel;
      what = "predict103_x16_kernel launch";
      waves = kX16Waves;
      wgs_per_cu = kX16Wgs;
      lds = (size_t)4 * kStepsOrb * 16 * 4;
      rows = g_orb_rows_dev;                            // kOrb103.src
      instance = kK4PredictX16;
    } else {
      // T <= 32: one 16-wave workgroup per CU, W (36.6 KB) staged once per CU (0.209 -> 0.199 ms);
      // T <= 512: slices of 64 or 96 targets, as few and as narrow as T allows
      slices = (tt + 2) / 3;
      const int per = slot;                             // 32-target tiles per slice: 1 only for tt == 1
      orb = per == 1 ? predict103_slice_kernel<1> : (per == 2 ? predict103_slice_kernel<2> : predict103_slice_kernel<3>);
      what = "predict103_slice_kernel launch";
      waves = slice_waves(per);
      lds = (size_t)2 * kStepsOrb2 * per * 32 * 4;
      rows = g_orb_rows_dev + 4 * kStepsOrb;            // kOrb2.src
      instance = kK4PredictSlice + (per - 1) * 2;
    }
    instance += pred_x2_arm(a.x, a.x_ps, a.x_cs) ? 0 : 1;   // the arm of pred_load10, pair 0's
    const int pix = 32 * waves;
    const int64_t tiles = (a.npix + pix - 1) / pix;
    gx = 256 * wgs_per_cu / slices;                     // one workgroup per CU in all (73 / 110 KB of LDS each), two for x16
    if (gx < 1) gx = 1;
    if (tiles < gx) gx = (int)tiles;
    threads = 64 * waves;
    kern = reinterpret_cast<const void*>(orb);
  } else {
    lds = predict_generic_lds(a.kpad, a.n_in);
    HSR_REQUIRE(slot >= 4, HSR_ERR_UNSUPPORTED, "hsr_polyfeat_predict: %zu bytes of LDS needed", lds);
    const int64_t tiles = (a.npix + kPredPix - 1) / kPredPix;
    gx = (int)(tiles < 512 ? tiles : 512);
    threads = kPredThreads;
    generic = slot == 4 ? predict_kernel<1> : (slot == 5 ? predict_kernel<2> : predict_kernel<4>);
    what = "predict_kernel launch";
    kern = reinterpret_cast<const void*>(generic);
    instance = kK4Predict + slot - 4;
  }
  // a batch shares the chip's workgroups among its pairs: fewer per pair, each walking more of its pair's tiles with W staged once
  // (which workgroup computes a tile does not change its bits)
  if (npairs > 1) gx = (gx + npairs - 1) / npairs;
  raise_lds_limit(kern, lds, configured[slot]);
  if (orb) hipLaunchKernelGGL(orb, dim3(gx, slices, npairs), dim3(threads), lds, s, a, rows);
  else hipLaunchKernelGGL(generic, dim3(gx, 1, npairs), dim3(threads), lds, s, a);
  return launched(kLaunchK4, what, instance);
}

static int ensure_table(int n_in, int degree) {
  if (g_table_nin == n_in && g_table_deg == degree && g_table_dev) return g_table_nfeat;
  const int nf = build_table(n_in, degree);
  if (nf < 0) return -1;
  std::vector<uint8_t> packed((size_t)nf * 4, 0);
  for (int f = 0; f < nf; ++f)
    for (int k = 0; k < 3; ++k) packed[(size_t)f * 4 + k] = g_table_host.idx[f][k];
  if (g_table_dev) (void)hipFree(g_table_dev);
  if (hipMalloc(&g_table_dev, packed.size()) != hipSuccess) return -1;
  if (hipMemcpy(g_table_dev, packed.data(), packed.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
  g_table_nin = n_in;
  g_table_deg = degree;
  g_table_nfeat = nf;
  if (g_orb_rows_dev == nullptr) {                     // the orbit orders of the predict103 kernels' K axis, once per process
    std::vector<int16_t> rows((size_t)4 * kStepsOrb + (size_t)2 * kStepsOrb2);
    for (int st = 0; st < kStepsOrb; ++st)
      for (int g = 0; g < 4; ++g) rows[(size_t)4 * st + g] = kOrb103.src[st][g];
    for (int st = 0; st < kStepsOrb2; ++st)
      for (int g = 0; g < 2; ++g) rows[(size_t)4 * kStepsOrb + 2 * st + g] = kOrb2.src[st][g];
    if (hipMalloc(&g_orb_rows_dev, rows.size() * sizeof(int16_t)) != hipSuccess ||
        hipMemcpy(g_orb_rows_dev, rows.data(), rows.size() * sizeof(int16_t), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      g_orb_rows_dev = nullptr;                        // without it the notebook's shape takes the generic kernel
    }
  }
  return nf;
}

}  // namespace hsr

using namespace hsr;

extern "C" int hsr_polyfeat_count(int32_t n_in, int32_t degree) {
  if (n_in < 1 || n_in > kMaxIn || degree < 1 || degree > 3) return -1;
  int64_t total = 0, c = 1;   // sum_{d=1..deg} C(n_in + d - 1, d)
  for (int d = 1; d <= degree; ++d) {
    c = c * (n_in + d - 1) / d;
    total += c;
  }
  return total <= kMaxFeat ? (int)total : -1;
}

extern "C" int hsr_polyfeat_table(int32_t n_in, int32_t degree, uint8_t* idx_out /* [nfeat][3] */) {
  const int nf = build_table(n_in, degree);
  HSR_REQUIRE(nf > 0 && idx_out, HSR_ERR_UNSUPPORTED, "hsr_polyfeat_table: n_in=%d degree=%d", n_in, degree);
  for (int f = 0; f < nf; ++f)
    for (int k = 0; k < 3; ++k) idx_out[f * 3 + k] = g_table_host.idx[f][k];
  g_table_nin = -1;   // host table was rebuilt: force the device copy to refresh on next use
  return HSR_OK;
}

extern "C" int hsr_polyfeat_predict_kernel(int32_t n_in, int32_t degree, int32_t T, int32_t orbit_rows) {
  const int nf = hsr_polyfeat_count(n_in, degree);
  const bool orb = orbit_rows < 0 ? g_orb_rows_dev != nullptr : orbit_rows != 0;
  const int slot = nf > 0 && T >= 1 ? predict_slot(n_in, nf, degree, T, orb) : -1;
  if (slot < 0) set_error("hsr_polyfeat_predict_kernel: no predict kernel for n_in=%d degree=%d T=%d", n_in, degree, T);
  return slot;
}

// Not a launch-path call: uploads the monomial table once per (n_in, degree) (hipMalloc + copy).
extern "C" int hsr_polyfeat_prepare(int32_t n_in, int32_t degree) {
  HSR_REQUIRE(hsr_polyfeat_count(n_in, degree) > 0, HSR_ERR_UNSUPPORTED, "hsr_polyfeat_prepare: n_in=%d degree=%d",
              n_in, degree);
  HSR_REQUIRE(ensure_table(n_in, degree) > 0, HSR_ERR_HIP, "hsr_polyfeat_prepare: table upload failed");
  return HSR_OK;
}

extern "C" int hsr_polyfeat_expand_f64(const float* x_dev, int64_t x_rs, int64_t x_cs, const double* mean_dev,
                                       const double* scale_dev, int64_t n, int32_t n_in, int32_t degree,
                                       double* p_dev, int64_t ldp, int32_t ncols, hsr_stream_t stream) {
  HSR_REQUIRE(x_dev && mean_dev && scale_dev && p_dev && n > 0, HSR_ERR_INVALID, "hsr_polyfeat_expand_f64: bad argument");
  HSR_REQUIRE(g_table_nin == n_in && g_table_deg == degree && g_table_dev, HSR_ERR_INVALID,
              "hsr_polyfeat_expand_f64: call hsr_polyfeat_prepare(%d, %d) first", n_in, degree);
  HSR_REQUIRE(ncols >= g_table_nfeat + 1 && ldp >= ncols && ncols <= 4096, HSR_ERR_INVALID,
              "hsr_polyfeat_expand_f64: ncols=%d ldp=%lld (need ncols >= %d)", ncols, (long long)ldp, g_table_nfeat + 1);
  hipLaunchKernelGGL(expand_f64_kernel, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, (hipStream_t)stream, x_dev, x_rs,
                     x_cs, mean_dev, scale_dev, n, n_in, g_table_nfeat, g_table_dev, p_dev, ldp, ncols);
  return launched(kLaunchK4, "expand_f64_kernel launch", kK4Expand);
}

extern "C" int hsr_pair_expand_f64(const float* x_dev, int64_t pair_x, const double* mean_dev, const double* scale_dev,
                                   int64_t pair_ms, const float* y_dev, int64_t pair_y, const uint8_t* mask_dev, int64_t pair_m,
                                   int64_t npix, int32_t n_in, int32_t degree, int32_t T, double eps, double* q_dev, int64_t ldq,
                                   int64_t pair_q, int32_t na, int32_t npairs, hsr_stream_t stream) {
  HSR_REQUIRE(x_dev && mean_dev && scale_dev && y_dev && mask_dev && q_dev && npix > 0 && T >= 1 && npairs >= 1 &&
              npairs <= 65535, HSR_ERR_INVALID, "hsr_pair_expand_f64: bad argument");
  HSR_REQUIRE(g_table_nin == n_in && g_table_deg == degree && g_table_dev, HSR_ERR_INVALID,
              "hsr_pair_expand_f64: call hsr_polyfeat_prepare(%d, %d) first", n_in, degree);
  HSR_REQUIRE(na >= g_table_nfeat + 1 && ldq >= (int64_t)na + T && ldq <= 4096, HSR_ERR_INVALID,
              "hsr_pair_expand_f64: na=%d ldq=%lld T=%d (need na >= %d, ldq >= na + T)", na, (long long)ldq, T, g_table_nfeat + 1);
  HSR_REQUIRE(npairs == 1 || pair_q >= npix * ldq, HSR_ERR_INVALID, "hsr_pair_expand_f64: pair stride of Q overlaps");
  PairExpandArgs a{x_dev, mean_dev, scale_dev, y_dev, mask_dev, q_dev, pair_x, pair_ms, pair_y, pair_m, pair_q, npix, ldq,
                   n_in, g_table_nfeat, T, na, eps, g_table_dev};
  hipLaunchKernelGGL(pair_expand_f64_kernel, dim3((unsigned)((npix + 31) / 32), (unsigned)npairs), dim3(256), 0,
                     (hipStream_t)stream, a);
  return launched(kLaunchK4, "pair_expand_f64_kernel launch", kK4PairExpand);
}

// ------------------------------------------------------------------------------------------------
// The small steps of PolyRidge.fit around Gram and Cholesky, as three kernels instead of ~40 torch launches
// (200 us of a 700 us fit): StandardScaler statistics, assembly of the ridge system, model read-out.
// ------------------------------------------------------------------------------------------------
constexpr int kStatsBlocks = 64;

// per-block sums of d = x - K and d^2 (K = the column's first sample: the "shifted data" form, so that
// M2 = sum d^2 - (sum d)^2 / n loses nothing to a large mean); fixed order inside the block: every thread walks its rows
// once with all columns in registers (acc[2c] = sum d, acc[2c + 1] = sum d^2 of column c), then block_join4 (hsr_tree_dev.h)
__global__ __launch_bounds__(256) void ridge_stats_partial_kernel(const float* __restrict__ x, int64_t x_rs, int64_t x_cs,
                                                                  int64_t n, int n_in, double* __restrict__ work) {
  __shared__ double red[4][32];
  const int t = threadIdx.x;
  const int64_t rows = (n + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * rows;
  const int64_t r1 = r0 + rows < n ? r0 + rows : n;
  double acc[32], K[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    acc[2 * c] = acc[2 * c + 1] = 0.0;
    K[c] = c < n_in ? (double)x[c * x_cs] : 0.0;
  }
  // four rows per pass with all their loads issued before the first sum (a block walks <= 1024 rows: one exposed round trip
  // instead of four; r03 trace: 11.9 us for 1.2 MB); the sums keep their row order
  for (int64_t rb = r0 + t; rb < r1; rb += 4 * 256) {
    float v[4][16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t r = rb + q * 256;
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (c < n_in && r < r1) v[q][c] = x[r * x_rs + c * x_cs];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (rb + q * 256 >= r1) break;
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (c < n_in) {
          const double d = (double)v[q][c] - K[c];
          acc[2 * c] += d;
          acc[2 * c + 1] += d * d;
        }
    }
  }
  double* out = work + (size_t)blockIdx.x * n_in * 2;
  block_join4<32, 2>(acc, red, 2 * n_in, [&](int m, double s) { out[m] = s; });
}

// the blocks' sums joined (one wave per column, a lane per block, xor butterfly: a fixed order) -> [n, mean.., M2..] (the
// layout of PolyRidge.local_stats), mean and scale (zero variance -> 1)
__global__ __launch_bounds__(1024) void ridge_stats_finish_kernel(const float* __restrict__ x, int64_t x_cs, int64_t n, int n_in,
                                                                  int nblocks, const double* __restrict__ work,
                                                                  double* __restrict__ stats, double* __restrict__ mean_out,
                                                                  double* __restrict__ scale_out) {
  const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (threadIdx.x == 0) stats[0] = (double)n;
  if (c >= n_in) return;
  const double s1 = wave_sum(lane < nblocks ? work[((size_t)lane * n_in + c) * 2] : 0.0);
  const double s2 = wave_sum(lane < nblocks ? work[((size_t)lane * n_in + c) * 2 + 1] : 0.0);
  if (lane != 0) return;
  const double K = (double)x[c * x_cs];
  const double mean = K + s1 / (double)n;
  double m2 = s2 - s1 * s1 / (double)n;
  if (m2 < 0.0) m2 = 0.0;
  stats[1 + c] = mean;
  stats[1 + n_in + c] = m2;
  mean_out[c] = mean;
  const double sc = sqrt(m2 / (double)n);
  scale_out[c] = sc == 0.0 ? 1.0 : sc;
}

// G (na, na + tp) = [1 | Phi]^T [1 | Phi | Y]  ->  A = Phi_c^T Phi_c + alpha I padded to npad with an identity block,
// B = Phi_c^T (Y - ybar) padded with zero rows (the centred normal equations of Ridge(fit_intercept=True)):
//   A_ij = G[1+i][1+j] - s_i s_j / cnt (+ alpha on the diagonal),  B_it = G[1+i][na+t] - s_i ybar_t,
//   s = G[0][1..nf] (column sums), cnt = G[0][0], ybar_t = G[0][na+t] / cnt.   Also clears the Cholesky status word.
// Batched form: blockIdx.y is the pair (G, A, Bm offset by their pair strides, one status word per pair), and a pair without a
// single training row (cnt == 0) gets the identity system instead of 0 / 0, so that its factorisation stays finite.
__global__ __launch_bounds__(256) void ridge_assemble_kernel(const double* __restrict__ G, int64_t ldg, int na, int nf, int T,
                                                             double alpha, double* __restrict__ A, int npad,
                                                             double* __restrict__ Bm, int64_t ldb, int32_t* __restrict__ info,
                                                             int64_t pair_g, int64_t pair_a, int64_t pair_b, int empty_identity) {
  G += blockIdx.y * pair_g;
  A += blockIdx.y * pair_a;
  Bm += blockIdx.y * pair_b;
  info += blockIdx.y;
  const double cnt = G[0];
  const bool empty = empty_identity && cnt == 0.0;
  const int64_t total = (int64_t)npad * (npad + T);
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int i = (int)(e / (npad + T)), j = (int)(e % (npad + T));
    if (j < npad) {
      double v = i == j ? 1.0 : 0.0;
      if (i < nf && j < nf && !empty) {
        v = G[(size_t)(1 + i) * ldg + 1 + j] - (G[1 + i] * G[1 + j]) / cnt;
        if (i == j) v += alpha;
      }
      A[(size_t)i * npad + j] = v;
    } else {
      const int t = j - npad;
      double v = 0.0;
      if (i < nf && !empty) v = G[(size_t)(1 + i) * ldg + na + t] - G[1 + i] * (G[na + t] / cnt);
      Bm[(size_t)i * ldb + t] = v;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *info = 0;
}

// W (nf, T) float64 solution -> intercept b = ybar - (s / cnt) . W (float64 and float32), W as float32 with a zero row up
// to kpad, mean and 1 / scale as float32: everything the predict kernels read.  A block owns 32 targets: s / cnt goes to
// LDS once, eight thread groups take every eighth feature (coalesced over the targets), partial sums joined in group
// order.  (First version: one thread per target walking all features with a division per step - 65 us for T = 32.)
// Batched form: blockIdx.y is the pair, every operand offset by its pair stride (FinishPairs); with `status` a pair's word
// becomes 0 (fitted), 1 (no training row) or 2 (non-positive pivot), and a pair whose word is not 0 gets NaN intercepts, so that
// every prediction of it is NaN whatever its failed factorisation left in W.
struct FinishPairs {
  int64_t g, w, ms, b, w32, mi;      // element strides between pairs: G, Wm, mean / scale, b64 / b32, W32, mean32 / inv32
  const int32_t* info;               // Cholesky status words, one per pair (batched form only)
  int32_t* status;
};

__global__ __launch_bounds__(256) void ridge_finish_kernel(const double* __restrict__ G, int na, int nf, int T,
                                                           const double* __restrict__ Wm, int64_t ldw, const double* __restrict__ mean,
                                                           const double* __restrict__ scale, int n_in, int kpad,
                                                           double* __restrict__ b64, float* __restrict__ b32,
                                                           float* __restrict__ W32, float* __restrict__ mean32,
                                                           float* __restrict__ inv32, const FinishPairs pp) {
  __shared__ double sc[kMaxFeat];
  __shared__ double part[8][32];
  const int64_t pr = blockIdx.y;
  G += pr * pp.g;
  Wm += pr * pp.w;
  mean += pr * pp.ms;
  scale += pr * pp.ms;
  b64 += pr * pp.b;
  b32 += pr * pp.b;
  W32 += pr * pp.w32;
  mean32 += pr * pp.mi;
  inv32 += pr * pp.mi;
  const double cnt = G[0];
  const int status = pp.status ? (cnt == 0.0 ? 1 : (pp.info[pr] != 0 ? 2 : 0)) : 0;
  if (pp.status && blockIdx.x == 0 && threadIdx.x == 0) pp.status[pr] = status;
  const int tid = threadIdx.x;
  for (int f = tid; f < nf; f += 256) sc[f] = G[1 + f] / cnt;
  __syncthreads();
  const int grp = tid >> 5, tt = tid & 31;
  const int t = blockIdx.x * 32 + tt;
  double acc = 0.0;
  if (t < T)
    for (int f = grp; f < nf; f += 8) acc += sc[f] * Wm[(size_t)f * ldw + t];
  part[grp][tt] = acc;
  __syncthreads();
  if (grp == 0 && t < T) {
    double a = part[0][tt];
#pragma unroll
    for (int g = 1; g < 8; ++g) a += part[g][tt];
    const double b = status != 0 ? __builtin_nan("") : G[na + t] / cnt - a;
    b64[t] = b;
    b32[t] = (float)b;
  }
  const int64_t gid = (int64_t)blockIdx.x * 256 + tid, gsz = (int64_t)gridDim.x * 256;
  for (int64_t e = gid; e < (int64_t)kpad * T; e += gsz) {
    const int f = (int)(e / T), tq = (int)(e % T);
    W32[e] = f < nf ? (float)Wm[(size_t)f * ldw + tq] : 0.0f;
  }
  for (int64_t c = gid; c < n_in; c += gsz) {
    mean32[c] = (float)mean[c];
    inv32[c] = (float)(1.0 / scale[c]);
  }
}

extern "C" size_t hsr_ridge_stats_work_bytes(int32_t n_in) {
  return n_in >= 1 && n_in <= 16 ? (size_t)kStatsBlocks * n_in * 2 * sizeof(double) : 0;
}

extern "C" int hsr_ridge_stats(const float* x_dev, int64_t x_rs, int64_t x_cs, int64_t n, int32_t n_in, double* work_dev,
                               double* stats_dev, double* mean_dev, double* scale_dev, hsr_stream_t stream) {
  HSR_REQUIRE(x_dev && work_dev && stats_dev && mean_dev && scale_dev, HSR_ERR_INVALID, "hsr_ridge_stats: NULL pointer");
  HSR_REQUIRE(n >= 1 && n_in >= 1 && n_in <= 16, HSR_ERR_INVALID, "hsr_ridge_stats: n=%lld n_in=%d", (long long)n, n_in);
  int nblocks = (int)((n + 1023) / 1024);
  if (nblocks > kStatsBlocks) nblocks = kStatsBlocks;
  hipLaunchKernelGGL(ridge_stats_partial_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, x_dev, x_rs, x_cs, n, n_in,
                     work_dev);
  static_assert(kStatsBlocks <= 64, "one lane per block");
  hipLaunchKernelGGL(ridge_stats_finish_kernel, dim3(1), dim3(64 * n_in), 0, (hipStream_t)stream, x_dev, x_cs, n, n_in, nblocks,
                     work_dev, stats_dev, mean_dev, scale_dev);
  return launched(kLaunchK4, "ridge_stats_kernel launch", kK4StatsPartial, kK4StatsFinish);
}

// One launch of ridge_assemble_kernel behind hsr_ridge_assemble (npairs = 1, strides 0, empty_identity = 0) and its batched form:
// the grid's x extent depends on the shape alone, so a pair gets the same bits alone as in a batch.  `who` names the entry point.
static int launch_assemble(const char* who, const double* g_dev, int64_t ldg, int32_t na, int32_t nf, int32_t T, double alpha,
                           double* a_dev, int32_t npad, double* b_dev, int64_t ldb, int32_t* info_dev, int64_t pair_g,
                           int64_t pair_a, int64_t pair_b, int32_t npairs, int empty_identity, hipStream_t s) {
  HSR_REQUIRE(g_dev && a_dev && b_dev && info_dev, HSR_ERR_INVALID, "%s: NULL pointer", who);
  HSR_REQUIRE(nf >= 1 && na >= nf + 1 && npad >= nf && T >= 1 && ldg >= na + T && ldb >= T, HSR_ERR_INVALID,
              "%s: bad shape (na=%d nf=%d npad=%d T=%d)", who, na, nf, npad, T);
  const int64_t total = (int64_t)npad * (npad + T);
  const int grid = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
  hipLaunchKernelGGL(ridge_assemble_kernel, dim3(grid, (unsigned)npairs), dim3(256), 0, s, g_dev, ldg, na, nf, T, alpha, a_dev,
                     npad, b_dev, ldb, info_dev, pair_g, pair_a, pair_b, empty_identity);
  return launched(kLaunchK4, "ridge_assemble_kernel launch", kK4Assemble);
}

// One launch of ridge_finish_kernel behind hsr_ridge_finish (npairs = 1, an empty FinishPairs: no status word, no NaN intercepts)
// and its batched form.  The overlap check stands here, after the feature limit, where the batched form always had it.
static int launch_finish(const char* who, const double* g_dev, int32_t na, int32_t nf, int32_t T, const double* w_dev, int64_t ldw,
                         const double* mean_dev, const double* scale_dev, int32_t n_in, int32_t kpad, double* b64_dev,
                         float* b32_dev, float* w32_dev, float* mean32_dev, float* inv32_dev, const FinishPairs& pp,
                         int32_t npairs, hipStream_t s) {
  HSR_REQUIRE(g_dev && w_dev && mean_dev && scale_dev && b64_dev && b32_dev && w32_dev && mean32_dev && inv32_dev,
              HSR_ERR_INVALID, "%s: NULL pointer", who);
  HSR_REQUIRE(nf >= 1 && na >= nf + 1 && T >= 1 && ldw >= T && kpad >= nf && n_in >= 1, HSR_ERR_INVALID, "%s: bad shape", who);
  HSR_REQUIRE(nf <= kMaxFeat, HSR_ERR_UNSUPPORTED, "%s: nf=%d > %d", who, nf, kMaxFeat);
  HSR_REQUIRE(npairs == 1 || (pp.b >= T && pp.w32 >= (int64_t)kpad * T && pp.mi >= n_in), HSR_ERR_INVALID,
              "%s: output pair strides overlap", who);
  int grid = (T + 31) / 32;                       // a block per 32 targets; the float32 copies ride along grid-strided,
  const int64_t cpy = ((int64_t)kpad * T + 1023) / 1024;   // so there are at least enough blocks for 4 elements per thread
  if (cpy > grid) grid = (int)(cpy < 64 ? cpy : 64);
  hipLaunchKernelGGL(ridge_finish_kernel, dim3(grid, (unsigned)npairs), dim3(256), 0, s, g_dev, na, nf, T, w_dev, ldw, mean_dev,
                     scale_dev, n_in, kpad, b64_dev, b32_dev, w32_dev, mean32_dev, inv32_dev, pp);
  return launched(kLaunchK4, "ridge_finish_kernel launch", kK4Finish);
}

extern "C" int hsr_ridge_assemble(const double* g_dev, int64_t ldg, int32_t na, int32_t nf, int32_t T, double alpha,
                                  double* a_dev, int32_t npad, double* b_dev, int64_t ldb, int32_t* info_dev,
                                  hsr_stream_t stream) {
  return launch_assemble("hsr_ridge_assemble", g_dev, ldg, na, nf, T, alpha, a_dev, npad, b_dev, ldb, info_dev, 0, 0, 0, 1, 0,
                         (hipStream_t)stream);
}

extern "C" int hsr_ridge_finish(const double* g_dev, int32_t na, int32_t nf, int32_t T, const double* w_dev, int64_t ldw,
                                const double* mean_dev, const double* scale_dev, int32_t n_in, int32_t kpad,
                                double* b64_dev, float* b32_dev, float* w32_dev, float* mean32_dev, float* inv32_dev,
                                hsr_stream_t stream) {
  return launch_finish("hsr_ridge_finish", g_dev, na, nf, T, w_dev, ldw, mean_dev, scale_dev, n_in, kpad, b64_dev, b32_dev, w32_dev,
                       mean32_dev, inv32_dev, FinishPairs{}, 1, (hipStream_t)stream);
}

extern "C" int hsr_ridge_assemble_batched(const double* g_dev, int64_t ldg, int64_t pair_g, int32_t na, int32_t nf, int32_t T,
                                          double alpha, double* a_dev, int32_t npad, int64_t pair_a, double* b_dev, int64_t ldb,
                                          int64_t pair_b, int32_t* info_dev, int32_t npairs, hsr_stream_t stream) {
  HSR_REQUIRE(npairs >= 1 && npairs <= 65535, HSR_ERR_INVALID, "hsr_ridge_assemble_batched: bad pair count P=%d", npairs);
  HSR_REQUIRE(npairs == 1 || (pair_g >= (int64_t)na * ldg && pair_a >= (int64_t)npad * npad && pair_b >= (int64_t)npad * ldb),
              HSR_ERR_INVALID, "hsr_ridge_assemble_batched: pair strides overlap");
  return launch_assemble("hsr_ridge_assemble_batched", g_dev, ldg, na, nf, T, alpha, a_dev, npad, b_dev, ldb, info_dev, pair_g,
                         pair_a, pair_b, npairs, 1, (hipStream_t)stream);
}

extern "C" int hsr_ridge_finish_batched(const double* g_dev, int64_t pair_g, int32_t na, int32_t nf, int32_t T, const double* w_dev,
                                        int64_t ldw, int64_t pair_w, const double* mean_dev, const double* scale_dev, int64_t pair_ms,
                                        int32_t n_in, int32_t kpad, double* b64_dev, float* b32_dev, int64_t pair_b, float* w32_dev,
                                        int64_t pair_w32, float* mean32_dev, float* inv32_dev, int64_t pair_mi,
                                        const int32_t* info_dev, int32_t* status_dev, int32_t npairs, hsr_stream_t stream) {
  HSR_REQUIRE(info_dev && status_dev, HSR_ERR_INVALID, "hsr_ridge_finish_batched: NULL pointer");
  HSR_REQUIRE(npairs >= 1 && npairs <= 65535, HSR_ERR_INVALID, "hsr_ridge_finish_batched: bad shape");
  return launch_finish("hsr_ridge_finish_batched", g_dev, na, nf, T, w_dev, ldw, mean_dev, scale_dev, n_in, kpad, b64_dev, b32_dev,
                       w32_dev, mean32_dev, inv32_dev,
                       FinishPairs{pair_g, pair_w, pair_ms, pair_b, pair_w32, pair_mi, info_dev, status_dev}, npairs,
                       (hipStream_t)stream);
}

// The checks, the PredArgs and the launch that the single (npairs = 1, pair strides 0) and the batched predict share.
static int predict_entry(const char* who, const float* x_dev, int64_t x_ps, int64_t x_cs, int64_t pair_x, const float* mean_dev,
                         const float* inv_scale_dev, int64_t pair_mi, int64_t npix, int32_t n_in, int32_t degree,
                         const float* w_dev, int64_t ldw, int64_t pair_w, const float* bias_dev, int64_t pair_b, int32_t T,
                         int32_t activation, int32_t nan_bad_pixels, float nodata, int32_t use_nodata, float* out_dev,
                         int64_t out_stride, int64_t pair_out, int32_t npairs, hipStream_t s) {
  HSR_REQUIRE(x_dev && mean_dev && inv_scale_dev && w_dev && bias_dev && out_dev, HSR_ERR_INVALID, "%s: NULL pointer", who);
  HSR_REQUIRE(npix > 0 && T >= 1 && ldw >= T && out_stride >= npix, HSR_ERR_INVALID, "%s: bad shape", who);
  HSR_REQUIRE(g_table_nin == n_in && g_table_deg == degree && g_table_dev, HSR_ERR_INVALID,
              "%s: call hsr_polyfeat_prepare(%d, %d) first", who, n_in, degree);
  const PredArgs a{x_dev, x_ps, x_cs, mean_dev, inv_scale_dev, npix, n_in, g_table_nfeat, (g_table_nfeat + 1) & ~1, g_table_dev,
                   w_dev, ldw, bias_dev, T, (T + 31) / 32, activation, nan_bad_pixels != 0, use_nodata != 0, nodata, out_dev,
                   out_stride, pair_x, pair_mi, pair_w, pair_b, pair_out};
  return launch_predict(a, degree, s, npairs);
}

extern "C" int hsr_polyfeat_predict(const float* x_dev, int64_t x_ps, int64_t x_cs, const float* mean_dev,
                                    const float* inv_scale_dev, int64_t npix, int32_t n_in, int32_t degree,
                                    const float* w_dev, int64_t ldw, const float* bias_dev, int32_t T,
                                    int32_t activation, float* out_dev, int64_t out_stride, hsr_stream_t stream) {
  return hsr_polyfeat_predict_cube(x_dev, x_ps, x_cs, mean_dev, inv_scale_dev, npix, n_in, degree, w_dev, ldw, bias_dev, T,
                                   activation, 0, 0.0f, 0, out_dev, out_stride, stream);
}

extern "C" int hsr_polyfeat_predict_cube(const float* x_dev, int64_t x_ps, int64_t x_cs, const float* mean_dev,
                                         const float* inv_scale_dev, int64_t npix, int32_t n_in, int32_t degree,
                                         const float* w_dev, int64_t ldw, const float* bias_dev, int32_t T,
                                         int32_t activation, int32_t nan_bad_pixels, float nodata, int32_t use_nodata,
                                         float* out_dev, int64_t out_stride, hsr_stream_t stream) {
  return predict_entry("hsr_polyfeat_predict", x_dev, x_ps, x_cs, 0, mean_dev, inv_scale_dev, 0, npix, n_in, degree, w_dev, ldw, 0,
                       bias_dev, 0, T, activation, nan_bad_pixels, nodata, use_nodata, out_dev, out_stride, 0, 1,
                       (hipStream_t)stream);
}

extern "C" int hsr_polyfeat_predict_cube_batched(const float* x_dev, int64_t x_ps, int64_t x_cs, int64_t pair_x,
                                                 const float* mean_dev, const float* inv_scale_dev, int64_t pair_mi, int64_t npix,
                                                 int32_t n_in, int32_t degree, const float* w_dev, int64_t ldw, int64_t pair_w,
                                                 const float* bias_dev, int64_t pair_b, int32_t T, int32_t activation,
                                                 int32_t nan_bad_pixels, float nodata, int32_t use_nodata, float* out_dev,
                                                 int64_t out_stride, int64_t pair_out, int32_t npairs, hsr_stream_t stream) {
  HSR_REQUIRE(npairs >= 1 && npairs <= 65535, HSR_ERR_INVALID, "hsr_polyfeat_predict_cube_batched: bad shape");
  HSR_REQUIRE(npairs == 1 || pair_out >= (int64_t)T * out_stride, HSR_ERR_INVALID,
              "hsr_polyfeat_predict_cube_batched: output pair stride %lld overlaps", (long long)pair_out);
  return predict_entry("hsr_polyfeat_predict_cube_batched", x_dev, x_ps, x_cs, pair_x, mean_dev, inv_scale_dev, pair_mi, npix, n_in,
                       degree, w_dev, ldw, pair_w, bias_dev, pair_b, T, activation, nan_bad_pixels, nodata, use_nodata, out_dev,
                       out_stride, pair_out, npairs, (hipStream_t)stream);
}
