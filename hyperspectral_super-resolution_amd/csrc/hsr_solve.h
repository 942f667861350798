// np.polyfit from the moment sums: the per-band solve shared by the stand-alone solve / reduce+solve kernels
// (hsr_poly.hip), the host-side hsr_poly_solve_host and the fused tail of K1 (hsr_srf.hip).  One definition, so that
// every caller produces the same bits.  jacobi_eigen, the sweep under its rank-revealing path, also serves the affine colour solve
// (hsr_color.hip, through solve_band_jacobi) and the shift model of the co-registration (hsr_coreg.hip, a 3 x 3 of its own).
#pragma once
#include "hsr_common.h"

namespace hsr {

// ------------------------------------------------------------------------------------------------
// solve: np.polyfit from the moments
// ------------------------------------------------------------------------------------------------
// np.polyfit(x, y, deg): V = vander(x, deg+1) (highest power first), s_j = ||V[:,j]||, least squares
// of (V/s) c' = y by SVD with rcond = len(x)*eps, c = c'/s.  From the moments:
//   A_jk = S_{(d-j)+(d-k)} / (s_j s_k),  s_j = sqrt(S_{2(d-j)}),  rhs_j = T_{d-j} / s_j,
// eigen-decompose A (cyclic Jacobi, <= 5x5) and apply the pseudo-inverse keeping the eigenvalues
// above max(rcond^2, kRankFloor) * max (singular values of V/s are the square roots).
// Rank-revealing path: symmetric cyclic Jacobi on the scaled Gram, pseudo-inverse with NumPy's cut-off.
//
// kRankFloor: the Gram is built from rounded power sums, so it resolves eigenvalues only down to its own rounding.  The null
// eigenvalue of an exactly rank-deficient band (repeated float32 values whose powers round in float64, e.g. x = 0.3) comes out
// at ~eps * lmax, not rcond^2 * lmax; proj / lambda then inflated noise into the null space (the fitted values on the training
// x stayed right, the polynomial elsewhere did not: np.polyfit returns the minimum-norm solution).  Measured with the host twin
// on NumPy-summed moments (1..4 distinct values, deg <= 4, scales 1e-3..1e3): 2 eps suffices up to 1e5 pixels; at 1e6 pixels the
// sums' own rounding puts the null eigenvalue at 4..8 eps.  A larger floor drops real directions of narrow-range bands (cond(V/s)
// ~3e7: at 8 eps, x in [0.79, 0.81] at deg 3 went from 5e-7 to 4e-5 off np.polyfit), so 4 eps it is; see DESIGN.md (solve).
constexpr double kRankFloor = 4 * 2.220446049250313e-16;
// Storage is flat and caller-provided (rows of kSolveLd doubles): the stand-alone kernels and the host hand in local
// arrays, the fused tail of K1 hands in LDS so that the dynamically indexed matrices do not make K1 a scratch-using
// kernel.  Same arithmetic in the same order either way.
constexpr int kSolveLd = HSR_MAX_DEG + 1;
constexpr int kSolveWork = 2 * kSolveLd * kSolveLd + 2 * kSolveLd;   // doubles of work space per band: A, V, rhs, s

// Eigen-decomposition of a symmetric n x n matrix (rows of LD doubles) by cyclic Jacobi, at most 40 sweeps: A ends diagonal (the
// eigenvalues), the columns of V are the eigenvectors.  The sweep only; every caller applies its own pseudo-inverse rule.
template <int LD>
__host__ __device__ inline void jacobi_eigen(double* A, double* V, int n) {
  for (int j = 0; j < n; ++j)
    for (int k = 0; k < n; ++k) V[j * LD + k] = j == k ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 40; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int p = 0; p < n; ++p) {
      diag += A[p * LD + p] * A[p * LD + p];
      for (int q = p + 1; q < n; ++q) off += A[p * LD + q] * A[p * LD + q];
    }
    if (off <= 1e-36 * diag) break;
    for (int p = 0; p < n; ++p) {
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[p * LD + q];
        if (fabs(apq) < 1e-300) continue;
        const double theta = (A[q * LD + q] - A[p * LD + p]) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), sn = tt * c;
        for (int k = 0; k < n; ++k) {
          const double akp = A[k * LD + p], akq = A[k * LD + q];
          A[k * LD + p] = c * akp - sn * akq;
          A[k * LD + q] = sn * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {
          const double apk = A[p * LD + k], aqk = A[q * LD + k];
          A[p * LD + k] = c * apk - sn * aqk;
          A[q * LD + k] = sn * apk + c * aqk;
        }
        for (int k = 0; k < n; ++k) {
          const double vkp = V[k * LD + p], vkq = V[k * LD + q];
          V[k * LD + p] = c * vkp - sn * vkq;
          V[k * LD + q] = sn * vkp + c * vkq;
        }
      }
    }
  }
}

__host__ __device__ inline void solve_band_jacobi(double* A, double* V, const double* rhs, const double* s, int n,
                                                  double count, double* coef) {
  jacobi_eigen<kSolveLd>(A, V, n);
  double lmax = 0.0;
  for (int i = 0; i < n; ++i) lmax = A[i * kSolveLd + i] > lmax ? A[i * kSolveLd + i] : lmax;
  const double rcond = count * 2.220446049250313e-16;
  const double thresh = (rcond * rcond > kRankFloor ? rcond * rcond : kRankFloor) * lmax;
  for (int j = 0; j < n; ++j) coef[j] = 0.0;
  for (int i = 0; i < n; ++i) {
    const double lam = A[i * kSolveLd + i];
    if (!(lam > thresh)) continue;
    double proj = 0.0;
    for (int k = 0; k < n; ++k) proj += V[k * kSolveLd + i] * rhs[k];
    proj /= lam;
    for (int j = 0; j < n; ++j) coef[j] += V[j * kSolveLd + i] * proj;
  }
  for (int j = 0; j < n; ++j) coef[j] /= s[j];
}

// Fast path: Cholesky of the scaled Gram with every loop unrolled (N is a template constant, so the
// whole factorisation lives in registers).  A pivot below 1e-13 (the scaled diagonal is exactly 1, so
// this is cond(V/s) > ~3e6) hands the band to the rank-revealing Jacobi path, which reproduces
// np.polyfit's singular-value cut-off; above it both paths agree to ~cond * eps.  So does
// trace(A^-1) = ||L^-1||_F^2 >= 1e14 (that trace lies in [1/lmin, n/lmin]): pivots bound lmin from
// above only, and an exactly rank-deficient Gram whose null vector has a small last component passes
// them with a last pivot of ~1e-12 (4 distinct x at deg 4, measured) - the Cholesky solve then puts
// noise into the null space.  1e14 leaves every band of cond(V/s) <~ 1e7 on this path, bits unchanged.
// EXTWORK: the Jacobi path works in ``work`` (kSolveWork doubles, e.g. LDS) instead of local arrays.
template <int DEG, bool EXTWORK = false>
__host__ __device__ inline void solve_band_t(const double* mom, long long min_count, double* coef, double* work = nullptr) {
  constexpr int n = DEG + 1;
  const double* S = mom;
  const double* T = mom + 2 * DEG + 1;
  const double count = S[0];
  if (!(count >= (double)min_count) || count < 1.0) {  // reference fallback: identity polynomial
#pragma unroll
    for (int j = 0; j < n; ++j) coef[j] = j == n - 2 ? 1.0 : 0.0;
    return;
  }
  double s[HSR_MAX_DEG + 1], A[HSR_MAX_DEG + 1][HSR_MAX_DEG + 1], rhs[HSR_MAX_DEG + 1];
#pragma unroll
  for (int j = 0; j < n; ++j) {
    const double d = S[2 * (DEG - j)];
    s[j] = d > 0.0 ? sqrt(d) : 1.0;
  }
#pragma unroll
  for (int j = 0; j < n; ++j) {
    rhs[j] = T[DEG - j] / s[j];
#pragma unroll
    for (int k = 0; k < n; ++k) A[j][k] = S[(DEG - j) + (DEG - k)] / (s[j] * s[k]);
  }
  double L[n][n];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < n; ++j) {
    double d = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    ok = ok && (d > 1e-13);
    const double ljj = sqrt(d > 1e-13 ? d : 1.0);
    L[j][j] = ljj;
#pragma unroll
    for (int i = j + 1; i < n; ++i) {
      double v = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v / ljj;
    }
  }
  if (ok) {
    double z[n];
#pragma unroll
    for (int i = 0; i < n; ++i) {
      double v = rhs[i];
#pragma unroll
      for (int k = 0; k < i; ++k) v -= L[i][k] * z[k];
      z[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = n - 1; i >= 0; --i) {
      double v = z[i];
#pragma unroll
      for (int k = i + 1; k < n; ++k) v -= L[k][i] * z[k];
      z[i] = v / L[i][i];
    }
#pragma unroll
    for (int j = 0; j < n; ++j) coef[j] = z[j] / s[j];
    // trace(A^-1), column i of L^-1 by forward substitution over rows i..n-1.  After the solve, so that its registers are
    // free again (the fused tail of K1 inlines this); a band that fails it is solved again below, overwriting coef.
    double tr = 0.0;
#pragma unroll
    for (int i = 0; i < n; ++i) {
      double w[n];
#pragma unroll
      for (int k = i; k < n; ++k) {
        double v = k == i ? 1.0 : 0.0;
#pragma unroll
        for (int m = i; m < k; ++m) v -= L[k][m] * w[m];
        w[k] = v / L[k][k];
        tr += w[k] * w[k];
      }
    }
    if (tr < 1e14) return;
  }
  // rank-revealing path: the matrices move to flat storage with static indices (no scratch when ``work`` is LDS).  A is
  // formed again from the moments (the same expression, so the same bits): it need not stay live through the factorisation.
  double* wk = work;
  double local[EXTWORK ? 1 : kSolveWork];
  if constexpr (!EXTWORK) wk = local;
  double* Af = wk;
  double* Vf = wk + kSolveLd * kSolveLd;
  double* rf = Vf + kSolveLd * kSolveLd;
  double* sf = rf + kSolveLd;
#pragma unroll
  for (int j = 0; j < n; ++j) {
    rf[j] = rhs[j];
    sf[j] = s[j];
#pragma unroll
    for (int k = 0; k < n; ++k) Af[j * kSolveLd + k] = S[(DEG - j) + (DEG - k)] / (s[j] * s[k]);
  }
  solve_band_jacobi(Af, Vf, rf, sf, n, count, coef);
}

// The same solve with the Jacobi matrices in caller-provided storage (kSolveWork doubles, e.g. LDS): keeps a kernel free
// of scratch memory.
__host__ __device__ inline void solve_band_work(const double* mom, int deg, long long min_count, double* coef, double* work) {
  switch (deg) {
    case 1: solve_band_t<1, true>(mom, min_count, coef, work); break;
    case 2: solve_band_t<2, true>(mom, min_count, coef, work); break;
    case 3: solve_band_t<3, true>(mom, min_count, coef, work); break;
    default: solve_band_t<4, true>(mom, min_count, coef, work); break;
  }
}

__host__ __device__ inline void solve_band(const double* mom, int deg, long long min_count, double* coef) {
  switch (deg) {
    case 1: solve_band_t<1>(mom, min_count, coef); break;
    case 2: solve_band_t<2>(mom, min_count, coef); break;
    case 3: solve_band_t<3>(mom, min_count, coef); break;
    default: solve_band_t<4>(mom, min_count, coef); break;
  }
}

}  // namespace hsr
