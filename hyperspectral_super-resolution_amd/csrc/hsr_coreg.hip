// Co-registration of an S2 scene to an EMIT scene on gfx950 (C ABI and the definitions: include/hsr_coreg.h): the score surface of
// every tie point, the peak records, the shift model with its host twin, and the cubic warp.
//
// Reference: s2_emit/arosics_coreg.py (coregister_s2_granule_to_emit_granule) hands the stage to AROSICS and rasterio; the
// algorithm here is the header's.  Structure:
//   surface  one workgroup per (tie point, phase).  A shift splits as dy = f qy + ry, dx = f qx + rx; for a fixed phase (ry, rx)
//            the box sums every candidate needs are ONE non-overlapping block-sum image of the region, (w + span)^2 doubles in
//            LDS (11 KB at w = 32, R = 12, f = 6), built from one pass over the S2 region.  A candidate is then a w x w
//            correlation of the EMIT window (LDS, float) against a shifted view of that image: a wave per candidate, no
//            workgroup barrier and no atomics after the staging.
//   peaks    one wave per tie point: a strided scan and a shuffle reduction that keeps the first of equal maxima.
//   fit      one thread of one workgroup: the sums are defined in record order.  It is bound by the latency of its loads (1 ms
//            for 1482 records); the host twin is the same code.
//   warp     a 64 x 16 output tile per workgroup and band; the tile's source footprint (bounding box of the corners, a 3-pixel
//            halo, the slope spread) is staged in LDS in the raw dtype and the 16 taps of a pixel come from there; a pixel whose
//            taps leave the staged box, or a tile whose box does not fit, reads its (clamped, in-plane) taps from global memory.
#include <math.h>
#include <string.h>

#include "hsr_common.h"
#include "hsr_cubic_dev.h"
#include "hsr_solve.h"
#include "hsr_tree_dev.h"
#include "../../include/hsr_coreg.h"

namespace hsr {

constexpr int kRec = HSR_COREG_RECORD, kModel = HSR_COREG_MODEL;
constexpr int kWarpTW = 64, kWarpTH = 16;            // output tile of the warp
constexpr size_t kWarpLdsLimit = 32 * 1024;          // a staged footprint above this goes to the direct-gather instance

__host__ __device__ inline int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
__host__ __device__ inline int ceil_div(int a, int b) { return -floor_div(-a, b); }

// The region test of hsr_coreg.h: the w x w window inside the EMIT plane and its whole search region inside the S2 plane.
__host__ __device__ inline bool region_inside(int64_t i0, int64_t j0, int w, int f, int R, int he, int we, int hs, int ws) {
  return i0 >= 0 && j0 >= 0 && i0 + w <= he && j0 + w <= we && f * i0 - R >= 0 && f * j0 - R >= 0 &&
         f * (i0 + w - 1) + R + f - 1 <= (int64_t)hs - 1 && f * (j0 + w - 1) + R + f - 1 <= (int64_t)ws - 1;
}

template <typename T>
__device__ __forceinline__ bool s2_valid(T v, bool has_nodata, double nodata);
template <>
__device__ __forceinline__ bool s2_valid<float>(float v, bool has_nodata, double nodata) {
  return finite_f32(v) && !(has_nodata && (double)v == nodata);
}
template <>
__device__ __forceinline__ bool s2_valid<uint16_t>(uint16_t v, bool has_nodata, double nodata) {
  return !(has_nodata && (double)v == nodata);
}

// ------------------------------------------------------------------------------------------------------------------------------
// stage 1: the score surfaces
// ------------------------------------------------------------------------------------------------------------------------------
struct SurfaceArgs {
  const float* emit;
  int64_t emit_rs;
  int he, we;
  const uint8_t* mask;
  int64_t mask_rs;
  const void* s2;
  int64_t s2_rs;
  int hs, ws;
  int has_nodata;
  double nodata;
  const int32_t* origins;
  int w, f, R, min_valid;
  double* surface;
};

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

template <typename T>
__global__ __launch_bounds__(256) void coreg_surface_kernel(const SurfaceArgs a) {
  extern __shared__ double coreg_smem[];
  const int f = a.f, R = a.R, w = a.w, D = 2 * R + 1;
  const int point = (int)(blockIdx.x / (unsigned)(f * f)), phase = (int)(blockIdx.x % (unsigned)(f * f));
  const int ry = phase / f, rx = phase % f;
  // the candidates of this phase: dy = f qy + ry in [-R, R], and the same for columns
  const int qy0 = ceil_div(-R - ry, f), qy1 = floor_div(R - ry, f);
  const int qx0 = ceil_div(-R - rx, f), qx1 = floor_div(R - rx, f);
  if (qy0 > qy1 || qx0 > qx1) return;
  const int ncy = qy1 - qy0 + 1, ncx = qx1 - qx0 + 1;
  const int i0 = a.origins[2 * point], j0 = a.origins[2 * point + 1];
  double* surf = a.surface + (size_t)point * D * D;
  const int tid = threadIdx.x;
  if (!region_inside(i0, j0, w, f, R, a.he, a.we, a.hs, a.ws)) {
    for (int c = tid; c < ncy * ncx; c += 256)
      surf[(size_t)(f * (qy0 + c / ncx) + ry + R) * D + (f * (qx0 + c % ncx) + rx + R)] = NAN;
    return;
  }
  const int nby = w + ncy - 1, nbx = w + ncx - 1;
  double* B = coreg_smem;                                       // block sums, NaN where a box is invalid
  float* E = reinterpret_cast<float*>(coreg_smem + nby * nbx);  // the EMIT window, NaN where a pixel is invalid
  for (int p = tid; p < w * w; p += 256) {
    const int i = p / w, j = p - i * w;
    const float v = a.emit[(int64_t)(i0 + i) * a.emit_rs + (j0 + j)];
    const bool ok = finite_f32(v) && (!a.mask || a.mask[(int64_t)(i0 + i) * a.mask_rs + (j0 + j)] != 0);
    E[p] = ok ? v : NAN;
  }
  const T* s2 = static_cast<const T*>(a.s2);
  const bool has_nodata = a.has_nodata != 0;
  for (int b = tid; b < nby * nbx; b += 256) {
    const int by = b / nbx, bx = b - by * nbx;
    const T* q = s2 + (int64_t)(f * (i0 + qy0 + by) + ry) * a.s2_rs + (f * (j0 + qx0 + bx) + rx);
    double sum = 0.0;
    bool ok = true;
    for (int r = 0; r < f; ++r) {
      double row = 0.0;
      for (int c = 0; c < f; ++c) {
        const T v = q[(int64_t)r * a.s2_rs + c];
        ok = ok && s2_valid<T>(v, has_nodata, a.nodata);
        row += (double)v;
      }
      sum += row;
    }
    B[b] = ok ? sum : (double)NAN;
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  const int step_i = 64 / w, step_j = 64 - step_i * w;
  for (int c = wave; c < ncy * ncx; c += 4) {
    const int oy = c / ncx, ox = c - oy * ncx;
    double n = 0.0, se = 0.0, sm = 0.0, see = 0.0, smm = 0.0, sem = 0.0;
    double emin = INFINITY, emax = -INFINITY, mmin = INFINITY, mmax = -INFINITY;
    int i = lane / w, j = lane - i * w;
    for (int p = lane; p < w * w; p += 64) {
      const double e = (double)E[p], m = B[(i + oy) * nbx + (j + ox)];
      if (!isnan(e) && !isnan(m)) {
        n += 1.0; se += e; sm += m; see += e * e; smm += m * m; sem += e * m;
        emin = fmin(emin, e); emax = fmax(emax, e); mmin = fmin(mmin, m); mmax = fmax(mmax, m);
      }
      i += step_i; j += step_j;
      if (j >= w) { j -= w; ++i; }
    }
    n = wave_sum(n); se = wave_sum(se); sm = wave_sum(sm); see = wave_sum(see); smm = wave_sum(smm); sem = wave_sum(sem);
    emin = wave_min(emin); emax = wave_max(emax); mmin = wave_min(mmin); mmax = wave_max(mmax);
    if (lane == 0) {
      double score = NAN;
      if (n >= (double)a.min_valid && emin < emax && mmin < mmax) {
        const double vee = see - se * se / n, vmm = smm - sm * sm / n, vem = sem - se * sm / n;
        if (vee > 0.0 && vmm > 0.0) score = vem / sqrt(vee * vmm);
      }
      surf[(size_t)(f * (qy0 + oy) + ry + R) * D + (f * (qx0 + ox) + rx + R)] = score;
    }
  }
}

// Largest block-sum image over the phases, in blocks per side.
static int surface_span(int w, int f, int R) {
  int best = 0;
  for (int r = 0; r < f; ++r) {
    const int q0 = ceil_div(-R - r, f), q1 = floor_div(R - r, f);
    if (q1 - q0 > best) best = q1 - q0;
  }
  return w + best;
}

// ------------------------------------------------------------------------------------------------------------------------------
// stage 2: the peak records
// ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double parabola_offset(double l, double c, double r) {
  const double den = (l - 2.0 * c) + r;
  double o = den < 0.0 ? 0.5 * (l - r) / den : 0.0;
  o = o < -0.5 ? -0.5 : (o > 0.5 ? 0.5 : o);
  return o;
}

__global__ __launch_bounds__(256) void coreg_peaks_kernel(const double* __restrict__ surface, const int32_t* __restrict__ origins,
                                                          int npoints, int w, int f, int R, int he, int we, int hs, int ws,
                                                          double min_score, double* __restrict__ table) {
  const int lane = threadIdx.x & 63;
  const int point = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (point >= npoints) return;
  const int D = 2 * R + 1, nent = D * D;
  const double* S = surface + (size_t)point * nent;
  const int i0 = origins[2 * point], j0 = origins[2 * point + 1];
  double best = -INFINITY;
  int bk = -1, count = 0;
  for (int k = lane; k < nent; k += 64) {
    const double v = S[k];
    if (isfinite(v)) {
      ++count;
      if (bk < 0 || v > best) { best = v; bk = k; }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(best, off, 64);
    const int ok = __shfl_xor(bk, off, 64);
    count += __shfl_xor(count, off, 64);
    if (ok >= 0 && (bk < 0 || ov > best || (ov == best && ok < bk))) { best = ov; bk = ok; }
  }
  const int py = bk >= 0 ? bk / D : 0, px = bk >= 0 ? bk - py * D : 0;
  double second = -INFINITY;
  int any = 0;
  if (bk >= 0) {
    for (int k = lane; k < nent; k += 64) {
      const int y = k / D, x = k - y * D;
      const double v = S[k];
      if (isfinite(v) && (y < py - 1 || y > py + 1 || x < px - 1 || x > px + 1)) {
        second = fmax(second, v);
        any = 1;
      }
    }
  }
  second = wave_max(second);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) any |= __shfl_xor(any, off, 64);
  if (lane != 0) return;
  double* rec = table + (size_t)point * kRec;
  int status = HSR_COREG_OK;
  double dy = 0.0, dx = 0.0, score = NAN, sharp = NAN;
  if (!region_inside(i0, j0, w, f, R, he, we, hs, ws)) {
    status = HSR_COREG_OUTSIDE;
  } else if (bk < 0) {
    status = HSR_COREG_NO_SCORE;
  } else {
    score = best;
    if (any) sharp = best - second;
    bool border = py == 0 || py == D - 1 || px == 0 || px == D - 1;
    double up = NAN, dn = NAN, lf = NAN, rt = NAN;
    if (!border) {
      up = S[bk - D]; dn = S[bk + D]; lf = S[bk - 1]; rt = S[bk + 1];
      border = !(isfinite(up) && isfinite(dn) && isfinite(lf) && isfinite(rt));
    }
    if (border) {
      status = HSR_COREG_BORDER;
    } else if (score < min_score) {
      status = HSR_COREG_LOW_SCORE;
    } else {
      dy = (double)(py - R) + parabola_offset(up, best, dn);
      dx = (double)(px - R) + parabola_offset(lf, best, rt);
    }
  }
  rec[0] = (double)f * ((double)i0 + 0.5 * (double)w) - 0.5;
  rec[1] = (double)f * ((double)j0 + 0.5 * (double)w) - 0.5;
  rec[2] = dy;
  rec[3] = dx;
  rec[4] = score;
  rec[5] = sharp;
  rec[6] = (double)count;
  rec[7] = (double)status;
}

// ------------------------------------------------------------------------------------------------------------------------------
// stage 3: the shift model (one definition for the kernel and the host twin)
// ------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline void model_shift(const double* m, double y, double x, double& dy, double& dx) {
  dy = (m[0] + m[1] * (x - m[6])) + m[2] * (y - m[7]);
  dx = (m[3] + m[4] * (x - m[6])) + m[5] * (y - m[7]);
}

// One fit on the OK records.
__host__ __device__ inline void fit_pass(const double* table, int n, int kind, int min_points, int hs, int ws, double* m) {
  const double xc = 0.5 * (double)(ws - 1), yc = 0.5 * (double)(hs - 1);
  const double hx = xc > 1.0 ? xc : 1.0, hy = yc > 1.0 ? yc : 1.0;
  double cnt = 0.0, sdy = 0.0, sdx = 0.0;
  for (int i = 0; i < n; ++i) {
    const double* r = table + (size_t)i * kRec;
    if (r[7] == (double)HSR_COREG_OK) { cnt += 1.0; sdy += r[2]; sdx += r[3]; }
  }
  for (int k = 0; k < kModel; ++k) m[k] = 0.0;
  if (cnt < (double)(min_points > 1 ? min_points : 1)) {
    m[9] = -1.0;
    return;
  }
  m[6] = xc; m[7] = yc; m[8] = cnt;
  m[0] = sdy / cnt;
  m[3] = sdx / cnt;
  if (kind != 1 || cnt < 3.0) return;
  double g[6] = {0, 0, 0, 0, 0, 0}, by[3] = {0, 0, 0}, bx[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const double* r = table + (size_t)i * kRec;
    if (r[7] != (double)HSR_COREG_OK) continue;
    const double u = (r[1] - xc) / hx, v = (r[0] - yc) / hy;
    g[0] += 1.0; g[1] += u; g[2] += v; g[3] += u * u; g[4] += u * v; g[5] += v * v;
    by[0] += r[2]; by[1] += u * r[2]; by[2] += v * r[2];
    bx[0] += r[3]; bx[1] += u * r[3]; bx[2] += v * r[3];
  }
  double A[3][3] = {{g[0], g[1], g[2]}, {g[1], g[3], g[4]}, {g[2], g[4], g[5]}}, V[3][3];
  jacobi_eigen<3>(&A[0][0], &V[0][0], 3);   // hsr_solve.h: A ends diagonal, the columns of V are the eigenvectors
  double lmin = A[0][0], lmax = A[0][0];
  for (int i = 1; i < 3; ++i) {
    lmin = A[i][i] < lmin ? A[i][i] : lmin;
    lmax = A[i][i] > lmax ? A[i][i] : lmax;
  }
  if (!(lmin >= 1e-10 * lmax) || !(lmax > 0.0)) return;          // collinear tie points: the translation stands
  double cy[3] = {0, 0, 0}, cx[3] = {0, 0, 0};
  for (int i = 0; i < 3; ++i) {
    double py = 0.0, px = 0.0;
    for (int k = 0; k < 3; ++k) { py += V[k][i] * by[k]; px += V[k][i] * bx[k]; }
    py /= A[i][i];
    px /= A[i][i];
    for (int j = 0; j < 3; ++j) { cy[j] += V[j][i] * py; cx[j] += V[j][i] * px; }
  }
  m[0] = cy[0]; m[1] = cy[1] / hx; m[2] = cy[2] / hy;
  m[3] = cx[0]; m[4] = cx[1] / hx; m[5] = cx[2] / hy;
  m[9] = 1.0;
}

__host__ __device__ inline void fit_model(double* table, int n, int kind, int min_points, double reject_px, int hs, int ws, double* m) {
  fit_pass(table, n, kind, min_points, hs, ws, m);
  if (m[9] < 0.0) return;
  bool any = false;
  for (int i = 0; i < n; ++i) {
    double* r = table + (size_t)i * kRec;
    if (r[7] != (double)HSR_COREG_OK) continue;
    double dy, dx;
    model_shift(m, r[0], r[1], dy, dx);
    if (hypot(r[2] - dy, r[3] - dx) > reject_px) {
      r[7] = (double)HSR_COREG_OUTLIER;
      r[2] = 0.0;
      r[3] = 0.0;
      any = true;
    }
  }
  if (any) fit_pass(table, n, kind, min_points, hs, ws, m);
}

__global__ __launch_bounds__(64) void coreg_fit_model_kernel(double* __restrict__ table, int n, int kind, int min_points,
                                                             double reject_px, int hs, int ws, double* __restrict__ model) {
  if (threadIdx.x != 0) return;
  double m[kModel];
  fit_model(table, n, kind, min_points, reject_px, hs, ws, m);
  for (int k = 0; k < kModel; ++k) model[k] = m[k];
}

// ------------------------------------------------------------------------------------------------------------------------------
// stage 4: the warp
// ------------------------------------------------------------------------------------------------------------------------------
struct WarpArgs {
  const void* in;
  int bands, h, w;
  int64_t in_bs, in_rs;
  const double* model;
  int has_nodata;
  double nodata, fill, max_abs_shift, max_abs_slope;
  void* out;
  int64_t out_bs, out_rs;
  int32_t* status;
  int cap;                 // elements of the staged footprint (LDS instance)
};

template <typename T>
__device__ __forceinline__ T warp_store_value(double v);
template <>
__device__ __forceinline__ float warp_store_value<float>(double v) { return (float)v; }
template <>
__device__ __forceinline__ uint16_t warp_store_value<uint16_t>(double v) {
  const double r = rint(v);                                      // round half to even
  return (uint16_t)(r >= 65535.0 ? 65535.0 : (r > 0.0 ? r : 0.0));   // NaN -> 0
}

template <typename T, bool LDS>
__global__ __launch_bounds__(256) void coreg_warp_kernel(const WarpArgs a) {
  extern __shared__ double coreg_smem[];
  T* tile = reinterpret_cast<T*>(coreg_smem);
  double m[kModel];
#pragma unroll
  for (int k = 0; k < kModel; ++k) m[k] = a.model[k];
  const int h = a.h, w = a.w, tid = threadIdx.x;
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
    // the model against the caller's bound: the shifts at the scene's corners (an affine field peaks there) and the slopes
    bool ok = fabs(m[1]) <= a.max_abs_slope && fabs(m[2]) <= a.max_abs_slope && fabs(m[4]) <= a.max_abs_slope &&
              fabs(m[5]) <= a.max_abs_slope;
    for (int c = 0; c < 4; ++c) {
      double dy, dx;
      model_shift(m, (c & 2) ? (double)(h - 1) : 0.0, (c & 1) ? (double)(w - 1) : 0.0, dy, dx);
      ok = ok && fabs(dy) <= a.max_abs_shift && fabs(dx) <= a.max_abs_shift;
    }
    *a.status = ok ? 0 : 1;
  }
  const int x0 = (int)blockIdx.x * kWarpTW, y0 = (int)blockIdx.y * kWarpTH;
  const int tw = w - x0 < kWarpTW ? w - x0 : kWarpTW, th = h - y0 < kWarpTH ? h - y0 : kWarpTH;
  // the staged box: the tile's corners, one pixel of slack for rounding, taps -1 .. +2, clamped to the plane
  int fy0 = 0, fy1 = -1, fx0 = 0, fx1 = -1, fw = 0;
  bool staged = false;
  if (LDS) {
    double ylo = INFINITY, yhi = -INFINITY, xlo = INFINITY, xhi = -INFINITY;
    bool finite = true;
    for (int c = 0; c < 4; ++c) {
      const double y = (double)(y0 + ((c & 2) ? th - 1 : 0)), x = (double)(x0 + ((c & 1) ? tw - 1 : 0));
      double dy, dx;
      model_shift(m, y, x, dy, dx);
      const double sy = y + dy, sx = x + dx;
      finite = finite && isfinite(sy) && isfinite(sx);
      ylo = fmin(ylo, sy); yhi = fmax(yhi, sy); xlo = fmin(xlo, sx); xhi = fmax(xhi, sx);
    }
    if (finite) {
      fy0 = clamp_to_int(floor(ylo) - 2.0, 0, h - 1);
      fy1 = clamp_to_int(floor(yhi) + 3.0, 0, h - 1);
      fx0 = clamp_to_int(floor(xlo) - 2.0, 0, w - 1);
      fx1 = clamp_to_int(floor(xhi) + 3.0, 0, w - 1);
      fw = fx1 - fx0 + 1;
      staged = (int64_t)fw * (fy1 - fy0 + 1) <= (int64_t)a.cap;
    }
  }
  const bool has_nodata = a.has_nodata != 0;
  const T fill = warp_store_value<T>(a.fill);
  const int lx = tid & 63, ly = tid >> 6;
  for (int b = 0; b < a.bands; ++b) {
    const T* plane = static_cast<const T*>(a.in) + (int64_t)b * a.in_bs;
    T* oplane = static_cast<T*>(a.out) + (int64_t)b * a.out_bs;
    if (LDS && staged) {
      if (b) __syncthreads();                                   // the previous band's taps are read
      const int fh = fy1 - fy0 + 1;
      for (int r = ly; r < fh; r += 4)
        for (int c = lx; c < fw; c += 64) tile[r * fw + c] = plane[(int64_t)(fy0 + r) * a.in_rs + (fx0 + c)];
      __syncthreads();
    }
    if (lx >= tw) continue;
    for (int yy = ly; yy < th; yy += 4) {
      const int y = y0 + yy, x = x0 + lx;
      double dy, dx;
      model_shift(m, (double)y, (double)x, dy, dx);
      const double sy = (double)y + dy, sx = (double)x + dx;
      T res = fill;
      if (sy >= 0.0 && sy <= (double)(h - 1) && sx >= 0.0 && sx <= (double)(w - 1)) {
        const double fy = floor(sy), fx = floor(sx);
        const int iy = (int)fy, ix = (int)fx;
        double wy[4], wx[4];
        keys_weights(sy - fy, wy);
        keys_weights(sx - fx, wx);
        int ty[4], tx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int r = iy - 1 + k, c = ix - 1 + k;
          ty[k] = r < 0 ? 0 : (r > h - 1 ? h - 1 : r);
          tx[k] = c < 0 ? 0 : (c > w - 1 ? w - 1 : c);
        }
        const bool in_box = LDS && staged && ty[0] >= fy0 && ty[3] <= fy1 && tx[0] >= fx0 && tx[3] <= fx1;
        bool ok = true;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          double row = 0.0;
          if (wy[k] != 0.0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              double term = 0.0;
              if (wx[c] != 0.0) {
                const T v = in_box ? tile[(ty[k] - fy0) * fw + (tx[c] - fx0)] : plane[(int64_t)ty[k] * a.in_rs + tx[c]];
                ok = ok && s2_valid<T>(v, has_nodata, a.nodata);
                term = wx[c] * (double)v;
              }
              row = c == 0 ? term : row + term;
            }
            row = wy[k] * row;
          }
          acc = k == 0 ? row : acc + row;
        }
        if (ok) res = warp_store_value<T>(acc);
      }
      oplane[(int64_t)y * a.out_rs + x] = res;
    }
  }
}

static bool coreg_ranges_ok(int window, int factor, int max_shift) {
  return window >= HSR_COREG_MIN_WINDOW && window <= HSR_COREG_MAX_WINDOW && factor >= 1 && factor <= HSR_COREG_MAX_FACTOR &&
         max_shift >= 1 && max_shift <= HSR_COREG_MAX_SHIFT;
}

}  // namespace hsr

using namespace hsr;

extern "C" int hsr_coreg_surface(const float* emit_dev, int64_t emit_rs, int32_t he, int32_t we, const uint8_t* emit_mask_dev,
                                 int64_t mask_rs, const void* s2_dev, int32_t s2_dtype, int64_t s2_rs, int32_t hs, int32_t ws,
                                 int32_t has_nodata, double nodata, const int32_t* origins_dev, int32_t npoints, int32_t window,
                                 int32_t factor, int32_t max_shift, int32_t min_valid, double* surface_dev, hsr_stream_t stream) {
  HSR_REQUIRE(emit_dev && s2_dev && origins_dev && surface_dev, HSR_ERR_INVALID, "hsr_coreg_surface: NULL pointer");
  HSR_REQUIRE(s2_dtype == 0 || s2_dtype == 1, HSR_ERR_INVALID, "hsr_coreg_surface: s2_dtype=%d outside {0,1}", s2_dtype);
  HSR_REQUIRE(coreg_ranges_ok(window, factor, max_shift), HSR_ERR_INVALID,
              "hsr_coreg_surface: window=%d outside [4,64], factor=%d outside [1,8] or max_shift=%d outside [1,24]", window, factor, max_shift);
  HSR_REQUIRE(min_valid >= 1 && npoints >= 0, HSR_ERR_INVALID, "hsr_coreg_surface: min_valid=%d < 1 or npoints=%d < 0", min_valid, npoints);
  HSR_REQUIRE(he >= 1 && we >= 1 && hs >= 1 && ws >= 1 && emit_rs >= we && s2_rs >= ws && (!emit_mask_dev || mask_rs >= we),
              HSR_ERR_INVALID, "hsr_coreg_surface: a plane extent < 1 or a row stride below its width");
  if (npoints == 0) return HSR_OK;
  const SurfaceArgs a{emit_dev, emit_rs, he, we, emit_mask_dev, mask_rs, s2_dev, s2_rs, hs, ws, has_nodata, nodata,
                      origins_dev, window, factor, max_shift, min_valid, surface_dev};
  const int span = surface_span(window, factor, max_shift);
  const size_t lds = ((size_t)span * span * sizeof(double) + (size_t)window * window * sizeof(float) + 15) & ~(size_t)15;
  const dim3 grid((unsigned)((int64_t)npoints * factor * factor));
  static size_t configured[2] = {64 * 1024, 64 * 1024};
  if (s2_dtype == 0) {
    raise_lds_limit(reinterpret_cast<const void*>(&coreg_surface_kernel<float>), lds, configured[0]);
    hipLaunchKernelGGL(coreg_surface_kernel<float>, grid, dim3(256), lds, (hipStream_t)stream, a);
  } else {
    raise_lds_limit(reinterpret_cast<const void*>(&coreg_surface_kernel<uint16_t>), lds, configured[1]);
    hipLaunchKernelGGL(coreg_surface_kernel<uint16_t>, grid, dim3(256), lds, (hipStream_t)stream, a);
  }
  return launched(kLaunchCoreg, "coreg_surface_kernel launch", kCoregSurface + s2_dtype);
}

extern "C" int hsr_coreg_peaks(const double* surface_dev, const int32_t* origins_dev, int32_t npoints, int32_t window,
                               int32_t factor, int32_t max_shift, int32_t he, int32_t we, int32_t hs, int32_t ws,
                               double min_score, double* table_dev, hsr_stream_t stream) {
  HSR_REQUIRE(surface_dev && origins_dev && table_dev, HSR_ERR_INVALID, "hsr_coreg_peaks: NULL pointer");
  HSR_REQUIRE(coreg_ranges_ok(window, factor, max_shift), HSR_ERR_INVALID,
              "hsr_coreg_peaks: window=%d outside [4,64], factor=%d outside [1,8] or max_shift=%d outside [1,24]", window, factor, max_shift);
  HSR_REQUIRE(npoints >= 0 && he >= 1 && we >= 1 && hs >= 1 && ws >= 1, HSR_ERR_INVALID,
              "hsr_coreg_peaks: npoints=%d < 0 or a plane extent < 1", npoints);
  if (npoints == 0) return HSR_OK;
  hipLaunchKernelGGL(coreg_peaks_kernel, dim3((unsigned)((npoints + 3) / 4)), dim3(256), 0, (hipStream_t)stream, surface_dev,
                     origins_dev, npoints, window, factor, max_shift, he, we, hs, ws, min_score, table_dev);
  return launched(kLaunchCoreg, "coreg_peaks_kernel launch", kCoregPeaks);
}

static int fit_args_ok(const char* who, const void* table, const void* model, int32_t npoints, int32_t kind, int32_t min_points,
                       double reject_px, int32_t hs, int32_t ws) {
  HSR_REQUIRE(table && model, HSR_ERR_INVALID, "%s: NULL pointer", who);
  HSR_REQUIRE(npoints >= 0 && (kind == 0 || kind == 1) && min_points >= 0, HSR_ERR_INVALID,
              "%s: npoints=%d < 0, kind=%d outside {0,1} or min_points=%d < 0", who, npoints, kind, min_points);
  HSR_REQUIRE(reject_px > 0.0 && hs >= 1 && ws >= 1, HSR_ERR_INVALID, "%s: reject_px not > 0 or a plane extent < 1", who);
  return HSR_OK;
}

extern "C" int hsr_coreg_fit_model(double* table_dev, int32_t npoints, int32_t kind, int32_t min_points, double reject_px,
                                   int32_t hs, int32_t ws, double* model_dev, hsr_stream_t stream) {
  const int rc = fit_args_ok("hsr_coreg_fit_model", table_dev, model_dev, npoints, kind, min_points, reject_px, hs, ws);
  if (rc != HSR_OK) return rc;
  hipLaunchKernelGGL(coreg_fit_model_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, table_dev, npoints, kind, min_points,
                     reject_px, hs, ws, model_dev);
  return launched(kLaunchCoreg, "coreg_fit_model_kernel launch", kCoregFitModel);
}

extern "C" int hsr_coreg_fit_model_host(double* table, int32_t npoints, int32_t kind, int32_t min_points, double reject_px,
                                        int32_t hs, int32_t ws, double* model) {
  const int rc = fit_args_ok("hsr_coreg_fit_model_host", table, model, npoints, kind, min_points, reject_px, hs, ws);
  if (rc != HSR_OK) return rc;
  fit_model(table, npoints, kind, min_points, reject_px, hs, ws, model);
  return HSR_OK;
}

extern "C" int hsr_coreg_warp(const void* s2_dev, int32_t s2_dtype, int32_t bands, int32_t h, int32_t w, int64_t in_bs,
                              int64_t in_rs, const double* model_dev, int32_t has_nodata, double nodata, double fill,
                              double max_abs_shift, double max_abs_slope, void* out_dev, int64_t out_bs, int64_t out_rs,
                              int32_t* status_dev, hsr_stream_t stream) {
  HSR_REQUIRE(s2_dev && model_dev && out_dev && status_dev, HSR_ERR_INVALID, "hsr_coreg_warp: NULL pointer");
  HSR_REQUIRE(s2_dtype == 0 || s2_dtype == 1, HSR_ERR_INVALID, "hsr_coreg_warp: s2_dtype=%d outside {0,1}", s2_dtype);
  HSR_REQUIRE(bands >= 1 && h >= 1 && w >= 1, HSR_ERR_INVALID, "hsr_coreg_warp: an extent < 1");
  const int64_t plane_in = (int64_t)(h - 1) * in_rs + w, plane_out = (int64_t)(h - 1) * out_rs + w;
  HSR_REQUIRE(in_rs >= w && out_rs >= w && in_bs >= plane_in && out_bs >= plane_out, HSR_ERR_INVALID,
              "hsr_coreg_warp: strides under which rows or bands overlap");
  HSR_REQUIRE(max_abs_shift >= 0.0 && max_abs_slope >= 0.0, HSR_ERR_INVALID, "hsr_coreg_warp: negative or NaN bound");
  const size_t esz = s2_dtype == 0 ? sizeof(float) : sizeof(uint16_t);
  const uintptr_t ib = (uintptr_t)s2_dev, ob = (uintptr_t)out_dev;
  const uintptr_t ie = ib + (uintptr_t)((int64_t)(bands - 1) * in_bs + plane_in) * esz;
  const uintptr_t oe = ob + (uintptr_t)((int64_t)(bands - 1) * out_bs + plane_out) * esz;
  HSR_REQUIRE(oe <= ib || ie <= ob, HSR_ERR_INVALID, "hsr_coreg_warp: out aliases the input scene");
  // the staged footprint of a tile: its own extent grown by the slope spread, a 3-pixel halo and 2 pixels of slack
  const double spread = max_abs_slope * (double)(kWarpTW + kWarpTH);
  int direct = 1, cap = 0;
  if (spread <= 4096.0) {
    const int64_t grow = (int64_t)ceil(spread) + 5;
    const int64_t elems = (kWarpTW + grow) * (kWarpTH + grow);
    if ((size_t)elems * esz <= kWarpLdsLimit) {
      direct = 0;
      cap = (int)elems;
    }
  }
  const WarpArgs a{s2_dev, bands, h, w, in_bs, in_rs, model_dev, has_nodata, nodata, fill, max_abs_shift, max_abs_slope,
                   out_dev, out_bs, out_rs, status_dev, cap};
  const dim3 grid((unsigned)((w + kWarpTW - 1) / kWarpTW), (unsigned)((h + kWarpTH - 1) / kWarpTH));
  const size_t lds = direct ? 0 : (((size_t)cap * esz + 15) & ~(size_t)15);
  hipStream_t s = (hipStream_t)stream;
  if (s2_dtype == 0) {
    if (direct) hipLaunchKernelGGL((coreg_warp_kernel<float, false>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((coreg_warp_kernel<float, true>), grid, dim3(256), lds, s, a);
  } else {
    if (direct) hipLaunchKernelGGL((coreg_warp_kernel<uint16_t, false>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((coreg_warp_kernel<uint16_t, true>), grid, dim3(256), lds, s, a);
  }
  return launched(kLaunchCoreg, "coreg_warp_kernel launch", kCoregWarp + 2 * s2_dtype + direct);
}
