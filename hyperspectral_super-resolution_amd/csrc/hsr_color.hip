// The cross-channel affine colour transfer out = x @ A + t on gfx950 (C ABI: include/hsr_color.h): the 4 x 4 / 4 x 3 moments of
// an image pair or of float64 sample rows, the fixed-order slot reduction with the np.linalg.lstsq solve, and the streaming apply.
//
// Reference: fit_ot_affine_rgb / apply_affine_rgb (Pairs_EMIT_S2_demo-2.ipynb, the cell after reproject_stack_to_grid) and the
// second half of ot_match_rgb_sinkhorn_pot (s2_emit/color.py:106-115); stretch expression s2_emit/color.py:33.  The moments and the
// apply are bound by their bytes (12 - 16 B per pixel and image), so all they do is keep wide loads in flight: a thread owns four
// consecutive pixels per pass, which a padded row image delivers as four 16-byte loads and a packed one as three.  No LDS staging,
// no atomics, no communication between workgroups.
#include <math.h>
#include <string.h>

#include "hsr_common.h"
#include "hsr_solve.h"
#include "hsr_tree_dev.h"
#include "../../include/hsr_color.h"

namespace hsr {

constexpr int kAM = HSR_AFFINE_MOMENTS;
enum : int { kDword = 0, kRow4 = 1, kPack3 = 2 };   // load / store mode of an image, see hsr_color.h

struct ColorImage {
  const float* p;
  int64_t bs, ps;
};

// A thread's four pixels pix[0..3] (on[j]: pixel j exists; the others come back as 0).  whole4: the four are consecutive, all
// exist and pix[0] is a multiple of 4 - what the three 16-byte accesses of a packed image need.
template <int MODE>
__device__ __forceinline__ void load_px(const ColorImage im, const int64_t (&pix)[4], const bool (&on)[4], bool whole4, float (&v)[4][3]) {
  if (MODE == kPack3 && whole4) {
    const float4* r = reinterpret_cast<const float4*>(im.p + pix[0] * 3);
    const float4 a = ld_stream(r), b = ld_stream(r + 1), c = ld_stream(r + 2);
    v[0][0] = a.x; v[0][1] = a.y; v[0][2] = a.z;
    v[1][0] = a.w; v[1][1] = b.x; v[1][2] = b.y;
    v[2][0] = b.z; v[2][1] = b.w; v[2][2] = c.x;
    v[3][0] = c.y; v[3][1] = c.z; v[3][2] = c.w;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (on[j]) {
      if (MODE == kRow4) {
        const float4 a = ld_stream(reinterpret_cast<const float4*>(im.p) + pix[j]);
        v[j][0] = a.x; v[j][1] = a.y; v[j][2] = a.z;
      } else {
        const float* q = im.p + pix[j] * im.ps;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[j][c] = ld_stream(q + c * im.bs);
      }
    } else {
      v[j][0] = v[j][1] = v[j][2] = 0.0f;
    }
  }
}

// pad: the image has rows of >= 4 floats, whose fourth is written as 0
template <int MODE>
__device__ __forceinline__ void store_px(float* o, int64_t bs, int64_t ps, bool pad, const int64_t (&pix)[4], const bool (&on)[4],
                                         bool whole4, const float (&v)[4][3]) {
  if (MODE == kPack3 && whole4) {
    float4* r = reinterpret_cast<float4*>(o + pix[0] * 3);
    st_stream(r, make_float4(v[0][0], v[0][1], v[0][2], v[1][0]));
    st_stream(r + 1, make_float4(v[1][1], v[1][2], v[2][0], v[2][1]));
    st_stream(r + 2, make_float4(v[2][2], v[3][0], v[3][1], v[3][2]));
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (on[j]) {
      if (MODE == kRow4) {
        st_stream(reinterpret_cast<float4*>(o) + pix[j], make_float4(v[j][0], v[j][1], v[j][2], 0.0f));
      } else {
        float* q = o + pix[j] * ps;
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c * bs] = v[j][c];
        if (pad) q[3] = 0.0f;
      }
    }
  }
}

// One usable row into the 22 sums, the order of hsr_color.h.
__device__ __forceinline__ void affine_add(double (&acc)[kAM], double x0, double x1, double x2, double y0, double y1, double y2) {
  acc[0] += x0 * x0; acc[1] += x0 * x1; acc[2] += x0 * x2; acc[3] += x0;
  acc[4] += x1 * x1; acc[5] += x1 * x2; acc[6] += x1;
  acc[7] += x2 * x2; acc[8] += x2;
  acc[9] += 1.0;
  acc[10] += x0 * y0; acc[11] += x0 * y1; acc[12] += x0 * y2;
  acc[13] += x1 * y0; acc[14] += x1 * y1; acc[15] += x1 * y2;
  acc[16] += x2 * y0; acc[17] += x2 * y1; acc[18] += x2 * y2;
  acc[19] += y0; acc[20] += y1; acc[21] += y2;
}

// The workgroup's 256 thread sums to one slot (block_join4, hsr_tree_dev.h).
__device__ __forceinline__ void slot_store(double (&acc)[kAM], double (&red)[4][kAM], double* slot) {
  block_join4<kAM>(acc, red, kAM, [&](int m, double s) { slot[m] = s; });
}

// Rows of a slot: ceil(npix / slots) rounded up to whole groups of four pixels, so that a group never straddles two slots.
__host__ __device__ inline int64_t slot_rows(int64_t npix, int slots) {
  const int64_t per = (npix + slots - 1) / slots;
  return (per + 3) & ~(int64_t)3;
}

struct AffineMomArgs {
  ColorImage x, y;
  const uint8_t* mask;
  int64_t npix;
  const double* lohi_x;
  const double* lohi_y;
  double* partials;
};

// One contiguous pixel range per slot; thread t takes the groups t, t + 256, ... of four pixels, each in pixel order - whatever
// the load modes, so the sums do not depend on the layout.
template <int LX, int LY>
__global__ __launch_bounds__(256) void affine_moments_kernel(const AffineMomArgs a) {
  __shared__ double red[4][kAM];
  const bool sx = a.lohi_x != nullptr, sy = a.lohi_y != nullptr;
  double lx[3][2], ly[3][2];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    lx[c][0] = sx ? a.lohi_x[2 * c] : 0.0; lx[c][1] = sx ? a.lohi_x[2 * c + 1] : 0.0;
    ly[c][0] = sy ? a.lohi_y[2 * c] : 0.0; ly[c][1] = sy ? a.lohi_y[2 * c + 1] : 0.0;
  }
  double acc[kAM];
#pragma unroll
  for (int m = 0; m < kAM; ++m) acc[m] = 0.0;
  const int64_t per = slot_rows(a.npix, (int)gridDim.x);
  const int64_t beg = (int64_t)blockIdx.x * per;
  int64_t end = beg + per;
  if (end > a.npix) end = a.npix;
  for (int64_t p0 = beg + (int64_t)threadIdx.x * 4; p0 < end; p0 += 256 * 4) {
    int64_t pix[4];
    bool on[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pix[j] = p0 + j;
      on[j] = pix[j] < end;
    }
    float xv[4][3], yv[4][3];
    load_px<LX>(a.x, pix, on, on[3], xv);
    load_px<LY>(a.y, pix, on, on[3], yv);
    uint8_t mk[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) mk[j] = on[j] ? (a.mask ? a.mask[pix[j]] : (uint8_t)1) : (uint8_t)0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bool ok = mk[j] != 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) ok = ok && finite_f32(xv[j][c]) && finite_f32(yv[j][c]);
      if (ok) {
        float xs[3], ys[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          xs[c] = sx ? stretch_f64(xv[j][c], lx[c][0], lx[c][1]) : xv[j][c];
          ys[c] = sy ? stretch_f64(yv[j][c], ly[c][0], ly[c][1]) : yv[j][c];
        }
        affine_add(acc, (double)xs[0], (double)xs[1], (double)xs[2], (double)ys[0], (double)ys[1], (double)ys[2]);
      }
    }
  }
  slot_store(acc, red, a.partials + (size_t)blockIdx.x * kAM);
}

// float64 sample rows (n, 3): no mask, no stretch, rows with a non-finite value skipped.  Thread t takes rows t, t + 256, ...
__global__ __launch_bounds__(256) void affine_moments_f64_kernel(const double* __restrict__ x, int64_t xrs,
                                                                 const double* __restrict__ y, int64_t yrs, int64_t npix,
                                                                 double* __restrict__ partials) {
  __shared__ double red[4][kAM];
  double acc[kAM];
#pragma unroll
  for (int m = 0; m < kAM; ++m) acc[m] = 0.0;
  const int64_t per = slot_rows(npix, (int)gridDim.x);
  const int64_t beg = (int64_t)blockIdx.x * per;
  int64_t end = beg + per;
  if (end > npix) end = npix;
  for (int64_t p = beg + threadIdx.x; p < end; p += 256) {
    const double* xr = x + p * xrs;
    const double* yr = y + p * yrs;
    const double x0 = xr[0], x1 = xr[1], x2 = xr[2], y0 = yr[0], y1 = yr[1], y2 = yr[2];
    if (isfinite(x0) && isfinite(x1) && isfinite(x2) && isfinite(y0) && isfinite(y1) && isfinite(y2))
      affine_add(acc, x0, x1, x2, y0, y1, y2);
  }
  slot_store(acc, red, partials + (size_t)blockIdx.x * kAM);
}

// np.linalg.lstsq(X_aug, Y, rcond=None) for output channel c from the 22 moments: W[:, c] into At[0 * 3 + c] .. At[3 * 3 + c] (A
// row-major, then t).  The 4 x 4 Gram is NOT column-scaled (np.polyfit scales, lstsq does not): solve_band_jacobi with s = 1 keeps
// the eigenvalues above max((eps * max(count, 4))^2, kRankFloor) * largest and applies the pseudo-inverse.  ``work``: kSolveWork
// doubles.  count < min_count or no row at all: the identity (the notebook's fallback).
__host__ __device__ inline void affine_solve_channel(const double* mom, long long min_count, int c, double* At, double* work) {
  const double count = mom[9];
  if (!(count >= (double)min_count) || count < 1.0) {
    for (int i = 0; i < 4; ++i) At[i * 3 + c] = i == c ? 1.0 : 0.0;
    return;
  }
  double* A = work;
  double* V = work + kSolveLd * kSolveLd;
  double* rhs = V + kSolveLd * kSolveLd;
  double* s = rhs + kSolveLd;
  const int tri[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
  for (int i = 0; i < 4; ++i) {
    for (int k = 0; k < 4; ++k) A[i * kSolveLd + k] = mom[tri[i][k]];
    rhs[i] = mom[10 + i * 3 + c];
    s[i] = 1.0;
  }
  double coef[kSolveLd];
  solve_band_jacobi(A, V, rhs, s, 4, count > 4.0 ? count : 4.0, coef);
  for (int i = 0; i < 4; ++i) At[i * 3 + c] = coef[i];
}

// One workgroup of 1024: "lane" l = thread / 16 takes lane_slot_sum (slots l, l + 64, ... in order) for the moments m and m + 16
// (m = thread % 16), thread m < 22 walks butterfly_tree64 over the 64 lane sums, then threads 0..2 solve a channel each.
__global__ __launch_bounds__(1024) void affine_reduce_solve_kernel(const double* __restrict__ partials, int slots,
                                                                   long long min_count, double* __restrict__ moments,
                                                                   double* __restrict__ At) {
  __shared__ double lsum[64][32];
  __shared__ double mom[kAM];
  __shared__ double work[3][kSolveWork];
  const int l = threadIdx.x >> 4, m = threadIdx.x & 15;
  lsum[l][m] = lane_slot_sum(l, slots, true, [&](int i) { return partials[(size_t)i * kAM + m]; });
  lsum[l][m + 16] = lane_slot_sum(l, slots, m + 16 < kAM, [&](int i) { return partials[(size_t)i * kAM + m + 16]; });
  __syncthreads();
  if (threadIdx.x < kAM) {
    const double s = butterfly_tree64(&lsum[0][threadIdx.x], 32);
    mom[threadIdx.x] = s;
    moments[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x < 3) affine_solve_channel(mom, min_count, (int)threadIdx.x, At, work[threadIdx.x]);
}

struct AffineApplyArgs {
  ColorImage x;
  const uint8_t* mask;
  const double* At;
  const double* lohi;
  int64_t npix;
  int32_t clip_mode;
  float* out;
  int64_t out_bs, out_ps;
  int32_t pad;
};

__device__ __forceinline__ float clip01f(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// A workgroup takes tiles of 1024 pixels (grid-stride), a thread four pixels of a tile.  With a packed image on either side the
// four are consecutive (thread t: 4t .. 4t + 3), which its three 16-byte accesses need; otherwise they are t, t + 256, t + 512,
// t + 768, so that every load and store instruction of a wave covers consecutive addresses (padded rows: 1 KiB per instruction).
// The first version gave every thread four consecutive pixels in all instances: a wave's 16-byte stores then lay 64 bytes apart,
// and the padded-row apply ran at 1.4 TB/s against 5.1 TB/s of hsr_poly_apply on the same buffers.
template <int LIN, int LOUT>
__global__ __launch_bounds__(256) void affine_apply_kernel(const AffineApplyArgs a) {
  double A[3][3], t[3], lo[3], hi[3];
  const bool st = a.lohi != nullptr;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int c = 0; c < 3; ++c) A[i][c] = a.At[i * 3 + c];
    t[i] = a.At[9 + i];
    lo[i] = st ? a.lohi[2 * i] : 0.0;
    hi[i] = st ? a.lohi[2 * i + 1] : 0.0;
  }
  constexpr bool kGrouped = LIN == kPack3 || LOUT == kPack3;
  for (int64_t base = (int64_t)blockIdx.x * 1024; base < a.npix; base += (int64_t)gridDim.x * 1024) {
    int64_t pix[4];
    bool on[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pix[j] = kGrouped ? base + threadIdx.x * 4 + j : base + j * 256 + threadIdx.x;
      on[j] = pix[j] < a.npix;
    }
    const bool whole4 = kGrouped && on[3];
    float v[4][3];
    load_px<LIN>(a.x, pix, on, whole4, v);
    uint8_t mk[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) mk[j] = on[j] ? (a.mask ? a.mask[pix[j]] : (uint8_t)1) : (uint8_t)0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (st) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[j][c] = stretch_f64(v[j][c], lo[c], hi[c]);
      }
      if (mk[j]) {
        const double v0 = (double)v[j][0], v1 = (double)v[j][1], v2 = (double)v[j][2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {      // x @ A + t, every product and sum rounded on its own
          const double o = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(v0, A[0][c]), __dmul_rn(v1, A[1][c])), __dmul_rn(v2, A[2][c])), t[c]);
          const float f = (float)o;
          v[j][c] = a.clip_mode ? clip01f(f) : f;
        }
      } else if (a.clip_mode == 2) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[j][c] = clip01f(v[j][c]);
      }
    }
    store_px<LOUT>(a.out, a.out_bs, a.out_ps, a.pad != 0, pix, on, whole4, v);
  }
}

// The layouts hsr_color.h admits for three channels over npix pixels.
static bool color_strides_ok(int64_t bs, int64_t ps, int64_t npix) {
  return (ps == 1 && bs >= npix && bs >= 1) || (bs == 1 && ps >= 3);
}

// The load / store mode of an image: the kernels' vector predicate, evaluated here and recorded with the launch.
static int color_mode(const void* p, int64_t bs, int64_t ps) {
  if (bs != 1 || (((uintptr_t)p) & 15) != 0) return kDword;
  return ps == 4 ? kRow4 : ps == 3 ? kPack3 : kDword;
}

static int affine_slots(int64_t npix) {
  const int64_t s = (npix + HSR_AFFINE_SLOT_PIXELS - 1) / HSR_AFFINE_SLOT_PIXELS;
  return (int)(s < 1 ? 1 : (s > HSR_AFFINE_MAX_SLOTS ? HSR_AFFINE_MAX_SLOTS : s));
}

template <int LX>
static void launch_moments_y(int ly, dim3 grid, hipStream_t s, const AffineMomArgs& a) {
  switch (ly) {
    case kRow4: hipLaunchKernelGGL((affine_moments_kernel<LX, kRow4>), grid, dim3(256), 0, s, a); break;
    case kPack3: hipLaunchKernelGGL((affine_moments_kernel<LX, kPack3>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((affine_moments_kernel<LX, kDword>), grid, dim3(256), 0, s, a); break;
  }
}

template <int LIN>
static void launch_apply_out(int lout, dim3 grid, hipStream_t s, const AffineApplyArgs& a) {
  switch (lout) {
    case kRow4: hipLaunchKernelGGL((affine_apply_kernel<LIN, kRow4>), grid, dim3(256), 0, s, a); break;
    case kPack3: hipLaunchKernelGGL((affine_apply_kernel<LIN, kPack3>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((affine_apply_kernel<LIN, kDword>), grid, dim3(256), 0, s, a); break;
  }
}

}  // namespace hsr

using namespace hsr;

extern "C" int hsr_affine_partial_slots(int64_t npix) {
  HSR_REQUIRE(npix >= 0, -1, "hsr_affine_partial_slots: npix < 0");
  return affine_slots(npix);
}

extern "C" size_t hsr_affine_partials_bytes(void) { return (size_t)HSR_AFFINE_MAX_SLOTS * kAM * sizeof(double); }

extern "C" int hsr_affine_moments(const float* x_dev, int64_t x_bs, int64_t x_ps, const float* y_dev, int64_t y_bs,
                                  int64_t y_ps, const uint8_t* mask_dev, int64_t npix, const double* lohi_x_dev,
                                  const double* lohi_y_dev, double* partials_dev, int32_t* slots_out, hsr_stream_t stream) {
  HSR_REQUIRE(x_dev && y_dev && partials_dev, HSR_ERR_INVALID, "hsr_affine_moments: NULL pointer");
  HSR_REQUIRE(npix >= 0, HSR_ERR_INVALID, "hsr_affine_moments: npix < 0");
  HSR_REQUIRE(color_strides_ok(x_bs, x_ps, npix) && color_strides_ok(y_bs, y_ps, npix), HSR_ERR_INVALID,
              "hsr_affine_moments: strides are neither planar nor rows of >= 3 floats");
  const AffineMomArgs a{{x_dev, x_bs, x_ps}, {y_dev, y_bs, y_ps}, mask_dev, npix, lohi_x_dev, lohi_y_dev, partials_dev};
  const int slots = affine_slots(npix);
  const int lx = color_mode(x_dev, x_bs, x_ps), ly = color_mode(y_dev, y_bs, y_ps);
  const dim3 grid(slots);
  hipStream_t s = (hipStream_t)stream;
  switch (lx) {
    case kRow4: launch_moments_y<kRow4>(ly, grid, s, a); break;
    case kPack3: launch_moments_y<kPack3>(ly, grid, s, a); break;
    default: launch_moments_y<kDword>(ly, grid, s, a); break;
  }
  const int rc = launched(kLaunchColor, "affine_moments_kernel launch", kColorMoments + 3 * lx + ly);
  if (rc != HSR_OK) return rc;
  if (slots_out) *slots_out = slots;
  return HSR_OK;
}

extern "C" int hsr_affine_moments_f64(const double* x_dev, int64_t x_rs, const double* y_dev, int64_t y_rs, int64_t npix,
                                      double* partials_dev, int32_t* slots_out, hsr_stream_t stream) {
  HSR_REQUIRE(x_dev && y_dev && partials_dev, HSR_ERR_INVALID, "hsr_affine_moments_f64: NULL pointer");
  HSR_REQUIRE(npix >= 0, HSR_ERR_INVALID, "hsr_affine_moments_f64: npix < 0");
  HSR_REQUIRE(x_rs >= 3 && y_rs >= 3, HSR_ERR_INVALID, "hsr_affine_moments_f64: rows of fewer than 3 doubles overlap");
  const int slots = affine_slots(npix);
  hipLaunchKernelGGL(affine_moments_f64_kernel, dim3(slots), dim3(256), 0, (hipStream_t)stream, x_dev, x_rs, y_dev, y_rs, npix,
                     partials_dev);
  const int rc = launched(kLaunchColor, "affine_moments_f64_kernel launch", kColorMomentsF64);
  if (rc != HSR_OK) return rc;
  if (slots_out) *slots_out = slots;
  return HSR_OK;
}

extern "C" int hsr_affine_reduce_solve(const double* partials_dev, int32_t slots, int64_t min_count, double* moments_dev,
                                       double* At_dev, hsr_stream_t stream) {
  HSR_REQUIRE(partials_dev && moments_dev && At_dev, HSR_ERR_INVALID, "hsr_affine_reduce_solve: NULL pointer");
  HSR_REQUIRE(slots >= 1 && slots <= HSR_AFFINE_MAX_SLOTS, HSR_ERR_INVALID, "hsr_affine_reduce_solve: slots=%d outside [1,%d]",
              slots, HSR_AFFINE_MAX_SLOTS);
  hipLaunchKernelGGL(affine_reduce_solve_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, partials_dev, slots,
                     (long long)min_count, moments_dev, At_dev);
  return launched(kLaunchColor, "affine_reduce_solve_kernel launch", kColorReduceSolve);
}

extern "C" int hsr_affine_solve_host(const double* moments, int64_t min_count, double* At) {
  HSR_REQUIRE(moments && At, HSR_ERR_INVALID, "hsr_affine_solve_host: NULL pointer");
  double work[kSolveWork];
  for (int c = 0; c < 3; ++c) affine_solve_channel(moments, (long long)min_count, c, At, work);
  return HSR_OK;
}

extern "C" int hsr_affine_apply(const float* x_dev, int64_t x_bs, int64_t x_ps, const uint8_t* mask_dev, const double* At_dev,
                                int64_t npix, const double* lohi_dev, int32_t clip_mode, float* out_dev, int64_t out_bs,
                                int64_t out_ps, hsr_stream_t stream) {
  HSR_REQUIRE(x_dev && At_dev && out_dev, HSR_ERR_INVALID, "hsr_affine_apply: NULL pointer");
  HSR_REQUIRE(npix >= 0, HSR_ERR_INVALID, "hsr_affine_apply: npix < 0");
  HSR_REQUIRE(clip_mode >= 0 && clip_mode <= 2, HSR_ERR_INVALID, "hsr_affine_apply: clip_mode=%d outside {0,1,2}", clip_mode);
  HSR_REQUIRE(color_strides_ok(x_bs, x_ps, npix) && color_strides_ok(out_bs, out_ps, npix), HSR_ERR_INVALID,
              "hsr_affine_apply: strides are neither planar nor rows of >= 3 floats");
  if (npix == 0) return HSR_OK;
  const AffineApplyArgs a{{x_dev, x_bs, x_ps}, mask_dev, At_dev, lohi_dev, npix, clip_mode, out_dev, out_bs, out_ps,
                          out_bs == 1 && out_ps >= 4 ? 1 : 0};
  const int lin = color_mode(x_dev, x_bs, x_ps), lout = color_mode(out_dev, out_bs, out_ps);
  // tiles of 1024 pixels; up to 2048 workgroups (8 per CU), grid-stride beyond
  int64_t gb = (npix + 1023) / 1024;
  if (gb > 2048) gb = 2048;
  const dim3 grid((unsigned)gb);
  hipStream_t s = (hipStream_t)stream;
  switch (lin) {
    case kRow4: launch_apply_out<kRow4>(lout, grid, s, a); break;
    case kPack3: launch_apply_out<kPack3>(lout, grid, s, a); break;
    default: launch_apply_out<kDword>(lout, grid, s, a); break;
  }
  return launched(kLaunchColor, "affine_apply_kernel launch", kColorApply + 3 * lin + lout);
}
