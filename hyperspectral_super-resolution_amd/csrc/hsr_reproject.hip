// An EMIT scene on its geographic grid onto the Sentinel-2 UTM grid on gfx950 (C ABI and the definitions: include/hsr_reproject.h):
// the source index of every output cell by the inverse transverse Mercator projection, with its host twin, and the cubic remap
// under any such field.
//
// Reference: emit_proj.py:876-940 hands the stage to `gdalwarp -r cubic`; the algorithm here is the header's.  Structure:
//   coords   one thread per output cell; the series' coefficients come from the host, the same code is the host twin.
//   warp     a 64 x 8 output tile per workgroup of 512 threads, one pixel per thread.  The geometry is the same for every band, so a pixel's
//            coordinate, its eight weights, its clamped taps and its "outside" decision are computed ONCE, kept in registers
//            and reused by the band loop, which is left with 16 LDS reads and 16 multiply-adds per sample.  The tile's source
//            footprint is the min / max over the taps of its own inside pixels (the field is arbitrary: corners say nothing);
//            that box of up to 8 bands at a time is staged in LDS and the taps come from there.  A tile whose box exceeds the staged capacity
//            - a discontinuous field, strong minification - reads its clamped, in-plane taps from global memory; a pixel whose
//            coordinate is outside or non-finite reads nothing at all.  DIRECT is the same kernel without the staging.
#include <limits.h>
#include <math.h>

#include "hsr_common.h"
#include "hsr_cubic_dev.h"
#include "../../include/hsr_reproject.h"

namespace hsr {

constexpr int kRpTW = HSR_REPROJECT_TILE_W, kRpTH = HSR_REPROJECT_TILE_H;
constexpr int kRpThreads = 512, kRpWaves = kRpThreads / 64;
constexpr int kRpPix = kRpTH / kRpWaves;             // pixels of a thread: 1
constexpr size_t kRpLdsLimit = 32 * 1024;            // a staged box above this goes to the direct-gather instance
constexpr size_t kRpLdsGroup = 64 * 1024;            // LDS of a workgroup: as many boxes (bands) as fit, at most kRpMaxGroup
constexpr int kRpMaxGroup = 8;

// ------------------------------------------------------------------------------------------------------------------------------
// stage 1: the coordinate field (one definition for the kernel and the host twin)
// ------------------------------------------------------------------------------------------------------------------------------
struct TmArgs {
  double e0, n0, dx, dy;
  int h, w;
  double lon0, fe, fn, k0A, e, e2m;   // k0 * A; the eccentricity; 1 - e^2
  double beta[6];
  double g0, g1, g3, g5;
};

static TmArgs tm_args(double e0, double n0, double dx, double dy, int h, int w, double lon0, double k0, double fe, double fn,
                      double a, double inv_f, double g0, double g1, double g3, double g5) {
  TmArgs t;
  t.e0 = e0; t.n0 = n0; t.dx = dx; t.dy = dy; t.h = h; t.w = w; t.lon0 = lon0; t.fe = fe; t.fn = fn;
  t.g0 = g0; t.g1 = g1; t.g3 = g3; t.g5 = g5;
  const double f = 1.0 / inv_f, n = f / (2.0 - f);
  const double n2 = n * n, n3 = n2 * n, n4 = n2 * n2, n5 = n4 * n, n6 = n3 * n3;
  t.k0A = k0 * (a / (1.0 + n) * (1.0 + n2 / 4.0 + n4 / 64.0 + n6 / 256.0));
  const double e2 = f * (2.0 - f);
  t.e = sqrt(e2);
  t.e2m = 1.0 - e2;
  t.beta[0] = n / 2.0 - 2.0 / 3.0 * n2 + 37.0 / 96.0 * n3 - 1.0 / 360.0 * n4 - 81.0 / 512.0 * n5 + 96199.0 / 604800.0 * n6;
  t.beta[1] = 1.0 / 48.0 * n2 + 1.0 / 15.0 * n3 - 437.0 / 1440.0 * n4 + 46.0 / 105.0 * n5 - 1118711.0 / 3870720.0 * n6;
  t.beta[2] = 17.0 / 480.0 * n3 - 37.0 / 840.0 * n4 - 209.0 / 4480.0 * n5 + 5569.0 / 90720.0 * n6;
  t.beta[3] = 4397.0 / 161280.0 * n4 - 11.0 / 504.0 * n5 - 830251.0 / 7257600.0 * n6;
  t.beta[4] = 4583.0 / 161280.0 * n5 - 108847.0 / 3991680.0 * n6;
  t.beta[5] = 20648693.0 / 638668800.0 * n6;
  return t;
}

// Steps 1 - 5 of hsr_reproject_coords for the cell (r, c).
__host__ __device__ inline void tm_source_index(const TmArgs& t, int r, int c, double& sy, double& sx) {
  const double kDeg = 57.295779513082320876798154814105;
  const double E = t.e0 + ((double)c + 0.5) * t.dx, N = t.n0 - ((double)r + 0.5) * t.dy;
  const double xi = (N - t.fn) / t.k0A, eta = (E - t.fe) / t.k0A;
  double xip = xi, etap = eta;
  for (int j = 1; j <= 6; ++j) {
    const double ax = 2.0 * (double)j * xi, ae = 2.0 * (double)j * eta;
    xip -= t.beta[j - 1] * sin(ax) * cosh(ae);
    etap -= t.beta[j - 1] * cos(ax) * sinh(ae);
  }
  const double sh = sinh(etap), cx = cos(xip);
  const double taup = sin(xip) / sqrt(sh * sh + cx * cx);
  const double lam = atan2(sh, cx);
  double tau = taup;
  for (int it = 0; it < 3; ++it) {
    const double t1 = sqrt(1.0 + tau * tau);
    const double sigma = sinh(t.e * atanh(t.e * tau / t1));
    const double taupi = tau * sqrt(1.0 + sigma * sigma) - sigma * t1;
    tau += (taup - taupi) / sqrt(1.0 + taupi * taupi) * (1.0 + t.e2m * tau * tau) / (t.e2m * t1);
  }
  const double lat = atan(tau) * kDeg, lon = t.lon0 + lam * kDeg;
  sx = (lon - t.g0) / t.g1 - 0.5;
  sy = (lat - t.g3) / t.g5 - 0.5;
}

__global__ __launch_bounds__(256) void reproject_coords_kernel(const TmArgs t, double* __restrict__ coords) {
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= (int64_t)t.h * t.w) return;
  const int r = (int)(cell / t.w), c = (int)(cell - (int64_t)r * t.w);
  double sy, sx;
  tm_source_index(t, r, c, sy, sx);
  reinterpret_cast<double2*>(coords)[cell] = make_double2(sy, sx);
}

// ------------------------------------------------------------------------------------------------------------------------------
// stage 2: the remap
// ------------------------------------------------------------------------------------------------------------------------------
struct RemapArgs {
  const float* src;
  int bands, hs, ws;
  int64_t src_bs, src_rs;
  const double* coords;
  int h, w;
  int has_nodata;          // 0 also when no float32 equals the caller's nodata
  float nodata_f;
  float fill;
  float* out;
  int64_t out_bs, out_rs;
  unsigned long long* counts;
  int32_t* status;
  int cap, box_w, box_h;   // elements of the staged box (LDS instance); the caller's bound of a tile's footprint
  int group;               // bands staged together (LDS instance)
};

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
  return v;
}
__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <bool LDS, bool RENORM>
__global__ __launch_bounds__(kRpThreads, 4) void reproject_warp_kernel(const RemapArgs a) {
  extern __shared__ float reproject_tile[];
  __shared__ int box[kRpWaves][4];
  const int tid = threadIdx.x, lx = tid & 63, ly = tid >> 6;
  const int x0 = (int)blockIdx.x * kRpTW, y0 = (int)blockIdx.y * kRpTH;
  const int hs = a.hs, ws = a.ws;
  const int x = x0 + lx;

  // the geometry of this thread's pixels, once for every band
  double wy[kRpPix][4], wx[kRpPix][4];
  int ty[kRpPix][4], tx[kRpPix][4];
  bool live[kRpPix], inside[kRpPix];
  int nearbit[kRpPix];                                            // the bit of the nearest pixel's tap in a 4 x 4 mask
  unsigned consult[kRpPix];                                       // bit 4 k + c: neither wy[k] nor wx[c] is exactly 0
  int ylo = INT_MAX, yhi = INT_MIN, xlo = INT_MAX, xhi = INT_MIN;
  unsigned n_outside = 0;
#pragma unroll
  for (int j = 0; j < kRpPix; ++j) {
    const int y = y0 + ly + kRpWaves * j;
    live[j] = x < a.w && y < a.h;
    inside[j] = false;
    nearbit[j] = 0;
    consult[j] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { wy[j][k] = 0.0; wx[j][k] = 0.0; ty[j][k] = 0; tx[j][k] = 0; }
    if (!live[j]) continue;
    const double2 s = reinterpret_cast<const double2*>(a.coords)[(int64_t)y * a.w + x];
    const double sy = s.x, sx = s.y;
    // NaN fails every comparison and an infinity one of them: only a bounded double is floored and converted
    if (sy >= 0.0 && sy <= (double)(hs - 1) && sx >= 0.0 && sx <= (double)(ws - 1)) {
      inside[j] = true;
      const double fy = floor(sy), fx = floor(sx);
      const int iy = (int)fy, ix = (int)fx;
      const double t_y = sy - fy, t_x = sx - fx;
      keys_weights(t_y, wy[j]);
      keys_weights(t_x, wx[j]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int r = iy - 1 + k, c = ix - 1 + k;
        ty[j][k] = r < 0 ? 0 : (r > hs - 1 ? hs - 1 : r);
        tx[j][k] = c < 0 ? 0 : (c > ws - 1 ? ws - 1 : c);
      }
      nearbit[j] = 4 * (t_y >= 0.5 ? 2 : 1) + (t_x >= 0.5 ? 2 : 1);
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) consult[j] |= (wy[j][k] != 0.0 && wx[j][c] != 0.0 ? 1u : 0u) << (4 * k + c);
      ylo = min(ylo, ty[j][0]); yhi = max(yhi, ty[j][3]); xlo = min(xlo, tx[j][0]); xhi = max(xhi, tx[j][3]);
    } else {
      ++n_outside;
    }
  }
  // the tile's footprint: min / max over its own inside pixels
  ylo = wave_min_i(ylo); yhi = wave_max_i(yhi); xlo = wave_min_i(xlo); xhi = wave_max_i(xhi);
  if (lx == 0) { box[ly][0] = ylo; box[ly][1] = yhi; box[ly][2] = xlo; box[ly][3] = xhi; }
  __syncthreads();
  int fy0 = box[0][0], fy1 = box[0][1], fx0 = box[0][2], fx1 = box[0][3];
#pragma unroll
  for (int k = 1; k < kRpWaves; ++k) {
    fy0 = min(fy0, box[k][0]); fy1 = max(fy1, box[k][1]); fx0 = min(fx0, box[k][2]); fx1 = max(fx1, box[k][3]);
  }
  const bool any_inside = fy1 >= fy0;
  const int fw = any_inside ? fx1 - fx0 + 1 : 0, fh = any_inside ? fy1 - fy0 + 1 : 0;
  if (tid == 0 && (fw > a.box_w || fh > a.box_h)) atomicOr(a.status, 1);
  const bool staged = LDS && any_inside && (int64_t)fw * fh <= (int64_t)a.cap;
  if (a.counts) {
    n_outside = wave_sum_u(n_outside);
    if (lx == 0 && n_outside) atomicAdd(&a.counts[0], (unsigned long long)n_outside);
  }

  if (staged) {                                                   // taps as offsets into the staged box: row offset and column
#pragma unroll
    for (int j = 0; j < kRpPix; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) { ty[j][k] = (ty[j][k] - fy0) * fw; tx[j][k] -= fx0; }
  }
  const bool has_nodata = a.has_nodata != 0;
  unsigned n_fill = 0;
  // A staged tile takes its box of `group` bands at a time: one band's box is a few KB, and a workgroup that waits for memory
  // once a band spends its time waiting; the loads of a group are in flight together.
  const int group = staged ? a.group : 1, box_elems = fw * fh;
  for (int b0 = 0; b0 < a.bands; b0 += group) {
    const int nb = min(group, a.bands - b0);
    if (staged) {                                                 // uniform over the workgroup
      if (b0) __syncthreads();                                    // the previous group's taps are read
      for (int r = ly; r < fh; r += kRpWaves)
        for (int c = lx; c < fw; c += 64) {
          const float* p = a.src + (int64_t)b0 * a.src_bs + (int64_t)(fy0 + r) * a.src_rs + (fx0 + c);
#pragma unroll 4
          for (int g = 0; g < nb; ++g) reproject_tile[g * box_elems + r * fw + c] = p[(int64_t)g * a.src_bs];
        }
      __syncthreads();
    }
    for (int b = b0; b < b0 + nb; ++b) {
      const float* plane = a.src + (int64_t)b * a.src_bs;
      float* oplane = a.out + (int64_t)b * a.out_bs;
      const float* tile = reproject_tile + (b - b0) * box_elems;
#pragma unroll
      for (int j = 0; j < kRpPix; ++j) {
        if (!live[j]) continue;
        float res = a.fill;
        if (inside[j]) {
          // The geometry is per pixel, not per band: these two keep the 16 tap addresses and the 16 "consulted" lane masks from
          // being hoisted out of the band loop into registers of their own, which costs the CU a workgroup.
          unsigned cm = consult[j];
          asm volatile("" : "+v"(cm));
          // every tap is clamped into the plane (and the staged box covers it), so it can be loaded whether consulted or not
          float v[4][4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            int r = ty[j][k];
            asm volatile("" : "+v"(r));
#pragma unroll
            for (int c = 0; c < 4; ++c) v[k][c] = staged ? tile[r + tx[j][c]] : plane[(int64_t)r * a.src_rs + tx[j][c]];
          }
          // all 16 finite and none the nodata value, in integer arithmetic: the largest magnitude pattern is below infinity's
          unsigned top = 0;
          bool clean = true;
#pragma unroll
          for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              top = max(top, __float_as_uint(v[k][c]) & 0x7fffffffu);
              clean = clean && !(has_nodata && v[k][c] == a.nodata_f);
            }
          unsigned valid = cm;                                      // bit 4 k + c: the tap is consulted and valid
          double acc = 0.0;
          if (cm == 0xffffu && clean && top < 0x7f800000u) {
            // the common case - no weight exactly 0, every sample valid: the definition without its selections
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const double row = ((wx[j][0] * (double)v[k][0] + wx[j][1] * (double)v[k][1]) + wx[j][2] * (double)v[k][2]) +
                                 wx[j][3] * (double)v[k][3];
              acc = k == 0 ? wy[j][k] * row : acc + wy[j][k] * row;
            }
          } else {
            valid = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              double row = 0.0;
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                const bool ok = finite_f32(v[k][c]) && !(has_nodata && v[k][c] == a.nodata_f);
                const bool use = ((cm >> (4 * k + c)) & 1u) && ok;
                if (use) valid |= 1u << (4 * k + c);
                const double term = use ? wx[j][c] * (double)v[k][c] : 0.0;
                row = c == 0 ? term : row + term;
              }
              row = (cm >> (4 * k)) & 0xfu ? wy[j][k] * row : 0.0;
              acc = k == 0 ? row : acc + row;
            }
          }
          const bool bad = valid != cm;
          if (!bad) {
            res = (float)acc;
          } else if (RENORM && ((valid >> nearbit[j]) & 1u)) {
            double wsum = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              double roww = 0.0;
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                const double term = (valid >> (4 * k + c)) & 1u ? wx[j][c] : 0.0;
                roww = c == 0 ? term : roww + term;
              }
              roww = (cm >> (4 * k)) & 0xfu ? wy[j][k] * roww : 0.0;
              wsum = k == 0 ? roww : wsum + roww;
            }
            res = (float)(acc / wsum);
          } else {
            ++n_fill;
          }
        }
        st_stream(&oplane[(int64_t)(y0 + ly + kRpWaves * j) * a.out_rs + x], res);
      }
    }
  }
  if (a.counts) {
    n_fill = wave_sum_u(n_fill);
    if (lx == 0 && n_fill) atomicAdd(&a.counts[1], (unsigned long long)n_fill);
  }
}

static int coords_args_ok(const char* who, double e0, double n0, double dx, double dy, int32_t h, int32_t w, double lon0, double k0,
                          double fe, double fn, double a, double inv_f, double g0, double g1, double g3, double g5,
                          const void* coords) {
  HSR_REQUIRE(coords, HSR_ERR_INVALID, "%s: NULL pointer", who);
  HSR_REQUIRE(h >= 1 && w >= 1, HSR_ERR_INVALID, "%s: an extent < 1 (h=%d, w=%d)", who, h, w);
  HSR_REQUIRE(isfinite(e0) && isfinite(n0) && isfinite(dx) && isfinite(dy) && isfinite(lon0) && isfinite(k0) && isfinite(fe) &&
                  isfinite(fn) && isfinite(a) && isfinite(inv_f) && isfinite(g0) && isfinite(g1) && isfinite(g3) && isfinite(g5),
              HSR_ERR_INVALID, "%s: a non-finite geometry parameter", who);
  HSR_REQUIRE(dx > 0.0 && dy > 0.0 && g1 > 0.0 && g5 < 0.0, HSR_ERR_INVALID,
              "%s: cell sizes dx=%g, dy=%g, g1=%g, -g5=%g must be > 0 (north-up grids)", who, dx, dy, g1, -g5);
  HSR_REQUIRE(a > 0.0 && k0 > 0.0 && inv_f > 1.0, HSR_ERR_INVALID, "%s: ellipsoid a=%g or k0=%g <= 0, or inv_f=%g <= 1", who, a, k0,
              inv_f);
  return HSR_OK;
}

}  // namespace hsr

using namespace hsr;

extern "C" int hsr_reproject_coords(double e0, double n0, double dx, double dy, int32_t h, int32_t w, double lon0_deg, double k0,
                                    double false_easting, double false_northing, double a, double inv_f, double g0, double g1,
                                    double g3, double g5, double* coords_dev, hsr_stream_t stream) {
  const int rc = coords_args_ok("hsr_reproject_coords", e0, n0, dx, dy, h, w, lon0_deg, k0, false_easting, false_northing, a, inv_f,
                                g0, g1, g3, g5, coords_dev);
  if (rc != HSR_OK) return rc;
  const TmArgs t = tm_args(e0, n0, dx, dy, h, w, lon0_deg, k0, false_easting, false_northing, a, inv_f, g0, g1, g3, g5);
  const int64_t cells = (int64_t)h * w;
  hipLaunchKernelGGL(reproject_coords_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t, coords_dev);
  return launched(kLaunchReproject, "reproject_coords_kernel launch", kReprojectCoords);
}

extern "C" int hsr_reproject_coords_host(double e0, double n0, double dx, double dy, int32_t h, int32_t w, double lon0_deg, double k0,
                                         double false_easting, double false_northing, double a, double inv_f, double g0, double g1,
                                         double g3, double g5, double* coords) {
  const int rc = coords_args_ok("hsr_reproject_coords_host", e0, n0, dx, dy, h, w, lon0_deg, k0, false_easting, false_northing, a,
                                inv_f, g0, g1, g3, g5, coords);
  if (rc != HSR_OK) return rc;
  const TmArgs t = tm_args(e0, n0, dx, dy, h, w, lon0_deg, k0, false_easting, false_northing, a, inv_f, g0, g1, g3, g5);
  for (int r = 0; r < h; ++r)
    for (int c = 0; c < w; ++c) {
      double* o = coords + 2 * ((size_t)r * w + c);
      tm_source_index(t, r, c, o[0], o[1]);
    }
  return HSR_OK;
}

extern "C" int hsr_reproject_warp(const float* src_dev, int32_t bands, int32_t hs, int32_t ws, int64_t src_bs, int64_t src_rs,
                                  const double* coords_dev, int32_t h, int32_t w, int32_t has_nodata, double nodata, double fill,
                                  int32_t rule, double max_footprint, float* out_dev, int64_t out_bs, int64_t out_rs,
                                  int64_t* counts_dev, int32_t* status_dev, hsr_stream_t stream) {
  HSR_REQUIRE(src_dev && coords_dev && out_dev && status_dev, HSR_ERR_INVALID, "hsr_reproject_warp: NULL pointer");
  HSR_REQUIRE(rule == HSR_REPROJECT_STRICT || rule == HSR_REPROJECT_RENORM, HSR_ERR_INVALID, "hsr_reproject_warp: rule=%d outside {0,1}",
              rule);
  HSR_REQUIRE(bands >= 1 && hs >= 1 && ws >= 1 && h >= 1 && w >= 1, HSR_ERR_INVALID, "hsr_reproject_warp: an extent < 1");
  const int64_t plane_in = (int64_t)(hs - 1) * src_rs + ws, plane_out = (int64_t)(h - 1) * out_rs + w;
  HSR_REQUIRE(src_rs >= ws && out_rs >= w && src_bs >= plane_in && out_bs >= plane_out, HSR_ERR_INVALID,
              "hsr_reproject_warp: strides under which rows or bands overlap");
  HSR_REQUIRE(max_footprint >= 0.0, HSR_ERR_INVALID, "hsr_reproject_warp: negative or NaN max_footprint bound");
  const uintptr_t ib = (uintptr_t)src_dev, ob = (uintptr_t)out_dev, cb = (uintptr_t)coords_dev;
  const uintptr_t ie = ib + (uintptr_t)((int64_t)(bands - 1) * src_bs + plane_in) * sizeof(float);
  const uintptr_t oe = ob + (uintptr_t)((int64_t)(bands - 1) * out_bs + plane_out) * sizeof(float);
  const uintptr_t ce = cb + (uintptr_t)((int64_t)h * w) * 2 * sizeof(double);
  HSR_REQUIRE(oe <= ib || ie <= ob, HSR_ERR_INVALID, "hsr_reproject_warp: out aliases the source scene");
  HSR_REQUIRE(oe <= cb || ce <= ob, HSR_ERR_INVALID, "hsr_reproject_warp: out aliases the coordinate field");
  // the staged box of a tile: its footprint under the bound, taps -1 .. +2 and one pixel of slack either way
  int direct = 1, cap = 0, box_w = INT_MAX, box_h = INT_MAX, group = 1;
  if (max_footprint <= 1024.0) {
    box_w = (int)ceil((double)kRpTW * max_footprint) + 5;
    box_h = (int)ceil((double)kRpTH * max_footprint) + 5;
    const int64_t elems = (int64_t)box_w * box_h;
    if ((size_t)elems * sizeof(float) <= kRpLdsLimit) {
      direct = 0;
      cap = (int)elems;
      group = (int)(kRpLdsGroup / ((size_t)elems * sizeof(float)));
      group = group > kRpMaxGroup ? kRpMaxGroup : group;
      group = group > bands ? bands : group;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  int rc = check_hip(hipMemsetAsync(status_dev, 0, sizeof(int32_t), s), "hsr_reproject_warp: clearing the status word");
  if (rc == HSR_OK && counts_dev) rc = check_hip(hipMemsetAsync(counts_dev, 0, 2 * sizeof(int64_t), s), "hsr_reproject_warp: clearing the counts");
  if (rc != HSR_OK) return rc;
  // a float32 sample equals the double nodata exactly when nodata is a float32 and the sample is that one (NaN equals nothing)
  const float nodata_f = (float)nodata;
  const int nodata_on = has_nodata != 0 && (double)nodata_f == nodata ? 1 : 0;
  const RemapArgs a{src_dev, bands, hs, ws, src_bs, src_rs, coords_dev, h, w, nodata_on, nodata_f, (float)fill, out_dev, out_bs, out_rs,
                    reinterpret_cast<unsigned long long*>(counts_dev), status_dev, cap, box_w, box_h, group};
  const dim3 grid((unsigned)((w + kRpTW - 1) / kRpTW), (unsigned)((h + kRpTH - 1) / kRpTH));
  const size_t lds = direct ? 0 : (((size_t)group * cap * sizeof(float) + 15) & ~(size_t)15);
  if (direct) {
    if (rule) hipLaunchKernelGGL((reproject_warp_kernel<false, true>), grid, dim3(kRpThreads), 0, s, a);
    else hipLaunchKernelGGL((reproject_warp_kernel<false, false>), grid, dim3(kRpThreads), 0, s, a);
  } else {
    if (rule) hipLaunchKernelGGL((reproject_warp_kernel<true, true>), grid, dim3(kRpThreads), lds, s, a);
    else hipLaunchKernelGGL((reproject_warp_kernel<true, false>), grid, dim3(kRpThreads), lds, s, a);
  }
  return launched(kLaunchReproject, "reproject_warp_kernel launch", kReprojectWarp + 2 * direct + rule);
}
