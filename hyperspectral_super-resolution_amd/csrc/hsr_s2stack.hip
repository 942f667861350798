// The Sentinel-2 band planes of a granule to the cropped 10 m stack on gfx950 (C ABI and the definition: include/hsr_s2stack.h):
// the resampling of the 20 m bands, the stacking and the crop in one launch, its host twin, and a byte plane under the same window.
//
// Reference: s2_data/s2_utils.py:505-614 (download_s2_spectral_stack: band_order, nearest / bilinear) and :617-783
// (crop_s2_stack_to_te) make the stack with rasterio on the host; the taps, the nodata rules and the rounding are the header's.
// Structure:
//   stack    a workgroup of four waves per (band, tile of 16 x 512 output pixels).  Phase 1: the source rectangle of the tile - for a
//            bilinear band half the tile plus a one-pixel halo - goes to LDS once, a wave per source row: 16-byte loads between the
//            row's first and last 16-byte boundary, single elements outside.  A staged row keeps the alignment of its global row
//            (it starts `shift` elements into its LDS row), so a 16-byte load lands on a 16-byte LDS address.  Phase 2: a wave per
//            output row; a thread makes eight neighbouring outputs.  A bilinear thread reads two rows of six staged taps, and when
//            all twelve are valid - the common case - the sums separate: six vertical sums, then two multiplies per output.  Every
//            other case (an invalid tap, one-tap bands, the elements before the row's first 16-byte boundary) goes through pixel(),
//            which IS the definition.  Stores are 16 bytes wide from the row's first 16-byte boundary on.  The count of invalid
//            outputs is a register per thread, a wave sum and one integer atomic per wave that has any.
//            stage(), pixel(), fast8() and compute() are __host__ __device__ and templated on the 16-byte accessor: the host twin
//            runs them for every (wave, lane) of every tile on host planes.
//   expand   a thread per 16 output bytes of a row, aligned to the row's 16-byte boundaries.
#include <limits.h>
#include <math.h>
#include <string.h>

#include "hsr_common.h"
#include "../../include/hsr_s2stack.h"

namespace hsr {

constexpr int kS2Threads = 256, kS2Waves = kS2Threads / 64;
constexpr int kS2TH = HSR_S2_TILE_H, kS2TW = HSR_S2_TILE_W;
constexpr int kS2Px = 8;                             // outputs of a thread: one 16-byte store of uint16, two of float32
constexpr int kS2SW = kS2TW + 8;                     // elements of a staged row: 512 taps and a shift of at most 7
static_assert(kS2TW == 64 * kS2Px, "a wave covers a tile row from its first 16-byte boundary on");
static_assert(kS2TW / 2 + 2 + 7 <= kS2SW && kS2TH / 2 + 2 <= kS2TH, "the staged rectangle of a bilinear band fits");

struct S2Args {
  hsr_s2_band band[HSR_S2_MAX_BANDS];
  int nbands, row0, col0, h, w, tiles_x;
  int has_nodata, nodata_in, nodata_out;
  float fill;
  double quant;
  void* out;
  int64_t obs, ors;
  unsigned long long* invalid;
};

struct S2Tile {                                      // a workgroup's tile of one band
  const uint16_t* plane;
  int64_t rs;
  int H, W, up, bil, off;
  int y0, x0, th, tw;                                // the tile in the window
  int Y0, X0;                                        // ... and in the granule
  int ilo, ihi, jlo, jhi;                            // the staged source rectangle, in plane pixels
};

struct S2Acc {
  unsigned N;
  int Wt;
  bool ok;
};

// The 16-byte accessors: copy16 moves an aligned segment (global -> LDS), store16 writes eight uint16 or four float32 outputs.
struct DevMem {
  static __device__ __forceinline__ void copy16(void* d, const void* s) { *static_cast<uint4*>(d) = *static_cast<const uint4*>(s); }
  static __device__ __forceinline__ void store16(uint16_t* d, const uint16_t* v) {
    *reinterpret_cast<uint4*>(d) = make_uint4(v[0] | (uint32_t)v[1] << 16, v[2] | (uint32_t)v[3] << 16, v[4] | (uint32_t)v[5] << 16,
                                              v[6] | (uint32_t)v[7] << 16);
  }
  static __device__ __forceinline__ void store16(float* d, const float* v) { *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]); }
};
struct HostMem {
  static void copy16(void* d, const void* s) { memcpy(d, s, 16); }
  static void store16(uint16_t* d, const uint16_t* v) { memcpy(d, v, 16); }
  static void store16(float* d, const float* v) { memcpy(d, v, 16); }
};

__host__ __device__ inline int s2_min(int a, int b) { return a < b ? a : b; }
__host__ __device__ inline int s2_max(int a, int b) { return a > b ? a : b; }
__host__ __device__ inline int s2_i0(int v) { return (v + 1) / 2 - 1; }          // floor((v - 1) / 2) for v >= 0: -1 at 0

__host__ __device__ inline S2Tile s2_tile(const S2Args& a, int b, int tile) {
  const hsr_s2_band& bd = a.band[b];
  S2Tile g;
  g.plane = static_cast<const uint16_t*>(bd.plane_dev);
  g.rs = bd.rs; g.H = bd.H; g.W = bd.W; g.up = bd.up; g.off = bd.add_offset;
  g.bil = bd.up == 2 && bd.method == HSR_S2_BILINEAR;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  g.y0 = ty * kS2TH; g.x0 = tx * kS2TW;
  g.th = s2_min(kS2TH, a.h - g.y0); g.tw = s2_min(kS2TW, a.w - g.x0);
  g.Y0 = a.row0 + g.y0; g.X0 = a.col0 + g.x0;
  const int Y1 = g.Y0 + g.th - 1, X1 = g.X0 + g.tw - 1;
  if (g.bil) {
    g.ilo = s2_max(s2_i0(g.Y0), 0); g.ihi = s2_min(s2_i0(Y1) + 1, g.H - 1);
    g.jlo = s2_max(s2_i0(g.X0), 0); g.jhi = s2_min(s2_i0(X1) + 1, g.W - 1);
  } else {
    const int s = g.up == 2 ? 1 : 0;
    g.ilo = g.Y0 >> s; g.ihi = Y1 >> s; g.jlo = g.X0 >> s; g.jhi = X1 >> s;
  }
  return g;
}

// Elements between the start of a staged LDS row and its first tap: the global row's offset into its 16-byte segment.
__host__ __device__ inline int s2_shift(const S2Tile& g, int i) {
  const uintptr_t addr = (uintptr_t)(g.plane + (int64_t)i * g.rs + g.jlo);
  return (addr & 1) ? 0 : (int)((addr & 15) >> 1);
}

__host__ __device__ inline unsigned s2_tap(const S2Tile& g, const uint16_t* lds, int i, int j) {
  return lds[(i - g.ilo) * kS2SW + s2_shift(g, i) + (j - g.jlo)];
}

// Phase 1: the rows wave, wave + 4, ... of the source rectangle.
template <class Mem>
__host__ __device__ inline void s2_stage(const S2Tile& g, uint16_t* lds, int wave, int lane) {
  const int nrows = g.ihi - g.ilo + 1, n = g.jhi - g.jlo + 1;
  for (int r = wave; r < nrows; r += kS2Waves) {
    const uint16_t* p = g.plane + (int64_t)(g.ilo + r) * g.rs + g.jlo;
    const uintptr_t addr = (uintptr_t)p;
    const bool odd = (addr & 1) != 0;
    const int shift = odd ? 0 : (int)((addr & 15) >> 1);
    uint16_t* d = lds + r * kS2SW + shift;
    const int head = odd ? n : s2_min((8 - shift) & 7, n);
    const int nv = (n - head) >> 3, tail0 = head + (nv << 3);
    for (int v = lane; v < nv; v += 64) Mem::copy16(d + head + 8 * v, p + head + 8 * v);
    const int edge = head + (n - tail0);             // before the first and after the last boundary: at most 14 on an even address
    for (int e = lane; e < edge; e += 64) {
      const int c = e < head ? e : tail0 + (e - head);
      d[c] = p[c];
    }
  }
}

// The definition for one output pixel (Y, X) of the granule: the taps that are used, N and Wt.
template <int RULE>
__host__ __device__ inline S2Acc s2_pixel(const S2Args& a, const S2Tile& g, const uint16_t* lds, int Y, int X) {
  S2Acc r;
  if (!g.bil) {
    const int s = g.up == 2 ? 1 : 0;
    const unsigned dn = s2_tap(g, lds, Y >> s, X >> s);
    r.N = dn; r.Wt = 1; r.ok = !(a.has_nodata && (int)dn == a.nodata_in);
    return r;
  }
  const int i0 = s2_i0(Y), j0 = s2_i0(X);
  const int wy[2] = {(Y & 1) ? 3 : 1, (Y & 1) ? 1 : 3}, wx[2] = {(X & 1) ? 3 : 1, (X & 1) ? 1 : 3};
  const int ii[2] = {s2_max(i0, 0), s2_min(i0 + 1, g.H - 1)}, jj[2] = {s2_max(j0, 0), s2_min(j0 + 1, g.W - 1)};
  unsigned N = 0;
  int Wt = 0;
  bool all = true, nine = true;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const unsigned dn = s2_tap(g, lds, ii[u], jj[v]);
      const int wt = wy[u] * wx[v];
      const bool ok = !(a.has_nodata && (int)dn == a.nodata_in);
      all = all && ok;
      if (wt == 9) nine = ok;
      if (RULE == HSR_S2_STRICT || ok) { N += (unsigned)wt * dn; Wt += wt; }
    }
  r.N = N; r.Wt = Wt; r.ok = RULE == HSR_S2_STRICT ? all : nine;
  return r;
}

template <int DT> struct S2Out;
template <> struct S2Out<HSR_S2_U16> { typedef uint16_t T; };
template <> struct S2Out<HSR_S2_F32> { typedef float T; };

template <int DT>
__host__ __device__ inline typename S2Out<DT>::T s2_value(const S2Args& a, const S2Acc& r, int off) {
  if constexpr (DT == HSR_S2_U16) {
    if (!r.ok) return (uint16_t)a.nodata_out;
    const unsigned q = r.Wt == 16 ? (2u * r.N + 16u) >> 5 : r.Wt == 1 ? r.N : (2u * r.N + (unsigned)r.Wt) / (2u * (unsigned)r.Wt);
    const int v = (int)q + off, lo = a.nodata_out == 0 ? 1 : 0, hi = a.nodata_out == 0 ? 65535 : 65534;
    return (uint16_t)(v < lo ? lo : v > hi ? hi : v);
  } else {
    if (!r.ok) return a.fill;
    // N / 16 and N / 1 are exact in float64: the scaling IS the correctly rounded division
    const double m = r.Wt == 16 ? (double)r.N * 0.0625 : r.Wt == 1 ? (double)r.N : (double)r.N / (double)r.Wt;
    return (float)((m + (double)off) / a.quant);
  }
}

// Eight neighbouring outputs of a bilinear row from two rows of six staged taps, when all twelve are valid (else false, and
// nothing is written).  P is the parity of X: output e has its left tap at column (e + 1 - P) >> 1 of the six.
template <int DT, int P>
__host__ __device__ inline bool s2_fast8(const S2Args& a, const S2Tile& g, const uint16_t* lds, int Y, int X,
                                         typename S2Out<DT>::T (&out)[kS2Px]) {
  const int i0 = s2_i0(Y), ia = s2_max(i0, 0), ib = s2_min(i0 + 1, g.H - 1), jb = s2_i0(X);
  const unsigned w1y = (Y & 1) ? 1u : 3u, w0y = 4u - w1y;
  const uint16_t* ra = lds + (ia - g.ilo) * kS2SW + s2_shift(g, ia);
  const uint16_t* rb = lds + (ib - g.ilo) * kS2SW + s2_shift(g, ib);
  unsigned V[6];
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const int j = s2_min(s2_max(jb + c, g.jlo), g.jhi) - g.jlo;   // the sixth column of an odd X is no tap of this thread: kept inside the rectangle
    const unsigned A = ra[j], B = rb[j];
    ok = ok && !(a.has_nodata && ((int)A == a.nodata_in || (int)B == a.nodata_in));
    V[c] = w0y * A + w1y * B;
  }
  if (!ok) return false;
#pragma unroll
  for (int e = 0; e < kS2Px; ++e) {
    const int rel = (e + 1 - P) >> 1;
    const unsigned w1x = ((P + e) & 1) ? 1u : 3u;
    S2Acc r;
    r.N = (4u - w1x) * V[rel] + w1x * V[rel + 1]; r.Wt = 16; r.ok = true;
    out[e] = s2_value<DT>(a, r, g.off);
  }
  return true;
}

// Phase 2: the output rows wave, wave + 4, ... of the tile; -> the invalid outputs this thread made.
template <class Mem, int DT, int RULE>
__host__ __device__ inline unsigned s2_compute(const S2Args& a, const S2Tile& g, const uint16_t* lds, int b, int wave, int lane) {
  typedef typename S2Out<DT>::T T;
  constexpr int E = (int)sizeof(T), VEC = 16 / E;
  unsigned bad = 0;
  for (int y = wave; y < g.th; y += kS2Waves) {
    T* dst = static_cast<T*>(a.out) + (int64_t)b * a.obs + (int64_t)(g.y0 + y) * a.ors + g.x0;
    const uintptr_t addr = (uintptr_t)dst;
    const int head = (addr % E) ? g.tw : s2_min((int)(((16 - (addr & 15)) & 15) / E), g.tw);
    const int Y = g.Y0 + y;
    for (int x = lane; x < head; x += 64) {          // before the first 16-byte boundary: at most 7 on an element-aligned row
      const S2Acc r = s2_pixel<RULE>(a, g, lds, Y, g.X0 + x);
      bad += r.ok ? 0u : 1u;
      dst[x] = s2_value<DT>(a, r, g.off);
    }
    const int x = head + lane * kS2Px;
    if (x >= g.tw) continue;
    const int n = s2_min(kS2Px, g.tw - x), X = g.X0 + x;
    T v[kS2Px];
    bool done = false;
    if (g.bil && n == kS2Px) done = (X & 1) ? s2_fast8<DT, 1>(a, g, lds, Y, X, v) : s2_fast8<DT, 0>(a, g, lds, Y, X, v);
    if (!done) {
#pragma unroll
      for (int e = 0; e < kS2Px; ++e)
        if (e < n) {
          const S2Acc r = s2_pixel<RULE>(a, g, lds, Y, X + e);
          bad += r.ok ? 0u : 1u;
          v[e] = s2_value<DT>(a, r, g.off);
        }
    }
#pragma unroll
    for (int c = 0; c < kS2Px / VEC; ++c) {
      if ((c + 1) * VEC <= n) {
        Mem::store16(dst + x + c * VEC, &v[c * VEC]);
      } else {
#pragma unroll
        for (int e = c * VEC; e < (c + 1) * VEC; ++e)
          if (e < n) const_cast<volatile T*>(dst)[x + e] = v[e];     // volatile: kept apart from the 16-byte store, which the compiler
                                                                     // otherwise splits into 12 + 4 bytes to share these instructions
      }
    }
  }
  return bad;
}

template <int DT, int RULE>
__global__ __launch_bounds__(kS2Threads) void s2_stack_kernel(const S2Args a) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[kS2TH * kS2SW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = (int)blockIdx.y;
  const S2Tile g = s2_tile(a, b, (int)blockIdx.x);
  s2_stage<DevMem>(g, lds, wave, lane);
  __syncthreads();
  unsigned bad = s2_compute<DevMem, DT, RULE>(a, g, lds, b, wave, lane);
  if (a.invalid) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) bad += __shfl_xor(bad, off, 64);
    if (lane == 0 && bad) atomicAdd(&a.invalid[b], (unsigned long long)bad);
  }
}

// The same tile code, every (wave, lane) of every tile in turn.
template <int DT, int RULE>
static void s2_stack_host(const S2Args& a, int64_t tiles) {
  static thread_local __attribute__((aligned(16))) uint16_t lds[kS2TH * kS2SW];
  for (int b = 0; b < a.nbands; ++b)
    for (int64_t t = 0; t < tiles; ++t) {
      const S2Tile g = s2_tile(a, b, (int)t);
      for (int wave = 0; wave < kS2Waves; ++wave)
        for (int lane = 0; lane < 64; ++lane) s2_stage<HostMem>(g, lds, wave, lane);
      unsigned long long bad = 0;
      for (int wave = 0; wave < kS2Waves; ++wave)
        for (int lane = 0; lane < 64; ++lane) bad += s2_compute<HostMem, DT, RULE>(a, g, lds, b, wave, lane);
      if (a.invalid) a.invalid[b] += bad;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// a byte plane under the window
// ------------------------------------------------------------------------------------------------------------------------------
struct ExpandArgs {
  const uint8_t* plane;
  int64_t rs;
  int row0, col0, h, w;
  uint8_t* out;
  int64_t ors;
};

template <int UP>
__global__ __launch_bounds__(kS2Threads) void s2_expand_kernel(const ExpandArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kS2Threads + threadIdx.x;   // segment t of a row ends at its t-th 16-byte boundary past the head
  for (int y = (int)blockIdx.y; y < a.h; y += (int)gridDim.y) {
    uint8_t* dst = a.out + (int64_t)y * a.ors;
    const uint8_t* src = a.plane + (int64_t)((a.row0 + y) / UP) * a.rs;
    const int head = s2_min((int)((16 - ((uintptr_t)dst & 15)) & 15), a.w);
    const int64_t x0 = head - 16 + 16 * t;
    if (x0 >= a.w) continue;
    if (x0 >= 0 && x0 + 16 <= a.w) {
      uint32_t q[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) m |= (uint32_t)src[(a.col0 + x0 + 4 * k + j) / UP] << (8 * j);
        q[k] = m;
      }
      *reinterpret_cast<uint4*>(dst + x0) = make_uint4(q[0], q[1], q[2], q[3]);
    } else {
      const int64_t lo = x0 < 0 ? 0 : x0, hi = x0 + 16 < a.w ? x0 + 16 : a.w;
      for (int64_t x = lo; x < hi; ++x) dst[x] = src[(a.col0 + x) / UP];
    }
  }
}

static bool s2_overlap(const void* p, int64_t pn, const void* q, int64_t qn) {
  const uintptr_t pb = (uintptr_t)p, qb = (uintptr_t)q;
  return !(pb + (uintptr_t)pn <= qb || qb + (uintptr_t)qn <= pb);
}

static int s2_window_ok(const char* who, int32_t H10, int32_t W10, int32_t row0, int32_t col0, int32_t h, int32_t w) {
  HSR_REQUIRE(H10 >= 1 && W10 >= 1 && h >= 1 && w >= 1, HSR_ERR_INVALID, "%s: an extent < 1 (grid %d x %d, window %d x %d)", who, H10, W10,
              h, w);
  HSR_REQUIRE(row0 >= 0 && col0 >= 0 && (int64_t)row0 + h <= H10 && (int64_t)col0 + w <= W10, HSR_ERR_INVALID,
              "%s: the window (%d, %d, %d, %d) leaves the %d x %d grid", who, row0, col0, h, w, H10, W10);
  return HSR_OK;
}

static int s2_plane_ok(const char* who, int b, const void* plane, int32_t H, int32_t W, int64_t rs, int32_t up, int32_t H10, int32_t W10) {
  HSR_REQUIRE(plane, HSR_ERR_INVALID, "%s: NULL pointer (the plane of band %d)", who, b);
  HSR_REQUIRE(up == 1 || up == 2, HSR_ERR_UNSUPPORTED, "%s: band %d has up=%d outside {1,2}", who, b, up);
  HSR_REQUIRE(H == (H10 + up - 1) / up && W == (W10 + up - 1) / up, HSR_ERR_INVALID,
              "%s: band %d is a %d x %d plane, not the ceil of the %d x %d grid over up=%d", who, b, H, W, H10, W10, up);
  HSR_REQUIRE(rs >= W, HSR_ERR_INVALID, "%s: band %d has a row stride %lld below W=%d", who, b, (long long)rs, W);
  return HSR_OK;
}

static int s2_stack_args(const char* who, const hsr_s2_band* bands, int32_t nbands, int32_t H10, int32_t W10, int32_t row0, int32_t col0,
                         int32_t h, int32_t w, int32_t has_nodata, int32_t nodata_in, int32_t rule, int32_t out_dtype, void* out,
                         int64_t out_bs, int64_t out_rs, int32_t nodata_out, float fill, double quantification, int64_t* invalid,
                         S2Args* a, int64_t* tiles) {
  HSR_REQUIRE(bands && out, HSR_ERR_INVALID, "%s: NULL pointer", who);
  HSR_REQUIRE(nbands >= 1 && nbands <= HSR_S2_MAX_BANDS, HSR_ERR_INVALID, "%s: nbands=%d outside [1,%d]", who, nbands, HSR_S2_MAX_BANDS);
  int rc = s2_window_ok(who, H10, W10, row0, col0, h, w);
  if (rc != HSR_OK) return rc;
  HSR_REQUIRE(rule == HSR_S2_STRICT || rule == HSR_S2_RENORM, HSR_ERR_INVALID, "%s: rule=%d outside {0,1}", who, rule);
  HSR_REQUIRE(out_dtype == HSR_S2_U16 || out_dtype == HSR_S2_F32, HSR_ERR_INVALID, "%s: out_dtype=%d outside {0,1}", who, out_dtype);
  HSR_REQUIRE(nodata_out == 0 || nodata_out == 65535, HSR_ERR_INVALID, "%s: nodata_out=%d not in {0,65535}", who, nodata_out);
  HSR_REQUIRE(isfinite(quantification) && quantification > 0.0, HSR_ERR_INVALID, "%s: quantification=%g not finite or <= 0", who,
              quantification);
  HSR_REQUIRE(out_rs >= w && out_bs >= (int64_t)(h - 1) * out_rs + w, HSR_ERR_INVALID,
              "%s: output strides (band %lld, row %lld) under which rows or bands overlap", who, (long long)out_bs, (long long)out_rs);
  const int64_t esize = out_dtype == HSR_S2_U16 ? 2 : 4;
  const int64_t out_bytes = ((int64_t)(nbands - 1) * out_bs + (int64_t)(h - 1) * out_rs + w) * esize;
  for (int b = 0; b < nbands; ++b) {
    const hsr_s2_band& bd = bands[b];
    rc = s2_plane_ok(who, b, bd.plane_dev, bd.H, bd.W, bd.rs, bd.up, H10, W10);
    if (rc != HSR_OK) return rc;
    HSR_REQUIRE(bd.method == HSR_S2_NEAREST || bd.method == HSR_S2_BILINEAR, HSR_ERR_INVALID, "%s: band %d has method=%d outside {0,1}",
                who, b, bd.method);
    HSR_REQUIRE(!s2_overlap(out, out_bytes, bd.plane_dev, ((int64_t)(bd.H - 1) * bd.rs + bd.W) * 2), HSR_ERR_INVALID,
                "%s: the output overlaps the plane of band %d", who, b);
    a->band[b] = bd;
  }
  const int tiles_x = (w + kS2TW - 1) / kS2TW;
  *tiles = (int64_t)tiles_x * ((h + kS2TH - 1) / kS2TH);
  HSR_REQUIRE(*tiles <= INT_MAX, HSR_ERR_UNSUPPORTED, "%s: %lld tiles of %d x %d, more than 2^31 - 1", who, (long long)*tiles, kS2TH, kS2TW);
  a->nbands = nbands; a->row0 = row0; a->col0 = col0; a->h = h; a->w = w; a->tiles_x = tiles_x;
  a->has_nodata = has_nodata != 0; a->nodata_in = nodata_in; a->nodata_out = nodata_out; a->fill = fill; a->quant = quantification;
  a->out = out; a->obs = out_bs; a->ors = out_rs; a->invalid = reinterpret_cast<unsigned long long*>(invalid);
  return HSR_OK;
}

}  // namespace hsr

using namespace hsr;

extern "C" int hsr_s2_stack(const hsr_s2_band* bands, int32_t nbands, int32_t H10, int32_t W10, int32_t row0, int32_t col0, int32_t h,
                            int32_t w, int32_t has_nodata, int32_t nodata_in, int32_t rule, int32_t out_dtype, void* out_dev,
                            int64_t out_bs, int64_t out_rs, int32_t nodata_out, float fill, double quantification, int64_t* invalid_dev,
                            hsr_stream_t stream) {
  S2Args a{};
  int64_t tiles = 0;
  int rc = s2_stack_args("hsr_s2_stack", bands, nbands, H10, W10, row0, col0, h, w, has_nodata, nodata_in, rule, out_dtype, out_dev,
                         out_bs, out_rs, nodata_out, fill, quantification, invalid_dev, &a, &tiles);
  if (rc != HSR_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (invalid_dev) {
    rc = check_hip(hipMemsetAsync(invalid_dev, 0, (size_t)nbands * sizeof(int64_t), s), "hsr_s2_stack: clearing the counts");
    if (rc != HSR_OK) return rc;
  }
  const dim3 grid((unsigned)tiles, (unsigned)nbands), block(kS2Threads);
  if (out_dtype == HSR_S2_U16) {
    if (rule == HSR_S2_STRICT) hipLaunchKernelGGL((s2_stack_kernel<HSR_S2_U16, HSR_S2_STRICT>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((s2_stack_kernel<HSR_S2_U16, HSR_S2_RENORM>), grid, block, 0, s, a);
  } else {
    if (rule == HSR_S2_STRICT) hipLaunchKernelGGL((s2_stack_kernel<HSR_S2_F32, HSR_S2_STRICT>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((s2_stack_kernel<HSR_S2_F32, HSR_S2_RENORM>), grid, block, 0, s, a);
  }
  return launched(kLaunchS2Stack, "s2_stack_kernel launch", kS2Stack + 2 * out_dtype + rule);
}

extern "C" int hsr_s2_stack_host(const hsr_s2_band* bands, int32_t nbands, int32_t H10, int32_t W10, int32_t row0, int32_t col0, int32_t h,
                                 int32_t w, int32_t has_nodata, int32_t nodata_in, int32_t rule, int32_t out_dtype, void* out,
                                 int64_t out_bs, int64_t out_rs, int32_t nodata_out, float fill, double quantification, int64_t* invalid) {
  S2Args a{};
  int64_t tiles = 0;
  const int rc = s2_stack_args("hsr_s2_stack_host", bands, nbands, H10, W10, row0, col0, h, w, has_nodata, nodata_in, rule, out_dtype, out,
                               out_bs, out_rs, nodata_out, fill, quantification, invalid, &a, &tiles);
  if (rc != HSR_OK) return rc;
  if (invalid)
    for (int b = 0; b < nbands; ++b) invalid[b] = 0;
  if (out_dtype == HSR_S2_U16) {
    if (rule == HSR_S2_STRICT) s2_stack_host<HSR_S2_U16, HSR_S2_STRICT>(a, tiles);
    else s2_stack_host<HSR_S2_U16, HSR_S2_RENORM>(a, tiles);
  } else {
    if (rule == HSR_S2_STRICT) s2_stack_host<HSR_S2_F32, HSR_S2_STRICT>(a, tiles);
    else s2_stack_host<HSR_S2_F32, HSR_S2_RENORM>(a, tiles);
  }
  return HSR_OK;
}

extern "C" int hsr_s2_expand_u8(const uint8_t* plane_dev, int32_t H, int32_t W, int64_t rs, int32_t up, int32_t H10, int32_t W10,
                                int32_t row0, int32_t col0, int32_t h, int32_t w, uint8_t* out_dev, int64_t out_rs, hsr_stream_t stream) {
  HSR_REQUIRE(plane_dev && out_dev, HSR_ERR_INVALID, "hsr_s2_expand_u8: NULL pointer");
  int rc = s2_window_ok("hsr_s2_expand_u8", H10, W10, row0, col0, h, w);
  if (rc != HSR_OK) return rc;
  rc = s2_plane_ok("hsr_s2_expand_u8", 0, plane_dev, H, W, rs, up, H10, W10);
  if (rc != HSR_OK) return rc;
  HSR_REQUIRE(out_rs >= w, HSR_ERR_INVALID, "hsr_s2_expand_u8: an output row stride %lld below w=%d", (long long)out_rs, w);
  HSR_REQUIRE(!s2_overlap(out_dev, (int64_t)(h - 1) * out_rs + w, plane_dev, (int64_t)(H - 1) * rs + W), HSR_ERR_INVALID,
              "hsr_s2_expand_u8: the output overlaps the plane");
  const ExpandArgs a{plane_dev, rs, row0, col0, h, w, out_dev, out_rs};
  const int64_t per_row = ((int64_t)w + 15) / 16 + 1;
  const dim3 grid((unsigned)((per_row + kS2Threads - 1) / kS2Threads), (unsigned)(h < 65535 ? h : 65535));
  if (up == 2) hipLaunchKernelGGL((s2_expand_kernel<2>), grid, dim3(kS2Threads), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((s2_expand_kernel<1>), grid, dim3(kS2Threads), 0, (hipStream_t)stream, a);
  return launched(kLaunchS2Stack, "s2_expand_kernel launch", kS2Expand + (up == 2 ? 1 : 0));
}
