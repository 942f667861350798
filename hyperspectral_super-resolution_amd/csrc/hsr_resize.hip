// Area resampling at any ratio and origin on gfx950 (C ABI and the definition: include/hsr_resize.h): the area-weighted mean of the
// source pixels under each destination cell, its host twin, and the grid of one geotransform in the pixels of another.
//
// Reference: s2_emit/viz.py:19-24 (resize_s2_rgb_to, cv2 INTER_AREA) and the notebook's downsample_s2_to_grid("average"); neither
// library's bits are claimed - the cells, the taps, the validity rules and the order of the sums are the header's.
// Structure: a workgroup of four waves per tile of 8 x 32 outputs; thread t owns column t & 31 of the tile throughout.
//   staged   Phase 1: the source rectangle under the tile goes to LDS once, a wave per source row: 16-byte loads between the row's
//            first and last 16-byte boundary, single bytes outside.  A staged row keeps the alignment of its global row (it starts
//            `addr & 15` bytes into its LDS row), so a 16-byte load lands on a 16-byte LDS address.  Phase 2, the row pass: thread
//            (t >> 5, t & 31) makes R, M and the "any tap invalid" flag of the source rows t >> 5, + 8, ... for its column and
//            writes them to the LDS intermediate (16 bytes and a flag byte per entry).  Phase 3, the column pass: thread
//            (t >> 5, t & 31) sums its cell's rows from the intermediate and stores; 32 lanes store one row of the tile.  A
//            pixel-major image is staged once with all its channels and runs phases 2 and 3 per channel.
//            A tile whose rectangle exceeded the capacity the host sized - the bound has slack, so none does - would take the
//            gather path for that tile: the same result, never an access outside the LDS.
//   gather   a thread per output; the same sums in the same order from global memory.
// area_stage(), area_rowpass(), area_colpass() and area_cell() are __host__ __device__: the host twin runs them for every thread
// of every workgroup on host images.
#include <limits.h>
#include <math.h>
#include <string.h>

#include <type_traits>

#include "hsr_common.h"
#include "../../include/hsr_resize.h"

namespace hsr {

constexpr int kArThreads = 256, kArWaves = kArThreads / 64;
constexpr int kArTH = HSR_AREA_TILE_H, kArTW = HSR_AREA_TILE_W;
static_assert(kArTH * kArTW == kArThreads && kArTW == 32, "a thread per output of the tile, a tile row per half wave");

struct AreaArgs {
  const void* src;
  void* dst;
  int64_t scs, srs, sps, dcs, drs, dps;
  int C, h, w, H, W, tiles_x;
  double y0, x0, sy, sx, nodata, mvf;
  int has_nodata, rule, nodata_out;
  float post, fill;
  unsigned long long* invalid;
  int cap_r, cap_c, pitch;                           // staged: rows and columns the LDS holds, bytes of a staged row
};

struct AreaSpan {                                    // the cells j0 .. j1 - 1 of an axis: [lo, hi] and the taps a .. b - 1
  double lo, hi;
  int a, b;                                          // a == b: outside
};

struct AreaTile {
  int Y0, X0, th, tw;                                // the tile in the destination
  int ilo, nr, jlo, nc;                              // the staged source rectangle
  bool fits;
};

__host__ __device__ inline AreaSpan area_span(double o, double s, int j0, int j1, int n) {
  const double e0 = o + (double)j0 * s, e1 = o + (double)j1 * s;
  AreaSpan p;
  p.lo = e0 > 0.0 ? e0 : 0.0;
  p.hi = e1 < (double)n ? e1 : (double)n;
  if (p.hi > p.lo) { p.a = (int)floor(p.lo); p.b = (int)ceil(p.hi); }
  else { p.a = 0; p.b = 0; }
  return p;
}

__host__ __device__ inline double area_w(const AreaSpan& p, int i) {
  const double u = (double)(i + 1), l = (double)i;
  return (p.hi < u ? p.hi : u) - (p.lo > l ? p.lo : l);
}

__host__ __device__ inline double area_full(const AreaSpan& p) {
  double F = 0.0;
  for (int i = p.a; i < p.b; ++i) F += area_w(p, i);
  return F;
}

template <class T>
__host__ __device__ inline bool area_valid(const AreaArgs& a, T v) {
  if constexpr (std::is_same<T, float>::value) {
    if (!__builtin_isfinite(v)) return false;
  }
  return !(a.has_nodata && (double)v == a.nodata);
}

// The row pass of one source row for one column: p is the tap px.a, the taps are `step` elements apart.  Four taps are fetched
// before the first is used, so that four loads are in flight instead of one round trip per trip of the loop; the fetch of a tap
// past the last is that of the last, and is dropped.  An
// invalid sample adds +0.0, which changes no bit of a sum that starts at +0.0 - skipped, not multiplied.
template <class T>
__host__ __device__ inline void area_row(const AreaArgs& a, const AreaSpan& px, const T* p, int64_t step, double& R, double& M, bool& bad) {
  R = 0.0; M = 0.0;
  const int last = px.b - 1;
  for (int i = px.a; i < px.b; i += 4) {
    T v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = p[(int64_t)((i + k < last ? i + k : last) - px.a) * step];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < px.b) {
        const double wx = area_w(px, i + k);
        const bool ok = area_valid<T>(a, v[k]);
        R += wx * (ok ? (double)v[k] : 0.0);
        M += ok ? wx : 0.0;
        bad = bad || !ok;
      }
  }
}

// The rules and the value of output (c, Y, X) -> 1 when it is invalid.
template <class O>
__host__ __device__ inline unsigned area_emit(const AreaArgs& a, int c, int Y, int X, bool outside, bool bad, double S, double A, double Full) {
  const bool ok = !outside && (a.rule == HSR_AREA_STRICT ? !bad : !(A == 0.0 || A < a.mvf * Full));
  O* d = static_cast<O*>(a.dst) + (int64_t)c * a.dcs + (int64_t)Y * a.drs + (int64_t)X * a.dps;
  if constexpr (std::is_same<O, float>::value) {
    *d = ok ? (float)(S / A) * a.post : a.fill;
  } else {
    constexpr double top = std::is_same<O, uint8_t>::value ? 255.0 : 65535.0;
    double q = ok ? rint(S / A) : (double)a.nodata_out;
    q = q < 0.0 ? 0.0 : q > top ? top : q;
    *d = (O)q;
  }
  return ok ? 0u : 1u;
}

// The definition for one output, taps from the source itself.
template <class T, class O>
__host__ __device__ inline unsigned area_cell(const AreaArgs& a, int c, int Y, int X) {
  const AreaSpan py = area_span(a.y0, a.sy, Y, Y + 1, a.h), px = area_span(a.x0, a.sx, X, X + 1, a.w);
  const bool outside = py.a == py.b || px.a == px.b;
  double S = 0.0, A = 0.0, Full = 0.0;
  bool bad = false;
  if (!outside) {
    const double F = area_full(px);
    const T* col = static_cast<const T*>(a.src) + (int64_t)c * a.scs + (int64_t)px.a * a.sps;
    for (int r = py.a; r < py.b; ++r) {
      double R, M;
      area_row<T>(a, px, col + (int64_t)r * a.srs, a.sps, R, M, bad);
      const double wy = area_w(py, r);
      S += wy * R; A += wy * M; Full += wy * F;
    }
  }
  return area_emit<O>(a, c, Y, X, outside, bad, S, A, Full);
}

__host__ __device__ inline AreaTile area_tile(const AreaArgs& a, int tile) {
  AreaTile g;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  g.Y0 = ty * kArTH; g.X0 = tx * kArTW;
  g.th = a.H - g.Y0 < kArTH ? a.H - g.Y0 : kArTH;
  g.tw = a.W - g.X0 < kArTW ? a.W - g.X0 : kArTW;
  const AreaSpan py = area_span(a.y0, a.sy, g.Y0, g.Y0 + g.th, a.h), px = area_span(a.x0, a.sx, g.X0, g.X0 + g.tw, a.w);
  g.ilo = py.a; g.nr = py.b - py.a; g.jlo = px.a; g.nc = px.b - px.a;
  g.fits = g.nr <= a.cap_r && g.nc <= a.cap_c;
  return g;
}

struct AreaDevMem {
  static __device__ __forceinline__ void copy16(void* d, const void* s) { *static_cast<uint4*>(d) = *static_cast<const uint4*>(s); }
};
struct AreaHostMem {
  static void copy16(void* d, const void* s) { memcpy(d, s, 16); }
};

// The first staged byte of source row ilo + r (channel `plane`, or all channels of a pixel-major image) and its length.
template <class T, bool PIX>
__host__ __device__ inline const unsigned char* area_src_row(const AreaArgs& a, const AreaTile& g, int plane, int r, int* nbytes) {
  const int64_t ps = PIX ? a.sps : 1;
  *nbytes = (int)(((int64_t)(g.nc - 1) * ps + (PIX ? a.C : 1)) * (int64_t)sizeof(T));
  return reinterpret_cast<const unsigned char*>(static_cast<const T*>(a.src) + (PIX ? 0 : (int64_t)plane * a.scs) + (int64_t)(g.ilo + r) * a.srs +
                                                (int64_t)g.jlo * ps);
}

// Phase 1: the rows wave, wave + 4, ... of the source rectangle.
template <class Mem, class T, bool PIX>
__host__ __device__ inline void area_stage(const AreaArgs& a, const AreaTile& g, unsigned char* lds, int plane, int tid) {
  if (g.nc < 1) return;
  const int wave = tid >> 6, lane = tid & 63;
  for (int r = wave; r < g.nr; r += kArWaves) {
    int n;
    const unsigned char* p = area_src_row<T, PIX>(a, g, plane, r, &n);
    const int shift = (int)((uintptr_t)p & 15);
    unsigned char* d = lds + (size_t)r * a.pitch + shift;
    const int head = ((16 - shift) & 15) < n ? ((16 - shift) & 15) : n;
    const int nv = (n - head) >> 4, tail0 = head + (nv << 4);
    for (int v = lane; v < nv; v += 64) Mem::copy16(d + head + 16 * v, p + head + 16 * v);
    const int edge = head + (n - tail0);             // before the first and after the last boundary: at most 30 bytes
    for (int e = lane; e < edge; e += 64) {
      const int c = e < head ? e : tail0 + (e - head);
      d[c] = p[c];
    }
  }
}

// Phase 2: R, M and the flag of the source rows tid >> 5, + 8, ... for column tid & 31, channel c of the staged pixels.
template <class T, bool PIX>
__host__ __device__ inline void area_rowpass(const AreaArgs& a, const AreaTile& g, unsigned char* lds, int plane, int c, int tid) {
  const int j = tid & (kArTW - 1);
  if (j >= g.tw) return;
  const AreaSpan px = area_span(a.x0, a.sx, g.X0 + j, g.X0 + j + 1, a.w);
  const int64_t ps = PIX ? a.sps : 1;
  double* inter = reinterpret_cast<double*>(lds + (size_t)a.cap_r * a.pitch);
  unsigned char* flag = lds + (size_t)a.cap_r * a.pitch + (size_t)a.cap_r * kArTW * 16;
  for (int r = tid >> 5; r < g.nr; r += kArTH) {
    double R = 0.0, M = 0.0;
    bool bad = false;
    if (px.a < px.b) {
      int n;
      const int shift = (int)((uintptr_t)area_src_row<T, PIX>(a, g, plane, r, &n) & 15);
      const T* row = reinterpret_cast<const T*>(lds + (size_t)r * a.pitch + shift);
      area_row<T>(a, px, row + (int64_t)(px.a - g.jlo) * ps + c, ps, R, M, bad);
    }
    inter[2 * (r * kArTW + j)] = R;
    inter[2 * (r * kArTW + j) + 1] = M;
    flag[r * kArTW + j] = bad ? 1 : 0;
  }
}

// Phase 3: output (tid >> 5, tid & 31) of the tile, channel `ch` of the destination -> 1 when it is invalid.
template <class O>
__host__ __device__ inline unsigned area_colpass(const AreaArgs& a, const AreaTile& g, const unsigned char* lds, int ch, int tid) {
  const int y = tid >> 5, j = tid & (kArTW - 1);
  if (y >= g.th || j >= g.tw) return 0u;
  const AreaSpan py = area_span(a.y0, a.sy, g.Y0 + y, g.Y0 + y + 1, a.h), px = area_span(a.x0, a.sx, g.X0 + j, g.X0 + j + 1, a.w);
  const bool outside = py.a == py.b || px.a == px.b;
  const double* inter = reinterpret_cast<const double*>(lds + (size_t)a.cap_r * a.pitch);
  const unsigned char* flag = lds + (size_t)a.cap_r * a.pitch + (size_t)a.cap_r * kArTW * 16;
  double S = 0.0, A = 0.0, Full = 0.0;
  bool bad = false;
  if (!outside) {
    const double F = area_full(px);
    const int last = py.b - 1;
    for (int r0 = py.a; r0 < py.b; r0 += 4) {          // four rows in flight, as in area_row
      double Rv[4], Mv[4];
      unsigned char fv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = ((r0 + k < last ? r0 + k : last) - g.ilo) * kArTW + j;
        Rv[k] = inter[2 * e]; Mv[k] = inter[2 * e + 1]; fv[k] = flag[e];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (r0 + k < py.b) {
          const double wy = area_w(py, r0 + k);
          S += wy * Rv[k]; A += wy * Mv[k]; Full += wy * F;
          bad = bad || fv[k] != 0;
        }
    }
  }
  return area_emit<O>(a, ch, g.Y0 + y, g.X0 + j, outside, bad, S, A, Full);
}

// The tile straight from the source: the gather instance, and a staged tile that does not fit.
template <class T, class O>
__host__ __device__ inline unsigned area_tile_direct(const AreaArgs& a, const AreaTile& g, int c, int tid) {
  const int y = tid >> 5, j = tid & (kArTW - 1);
  if (y >= g.th || j >= g.tw) return 0u;
  return area_cell<T, O>(a, c, g.Y0 + y, g.X0 + j);
}

__device__ __forceinline__ void area_count(const AreaArgs& a, int c, unsigned bad) {
  if (!a.invalid) return;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) bad += __shfl_xor(bad, off, 64);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&a.invalid[c], (unsigned long long)bad);
}

template <class T, class O, bool PIX>
__global__ __launch_bounds__(kArThreads) void area_staged_kernel(const AreaArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char area_lds[];
  const int tid = threadIdx.x, plane = PIX ? 0 : (int)blockIdx.y, nch = PIX ? a.C : 1;
  const AreaTile g = area_tile(a, (int)blockIdx.x);
  if (!g.fits) {                                     // the same for the whole workgroup
    for (int c = 0; c < nch; ++c) area_count(a, plane + c, area_tile_direct<T, O>(a, g, plane + c, tid));
    return;
  }
  area_stage<AreaDevMem, T, PIX>(a, g, area_lds, plane, tid);
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    area_rowpass<T, PIX>(a, g, area_lds, plane, c, tid);
    __syncthreads();
    area_count(a, plane + c, area_colpass<O>(a, g, area_lds, plane + c, tid));
    if (c + 1 < nch) __syncthreads();
  }
}

template <class T, class O>
__global__ __launch_bounds__(kArThreads) void area_gather_kernel(const AreaArgs a) {
  const AreaTile g = area_tile(a, (int)blockIdx.x);
  area_count(a, (int)blockIdx.y, area_tile_direct<T, O>(a, g, (int)blockIdx.y, (int)threadIdx.x));
}

// The same tile code, every thread of every workgroup in turn.
template <class T, class O>
static void area_host(const AreaArgs& a, int kind, int64_t tiles) {
  static thread_local __attribute__((aligned(16))) unsigned char lds[HSR_AREA_LDS_BYTES];
  const bool pix = kind == 1;
  for (int plane = 0; plane < (pix ? 1 : a.C); ++plane)
    for (int64_t t = 0; t < tiles; ++t) {
      const AreaTile g = area_tile(a, (int)t);
      const int nch = pix ? a.C : 1;
      if (kind == 2 || !g.fits) {
        for (int c = 0; c < nch; ++c) {
          unsigned long long bad = 0;
          for (int tid = 0; tid < kArThreads; ++tid) bad += area_tile_direct<T, O>(a, g, plane + c, tid);
          if (a.invalid) a.invalid[plane + c] += bad;
        }
        continue;
      }
      for (int tid = 0; tid < kArThreads; ++tid) {
        if (pix) area_stage<AreaHostMem, T, true>(a, g, lds, plane, tid);
        else area_stage<AreaHostMem, T, false>(a, g, lds, plane, tid);
      }
      for (int c = 0; c < nch; ++c) {
        for (int tid = 0; tid < kArThreads; ++tid) {
          if (pix) area_rowpass<T, true>(a, g, lds, plane, c, tid);
          else area_rowpass<T, false>(a, g, lds, plane, c, tid);
        }
        unsigned long long bad = 0;
        for (int tid = 0; tid < kArThreads; ++tid) bad += area_colpass<O>(a, g, lds, plane + c, tid);
        if (a.invalid) a.invalid[plane + c] += bad;
      }
    }
}

static int area_esize(int dt) { return dt == HSR_AREA_F32 ? 4 : dt == HSR_AREA_U8 ? 1 : 2; }

// <I, O> of the names: 0 <F32, F32>, 1 <U8, U8>, 2 <U8, F32>, 3 <U16, U16>, 4 <U16, F32>; -1: no such pair.
static int area_pair(int in, int out) {
  if (in == HSR_AREA_F32) return out == HSR_AREA_F32 ? 0 : -1;
  if (in == HSR_AREA_U8) return out == HSR_AREA_U8 ? 1 : out == HSR_AREA_F32 ? 2 : -1;
  if (in == HSR_AREA_U16) return out == HSR_AREA_U16 ? 3 : out == HSR_AREA_F32 ? 4 : -1;
  return -1;
}

// The instance for a layout, a dtype pair and a scale (the header's hsr_area_resample_instance): kind 0 staged planar, 1 staged
// pixel-major, 2 gather, and the capacities of a staged workgroup.
static int area_select(const char* who, int32_t in_dtype, int32_t out_dtype, int32_t C, int64_t scs, int64_t sps, double sy, double sx,
                       int* kind, int* cap_r, int* cap_c, int* pitch, size_t* lds) {
  HSR_REQUIRE(in_dtype >= 0 && in_dtype <= 2 && out_dtype >= 0 && out_dtype <= 2, HSR_ERR_INVALID, "%s: in_dtype=%d or out_dtype=%d outside {0,1,2}",
              who, in_dtype, out_dtype);
  const int pair = area_pair(in_dtype, out_dtype);
  HSR_REQUIRE(pair >= 0, HSR_ERR_INVALID, "%s: out_dtype=%d is neither in_dtype=%d nor float32", who, out_dtype, in_dtype);
  HSR_REQUIRE(C >= 1 && C <= HSR_AREA_MAX_CHANNELS, HSR_ERR_INVALID, "%s: C=%d outside [1,%d]", who, C, HSR_AREA_MAX_CHANNELS);
  HSR_REQUIRE(isfinite(sy) && isfinite(sx), HSR_ERR_INVALID, "%s: a scale (%g, %g) that is not finite", who, sy, sx);
  HSR_REQUIRE(sy >= 1.0 && sy <= HSR_AREA_MAX_SCALE && sx >= 1.0 && sx <= HSR_AREA_MAX_SCALE, HSR_ERR_UNSUPPORTED,
              "%s: scale (%g, %g) outside [1,%d]: enlarging is hsr_bilinear_upsample's", who, sy, sx, HSR_AREA_MAX_SCALE);
  *kind = sps == 1 ? 0 : (scs == 1 && sps >= C && sps <= 64) ? 1 : 2;
  *cap_r = *cap_c = *pitch = 0;
  *lds = 0;
  if (*kind != 2) {
    const int rows = (int)ceil(kArTH * sy) + 3, cols = (int)ceil(kArTW * sx) + 3;
    const int64_t elems = *kind == 1 ? (int64_t)(cols - 1) * sps + C : cols;
    const int64_t p = ((elems * area_esize(in_dtype) + 15) & ~(int64_t)15) + 16;
    const int64_t bytes = rows * p + (int64_t)rows * kArTW * 16 + (((int64_t)rows * kArTW + 15) & ~(int64_t)15);
    if (bytes > HSR_AREA_LDS_BYTES) *kind = 2;
    else { *cap_r = rows; *cap_c = cols; *pitch = (int)p; *lds = (size_t)bytes; }
  }
  return HSR_OK;
}

// Strides under which no two elements of a (C, rows, cols) image share an address: in ascending order of the stride, each is at
// least the extent of everything below it.  -> the image's extent in elements, 0 when refused.
static int64_t area_extent(int32_t C, int32_t rows, int32_t cols, int64_t cs, int64_t rs, int64_t ps) {
  int64_t st[3] = {cs, rs, ps}, n[3] = {C, rows, cols};
  for (int k = 0; k < 3; ++k)
    if (st[k] < 1 || st[k] > ((int64_t)1 << 40)) return 0;
  for (int u = 0; u < 3; ++u)
    for (int v = u + 1; v < 3; ++v)
      if (st[v] < st[u]) { const int64_t s = st[u], m = n[u]; st[u] = st[v]; n[u] = n[v]; st[v] = s; n[v] = m; }
  int64_t below = 1;
  for (int k = 0; k < 3; ++k) {
    if (n[k] == 1) continue;
    if (st[k] < below) return 0;
    below += (n[k] - 1) * st[k];
  }
  return below;
}

static bool area_overlap(const void* p, int64_t pn, const void* q, int64_t qn) {
  const uintptr_t pb = (uintptr_t)p, qb = (uintptr_t)q;
  return !(pb + (uintptr_t)pn <= qb || qb + (uintptr_t)qn <= pb);
}

static int area_args(const char* who, const void* src, int32_t in_dtype, int32_t C, int32_t h, int32_t w, int64_t scs, int64_t srs, int64_t sps,
                     double y0, double x0, double sy, double sx, int32_t has_nodata, double nodata, int32_t rule, double mvf, void* dst,
                     int32_t out_dtype, int32_t H, int32_t W, int64_t dcs, int64_t drs, int64_t dps, float post, float fill, int32_t nodata_out,
                     int64_t* invalid, AreaArgs* a, int* kind, size_t* lds, int64_t* tiles) {
  HSR_REQUIRE(src && dst, HSR_ERR_INVALID, "%s: NULL pointer", who);
  HSR_REQUIRE(h >= 1 && w >= 1 && H >= 1 && W >= 1, HSR_ERR_INVALID, "%s: an extent < 1 (source %d x %d, destination %d x %d)", who, h, w, H, W);
  HSR_REQUIRE(isfinite(y0) && isfinite(x0), HSR_ERR_INVALID, "%s: an origin (%g, %g) that is not finite", who, y0, x0);
  const int rc = area_select(who, in_dtype, out_dtype, C, scs, sps, sy, sx, kind, &a->cap_r, &a->cap_c, &a->pitch, lds);
  if (rc != HSR_OK) return rc;
  HSR_REQUIRE(rule == HSR_AREA_STRICT || rule == HSR_AREA_RENORM, HSR_ERR_INVALID, "%s: rule=%d outside {0,1}", who, rule);
  HSR_REQUIRE(mvf >= 0.0 && mvf <= 1.0, HSR_ERR_INVALID, "%s: min_valid_frac=%g outside [0,1]", who, mvf);
  const int es = area_esize(in_dtype), eo = area_esize(out_dtype);
  HSR_REQUIRE((uintptr_t)src % es == 0 && (uintptr_t)dst % eo == 0, HSR_ERR_INVALID, "%s: a pointer that is no multiple of its element size", who);
  HSR_REQUIRE(out_dtype == HSR_AREA_F32 || (nodata_out >= 0 && nodata_out <= (out_dtype == HSR_AREA_U8 ? 255 : 65535)), HSR_ERR_INVALID,
              "%s: nodata_out=%d is no value of the output type", who, nodata_out);
  const int64_t sn = area_extent(C, h, w, scs, srs, sps), dn = area_extent(C, H, W, dcs, drs, dps);
  HSR_REQUIRE(sn > 0, HSR_ERR_INVALID, "%s: source strides (%lld, %lld, %lld) < 1 or under which elements overlap", who, (long long)scs,
              (long long)srs, (long long)sps);
  HSR_REQUIRE(dn > 0, HSR_ERR_INVALID, "%s: destination strides (%lld, %lld, %lld) < 1 or under which elements overlap", who, (long long)dcs,
              (long long)drs, (long long)dps);
  HSR_REQUIRE(!area_overlap(dst, dn * eo, src, sn * es), HSR_ERR_INVALID, "%s: the output overlaps the input", who);
  const int tiles_x = (W + kArTW - 1) / kArTW;
  *tiles = (int64_t)tiles_x * ((H + kArTH - 1) / kArTH);
  HSR_REQUIRE(*tiles <= INT_MAX, HSR_ERR_UNSUPPORTED, "%s: %lld tiles of %d x %d, more than 2^31 - 1", who, (long long)*tiles, kArTH, kArTW);
  a->src = src; a->dst = dst; a->scs = scs; a->srs = srs; a->sps = sps; a->dcs = dcs; a->drs = drs; a->dps = dps;
  a->C = C; a->h = h; a->w = w; a->H = H; a->W = W; a->tiles_x = tiles_x;
  a->y0 = y0; a->x0 = x0; a->sy = sy; a->sx = sx; a->nodata = nodata; a->mvf = mvf;
  a->has_nodata = has_nodata != 0; a->rule = rule; a->nodata_out = nodata_out; a->post = post; a->fill = fill;
  a->invalid = reinterpret_cast<unsigned long long*>(invalid);
  return HSR_OK;
}

template <class T, class O>
static void area_launch(int kind, const AreaArgs& a, int64_t tiles, size_t lds, hipStream_t s) {
  const dim3 block(kArThreads);
  static thread_local size_t planar_lds = 64 * 1024, pix_lds = 64 * 1024;      // the dynamic-LDS limit each staged kernel has been given
  if (kind == 0) {
    raise_lds_limit(reinterpret_cast<const void*>(&area_staged_kernel<T, O, false>), lds, planar_lds);
    hipLaunchKernelGGL((area_staged_kernel<T, O, false>), dim3((unsigned)tiles, (unsigned)a.C), block, lds, s, a);
  } else if (kind == 1) {
    raise_lds_limit(reinterpret_cast<const void*>(&area_staged_kernel<T, O, true>), lds, pix_lds);
    hipLaunchKernelGGL((area_staged_kernel<T, O, true>), dim3((unsigned)tiles, 1), block, lds, s, a);
  } else hipLaunchKernelGGL((area_gather_kernel<T, O>), dim3((unsigned)tiles, (unsigned)a.C), block, 0, s, a);
}

}  // namespace hsr

using namespace hsr;

extern "C" int hsr_area_resample(const void* src_dev, int32_t in_dtype, int32_t C, int32_t h, int32_t w, int64_t src_cs, int64_t src_rs,
                                 int64_t src_ps, double y0, double x0, double sy, double sx, int32_t has_nodata, double nodata, int32_t rule,
                                 double min_valid_frac, void* dst_dev, int32_t out_dtype, int32_t H, int32_t W, int64_t dst_cs, int64_t dst_rs,
                                 int64_t dst_ps, float post_scale, float fill, int32_t nodata_out, int64_t* invalid_dev, hsr_stream_t stream) {
  AreaArgs a{};
  int kind = 0;
  size_t lds = 0;
  int64_t tiles = 0;
  int rc = area_args("hsr_area_resample", src_dev, in_dtype, C, h, w, src_cs, src_rs, src_ps, y0, x0, sy, sx, has_nodata, nodata, rule,
                     min_valid_frac, dst_dev, out_dtype, H, W, dst_cs, dst_rs, dst_ps, post_scale, fill, nodata_out, invalid_dev, &a, &kind, &lds,
                     &tiles);
  if (rc != HSR_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (invalid_dev) {
    rc = check_hip(hipMemsetAsync(invalid_dev, 0, (size_t)C * sizeof(int64_t), s), "hsr_area_resample: clearing the counts");
    if (rc != HSR_OK) return rc;
  }
  const int pair = area_pair(in_dtype, out_dtype);
  switch (pair) {
    case 0: area_launch<float, float>(kind, a, tiles, lds, s); break;
    case 1: area_launch<uint8_t, uint8_t>(kind, a, tiles, lds, s); break;
    case 2: area_launch<uint8_t, float>(kind, a, tiles, lds, s); break;
    case 3: area_launch<uint16_t, uint16_t>(kind, a, tiles, lds, s); break;
    default: area_launch<uint16_t, float>(kind, a, tiles, lds, s); break;
  }
  return launched(kLaunchResize, "area resample kernel launch", kAreaStaged + 5 * kind + pair);
}

extern "C" int hsr_area_resample_host(const void* src, int32_t in_dtype, int32_t C, int32_t h, int32_t w, int64_t src_cs, int64_t src_rs,
                                      int64_t src_ps, double y0, double x0, double sy, double sx, int32_t has_nodata, double nodata,
                                      int32_t rule, double min_valid_frac, void* dst, int32_t out_dtype, int32_t H, int32_t W, int64_t dst_cs,
                                      int64_t dst_rs, int64_t dst_ps, float post_scale, float fill, int32_t nodata_out, int64_t* invalid) {
  AreaArgs a{};
  int kind = 0;
  size_t lds = 0;
  int64_t tiles = 0;
  const int rc = area_args("hsr_area_resample_host", src, in_dtype, C, h, w, src_cs, src_rs, src_ps, y0, x0, sy, sx, has_nodata, nodata, rule,
                           min_valid_frac, dst, out_dtype, H, W, dst_cs, dst_rs, dst_ps, post_scale, fill, nodata_out, invalid, &a, &kind, &lds,
                           &tiles);
  if (rc != HSR_OK) return rc;
  if (invalid)
    for (int c = 0; c < C; ++c) invalid[c] = 0;
  switch (area_pair(in_dtype, out_dtype)) {
    case 0: area_host<float, float>(a, kind, tiles); break;
    case 1: area_host<uint8_t, uint8_t>(a, kind, tiles); break;
    case 2: area_host<uint8_t, float>(a, kind, tiles); break;
    case 3: area_host<uint16_t, uint16_t>(a, kind, tiles); break;
    default: area_host<uint16_t, float>(a, kind, tiles); break;
  }
  return HSR_OK;
}

extern "C" int hsr_area_resample_instance(int32_t in_dtype, int32_t out_dtype, int32_t C, int64_t src_cs, int64_t src_ps, double sy, double sx) {
  int kind = 0, cap_r, cap_c, pitch;
  size_t lds;
  const int rc = area_select("hsr_area_resample_instance", in_dtype, out_dtype, C, src_cs, src_ps, sy, sx, &kind, &cap_r, &cap_c, &pitch, &lds);
  if (rc != HSR_OK) return rc;
  return kAreaStaged + 5 * kind + area_pair(in_dtype, out_dtype);
}

extern "C" int hsr_area_grid_from_geotransforms(const double* src_gt, const double* dst_gt, double* grid) {
  const char* who = "hsr_area_grid_from_geotransforms";
  HSR_REQUIRE(src_gt && dst_gt && grid, HSR_ERR_INVALID, "%s: NULL pointer", who);
  for (int k = 0; k < 6; ++k)
    HSR_REQUIRE(isfinite(src_gt[k]) && isfinite(dst_gt[k]), HSR_ERR_INVALID, "%s: term %d of a geotransform is not finite", who, k);
  HSR_REQUIRE(src_gt[1] != 0.0 && src_gt[5] != 0.0 && dst_gt[1] != 0.0 && dst_gt[5] != 0.0, HSR_ERR_INVALID, "%s: a pixel size of 0", who);
  HSR_REQUIRE(src_gt[2] == 0.0 && src_gt[4] == 0.0 && dst_gt[2] == 0.0 && dst_gt[4] == 0.0, HSR_ERR_UNSUPPORTED,
              "%s: rotation terms (%g, %g) and (%g, %g)", who, src_gt[2], src_gt[4], dst_gt[2], dst_gt[4]);
  const double sx = dst_gt[1] / src_gt[1], sy = dst_gt[5] / src_gt[5];
  HSR_REQUIRE(sx > 0.0 && sy > 0.0, HSR_ERR_UNSUPPORTED, "%s: pixel sizes of differing sign (%g vs %g, %g vs %g)", who, src_gt[1], dst_gt[1],
              src_gt[5], dst_gt[5]);
  HSR_REQUIRE(sx >= 1.0 && sy >= 1.0, HSR_ERR_UNSUPPORTED, "%s: scale (%g, %g) below 1: enlarging is hsr_bilinear_upsample's", who, sy, sx);
  grid[0] = (dst_gt[3] - src_gt[3]) / src_gt[5];
  grid[1] = (dst_gt[0] - src_gt[0]) / src_gt[1];
  grid[2] = sy;
  grid[3] = sx;
  return HSR_OK;
}
