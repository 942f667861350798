// Polygon regions of interest on gfx950 (C ABI and the definitions: include/hsr_roi.h): a polygon set rasterised onto a north-up
// grid under the centre or the touched rule, the class histogram of a uint8 plane inside it, and the GLT clip + re-index of
// spatial_subset - each with the host twin compiled from the same element functions.
//
// Reference: rasterio.mask.mask in s2_data/cloud_utils.py:33-53 / :82-101 and s2_data/s2_utils.py:361-383; rioxarray's clip and the
// min / max / re-index of EMIT_data/emit_tools.py:557-600.  GDAL's bits are not claimed; the header's rules are the definition.
// Structure: one tile routine, three consumers.
//   tile     a workgroup of 256 threads owns 64 x 256 cells.  The edges are streamed from device memory, an edge a thread (with few
//            edges, up to 32 threads share one and take its rows in turn): its two
//            vertices go to pixel coordinates, and for every row of the tile the edge can reach, the crossing of the row's centre
//            line is evaluated once and becomes ONE toggle bit in LDS (bit k - 1, k the number of columns left of the crossing,
//            clamped to the tile: a crossing right of the tile toggles the last bit, one left of it nothing).  A row therefore holds
//            any number of crossings in 256 bits; the inside flags are the suffix parity of the toggle bits - five shifts a word and
//            a carry from the words to its right.  The touched rule ORs column ranges into a second bit plane.  The edge list is
//            never in LDS; 6 KB hold the three bit planes.
//   raster   a thread owns 16 consecutive cells: 16 bits of the plane become 16 bytes and one 16-byte store.  The runs are anchored on
//            the ADDRESS, row by row (10980 is no multiple of 16): single bytes before a row's first boundary and behind its last.
//   counts   the same 16 cells are LOADED - only where a bit is set - and counted into 13 register bins; a wave sum per bin, the four
//            waves joined in LDS, one integer atomic per non-zero bin and workgroup.
//   clip     a thread a column, 64 rows: coalesced (column, row) pairs in, the pair or (0, 0) out; min / max / count per thread, wave
//            and workgroup, then at most five integer atomics on the record.  The re-index reads the record from device memory.
#include <limits.h>
#include <math.h>

#include <vector>

#include "hsr_common.h"
#include "../../include/hsr_roi.h"

namespace hsr {

constexpr int kRoiThreads = 256, kRoiWaves = kRoiThreads / 64;
constexpr int kRoiTH = HSR_ROI_TILE_H, kRoiTW = HSR_ROI_TILE_W, kRoiWords = kRoiTW / 32, kRoiRun = HSR_ROI_RUN;
constexpr int kRoiClasses = 13;                      // bins in use: 0 .. 11 and "other"
constexpr int kRoiMaxExtent = 1 << 30;               // H and W: a tile past the last cell still has int coordinates
constexpr double kRoiCoordMax = 1e300;
static_assert(kRoiTW * kRoiTH == kRoiThreads * kRoiRun * 4, "raster / counts: four passes of 256 threads x 16 cells");
static_assert(kRoiTW == kRoiThreads, "clip: a thread a column");

struct RoiPoly {
  const double* verts;
  const int32_t* offs;
  int nrings, nverts;
  double x0, dx, y0, dy;
  int share;                                         // kernels only: log2 of the threads that share an edge, 0 .. 5
};

// ------------------------------------------------------------------------------------------------------------------------------
// the element functions: one definition for the kernels and the host twins
// ------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int roi_clamp_int(double v, int lo, int hi) {
  return v >= (double)hi ? hi : (v > (double)lo ? (int)v : lo);   // NaN -> lo
}

__host__ __device__ inline bool roi_finite(double t) { return t - t == 0.0; }

__host__ __device__ inline double roi_coord(double t) { return t > kRoiCoordMax ? kRoiCoordMax : (t < -kRoiCoordMax ? -kRoiCoordMax : t); }

// Edge e (vertex e to its ring's next vertex) in pixel coordinates; false: the edge is dropped (see THE POLYGON SET).
__host__ __device__ inline bool roi_edge(const RoiPoly& p, int e, double& ua, double& va, double& ub, double& vb) {
  int lo = 0, hi = p.nrings;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (p.offs[mid] <= e) lo = mid;
    else hi = mid;
  }
  const int start = p.offs[lo], end = p.offs[lo + 1];
  if (!(start >= 0 && start <= e && e < end && end <= p.nverts)) return false;
  const int n = e + 1 < end ? e + 1 : start;
  const double xa = p.verts[2 * (int64_t)e], ya = p.verts[2 * (int64_t)e + 1], xb = p.verts[2 * (int64_t)n], yb = p.verts[2 * (int64_t)n + 1];
  if (!(roi_finite(xa) && roi_finite(ya) && roi_finite(xb) && roi_finite(yb))) return false;
  ua = roi_coord((xa - p.x0) / p.dx);
  va = roi_coord((ya - p.y0) / p.dy);
  ub = roi_coord((xb - p.x0) / p.dx);
  vb = roi_coord((yb - p.y0) / p.dy);
  return true;
}

// THE CENTRE RULE's first condition on the line pv; xc = the right-hand side of its second.
__host__ __device__ inline bool roi_crossing(double ua, double va, double ub, double vb, double pv, double& xc) {
  if ((va <= pv) == (vb <= pv)) return false;
  xc = ua + (pv - va) * (ub - ua) / (vb - va);
  return true;
}

// ca + the number of columns c in [ca, cb) with c + 0.5 < xc: the floor proposes, the rule's own comparison decides.
__host__ __device__ inline int roi_cross_count(double xc, int ca, int cb) {
  int k = roi_clamp_int(floor(xc - 0.5), ca, cb);
  if (k < cb && (double)k + 0.5 < xc) ++k;
  return k;
}

// THE TOUCHED RULE's span of an edge in row r: false when the edge does not reach the row; else the covered columns flo .. fhi
// as integral doubles (not yet bounded).
__host__ __device__ inline bool roi_touch_span(double ua, double va, double ub, double vb, double r, double& flo, double& fhi) {
  const double vmin = va < vb ? va : vb, vmax = va < vb ? vb : va;
  if (!(floor(vmin) <= r && r <= floor(vmax))) return false;
  double u1 = ua, u2 = ub;
  if (va != vb) {
    const double lo = vmin > r ? vmin : r, hi = vmax < r + 1.0 ? vmax : r + 1.0;
    u1 = lo == va ? ua : (lo == vb ? ub : ua + (lo - va) * (ub - ua) / (vb - va));
    u2 = hi == va ? ua : (hi == vb ? ub : ua + (hi - va) * (ub - ua) / (vb - va));
  }
  flo = floor(u1 < u2 ? u1 : u2);
  fhi = floor(u1 < u2 ? u2 : u1);
  return true;
}

// max(g - lo, 0) in 64 bits
__host__ __device__ inline int32_t roi_reindex(int32_t g, int32_t lo) {
  const int64_t d = (int64_t)g - (int64_t)lo;
  return d > 0 ? (int32_t)d : 0;
}

// ------------------------------------------------------------------------------------------------------------------------------
// the tile: msk[row][word] = the inside (touched) flags of the 64 x 256 cells at grid (R0, C0)
// ------------------------------------------------------------------------------------------------------------------------------
struct RoiBits {
  uint32_t tog[kRoiTH][kRoiWords];
  uint32_t tch[kRoiTH][kRoiWords];
  uint32_t msk[kRoiTH][kRoiWords];
};

template <int RULE>
__device__ __forceinline__ void roi_tile_bits(const RoiPoly& p, int R0, int C0, RoiBits& b) {
  const int tid = threadIdx.x;
  for (int i = tid; i < kRoiTH * kRoiWords; i += kRoiThreads) {
    (&b.tog[0][0])[i] = 0;
    (&b.tch[0][0])[i] = 0;
  }
  __syncthreads();
  // 2^p.share threads share an edge and take its rows in turn: a five-edge footprint keeps 160 lanes busy instead of five
  const int sub = tid & ((1 << p.share) - 1);
  for (int e = tid >> p.share; e < p.nverts; e += kRoiThreads >> p.share) {
    double ua, va, ub, vb;
    if (!roi_edge(p, e, ua, va, ub, vb)) continue;
    const double vmin = va < vb ? va : vb, vmax = va < vb ? vb : va;
    // the rows the edge can reach under either rule: floor(vmin) - 1 .. floor(vmax) + 1, bounded to the tile; the rules decide
    const int ra = roi_clamp_int(floor(vmin) - 1.0, R0, R0 + kRoiTH), rb = roi_clamp_int(floor(vmax) + 1.0, R0 - 1, R0 + kRoiTH - 1);
    for (int r = ra + sub; r <= rb; r += 1 << p.share) {
      const int i = r - R0;
      double xc;
      if (roi_crossing(ua, va, ub, vb, (double)r + 0.5, xc)) {
        const int k = roi_cross_count(xc, C0, C0 + kRoiTW) - C0;      // 0 .. 256: the cells 0 .. k - 1 of the row lie left of it
        if (k > 0) atomicXor(&b.tog[i][(k - 1) >> 5], 1u << ((k - 1) & 31));
      }
      if constexpr (RULE == HSR_ROI_TOUCHED) {
        double flo, fhi;
        if (roi_touch_span(ua, va, ub, vb, (double)r, flo, fhi)) {
          const int cl = roi_clamp_int(flo, C0, C0 + kRoiTW) - C0, ch = roi_clamp_int(fhi, C0 - 1, C0 + kRoiTW - 1) - C0;
          for (int w = cl >> 5; cl <= ch && w <= (ch >> 5); ++w) {
            const uint32_t from = w == (cl >> 5) ? ~0u << (cl & 31) : ~0u, to = w == (ch >> 5) ? ~0u >> (31 - (ch & 31)) : ~0u;
            atomicOr(&b.tch[i][w], from & to);
          }
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < kRoiTH * kRoiWords; i += kRoiThreads) {
    const int row = i / kRoiWords, w = i - row * kRoiWords;
    uint32_t s = b.tog[row][w];                        // bit j becomes the parity of the bits j .. 31
    s ^= s >> 1;
    s ^= s >> 2;
    s ^= s >> 4;
    s ^= s >> 8;
    s ^= s >> 16;
    uint32_t right = 0;
    for (int j = w + 1; j < kRoiWords; ++j) right ^= b.tog[row][j];
    s ^= 0u - (uint32_t)(__popc(right) & 1);
    if constexpr (RULE == HSR_ROI_TOUCHED) s |= b.tch[row][w];
    b.msk[row][w] = s;
  }
  __syncthreads();
}

struct RoiArgs {
  RoiPoly p;
  int row_off, col_off, h, w, tiles_x;
  uint8_t in_v, out_v;
  uint8_t* out;                                       // raster
  int64_t ors;
  const uint8_t* plane;                               // counts: the plane's cell (row_off, col_off)
  int64_t prs;
  int32_t* counts;
  int32_t* inside;
  const int32_t* glt;                                 // clip
  int W;
  int32_t* oglt;
  int32_t* rec;
};

__device__ __forceinline__ unsigned roi_wave_sum(unsigned v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// four bits -> four bytes of 0 / 1
__device__ __forceinline__ uint32_t roi_spread4(uint32_t bits) { return ((bits & 0xfu) * 0x00204081u) & 0x01010101u; }

// 16 flags of a row of the tile from bit `at` (0 .. 240 + 15: the bits past the row's end read as 0)
__device__ __forceinline__ uint32_t roi_bits16(const uint32_t (&row)[kRoiWords], int at) {
  const int w = at >> 5;
  const uint64_t two = (uint64_t)row[w] | (w + 1 < kRoiWords ? (uint64_t)row[w + 1] << 32 : 0ull);
  return (uint32_t)(two >> (at & 31)) & 0xffffu;
}
__device__ __forceinline__ uint32_t roi_bit(const uint32_t (&row)[kRoiWords], int at) { return (row[at >> 5] >> (at & 31)) & 1u; }

// A row of the tile as 16 threads share it: 16-byte runs ANCHORED ON THE ADDRESS (a row stride of 10980 is no multiple of 16, and
// every row of the plane would otherwise fall back to single bytes): a0 bytes before the first 16-byte boundary, nv whole runs
// from there, and what is left behind the last; thread j owns run j, head byte j and tail byte j.
struct RoiRowSplit {
  int a0, nv, t0;
};
__device__ __forceinline__ RoiRowSplit roi_row_split(const void* row_start, int wt) {
  RoiRowSplit s;
  s.a0 = (int)((16u - (unsigned)((uintptr_t)row_start & 15u)) & 15u);
  s.nv = wt > s.a0 ? (wt - s.a0) >> 4 : 0;
  s.t0 = s.a0 + 16 * s.nv;
  return s;
}

template <int RULE>
__global__ __launch_bounds__(kRoiThreads) void roi_raster_kernel(const RoiArgs a) {
  __shared__ RoiBits b;
  const int tid = threadIdx.x;
  const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
  const int r0 = ty * kRoiTH, c0 = tx * kRoiTW;     // in the window
  roi_tile_bits<RULE>(a.p, a.row_off + r0, a.col_off + c0, b);
  const uint32_t base = (uint32_t)a.out_v * 0x01010101u, flip = (uint32_t)(a.in_v ^ a.out_v);
  const int j = tid & 15, wt = a.w - c0 < kRoiTW ? a.w - c0 : kRoiTW;
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int row = pass * 16 + (tid >> 4), r = r0 + row;
    if (r >= a.h) break;
    uint8_t* o = a.out + (int64_t)r * a.ors + c0;
    const RoiRowSplit sp = roi_row_split(o, wt);
    if (j < sp.nv) {
      const int at = sp.a0 + 16 * j;
      const uint32_t bits = roi_bits16(b.msk[row], at);
      uint32_t q[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = base ^ (roi_spread4(bits >> (4 * k)) * flip);
      *reinterpret_cast<uint4*>(o + at) = make_uint4(q[0], q[1], q[2], q[3]);
    }
    if (j < sp.a0 && j < wt) o[j] = roi_bit(b.msk[row], j) ? a.in_v : a.out_v;
    if (sp.t0 + j < wt) o[sp.t0 + j] = roi_bit(b.msk[row], sp.t0 + j) ? a.in_v : a.out_v;
  }
}

// one cell into the bins: v = its class value, or 0x100 (in no bin) where the cell is not inside
__device__ __forceinline__ void roi_count(unsigned (&bins)[kRoiClasses + 1], unsigned v) {
#pragma unroll
  for (int k = 0; k < kRoiClasses - 1; ++k) bins[k] += v == (unsigned)k ? 1u : 0u;
  bins[kRoiClasses - 1] += v >= (unsigned)(kRoiClasses - 1) && v < 0x100u ? 1u : 0u;
  bins[kRoiClasses] += v < 0x100u ? 1u : 0u;
}

template <int RULE>
__global__ __launch_bounds__(kRoiThreads) void roi_counts_kernel(const RoiArgs a) {
  __shared__ RoiBits b;
  __shared__ unsigned part[kRoiWaves][kRoiClasses + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
  const int r0 = ty * kRoiTH, c0 = tx * kRoiTW;
  roi_tile_bits<RULE>(a.p, a.row_off + r0, a.col_off + c0, b);
  unsigned bins[kRoiClasses + 1];                      // the last: the inside cells
#pragma unroll
  for (int k = 0; k <= kRoiClasses; ++k) bins[k] = 0;
  const int j = tid & 15, wt = a.w - c0 < kRoiTW ? a.w - c0 : kRoiTW;
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int row = pass * 16 + (tid >> 4), r = r0 + row;
    if (r >= a.h) break;
    const uint8_t* in = a.plane + (int64_t)r * a.prs + c0;
    const RoiRowSplit sp = roi_row_split(in, wt);
    if (j < sp.nv) {
      const int at = sp.a0 + 16 * j;
      const uint32_t bits = roi_bits16(b.msk[row], at);
      if (bits) {                                      // a run without an inside cell is not read
        const uint4 v = *reinterpret_cast<const uint4*>(in + at);
        const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < kRoiRun; ++i) roi_count(bins, (bits >> i) & 1u ? (q[i >> 2] >> (8 * (i & 3))) & 0xffu : 0x100u);
      }
    }
    if (j < sp.a0 && j < wt && roi_bit(b.msk[row], j)) roi_count(bins, in[j]);
    if (sp.t0 + j < wt && roi_bit(b.msk[row], sp.t0 + j)) roi_count(bins, in[sp.t0 + j]);
  }
#pragma unroll
  for (int k = 0; k <= kRoiClasses; ++k) {
    const unsigned s = roi_wave_sum(bins[k]);
    if (lane == 0) part[wave][k] = s;
  }
  __syncthreads();
  if (tid <= kRoiClasses) {
    unsigned s = 0;
#pragma unroll
    for (int w = 0; w < kRoiWaves; ++w) s += part[w][tid];
    if (s) atomicAdd(tid < kRoiClasses ? &a.counts[tid] : a.inside, (int)s);
  }
}

__global__ void roi_record_init_kernel(int32_t* rec) {
  const int t = threadIdx.x;
  if (t < HSR_ROI_RECORD) rec[t] = t == 0 || t == 2 ? INT_MAX : (t == 1 || t == 3 ? -1 : 0);
}

__device__ __forceinline__ int roi_wave_min(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ int roi_wave_max(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(kRoiThreads) void roi_glt_clip_kernel(const RoiArgs a) {
  __shared__ RoiBits b;
  __shared__ int red[kRoiWaves][5];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
  const int r0 = ty * kRoiTH, c0 = tx * kRoiTW;
  roi_tile_bits<HSR_ROI_TOUCHED>(a.p, a.row_off + r0, a.col_off + c0, b);
  int ylo = INT_MAX, yhi = 0, xlo = INT_MAX, xhi = 0, n = 0;       // one-based: 0 = none
  const int c = c0 + tid;
  if (c < a.w) {
    const int rows = a.h - r0 < kRoiTH ? a.h - r0 : kRoiTH;
    const int2* in = reinterpret_cast<const int2*>(a.glt) + ((int64_t)(a.row_off + r0) * a.W + a.col_off + c);
    int2* out = reinterpret_cast<int2*>(a.oglt) + ((int64_t)r0 * a.w + c);
    for (int row = 0; row < rows; ++row, in += a.W, out += a.w) {
      int2 g = make_int2(0, 0);
      if ((b.msk[row][tid >> 5] >> (tid & 31)) & 1u) {
        g = *in;
        if (g.x > 0) { xlo = g.x < xlo ? g.x : xlo; xhi = g.x > xhi ? g.x : xhi; }
        if (g.y > 0) { ylo = g.y < ylo ? g.y : ylo; yhi = g.y > yhi ? g.y : yhi; }
        n += g.x > 0 && g.y > 0 ? 1 : 0;
      }
      *out = g;
    }
  }
  ylo = roi_wave_min(ylo); yhi = roi_wave_max(yhi); xlo = roi_wave_min(xlo); xhi = roi_wave_max(xhi); n = (int)roi_wave_sum((unsigned)n);
  if (lane == 0) { red[wave][0] = ylo; red[wave][1] = yhi; red[wave][2] = xlo; red[wave][3] = xhi; red[wave][4] = n; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kRoiWaves; ++w) {
      ylo = red[w][0] < ylo ? red[w][0] : ylo; yhi = red[w][1] > yhi ? red[w][1] : yhi;
      xlo = red[w][2] < xlo ? red[w][2] : xlo; xhi = red[w][3] > xhi ? red[w][3] : xhi;
      n += red[w][4];
    }
    if (yhi > 0) { atomicMin(&a.rec[0], ylo - 1); atomicMax(&a.rec[1], yhi - 1); }
    if (xhi > 0) { atomicMin(&a.rec[2], xlo - 1); atomicMax(&a.rec[3], xhi - 1); }
    if (n) atomicAdd(&a.rec[4], n);
  }
}

__global__ __launch_bounds__(kRoiThreads) void roi_glt_reindex_kernel(int32_t* glt, int64_t n, const int32_t* __restrict__ rec) {
  const int32_t down_lo = rec[0], cross_lo = rec[2];
  int2* g = reinterpret_cast<int2*>(glt);
  for (int64_t i = (int64_t)blockIdx.x * kRoiThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRoiThreads) {
    const int2 v = g[i];
    g[i] = make_int2(roi_reindex(v.x, cross_lo), roi_reindex(v.y, down_lo));
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// the host side: the checks, the host twins
// ------------------------------------------------------------------------------------------------------------------------------
static int roi_counts_ok(const char* who, const void* verts, const void* offs, int32_t nrings, int32_t nverts) {
  HSR_REQUIRE(verts && offs, HSR_ERR_INVALID, "%s: NULL polygon arrays", who);
  HSR_REQUIRE(nrings >= 1, HSR_ERR_INVALID, "%s: nrings=%d < 1", who, nrings);
  HSR_REQUIRE(nverts <= HSR_ROI_MAX_EDGES, HSR_ERR_INVALID, "%s: %d edges, more than HSR_ROI_MAX_EDGES = %d", who, nverts, HSR_ROI_MAX_EDGES);
  HSR_REQUIRE((int64_t)nverts >= 3 * (int64_t)nrings, HSR_ERR_INVALID, "%s: %d vertices for %d rings: a ring has at least 3 vertices", who,
              nverts, nrings);
  return HSR_OK;
}

static int roi_contents_ok(const char* who, const double* verts, const int32_t* offs, int32_t nrings, int32_t nverts) {
  const int rc = roi_counts_ok(who, verts, offs, nrings, nverts);
  if (rc != HSR_OK) return rc;
  HSR_REQUIRE(offs[0] == 0 && offs[nrings] == nverts, HSR_ERR_INVALID, "%s: ring_offsets run from %d to %d, not from 0 to nverts=%d", who,
              offs[0], offs[nrings], nverts);
  for (int k = 0; k < nrings; ++k)
    HSR_REQUIRE((int64_t)offs[k + 1] - offs[k] >= 3, HSR_ERR_INVALID, "%s: ring %d has %lld vertices: a ring has at least 3 vertices", who, k,
                (long long)offs[k + 1] - offs[k]);
  for (int i = 0; i < 2 * nverts; ++i)
    HSR_REQUIRE(roi_finite(verts[i]), HSR_ERR_INVALID, "%s: vertex %d has a non-finite coordinate", who, i / 2);
  return HSR_OK;
}

static int roi_grid_ok(const char* who, const double* gt, int32_t H, int32_t W, int32_t rule, int32_t row_off, int32_t col_off, int32_t h,
                       int32_t w) {
  HSR_REQUIRE(gt, HSR_ERR_INVALID, "%s: NULL geotransform", who);
  for (int i = 0; i < 6; ++i) HSR_REQUIRE(roi_finite(gt[i]), HSR_ERR_INVALID, "%s: geotransform term %d is not finite", who, i);
  HSR_REQUIRE(gt[2] == 0.0 && gt[4] == 0.0, HSR_ERR_UNSUPPORTED, "%s: a geotransform with rotation terms (%g, %g)", who, gt[2], gt[4]);
  HSR_REQUIRE(gt[1] != 0.0 && gt[5] != 0.0, HSR_ERR_INVALID, "%s: a pixel size of 0 (dx=%g, dy=%g)", who, gt[1], gt[5]);
  HSR_REQUIRE(H >= 1 && W >= 1 && h >= 1 && w >= 1, HSR_ERR_INVALID, "%s: an extent < 1 (grid %d x %d, window %d x %d)", who, H, W, h, w);
  HSR_REQUIRE(H <= kRoiMaxExtent && W <= kRoiMaxExtent, HSR_ERR_UNSUPPORTED, "%s: a grid of %d x %d cells, more than 2^30 a side", who, H, W);
  HSR_REQUIRE(row_off >= 0 && col_off >= 0 && (int64_t)row_off + h <= H && (int64_t)col_off + w <= W, HSR_ERR_INVALID,
              "%s: the window (%d, %d, %d, %d) leaves the %d x %d grid", who, row_off, col_off, h, w, H, W);
  HSR_REQUIRE(rule == HSR_ROI_CENTER || rule == HSR_ROI_TOUCHED, HSR_ERR_INVALID, "%s: rule=%d outside {0,1}", who, rule);
  const int64_t tiles = (int64_t)((w + kRoiTW - 1) / kRoiTW) * ((h + kRoiTH - 1) / kRoiTH);
  HSR_REQUIRE(tiles <= INT_MAX, HSR_ERR_UNSUPPORTED, "%s: %lld tiles of %d x %d, more than 2^31 - 1", who, (long long)tiles, kRoiTH, kRoiTW);
  return HSR_OK;
}

static RoiArgs roi_args(const double* verts, const int32_t* offs, int32_t nrings, int32_t nverts, const double* gt, int32_t row_off,
                        int32_t col_off, int32_t h, int32_t w) {
  RoiArgs a{};
  a.p = RoiPoly{verts, offs, nrings, nverts, gt[0], gt[1], gt[3], gt[5], 0};
  while (a.p.share < 5 && ((int64_t)nverts << (a.p.share + 1)) <= kRoiThreads) ++a.p.share;
  a.row_off = row_off; a.col_off = col_off; a.h = h; a.w = w;
  a.tiles_x = (w + kRoiTW - 1) / kRoiTW;
  return a;
}

static unsigned roi_tiles(const RoiArgs& a) { return (unsigned)(a.tiles_x * ((a.h + kRoiTH - 1) / kRoiTH)); }

static bool roi_overlap(const void* p, int64_t pn, const void* q, int64_t qn) {
  const uintptr_t pb = (uintptr_t)p, qb = (uintptr_t)q;
  return !(pb + (uintptr_t)pn <= qb || qb + (uintptr_t)qn <= pb);
}

// The inside (touched) flags of the w cells of grid row r from column c0: every edge once, the element functions of the kernels.
static void roi_row_host(const RoiPoly& p, int rule, int r, int c0, int w, std::vector<uint8_t>& flip, std::vector<int32_t>& diff,
                         uint8_t* inside) {
  flip.assign((size_t)w + 1, 0);
  diff.assign((size_t)w + 1, 0);
  for (int e = 0; e < p.nverts; ++e) {
    double ua, va, ub, vb, xc, flo, fhi;
    if (!roi_edge(p, e, ua, va, ub, vb)) continue;
    if (roi_crossing(ua, va, ub, vb, (double)r + 0.5, xc)) flip[(size_t)(roi_cross_count(xc, c0, c0 + w) - c0)] ^= 1;
    if (rule == HSR_ROI_TOUCHED && roi_touch_span(ua, va, ub, vb, (double)r, flo, fhi)) {
      const int cl = roi_clamp_int(flo, c0, c0 + w) - c0, ch = roi_clamp_int(fhi, c0 - 1, c0 + w - 1) - c0;
      if (cl <= ch) {
        diff[(size_t)cl] += 1;
        diff[(size_t)ch + 1] -= 1;
      }
    }
  }
  uint8_t par = 0;
  for (int c = w - 1; c >= 0; --c) {
    par ^= flip[(size_t)c + 1];
    inside[c] = par;
  }
  int32_t run = 0;
  for (int c = 0; c < w; ++c) {
    run += diff[(size_t)c];
    inside[c] |= run > 0 ? 1 : 0;
  }
}

}  // namespace hsr

using namespace hsr;

extern "C" int hsr_roi_check_host(const double* verts, const int32_t* ring_offsets, int32_t nrings, int32_t nverts) {
  return roi_contents_ok("hsr_roi_check_host", verts, ring_offsets, nrings, nverts);
}

extern "C" int hsr_roi_rasterize(const double* verts_dev, const int32_t* ring_offsets_dev, int32_t nrings, int32_t nverts, const double* gt,
                                 int32_t H, int32_t W, int32_t rule, int32_t row_off, int32_t col_off, int32_t h, int32_t w,
                                 uint8_t inside_value, uint8_t outside_value, uint8_t* out_dev, int64_t out_rs, hsr_stream_t stream) {
  int rc = roi_counts_ok("hsr_roi_rasterize", verts_dev, ring_offsets_dev, nrings, nverts);
  if (rc != HSR_OK) return rc;
  rc = roi_grid_ok("hsr_roi_rasterize", gt, H, W, rule, row_off, col_off, h, w);
  if (rc != HSR_OK) return rc;
  HSR_REQUIRE(out_dev, HSR_ERR_INVALID, "hsr_roi_rasterize: NULL output");
  HSR_REQUIRE(out_rs >= w, HSR_ERR_INVALID, "hsr_roi_rasterize: a row stride %lld below w=%d", (long long)out_rs, w);
  RoiArgs a = roi_args(verts_dev, ring_offsets_dev, nrings, nverts, gt, row_off, col_off, h, w);
  a.in_v = inside_value; a.out_v = outside_value; a.out = out_dev; a.ors = out_rs;
  hipStream_t s = (hipStream_t)stream;
  if (rule == HSR_ROI_TOUCHED) hipLaunchKernelGGL((roi_raster_kernel<HSR_ROI_TOUCHED>), dim3(roi_tiles(a)), dim3(kRoiThreads), 0, s, a);
  else hipLaunchKernelGGL((roi_raster_kernel<HSR_ROI_CENTER>), dim3(roi_tiles(a)), dim3(kRoiThreads), 0, s, a);
  return launched(kLaunchRoi, "roi_raster_kernel launch", kRoiRaster + rule);
}

extern "C" int hsr_roi_rasterize_host(const double* verts, const int32_t* ring_offsets, int32_t nrings, int32_t nverts, const double* gt,
                                      int32_t H, int32_t W, int32_t rule, int32_t row_off, int32_t col_off, int32_t h, int32_t w,
                                      uint8_t inside_value, uint8_t outside_value, uint8_t* out, int64_t out_rs) {
  int rc = roi_contents_ok("hsr_roi_rasterize_host", verts, ring_offsets, nrings, nverts);
  if (rc != HSR_OK) return rc;
  rc = roi_grid_ok("hsr_roi_rasterize_host", gt, H, W, rule, row_off, col_off, h, w);
  if (rc != HSR_OK) return rc;
  HSR_REQUIRE(out, HSR_ERR_INVALID, "hsr_roi_rasterize_host: NULL output");
  HSR_REQUIRE(out_rs >= w, HSR_ERR_INVALID, "hsr_roi_rasterize_host: a row stride %lld below w=%d", (long long)out_rs, w);
  const RoiArgs a = roi_args(verts, ring_offsets, nrings, nverts, gt, row_off, col_off, h, w);
  std::vector<uint8_t> flip, row((size_t)w);
  std::vector<int32_t> diff;
  for (int r = 0; r < h; ++r) {
    roi_row_host(a.p, rule, row_off + r, col_off, w, flip, diff, row.data());
    uint8_t* o = out + (int64_t)r * out_rs;
    for (int c = 0; c < w; ++c) o[c] = row[(size_t)c] ? inside_value : outside_value;
  }
  return HSR_OK;
}

extern "C" int hsr_roi_class_counts(const double* verts_dev, const int32_t* ring_offsets_dev, int32_t nrings, int32_t nverts,
                                    const double* gt, int32_t H, int32_t W, int32_t rule, int32_t row_off, int32_t col_off, int32_t h,
                                    int32_t w, const uint8_t* plane_dev, int64_t rs, int32_t* counts_dev, int32_t* inside_dev,
                                    hsr_stream_t stream) {
  int rc = roi_counts_ok("hsr_roi_class_counts", verts_dev, ring_offsets_dev, nrings, nverts);
  if (rc != HSR_OK) return rc;
  rc = roi_grid_ok("hsr_roi_class_counts", gt, H, W, rule, row_off, col_off, h, w);
  if (rc != HSR_OK) return rc;
  HSR_REQUIRE(plane_dev && counts_dev && inside_dev, HSR_ERR_INVALID, "hsr_roi_class_counts: NULL pointer");
  HSR_REQUIRE(rs >= W, HSR_ERR_INVALID, "hsr_roi_class_counts: a row stride %lld below W=%d", (long long)rs, W);
  HSR_REQUIRE((int64_t)h * w <= INT_MAX, HSR_ERR_INVALID, "hsr_roi_class_counts: a window of %lld cells, more than 2^31 - 1", (long long)h * w);
  hipStream_t s = (hipStream_t)stream;
  rc = check_hip(hipMemsetAsync(counts_dev, 0, HSR_SCL_BINS * sizeof(int32_t), s), "hsr_roi_class_counts: clearing the counts");
  if (rc != HSR_OK) return rc;
  rc = check_hip(hipMemsetAsync(inside_dev, 0, sizeof(int32_t), s), "hsr_roi_class_counts: clearing the inside count");
  if (rc != HSR_OK) return rc;
  RoiArgs a = roi_args(verts_dev, ring_offsets_dev, nrings, nverts, gt, row_off, col_off, h, w);
  a.plane = plane_dev + (int64_t)row_off * rs + col_off; a.prs = rs; a.counts = counts_dev; a.inside = inside_dev;
  if (rule == HSR_ROI_TOUCHED) hipLaunchKernelGGL((roi_counts_kernel<HSR_ROI_TOUCHED>), dim3(roi_tiles(a)), dim3(kRoiThreads), 0, s, a);
  else hipLaunchKernelGGL((roi_counts_kernel<HSR_ROI_CENTER>), dim3(roi_tiles(a)), dim3(kRoiThreads), 0, s, a);
  return launched(kLaunchRoi, "roi_counts_kernel launch", kRoiCounts + rule);
}

static int roi_clip_ok(const char* who, const int32_t* glt, int32_t H, int32_t W, int32_t h, int32_t w, const int32_t* out_glt,
                       const int32_t* record) {
  HSR_REQUIRE(glt && out_glt && record, HSR_ERR_INVALID, "%s: NULL pointer", who);
  HSR_REQUIRE(!roi_overlap(glt, (int64_t)H * W * 8, out_glt, (int64_t)h * w * 8), HSR_ERR_INVALID, "%s: the output overlaps the table", who);
  return HSR_OK;
}

extern "C" int hsr_roi_glt_clip(const double* verts_dev, const int32_t* ring_offsets_dev, int32_t nrings, int32_t nverts, const double* gt,
                                int32_t H, int32_t W, const int32_t* glt_dev, int32_t row_off, int32_t col_off, int32_t h, int32_t w,
                                int32_t* out_glt_dev, int32_t* record_dev, hsr_stream_t stream) {
  int rc = roi_counts_ok("hsr_roi_glt_clip", verts_dev, ring_offsets_dev, nrings, nverts);
  if (rc != HSR_OK) return rc;
  rc = roi_grid_ok("hsr_roi_glt_clip", gt, H, W, HSR_ROI_TOUCHED, row_off, col_off, h, w);
  if (rc != HSR_OK) return rc;
  rc = roi_clip_ok("hsr_roi_glt_clip", glt_dev, H, W, h, w, out_glt_dev, record_dev);
  if (rc != HSR_OK) return rc;
  HSR_REQUIRE((((uintptr_t)glt_dev | (uintptr_t)out_glt_dev) & 7) == 0, HSR_ERR_INVALID, "hsr_roi_glt_clip: a table that is not 8-byte aligned");
  RoiArgs a = roi_args(verts_dev, ring_offsets_dev, nrings, nverts, gt, row_off, col_off, h, w);
  a.glt = glt_dev; a.W = W; a.oglt = out_glt_dev; a.rec = record_dev;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(roi_record_init_kernel, dim3(1), dim3(64), 0, s, record_dev);
  hipLaunchKernelGGL(roi_glt_clip_kernel, dim3(roi_tiles(a)), dim3(kRoiThreads), 0, s, a);
  return launched(kLaunchRoi, "roi_glt_clip_kernel launch", kRoiRecordInit, kRoiGltClip);
}

extern "C" int hsr_roi_glt_clip_host(const double* verts, const int32_t* ring_offsets, int32_t nrings, int32_t nverts, const double* gt,
                                     int32_t H, int32_t W, const int32_t* glt, int32_t row_off, int32_t col_off, int32_t h, int32_t w,
                                     int32_t* out_glt, int32_t* record) {
  int rc = roi_contents_ok("hsr_roi_glt_clip_host", verts, ring_offsets, nrings, nverts);
  if (rc != HSR_OK) return rc;
  rc = roi_grid_ok("hsr_roi_glt_clip_host", gt, H, W, HSR_ROI_TOUCHED, row_off, col_off, h, w);
  if (rc != HSR_OK) return rc;
  rc = roi_clip_ok("hsr_roi_glt_clip_host", glt, H, W, h, w, out_glt, record);
  if (rc != HSR_OK) return rc;
  const RoiArgs a = roi_args(verts, ring_offsets, nrings, nverts, gt, row_off, col_off, h, w);
  std::vector<uint8_t> flip, row((size_t)w);
  std::vector<int32_t> diff;
  int64_t ylo = INT_MAX, yhi = 0, xlo = INT_MAX, xhi = 0, n = 0;   // one-based: 0 = none
  for (int r = 0; r < h; ++r) {
    roi_row_host(a.p, HSR_ROI_TOUCHED, row_off + r, col_off, w, flip, diff, row.data());
    const int32_t* in = glt + ((int64_t)(row_off + r) * W + col_off) * 2;
    int32_t* o = out_glt + (int64_t)r * w * 2;
    for (int c = 0; c < w; ++c) {
      int32_t gx = 0, gy = 0;
      if (row[(size_t)c]) {
        gx = in[2 * c]; gy = in[2 * c + 1];
        if (gx > 0) { xlo = gx < xlo ? gx : xlo; xhi = gx > xhi ? gx : xhi; }
        if (gy > 0) { ylo = gy < ylo ? gy : ylo; yhi = gy > yhi ? gy : yhi; }
        n += gx > 0 && gy > 0 ? 1 : 0;
      }
      o[2 * c] = gx; o[2 * c + 1] = gy;
    }
  }
  for (int i = 0; i < HSR_ROI_RECORD; ++i) record[i] = 0;
  record[0] = yhi > 0 ? (int32_t)(ylo - 1) : INT_MAX; record[1] = (int32_t)(yhi - 1);
  record[2] = xhi > 0 ? (int32_t)(xlo - 1) : INT_MAX; record[3] = (int32_t)(xhi - 1);
  record[4] = (int32_t)n;
  return HSR_OK;
}

static int roi_reindex_ok(const char* who, const int32_t* glt, int32_t h, int32_t w, const int32_t* record) {
  HSR_REQUIRE(glt && record, HSR_ERR_INVALID, "%s: NULL pointer", who);
  HSR_REQUIRE(h >= 1 && w >= 1, HSR_ERR_INVALID, "%s: an extent < 1 (%d x %d)", who, h, w);
  HSR_REQUIRE((int64_t)h * w <= INT_MAX, HSR_ERR_INVALID, "%s: %lld cells, more than 2^31 - 1", who, (long long)h * w);
  return HSR_OK;
}

extern "C" int hsr_roi_glt_reindex(int32_t* glt_dev, int32_t h, int32_t w, const int32_t* record_dev, hsr_stream_t stream) {
  const int rc = roi_reindex_ok("hsr_roi_glt_reindex", glt_dev, h, w, record_dev);
  if (rc != HSR_OK) return rc;
  HSR_REQUIRE(((uintptr_t)glt_dev & 7) == 0, HSR_ERR_INVALID, "hsr_roi_glt_reindex: a table that is not 8-byte aligned");
  const int64_t n = (int64_t)h * w, blocks = (n + kRoiThreads - 1) / kRoiThreads;
  hipLaunchKernelGGL(roi_glt_reindex_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kRoiThreads), 0, (hipStream_t)stream, glt_dev,
                     n, record_dev);
  return launched(kLaunchRoi, "roi_glt_reindex_kernel launch", kRoiGltReindex);
}

extern "C" int hsr_roi_glt_reindex_host(int32_t* glt, int32_t h, int32_t w, const int32_t* record) {
  const int rc = roi_reindex_ok("hsr_roi_glt_reindex_host", glt, h, w, record);
  if (rc != HSR_OK) return rc;
  for (int64_t i = 0; i < (int64_t)h * w; ++i) {
    glt[2 * i] = roi_reindex(glt[2 * i], record[2]);
    glt[2 * i + 1] = roi_reindex(glt[2 * i + 1], record[0]);
  }
  return HSR_OK;
}
