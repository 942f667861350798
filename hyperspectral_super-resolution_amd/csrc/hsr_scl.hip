// The Sentinel-2 scene classification layer on gfx950 (C ABI and the definitions: include/hsr_scl.h): class histograms per window,
// the buffered class mask with its host twin, the mask on the EMIT grid, the byte tile gather and the blanking of a cube.
//
// Reference: s2_data/cloud_utils.py:33-53 (count_cloud_pixels) and :82-101 (scl_metrics) read the SCL to choose a granule; the
// histogram gives their counts, everything else is the header's.  Structure:
//   counts   a workgroup of four waves per window and row chunk, a wave per row: 16-byte loads between the row's first and last
//            16-byte boundary, single bytes outside; the 13 bins of a thread are registers (13 compare-and-adds a byte: no
//            dependent LDS round trip, no atomics); a wave sum per bin, the four waves' sums joined in LDS and one integer atomic
//            per non-zero bin when the workgroup leaves the window.
//   mask     a 64 x 32 output tile per workgroup.  The staged box (tile + halo r, at most 128 x 96) is kept as bits: a wave's
//            ballot over 64 columns IS the row of flags, so a staged row is two 64-bit words.  rowdist of a pixel is two bit scans
//            of its row; the vertical pass reads one byte per dy, and skips rows that hold no flag.  No flag in the whole box: the
//            workgroup writes the flat classes and leaves.  The same tile code, written sequentially, is the host twin.
//   coarse   a thread per EMIT cell; the window sums are aggregated per wave (ballot + popcount) before the integer atomic.
//   gather   a thread per byte.
//   apply    a thread per four pixels of a row: their mask bytes once, then per band one 16-byte store where all four lie under the
//            mask and the address allows it, single stores for the others - or none.
#include <limits.h>

#include "hsr_common.h"
#include "../../include/hsr_scl.h"

namespace hsr {

constexpr int kSclClasses = 13;                      // bins in use: 0 .. 11 and "other"
constexpr int kSclThreads = 256, kSclWaves = kSclThreads / 64;
constexpr int kMaskTW = 64, kMaskTH = 32;            // the output tile of a workgroup
constexpr int kMaskSH = kMaskTH + 2 * HSR_SCL_MAX_RADIUS;   // staged rows, at most
constexpr int kLookupBytes = 16;                     // bytes of a thread of the lookup instance

__device__ __forceinline__ unsigned scl_wave_sum(unsigned v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------------------------------------
// class counts
// ------------------------------------------------------------------------------------------------------------------------------
// bins[v < 12 ? v : 12] += 1 on bins that are registers: every index is a constant
__device__ __forceinline__ void count_class(unsigned (&bins)[kSclClasses], unsigned v) {
#pragma unroll
  for (int b = 0; b < kSclClasses - 1; ++b) bins[b] += v == (unsigned)b ? 1u : 0u;
  bins[kSclClasses - 1] += v >= (unsigned)(kSclClasses - 1) ? 1u : 0u;
}

__global__ __launch_bounds__(kSclThreads) void scl_counts_kernel(const uint8_t* __restrict__ scl, int64_t rs, int tile_h, int tile_w,
                                                                  int nx, int32_t* __restrict__ counts) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned bins[kSclClasses];
#pragma unroll
  for (int b = 0; b < kSclClasses; ++b) bins[b] = 0;
  const int win = (int)blockIdx.x, wy = win / nx, wx = win - wy * nx;
  const uint8_t* base = scl + (int64_t)wy * tile_h * rs + (int64_t)wx * tile_w;
  for (int r = (int)blockIdx.y * kSclWaves + wave; r < tile_h; r += (int)gridDim.y * kSclWaves) {
    const uint8_t* row = base + (int64_t)r * rs;
    int head = (int)((16 - ((uintptr_t)row & 15)) & 15);
    head = head > tile_w ? tile_w : head;
    const int nv = (tile_w - head) >> 4, tail0 = head + (nv << 4);
    const uint4* vp = reinterpret_cast<const uint4*>(row + head);
    for (int i = lane; i < nv; i += 64) {
      const uint4 q = vp[i];
      const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          count_class(bins, (w[k] >> (8 * j)) & 0xffu);
        }
    }
    const int edge = head + (tile_w - tail0);          // the bytes before the first and after the last boundary: at most 30
    if (lane < edge) {
      count_class(bins, row[lane < head ? lane : tail0 + (lane - head)]);
    }
  }
  __shared__ unsigned part[kSclWaves][kSclClasses];
#pragma unroll
  for (int b = 0; b < kSclClasses; ++b) {
    const unsigned s = scl_wave_sum(bins[b]);
    if (lane == 0) part[wave][b] = s;
  }
  __syncthreads();
  if (tid < kSclClasses) {                             // atomics on one address serialise: one per bin and workgroup, not per wave
    unsigned s = 0;
#pragma unroll
    for (int w = 0; w < kSclWaves; ++w) s += part[w][tid];
    if (s) atomicAdd(&counts[(int64_t)win * HSR_SCL_BINS + tid], (int)s);
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// the mask (one definition of the class test, of rowdist and of the half widths for the kernel and the host twin)
// ------------------------------------------------------------------------------------------------------------------------------
struct MaskArgs {
  const uint8_t* scl;
  int H, W;
  int64_t rs;
  uint32_t grow, flat;
  int r;
  uint8_t* mask;
  int64_t mrs;
  int tiles_x;
  int vec;                                           // lookup: both bases and both strides are multiples of 16
  uint8_t hw[HSR_SCL_MAX_RADIUS + 1];                // hw[d], d = |dy| = 0 .. r
};

__host__ __device__ inline unsigned class_bit(uint32_t set, unsigned v) { return v < 32u ? (set >> v) & 1u : 0u; }

// The distance from column c (0 .. 127) of a staged row - lo holds the columns 0 .. 63, hi 64 .. 127 - to its nearest set flag, at most cap.
__host__ __device__ inline int row_dist(uint64_t lo, uint64_t hi, int c, int cap) {
  uint64_t rlo, rhi;                                 // the columns >= c, column c at bit 0
  if (c == 0) { rlo = lo; rhi = hi; }
  else if (c < 64) { rlo = (lo >> c) | (hi << (64 - c)); rhi = hi >> c; }
  else { rlo = hi >> (c - 64); rhi = 0; }
  int d = cap;
  if (rlo) { const int t = __builtin_ctzll(rlo); d = t < d ? t : d; }
  else if (rhi) { const int t = 64 + __builtin_ctzll(rhi); d = t < d ? t : d; }
  const int s = 127 - c;                             // the columns <= c, column c at bit 127
  uint64_t llo, lhi;
  if (s == 0) { llo = lo; lhi = hi; }
  else if (s < 64) { lhi = (hi << s) | (lo >> (64 - s)); llo = lo << s; }
  else { lhi = lo << (s - 64); llo = 0; }
  if (lhi) { const int t = __builtin_clzll(lhi); d = t < d ? t : d; }
  else if (llo) { const int t = 64 + __builtin_clzll(llo); d = t < d ? t : d; }
  return d;
}

// hw(d) = floor(sqrt(r^2 - d^2)) in integers (disc), r (square).
static void half_widths(int r, int shape, uint8_t* hw) {
  for (int d = 0; d <= r; ++d) {
    int w = r;
    if (shape == HSR_SCL_DISC)
      while (w * w + d * d > r * r) --w;
    hw[d] = (uint8_t)w;
  }
}

enum MaskMode : int { kMaskLookup = 0, kMaskDisc = 1, kMaskSquare = 2 };

template <int MODE>
__global__ __launch_bounds__(kSclThreads) void scl_mask_kernel(const MaskArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if constexpr (MODE == kMaskLookup) {
    const uint32_t set = a.grow | a.flat;
    const int64_t x = ((int64_t)blockIdx.x * kSclThreads + tid) * kLookupBytes;
    if (x >= a.W) return;
    for (int y = (int)blockIdx.y; y < a.H; y += (int)gridDim.y) {
      const uint8_t* in = a.scl + (int64_t)y * a.rs + x;
      uint8_t* out = a.mask + (int64_t)y * a.mrs + x;
      if (a.vec && x + kLookupBytes <= a.W) {
        const uint4 q = *reinterpret_cast<const uint4*>(in);
        unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          unsigned m = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) m |= class_bit(set, (w[k] >> (8 * j)) & 0xffu) << (8 * j);
          w[k] = m;
        }
        *reinterpret_cast<uint4*>(out) = make_uint4(w[0], w[1], w[2], w[3]);
      } else {
        const int n = a.W - x < kLookupBytes ? (int)(a.W - x) : kLookupBytes;
        for (int j = 0; j < n; ++j) out[j] = (uint8_t)class_bit(set, in[j]);
      }
    }
  } else {
    __shared__ uint64_t gbits[kMaskSH][2];           // the grow flags of the staged box, a bit a pixel
    __shared__ uint64_t fbits[kMaskTH];              // the flat flags of the tile
    __shared__ uint8_t dist[kMaskSH][kMaskTW];       // rowdist of the tile's columns
    const int tile_y = (int)blockIdx.x / a.tiles_x, tile_x = (int)blockIdx.x - tile_y * a.tiles_x;
    const int x0 = tile_x * kMaskTW, y0 = tile_y * kMaskTH, r = a.r, sh = kMaskTH + 2 * r, sw = kMaskTW + 2 * r;
    int any = 0;
    for (int sr = wave; sr < sh; sr += kSclWaves) {
      const int gy = y0 - r + sr;
      uint64_t b0 = 0, b1 = 0, f = 0;
      if (gy >= 0 && gy < a.H) {                     // uniform over the wave
        const uint8_t* row = a.scl + (int64_t)gy * a.rs;
        const int gx0 = x0 - r + lane, gx1 = gx0 + 64;
        const unsigned v0 = gx0 >= 0 && gx0 < a.W ? row[gx0] : 255u;          // outside the plane: in neither set
        const unsigned v1 = lane + 64 < sw && gx1 >= 0 && gx1 < a.W ? row[gx1] : 255u;
        b0 = __ballot(class_bit(a.grow, v0));
        b1 = __ballot(class_bit(a.grow, v1));
        if (sr >= r && sr < r + kMaskTH) {
          const unsigned vc = x0 + lane < a.W ? row[x0 + lane] : 255u;
          f = __ballot(class_bit(a.flat, vc));
        }
      }
      if (lane == 0) {
        gbits[sr][0] = b0;
        gbits[sr][1] = b1;
        if (sr >= r && sr < r + kMaskTH) fbits[sr - r] = f;
      }
      any |= (b0 | b1) != 0;
    }
    const int some = __syncthreads_or(any);           // also publishes gbits and fbits
    if (some) {
      for (int sr = wave; sr < sh; sr += kSclWaves) {
        const uint64_t lo = gbits[sr][0], hi = gbits[sr][1];
        if (lo | hi) dist[sr][lane] = (uint8_t)row_dist(lo, hi, lane + r, r + 1);
      }
      __syncthreads();
    }
    const int x = x0 + lane;
    for (int ly = wave; ly < kMaskTH; ly += kSclWaves) {
      const int y = y0 + ly;
      if (y >= a.H) break;
      unsigned m = (unsigned)(fbits[ly] >> lane) & 1u;
      if (some) {
        for (int dy = -r; dy <= r; ++dy) {
          const int sr = ly + r + dy;
          if (!(gbits[sr][0] | gbits[sr][1])) continue;                        // a row without a flag: uniform
          const int h = MODE == kMaskSquare ? r : (int)a.hw[dy < 0 ? -dy : dy];
          m |= (int)dist[sr][lane] <= h ? 1u : 0u;
        }
      }
      if (x < a.W) a.mask[(int64_t)y * a.mrs + x] = (uint8_t)m;
    }
  }
}

// The tile code of scl_mask_kernel for one tile, sequentially: the staged bit rows, rowdist, the vertical OR.
static void mask_tile_host(const MaskArgs& a, int shape, int x0, int y0) {
  static thread_local uint64_t gbits[kMaskSH][2];
  static thread_local uint8_t dist[kMaskSH][kMaskTW];
  const int r = a.r, sh = kMaskTH + 2 * r, sw = kMaskTW + 2 * r;
  for (int sr = 0; sr < sh; ++sr) {
    const int gy = y0 - r + sr;
    uint64_t b[2] = {0, 0};
    if (gy >= 0 && gy < a.H)
      for (int sc = 0; sc < sw; ++sc) {
        const int gx = x0 - r + sc;
        const unsigned v = gx >= 0 && gx < a.W ? a.scl[(int64_t)gy * a.rs + gx] : 255u;
        b[sc >> 6] |= (uint64_t)class_bit(a.grow, v) << (sc & 63);
      }
    gbits[sr][0] = b[0];
    gbits[sr][1] = b[1];
    for (int c = 0; c < kMaskTW; ++c) dist[sr][c] = (uint8_t)row_dist(b[0], b[1], c + r, r + 1);
  }
  for (int ly = 0; ly < kMaskTH && y0 + ly < a.H; ++ly)
    for (int c = 0; c < kMaskTW && x0 + c < a.W; ++c) {
      unsigned m = class_bit(a.flat, a.scl[(int64_t)(y0 + ly) * a.rs + x0 + c]);
      for (int dy = -r; dy <= r; ++dy) {
        const int h = shape == HSR_SCL_SQUARE ? r : (int)a.hw[dy < 0 ? -dy : dy];
        m |= (int)dist[ly + r + dy][c] <= h ? 1u : 0u;
      }
      a.mask[(int64_t)(y0 + ly) * a.mrs + x0 + c] = (uint8_t)m;
    }
}

static int mask_args_ok(const char* who, const uint8_t* scl, int32_t H, int32_t W, int64_t rs, int32_t r, int32_t shape,
                        const uint8_t* mask, int64_t mask_rs) {
  HSR_REQUIRE(scl && mask, HSR_ERR_INVALID, "%s: NULL pointer", who);
  HSR_REQUIRE(H >= 1 && W >= 1, HSR_ERR_INVALID, "%s: an extent < 1 (H=%d, W=%d)", who, H, W);
  HSR_REQUIRE(rs >= W && mask_rs >= W, HSR_ERR_INVALID, "%s: a row stride (%lld, %lld) below W=%d", who, (long long)rs,
              (long long)mask_rs, W);
  HSR_REQUIRE(r >= 0 && r <= HSR_SCL_MAX_RADIUS, HSR_ERR_INVALID, "%s: radius r=%d outside [0,%d]", who, r, HSR_SCL_MAX_RADIUS);
  HSR_REQUIRE(shape == HSR_SCL_DISC || shape == HSR_SCL_SQUARE, HSR_ERR_INVALID, "%s: shape=%d outside {0,1}", who, shape);
  const uintptr_t ib = (uintptr_t)scl, ob = (uintptr_t)mask;
  const uintptr_t ie = ib + (uintptr_t)((int64_t)(H - 1) * rs + W), oe = ob + (uintptr_t)((int64_t)(H - 1) * mask_rs + W);
  HSR_REQUIRE(oe <= ib || ie <= ob, HSR_ERR_INVALID, "%s: mask aliases the scl plane", who);
  const int64_t tiles = (int64_t)((W + kMaskTW - 1) / kMaskTW) * ((H + kMaskTH - 1) / kMaskTH);
  HSR_REQUIRE(tiles <= INT_MAX, HSR_ERR_UNSUPPORTED, "%s: %lld tiles of %d x %d, more than 2^31 - 1", who, (long long)tiles, kMaskTW,
              kMaskTH);
  return HSR_OK;
}

static MaskArgs mask_args(const uint8_t* scl, int32_t H, int32_t W, int64_t rs, uint32_t grow, uint32_t flat, int32_t r, int32_t shape,
                          uint8_t* mask, int64_t mask_rs) {
  MaskArgs a{};
  a.scl = scl; a.H = H; a.W = W; a.rs = rs; a.grow = grow; a.flat = flat; a.r = r; a.mask = mask; a.mrs = mask_rs;
  a.tiles_x = (W + kMaskTW - 1) / kMaskTW;
  a.vec = (((uintptr_t)scl | (uintptr_t)mask | (uintptr_t)rs | (uintptr_t)mask_rs) & 15) == 0;
  half_widths(r, shape, a.hw);
  return a;
}

// ------------------------------------------------------------------------------------------------------------------------------
// the mask on the EMIT grid
// ------------------------------------------------------------------------------------------------------------------------------
struct CoarseArgs {
  const uint8_t* mask;
  int64_t rs;
  int k, max_bad, hc, wc;
  uint8_t* clear;
  uint8_t* cell_bad;
  int ce_h, ce_w, nwy, nwx;
  int32_t* win;
};

__global__ __launch_bounds__(kSclThreads) void scl_coarse_kernel(const CoarseArgs a) {
  const int lane = threadIdx.x & 63;
  const int cx = (int)blockIdx.x * kSclThreads + (int)threadIdx.x;   // a whole wave stays in the loop: the ballots need every lane
  const bool live = cx < a.wc;
  const int wxi = a.win ? cx / a.ce_w : 0;
  for (int cy = (int)blockIdx.y; cy < a.hc; cy += (int)gridDim.y) {
    int n = 0;
    if (live) {
      const uint8_t* p = a.mask + (int64_t)cy * a.k * a.rs + (int64_t)cx * a.k;
      for (int i = 0; i < a.k; ++i, p += a.rs)
        for (int j = 0; j < a.k; ++j) n += p[j] != 0;
      const int64_t at = (int64_t)cy * a.wc + cx;
      a.clear[at] = n <= a.max_bad ? 1 : 0;
      if (a.cell_bad) a.cell_bad[at] = (uint8_t)(n < 255 ? n : 255);
    }
    if (a.win) {
      const int wy = cy / a.ce_h;
      const bool cnt = live && n > a.max_bad && wy < a.nwy && wxi < a.nwx;
      uint64_t pend = __ballot(cnt);
      while (pend) {                                               // uniform: one round per window the wave touches
        const int leader = __builtin_ctzll(pend);
        const int w = __shfl(wxi, leader, 64);
        const uint64_t same = __ballot(cnt && wxi == w);
        if (lane == leader) atomicAdd(&a.win[(int64_t)wy * a.nwx + w], (int)__popcll(same));
        pend &= ~same;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// the byte gather and the blanking
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSclThreads) void scl_gather_kernel(const uint8_t* __restrict__ plane, int H, int W, int64_t rs,
                                                                  const int32_t* __restrict__ origins, int th, int tw,
                                                                  uint8_t* __restrict__ out) {
  const int tile = (int)blockIdx.x;
  const int64_t oy = origins[2 * (int64_t)tile], ox = origins[2 * (int64_t)tile + 1];
  if (oy < 0 || ox < 0 || oy + th > H || ox + tw > W) return;      // a window that leaves the plane: skipped, never dereferenced
  const int64_t n = (int64_t)th * tw;
  uint8_t* o = out + (int64_t)tile * n;
  for (int64_t e = (int64_t)blockIdx.y * kSclThreads + threadIdx.x; e < n; e += (int64_t)gridDim.y * kSclThreads) {
    const int64_t r = e / tw, c = e - r * tw;
    o[e] = plane[(oy + r) * rs + ox + c];
  }
}

struct ApplyArgs {
  float* cube;
  int T, H, W;
  int64_t bs, rs;
  const uint8_t* mask;
  int64_t mrs;
  float fill;
  unsigned long long* count;
  int vec;                                           // the cube's base and both strides are multiples of four elements
};

template <int UP>
__global__ __launch_bounds__(kSclThreads) void scl_apply_kernel(const ApplyArgs a) {
  const int64_t x = ((int64_t)blockIdx.x * kSclThreads + threadIdx.x) * 4;
  unsigned n = 0;
  if (x < a.W) {
    const int px = a.W - x < 4 ? (int)(a.W - x) : 4;
    for (int y = (int)blockIdx.y; y < a.H; y += (int)gridDim.y) {
      const uint8_t* m = a.mask + (int64_t)(y / UP) * a.mrs;
      unsigned hit = 0;
      for (int j = 0; j < px; ++j) hit |= (m[(x + j) / UP] != 0 ? 1u : 0u) << j;
      if (!hit) continue;
      n += __popc(hit);
      float* p = a.cube + (int64_t)y * a.rs + x;
      if (hit == 0xfu && a.vec) {
        const float4 f = make_float4(a.fill, a.fill, a.fill, a.fill);
        for (int t = 0; t < a.T; ++t, p += a.bs) *reinterpret_cast<float4*>(p) = f;
      } else {
        for (int t = 0; t < a.T; ++t, p += a.bs)
          for (int j = 0; j < px; ++j)
            if ((hit >> j) & 1u) p[j] = a.fill;
      }
    }
  }
  if (a.count) {
    n = scl_wave_sum(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(a.count, (unsigned long long)n);
  }
}

}  // namespace hsr

using namespace hsr;

extern "C" int hsr_scl_class_counts(const uint8_t* scl_dev, int32_t H, int32_t W, int64_t rs, int32_t tile_h, int32_t tile_w,
                                    int32_t* counts_dev, hsr_stream_t stream) {
  HSR_REQUIRE(scl_dev && counts_dev, HSR_ERR_INVALID, "hsr_scl_class_counts: NULL pointer");
  HSR_REQUIRE(H >= 1 && W >= 1 && tile_h >= 1 && tile_w >= 1, HSR_ERR_INVALID,
              "hsr_scl_class_counts: an extent < 1 (H=%d, W=%d, tile %d x %d)", H, W, tile_h, tile_w);
  HSR_REQUIRE(tile_h <= H && tile_w <= W, HSR_ERR_INVALID, "hsr_scl_class_counts: a tile of %d x %d is larger than the %d x %d plane",
              tile_h, tile_w, H, W);
  HSR_REQUIRE(rs >= W, HSR_ERR_INVALID, "hsr_scl_class_counts: a row stride %lld below W=%d", (long long)rs, W);
  HSR_REQUIRE((int64_t)tile_h * tile_w <= INT_MAX, HSR_ERR_INVALID, "hsr_scl_class_counts: a window of %lld pixels, more than 2^31 - 1",
              (long long)tile_h * tile_w);
  const int ny = H / tile_h, nx = W / tile_w;
  const int64_t nwin = (int64_t)ny * nx;
  HSR_REQUIRE(nwin <= INT_MAX / HSR_SCL_BINS, HSR_ERR_UNSUPPORTED, "hsr_scl_class_counts: %lld windows", (long long)nwin);
  hipStream_t s = (hipStream_t)stream;
  const int rc = check_hip(hipMemsetAsync(counts_dev, 0, (size_t)nwin * HSR_SCL_BINS * sizeof(int32_t), s),
                           "hsr_scl_class_counts: clearing the counts");
  if (rc != HSR_OK) return rc;
  int64_t gy = 1024 / nwin;                            // about 1024 workgroups (their atomics meet on 13 addresses), each wave at least one row
  const int64_t chunks = ((int64_t)tile_h + kSclWaves - 1) / kSclWaves;
  gy = gy < 1 ? 1 : (gy > chunks ? chunks : gy);
  hipLaunchKernelGGL(scl_counts_kernel, dim3((unsigned)nwin, (unsigned)gy), dim3(kSclThreads), 0, s, scl_dev, rs, tile_h, tile_w, nx,
                     counts_dev);
  return launched(kLaunchScl, "scl_counts_kernel launch", kSclCounts);
}

extern "C" int hsr_scl_mask(const uint8_t* scl_dev, int32_t H, int32_t W, int64_t rs, uint32_t grow_bits, uint32_t flat_bits, int32_t r,
                            int32_t shape, uint8_t* mask_dev, int64_t mask_rs, hsr_stream_t stream) {
  const int rc = mask_args_ok("hsr_scl_mask", scl_dev, H, W, rs, r, shape, mask_dev, mask_rs);
  if (rc != HSR_OK) return rc;
  const MaskArgs a = mask_args(scl_dev, H, W, rs, grow_bits, flat_bits, r, shape, mask_dev, mask_rs);
  hipStream_t s = (hipStream_t)stream;
  if (r == 0) {
    const int64_t per_row = ((int64_t)W + kLookupBytes - 1) / kLookupBytes;
    const dim3 grid((unsigned)((per_row + kSclThreads - 1) / kSclThreads), (unsigned)(H < 65535 ? H : 65535));
    hipLaunchKernelGGL((scl_mask_kernel<kMaskLookup>), grid, dim3(kSclThreads), 0, s, a);
    return launched(kLaunchScl, "scl_mask_kernel launch", kSclMask + kMaskLookup);
  }
  const dim3 grid((unsigned)(a.tiles_x * ((H + kMaskTH - 1) / kMaskTH)));
  if (shape == HSR_SCL_SQUARE) hipLaunchKernelGGL((scl_mask_kernel<kMaskSquare>), grid, dim3(kSclThreads), 0, s, a);
  else hipLaunchKernelGGL((scl_mask_kernel<kMaskDisc>), grid, dim3(kSclThreads), 0, s, a);
  return launched(kLaunchScl, "scl_mask_kernel launch", kSclMask + (shape == HSR_SCL_SQUARE ? kMaskSquare : kMaskDisc));
}

extern "C" int hsr_scl_mask_host(const uint8_t* scl, int32_t H, int32_t W, int64_t rs, uint32_t grow_bits, uint32_t flat_bits, int32_t r,
                                 int32_t shape, uint8_t* mask, int64_t mask_rs) {
  const int rc = mask_args_ok("hsr_scl_mask_host", scl, H, W, rs, r, shape, mask, mask_rs);
  if (rc != HSR_OK) return rc;
  const MaskArgs a = mask_args(scl, H, W, rs, grow_bits, flat_bits, r, shape, mask, mask_rs);
  for (int y0 = 0; y0 < H; y0 += kMaskTH)
    for (int x0 = 0; x0 < W; x0 += kMaskTW) mask_tile_host(a, shape, x0, y0);
  return HSR_OK;
}

extern "C" int hsr_scl_coarse(const uint8_t* mask_dev, int32_t H, int32_t W, int64_t rs, int32_t k, int32_t max_bad, uint8_t* clear_dev,
                              uint8_t* cell_bad_dev, int32_t ce_h, int32_t ce_w, int32_t* win_counts_dev, hsr_stream_t stream) {
  HSR_REQUIRE(mask_dev && clear_dev, HSR_ERR_INVALID, "hsr_scl_coarse: NULL pointer");
  HSR_REQUIRE(H >= 1 && W >= 1, HSR_ERR_INVALID, "hsr_scl_coarse: an extent < 1 (H=%d, W=%d)", H, W);
  HSR_REQUIRE(rs >= W, HSR_ERR_INVALID, "hsr_scl_coarse: a row stride %lld below W=%d", (long long)rs, W);
  HSR_REQUIRE(k >= 1 && k <= HSR_SCL_MAX_K && k <= H && k <= W, HSR_ERR_INVALID,
              "hsr_scl_coarse: block k=%d outside [1,%d] or larger than the %d x %d plane", k, HSR_SCL_MAX_K, H, W);
  HSR_REQUIRE(max_bad >= 0, HSR_ERR_INVALID, "hsr_scl_coarse: max_bad=%d < 0", max_bad);
  const int hc = H / k, wc = W / k;
  int nwy = 0, nwx = 0;
  if (win_counts_dev) {
    HSR_REQUIRE(ce_h >= 1 && ce_w >= 1 && ce_h <= hc && ce_w <= wc, HSR_ERR_INVALID,
                "hsr_scl_coarse: a cell-window of %d x %d on the %d x %d grid", ce_h, ce_w, hc, wc);
    nwy = hc / ce_h;
    nwx = wc / ce_w;
  }
  hipStream_t s = (hipStream_t)stream;
  if (win_counts_dev) {
    const int rc = check_hip(hipMemsetAsync(win_counts_dev, 0, (size_t)nwy * nwx * sizeof(int32_t), s),
                             "hsr_scl_coarse: clearing the window counts");
    if (rc != HSR_OK) return rc;
  }
  const CoarseArgs a{mask_dev, rs, k, max_bad, hc, wc, clear_dev, cell_bad_dev, win_counts_dev ? ce_h : 1, win_counts_dev ? ce_w : 1,
                     nwy, nwx, win_counts_dev};
  const dim3 grid((unsigned)((wc + kSclThreads - 1) / kSclThreads), (unsigned)(hc < 65535 ? hc : 65535));
  hipLaunchKernelGGL(scl_coarse_kernel, grid, dim3(kSclThreads), 0, s, a);
  return launched(kLaunchScl, "scl_coarse_kernel launch", kSclCoarse);
}

extern "C" int hsr_scl_gather_tiles(const uint8_t* plane_dev, int32_t H, int32_t W, int64_t rs, const int32_t* origins_dev,
                                    int32_t ntiles, int32_t th, int32_t tw, uint8_t* out_dev, hsr_stream_t stream) {
  HSR_REQUIRE(plane_dev && origins_dev && out_dev, HSR_ERR_INVALID, "hsr_scl_gather_tiles: NULL pointer");
  HSR_REQUIRE(H >= 1 && W >= 1 && th >= 1 && tw >= 1 && ntiles >= 1, HSR_ERR_INVALID,
              "hsr_scl_gather_tiles: an extent < 1 (H=%d, W=%d, %d tiles of %d x %d)", H, W, ntiles, th, tw);
  HSR_REQUIRE(rs >= W, HSR_ERR_INVALID, "hsr_scl_gather_tiles: a row stride %lld below W=%d", (long long)rs, W);
  const int64_t blocks = ((int64_t)th * tw + 4 * kSclThreads - 1) / (4 * kSclThreads);
  const dim3 grid((unsigned)ntiles, (unsigned)(blocks < 64 ? blocks : 64));
  hipLaunchKernelGGL(scl_gather_kernel, grid, dim3(kSclThreads), 0, (hipStream_t)stream, plane_dev, H, W, rs, origins_dev, th, tw,
                     out_dev);
  return launched(kLaunchScl, "scl_gather_kernel launch", kSclGather);
}

extern "C" int hsr_scl_apply(float* cube_dev, int32_t T, int32_t H, int32_t W, int64_t bs, int64_t rs, const uint8_t* mask_dev,
                             int32_t Hm, int32_t Wm, int64_t mask_rs, int32_t up, float fill, int64_t* count_dev, hsr_stream_t stream) {
  HSR_REQUIRE(cube_dev && mask_dev, HSR_ERR_INVALID, "hsr_scl_apply: NULL pointer");
  HSR_REQUIRE(T >= 1 && H >= 1 && W >= 1 && Hm >= 1 && Wm >= 1, HSR_ERR_INVALID, "hsr_scl_apply: an extent < 1");
  HSR_REQUIRE(up == 1 || up == 2, HSR_ERR_INVALID, "hsr_scl_apply: up=%d outside {1,2}", up);
  HSR_REQUIRE(H <= (int64_t)Hm * up && W <= (int64_t)Wm * up, HSR_ERR_INVALID,
              "hsr_scl_apply: the %d x %d cube is larger than the %d x %d mask at up=%d", H, W, Hm, Wm, up);
  HSR_REQUIRE(rs >= W && bs >= (int64_t)(H - 1) * rs + W && mask_rs >= Wm, HSR_ERR_INVALID,
              "hsr_scl_apply: strides under which rows or bands overlap");
  hipStream_t s = (hipStream_t)stream;
  if (count_dev) {
    const int rc = check_hip(hipMemsetAsync(count_dev, 0, sizeof(int64_t), s), "hsr_scl_apply: clearing the count");
    if (rc != HSR_OK) return rc;
  }
  const int vec = ((((uintptr_t)cube_dev >> 2) | (uintptr_t)bs | (uintptr_t)rs) & 3) == 0 && ((uintptr_t)cube_dev & 3) == 0;
  const ApplyArgs a{cube_dev, T, H, W, bs, rs, mask_dev, mask_rs, fill, reinterpret_cast<unsigned long long*>(count_dev), vec};
  const int64_t per_row = ((int64_t)W + 3) / 4;
  const dim3 grid((unsigned)((per_row + kSclThreads - 1) / kSclThreads), (unsigned)(H < 65535 ? H : 65535));
  if (up == 2) hipLaunchKernelGGL((scl_apply_kernel<2>), grid, dim3(kSclThreads), 0, s, a);
  else hipLaunchKernelGGL((scl_apply_kernel<1>), grid, dim3(kSclThreads), 0, s, a);
  return launched(kLaunchScl, "scl_apply_kernel launch", kSclApply + (up == 2 ? 1 : 0));
}
