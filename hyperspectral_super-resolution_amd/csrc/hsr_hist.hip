// Exact masked histogram matching on gfx950 (C ABI and the definition: include/hsr_hist.h): the keys of every channel of both
// images in one pass, a batched keys-only radix sort, pivot tables and an exact rank lookup per pixel, and the host twin.
//
// Reference: s2_emit/color.py:36-63 (histogram_match_rgb: np.unique with counts, cumulative sums, np.interp, per channel on the
// host).  Structure:
//   keys     a thread per pixel: its C source and C reference samples and the mask -> 2 C keys; an invalid pixel gets the sentinel,
//            so nothing is compacted.  The counts are a ballot per wave and channel, a register, four LDS adds and one integer atomic per
//            workgroup of 8192 pixels and channel.
//   sort     4 passes of 8 bits over all planes at once (plane = blockIdx.y).  count: LDS integer atomics per tile of 8192 keys ->
//            counters[plane][digit][tile].  scan: ONE workgroup per plane walks its 256 * tiles counters in steps of 4096 with a
//            carry - no workgroup reads what another writes in the same launch.  scatter: wave w of a tile owns keys
//            [1024 w, 1024 w + 1024) in 16 rounds of 64; a round finds each lane's peers of equal digit with 8 ballots, the peers'
//            first lane bumps the WAVE's own LDS counter, so a key's rank among the equal digits of its wave needs no barrier;
//            wave and digit starts come from one pass over 8 x 256 counters; the tile is ordered in LDS and leaves in runs.
//   pivots   level l of a plane: the last key of every 256^l of its n valid keys, straight from the sorted plane.
//   lookup   hist_pixel() IS the definition; hist_rank_le() is a binary search in the top level (LDS on the device) and at most 8
//            steps in a 256-entry window per level below.  Both are __host__ __device__: hsr_hist_match_host runs them on host
//            planes sorted by std::sort.
#include <limits.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "hsr_common.h"
#include "../../include/hsr_hist.h"

namespace hsr {

constexpr int kHistTile = HSR_HIST_SORT_TILE, kHistBins = 1 << HSR_HIST_SORT_BITS, kHistPasses = 32 / HSR_HIST_SORT_BITS;
constexpr int kSortThreads = 512, kSortWaves = kSortThreads / 64, kSortRounds = kHistTile / kSortThreads;
constexpr int kWaveKeys = kHistTile / kSortWaves;
constexpr int kScanThreads = 1024, kScanPer = HSR_HIST_SCAN_STEP / kScanThreads;
constexpr int kPivot = HSR_HIST_PIVOT;
constexpr int kLookThreads = 256, kLookPer = 4;
constexpr int kKeysIters = 32;                        // a workgroup of the keys kernel takes 32 x 256 pixels
constexpr uint32_t kSentinel = HSR_HIST_SENTINEL;
static_assert(kHistBins == 256 && kHistPasses == 4 && kSortRounds == 16 && kWaveKeys == 64 * kSortRounds, "the sort's geometry");
static_assert(kScanPer == 4 && kPivot == 256, "the scan's and the tables' geometry");

// ------------------------------------------------------------------------------------------------------------------------------
// the key, the pivot tables, the rank and the rule of a pixel: host and device
// ------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t hist_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
__host__ __device__ inline bool hist_finite(float v) { return (hist_bits(v) & 0x7f800000u) != 0x7f800000u; }
// f32_key of hsr_select_dev.h with -0.0 taken as +0.0
__host__ __device__ inline uint32_t hist_key(float v) {
  uint32_t u = hist_bits(v);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float hist_value(uint32_t k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__host__ __device__ inline float hist_clip(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }   // NaN passes both compares

__host__ __device__ inline uint32_t hist_ceil_div(uint32_t a, uint32_t b) { return a / b + (a % b ? 1u : 0u); }

struct HistCaps { uint32_t cap[4]; uint32_t total; };   // cap[l]: entries of level l at n == npix; total: cap1 + cap2 + cap3 rounded to 64
__host__ __device__ inline HistCaps hist_caps(uint32_t npix) {
  HistCaps c;
  c.cap[0] = npix;
  c.cap[1] = hist_ceil_div(npix, kPivot);
  c.cap[2] = hist_ceil_div(c.cap[1], kPivot);
  c.cap[3] = hist_ceil_div(c.cap[2], kPivot);
  c.total = (c.cap[1] + c.cap[2] + c.cap[3] + 63u) & ~63u;
  return c;
}

// Entry e of a plane's pivot storage (levels 1, 2, 3 one after the other): the last of every 256^l of the plane's first n keys.
__host__ __device__ inline void hist_pivot_entry(const uint32_t* keys, uint32_t* piv, const HistCaps& hc, uint32_t n, uint32_t e) {
  uint32_t j = e;
  uint64_t span = kPivot;
  int l = 1;
  if (j >= hc.cap[1]) { j -= hc.cap[1]; span *= kPivot; l = 2; }
  if (l == 2 && j >= hc.cap[2]) { j -= hc.cap[2]; span *= kPivot; l = 3; }
  if (l == 3 && j >= hc.cap[3]) return;
  const uint64_t first = (uint64_t)j * span;
  if (first >= n) return;                                 // beyond the level's count: never read
  const uint64_t end = first + span < n ? first + span : n;
  piv[e] = keys[end - 1];
}

struct HistTab {
  const uint32_t* lvl[4];   // 0: the sorted keys; 1..3: the pivot levels
  uint32_t cnt[4];
  int top;                  // the first level with at most 256 entries
};
__host__ __device__ inline HistTab hist_tab(const uint32_t* keys, const uint32_t* piv, const HistCaps& hc, uint32_t n) {
  HistTab t;
  t.lvl[0] = keys; t.lvl[1] = piv; t.lvl[2] = piv + hc.cap[1]; t.lvl[3] = piv + hc.cap[1] + hc.cap[2];
  t.cnt[0] = n;
  t.cnt[1] = hist_ceil_div(n, kPivot); t.cnt[2] = hist_ceil_div(t.cnt[1], kPivot); t.cnt[3] = hist_ceil_div(t.cnt[2], kPivot);
  t.top = t.cnt[0] <= (uint32_t)kPivot ? 0 : (t.cnt[1] <= (uint32_t)kPivot ? 1 : (t.cnt[2] <= (uint32_t)kPivot ? 2 : 3));
  return t;
}

// #{p[lo..hi) <= key} + lo in an ascending array
__host__ __device__ inline uint32_t hist_upper(const uint32_t* p, uint32_t lo, uint32_t hi, uint32_t key) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (p[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// #{keys[0..n) <= key}.  top: the table's top level (a copy in LDS on the device).
__host__ __device__ inline uint32_t hist_rank_le(const HistTab& t, const uint32_t* top, uint32_t key) {
  uint32_t c = hist_upper(top, 0u, t.cnt[t.top], key);
#pragma unroll
  for (int l = 2; l >= 0; --l) {
    if (l < t.top) {
      if (c >= t.cnt[l + 1]) {
        c = t.cnt[l];                                       // every block of level l ends on a key <= key
      } else {
        const uint32_t lo = c * (uint32_t)kPivot, end = lo + (uint32_t)kPivot;
        c = hist_upper(t.lvl[l], lo, end < t.cnt[l] ? end : t.cnt[l], key);
      }
    }
  }
  return c;
}

// The definition for one pixel of one channel.  n > 0 only when valid.
__host__ __device__ inline float hist_pixel(const HistTab& S, const uint32_t* topS, const HistTab& R, const uint32_t* topR, float v,
                                            bool valid) {
  const uint32_t n = S.cnt[0];
  if (!valid || n == 0u) return hist_clip(v);
  const uint32_t cs = hist_rank_le(S, topS, hist_key(v));
  if (cs == 0u) return hist_clip(v);                        // v below every key: the planes are not those of this image
  const uint32_t* Rk = R.lvl[0];
  const uint32_t ka = Rk[cs - 1];
  const float a = hist_value(ka);
  double res = (double)a;
  const uint32_t hi = (cs == n || Rk[cs] > ka) ? cs : hist_rank_le(R, topR, ka);
  if (hi != cs) {
    const uint32_t lo = (cs >= 2u && Rk[cs - 2] < ka) ? cs - 1u : hist_rank_le(R, topR, ka - 1u);   // ka > 0: the least finite key is 0x00800000
    if (lo != 0u) {
      const double b = (double)hist_value(Rk[lo - 1]), dn = (double)n;
      const double flo = (double)lo / dn;
      const double slope = ((double)a - b) / ((double)hi / dn - flo);
      const double step = slope * ((double)cs / dn - flo);
      res = step + b;
    }
  }
  return hist_clip((float)res);
}

// ------------------------------------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------------------------------------
struct HistImage { const float* p; int64_t cs, ps; };

template <bool PLANAR>
__device__ __forceinline__ float hist_load(const HistImage& im, int c, int64_t i) {
  return PLANAR ? im.p[(int64_t)c * im.cs + i] : im.p[i * im.ps + c];
}

// A workgroup takes kKeysIters x 256 consecutive pixels: the counts are a ballot per wave and channel, summed in a register over the
// workgroup's pixels, then in LDS over its four waves, and leave as ONE integer atomic per workgroup and channel (one per wave and 64
// pixels put 49 152 atomics on three words at 1024 x 1024 x 3: 0.6 ms for a pass that streams 51 MB, profiles/r24_histmatch.md).
template <bool PLANAR>
__global__ __launch_bounds__(256) void hist_keys_kernel(HistImage src, HistImage ref, const uint8_t* mask, uint32_t npix, int C,
                                                        uint32_t* keys, int64_t stride, unsigned long long* n_valid) {
  __shared__ uint32_t total[HSR_HIST_MAX_CHANNELS];
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < HSR_HIST_MAX_CHANNELS) total[threadIdx.x] = 0u;
  __syncthreads();
  const int64_t first = (int64_t)blockIdx.x * (kKeysIters * 256) + threadIdx.x;
#pragma unroll 1
  for (int c = 0; c < C; ++c) {
    uint32_t count = 0u;
#pragma unroll 4
    for (int it = 0; it < kKeysIters; ++it) {
      const int64_t i = first + (int64_t)it * 256;
      bool valid = false;
      if (i < (int64_t)npix) {
        uint32_t ks = kSentinel, kr = kSentinel;
        const float s = hist_load<PLANAR>(src, c, i), r = hist_load<PLANAR>(ref, c, i);
        valid = mask[i] != 0 && hist_finite(s) && hist_finite(r);
        if (valid) { ks = hist_key(s); kr = hist_key(r); }
        keys[(int64_t)c * stride + i] = ks;
        keys[(int64_t)(C + c) * stride + i] = kr;
      }
      count += (uint32_t)__popcll(__ballot(valid));
    }
    if (lane == 0 && count) atomicAdd(&total[c], count);
  }
  __syncthreads();
  if ((int)threadIdx.x < C && total[threadIdx.x]) atomicAdd(&n_valid[threadIdx.x], (unsigned long long)total[threadIdx.x]);
}

template <int PASS>
__global__ __launch_bounds__(kSortThreads) void hist_count_kernel(const uint32_t* keys, int64_t stride, uint32_t npix, uint32_t ntiles,
                                                                  uint32_t* counters) {
  __shared__ uint32_t hist[kHistBins];
  const uint32_t tile = blockIdx.x, plane = blockIdx.y;
  const uint32_t* src = keys + (int64_t)plane * stride;
  const uint32_t t0 = tile * (uint32_t)kHistTile;
  const uint32_t tn = npix - t0 < (uint32_t)kHistTile ? npix - t0 : (uint32_t)kHistTile;
  if (threadIdx.x < kHistBins) hist[threadIdx.x] = 0u;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r) {
    const uint32_t idx = (uint32_t)r * kSortThreads + threadIdx.x;
    if (idx < tn) atomicAdd(&hist[(src[t0 + idx] >> (HSR_HIST_SORT_BITS * PASS)) & 255u], 1u);
  }
  __syncthreads();
  if (threadIdx.x < kHistBins) counters[((size_t)plane * kHistBins + threadIdx.x) * ntiles + tile] = hist[threadIdx.x];
}

// Exclusive scan of a plane's 256 * ntiles counters in place, in (digit, tile) order.
__global__ __launch_bounds__(kScanThreads) void hist_scan_kernel(uint32_t* counters, uint32_t ntiles) {
  __shared__ uint32_t wsum[kScanThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t total = (size_t)kHistBins * ntiles;
  uint32_t* c = counters + (size_t)blockIdx.y * total;
  uint32_t carry = 0u;
  for (size_t base = 0; base < total; base += HSR_HIST_SCAN_STEP) {
    const size_t e0 = base + (size_t)tid * kScanPer;
    uint32_t v[kScanPer], sum = 0u;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
      v[k] = e0 + k < total ? c[e0 + k] : 0u;
      sum += v[k];
    }
    uint32_t inc = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o = __shfl_up(inc, off, 64);
      if (lane >= off) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
#pragma unroll
    for (int w = 0; w < kScanThreads / 64; ++w) {
      const uint32_t s = wsum[w];
      if (w < wave) before += s;
      all += s;
    }
    uint32_t run = carry + before + (inc - sum);
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
      if (e0 + k < total) c[e0 + k] = run;
      run += v[k];
    }
    carry += all;
    __syncthreads();
  }
}

template <int PASS>
__global__ __launch_bounds__(kSortThreads) void hist_scatter_kernel(const uint32_t* in, uint32_t* out, int64_t stride, uint32_t npix,
                                                                    uint32_t ntiles, const uint32_t* offsets) {
  __shared__ uint32_t skeys[kHistTile];
  __shared__ uint32_t whist[kSortWaves][kHistBins];   // a wave's running counts per digit; then its start inside the digit's run
  __shared__ uint32_t dtot[kHistBins], dstart[kHistBins], gbase[kHistBins];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t tile = blockIdx.x, plane = blockIdx.y;
  const uint32_t* src = in + (int64_t)plane * stride;
  uint32_t* dst = out + (int64_t)plane * stride;
  const uint32_t t0 = tile * (uint32_t)kHistTile;
  const uint32_t tn = npix - t0 < (uint32_t)kHistTile ? npix - t0 : (uint32_t)kHistTile;
  for (int i = tid; i < kSortWaves * kHistBins; i += kSortThreads) (&whist[0][0])[i] = 0u;
  uint32_t key[kSortRounds], rnk[kSortRounds];
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r) {
    const uint32_t idx = (uint32_t)(wave * kWaveKeys + r * 64 + lane);
    key[r] = idx < tn ? src[t0 + idx] : kSentinel;
  }
  __syncthreads();
  volatile uint32_t* mine = whist[wave];
  const unsigned long long below_mask = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r) {
    const uint32_t idx = (uint32_t)(wave * kWaveKeys + r * 64 + lane);
    const bool ok = idx < tn;
    const uint32_t d = (key[r] >> (HSR_HIST_SORT_BITS * PASS)) & 255u;
    unsigned long long peers = __ballot(ok);
#pragma unroll
    for (int b = 0; b < HSR_HIST_SORT_BITS; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(ok && bit);
      peers &= bit ? bal : ~bal;
    }
    const uint32_t below = (uint32_t)__popcll(peers & below_mask);
    uint32_t pre = 0u;
    if (ok && below == 0u) {                           // the first lane of its peers: one lane per digit present, distinct words
      pre = mine[d];
      mine[d] = pre + (uint32_t)__popcll(peers);
    }
    const int leader = ok ? __ffsll((unsigned long long)peers) - 1 : lane;
    pre = __shfl(pre, leader, 64);
    rnk[r] = pre + below;
  }
  __syncthreads();
  if (tid < kHistBins) {
    uint32_t s = 0u;
#pragma unroll
    for (int w = 0; w < kSortWaves; ++w) {
      const uint32_t t = whist[w][tid];
      whist[w][tid] = s;
      s += t;
    }
    dtot[tid] = s;
    gbase[tid] = offsets[((size_t)plane * kHistBins + tid) * ntiles + tile];
  }
  __syncthreads();
  if (wave == 0) {                                     // the digits' starts inside the tile: lane l scans digits 4 l .. 4 l + 3
    uint32_t v[4], sum = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = dtot[4 * lane + k]; sum += v[k]; }
    uint32_t inc = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o = __shfl_up(inc, off, 64);
      if (lane >= off) inc += o;
    }
    uint32_t run = inc - sum;
#pragma unroll
    for (int k = 0; k < 4; ++k) { dstart[4 * lane + k] = run; run += v[k]; }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r) {
    const uint32_t idx = (uint32_t)(wave * kWaveKeys + r * 64 + lane);
    const uint32_t d = (key[r] >> (HSR_HIST_SORT_BITS * PASS)) & 255u;
    if (idx < tn) {
      const uint32_t pos = dstart[d] + whist[wave][d] + rnk[r];
      if (pos < tn) skeys[pos] = key[r];               // pos < tn by construction; the compare keeps a fault inside LDS
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r) {
    const uint32_t i = (uint32_t)(r * kSortThreads + tid);
    if (i < tn) {
      const uint32_t k = skeys[i], d = (k >> (HSR_HIST_SORT_BITS * PASS)) & 255u;
      const uint32_t g = gbase[d] + (i - dstart[d]);
      if (g < npix) dst[g] = k;                        // g < npix by construction; the compare keeps a fault inside the plane
    }
  }
}

__device__ __forceinline__ uint32_t hist_count_of(const long long* n_valid, int c, uint32_t npix) {
  const long long n = n_valid[c];
  return n < 0 || n > (long long)npix ? npix : (uint32_t)n;
}

__global__ __launch_bounds__(256) void hist_pivots_kernel(const uint32_t* sorted, int64_t stride, const long long* n_valid, int C,
                                                          uint32_t npix, uint32_t* pivots) {
  const HistCaps hc = hist_caps(npix);
  const uint32_t plane = blockIdx.y;
  const uint32_t n = hist_count_of(n_valid, (int)(plane % (uint32_t)C), npix);
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < (uint64_t)hc.cap[1] + hc.cap[2] + hc.cap[3])
    hist_pivot_entry(sorted + (int64_t)plane * stride, pivots + (size_t)plane * hc.total, hc, n, (uint32_t)e);
}

template <bool PLANAR>
__global__ __launch_bounds__(kLookThreads) void hist_lookup_kernel(const uint32_t* sorted, int64_t stride, const long long* n_valid,
                                                                   const uint32_t* pivots, HistImage src, HistImage ref,
                                                                   const uint8_t* mask, uint32_t npix, int C, float* out, int64_t ocs,
                                                                   int64_t ops) {
  __shared__ uint32_t top[2][kPivot];
  const int c = (int)blockIdx.y, tid = threadIdx.x;
  const HistCaps hc = hist_caps(npix);
  const uint32_t n = hist_count_of(n_valid, c, npix);
  const HistTab S = hist_tab(sorted + (int64_t)c * stride, pivots + (size_t)c * hc.total, hc, n);
  const HistTab R = hist_tab(sorted + (int64_t)(C + c) * stride, pivots + (size_t)(C + c) * hc.total, hc, n);
  if ((uint32_t)tid < S.cnt[S.top]) {                    // S and R have the same n: the same top level and count, <= 256
    top[0][tid] = S.lvl[S.top][tid];
    top[1][tid] = R.lvl[R.top][tid];
  }
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < kLookPer; ++k) {
    const int64_t i = ((int64_t)blockIdx.x * kLookPer + k) * kLookThreads + tid;
    if (i >= (int64_t)npix) break;
    const float v = hist_load<PLANAR>(src, c, i);
    const bool valid = mask[i] != 0 && hist_finite(v) && hist_finite(hist_load<PLANAR>(ref, c, i));
    const float o = hist_pixel(S, top[0], R, top[1], v, valid);
    out[PLANAR ? (int64_t)c * ocs + i : i * ops + c] = o;
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// arguments
// ------------------------------------------------------------------------------------------------------------------------------
static bool hist_overlap(const void* p, uint64_t pn, const void* q, uint64_t qn) {
  const uintptr_t pb = (uintptr_t)p, qb = (uintptr_t)q;
  return !(pb + pn <= qb || qb + qn <= pb);
}

static int hist_size_ok(const char* who, int64_t npix, int32_t C, int32_t cmax) {
  HSR_REQUIRE(C >= 1 && C <= cmax, HSR_ERR_INVALID, "%s: %d channels or planes outside [1,%d]", who, C, cmax);
  HSR_REQUIRE(npix >= 1, HSR_ERR_INVALID, "%s: npix=%lld < 1", who, (long long)npix);
  HSR_REQUIRE(npix <= HSR_HIST_MAX_NPIX, HSR_ERR_UNSUPPORTED, "%s: npix=%lld beyond the 32-bit ranks (%d)", who, (long long)npix,
              HSR_HIST_MAX_NPIX);
  return HSR_OK;
}

// The layout of an image (0 pixel-major, 1 planar) after checking its strides; its extent in bytes.
static int hist_image_ok(const char* who, const char* what, const void* p, int64_t cs, int64_t ps, int64_t npix, int32_t C, int* planar,
                         uint64_t* bytes) {
  HSR_REQUIRE(p, HSR_ERR_INVALID, "%s: NULL pointer (%s)", who, what);
  if (ps == 1 && (C == 1 || cs >= npix)) {
    *planar = 1;
    *bytes = ((uint64_t)(C - 1) * (uint64_t)(C == 1 ? 0 : cs) + (uint64_t)npix) * 4u;
  } else if (cs == 1 && ps >= C) {
    *planar = 0;
    *bytes = ((uint64_t)(npix - 1) * (uint64_t)ps + (uint64_t)C) * 4u;
  } else {
    set_error("%s: %s has strides (channel %lld, pixel %lld) that are neither planar (pixel 1, channel >= npix=%lld) nor "
              "pixel-major (channel 1, pixel >= C=%d)", who, what, (long long)cs, (long long)ps, (long long)npix, C);
    return HSR_ERR_INVALID;
  }
  return HSR_OK;
}

struct HistImages {
  int planar;
  uint64_t src_bytes, ref_bytes, out_bytes;
};

static int hist_images_ok(const char* who, const float* src, int64_t scs, int64_t sps, const float* ref, int64_t rcs, int64_t rps,
                          const uint8_t* mask, int64_t npix, int32_t C, float* out, int64_t ocs, int64_t ops, bool with_out,
                          HistImages* im) {
  int rc = hist_size_ok(who, npix, C, HSR_HIST_MAX_CHANNELS);
  if (rc != HSR_OK) return rc;
  HSR_REQUIRE(mask, HSR_ERR_INVALID, "%s: NULL pointer (mask)", who);
  int ps = 0, pr = 0, po = 0;
  if ((rc = hist_image_ok(who, "src", src, scs, sps, npix, C, &ps, &im->src_bytes)) != HSR_OK) return rc;
  if ((rc = hist_image_ok(who, "ref", ref, rcs, rps, npix, C, &pr, &im->ref_bytes)) != HSR_OK) return rc;
  HSR_REQUIRE(ps == pr, HSR_ERR_INVALID, "%s: src and ref differ in the kind of layout", who);
  im->planar = ps;
  im->out_bytes = 0;
  if (with_out) {
    if ((rc = hist_image_ok(who, "out", out, ocs, ops, npix, C, &po, &im->out_bytes)) != HSR_OK) return rc;
    HSR_REQUIRE(po == ps, HSR_ERR_INVALID, "%s: src and out differ in the kind of layout", who);
    const bool in_place = (const float*)out == src && ocs == scs && ops == sps;
    HSR_REQUIRE(in_place || !hist_overlap(out, im->out_bytes, src, im->src_bytes), HSR_ERR_INVALID,
                "%s: the output overlaps src without being src under the same strides", who);
    HSR_REQUIRE(!hist_overlap(out, im->out_bytes, ref, im->ref_bytes), HSR_ERR_INVALID, "%s: the output overlaps ref", who);
    HSR_REQUIRE(!hist_overlap(out, im->out_bytes, mask, (uint64_t)npix), HSR_ERR_INVALID, "%s: the output overlaps the mask", who);
  }
  return HSR_OK;
}

static uint64_t hist_planes_bytes(int64_t stride, int64_t npix, int32_t P) { return ((uint64_t)(P - 1) * (uint64_t)stride + (uint64_t)npix) * 4u; }

static int hist_keys_launch(const char* who, const float* src, int64_t scs, int64_t sps, const float* ref, int64_t rcs, int64_t rps,
                            const uint8_t* mask, int64_t npix, int32_t C, int planar, uint32_t* keys, int64_t stride, int64_t* n_valid,
                            hipStream_t s) {
  int rc = check_hip(hipMemsetAsync(n_valid, 0, (size_t)C * sizeof(int64_t), s), "hsr_hist_keys: clearing the counts");
  if (rc != HSR_OK) return rc;
  const HistImage si{src, scs, sps}, ri{ref, rcs, rps};
  const dim3 grid((unsigned)((npix + kKeysIters * 256 - 1) / (kKeysIters * 256)));
  unsigned long long* nv = reinterpret_cast<unsigned long long*>(n_valid);
  if (planar) hipLaunchKernelGGL((hist_keys_kernel<true>), grid, dim3(256), 0, s, si, ri, mask, (uint32_t)npix, (int)C, keys, stride, nv);
  else hipLaunchKernelGGL((hist_keys_kernel<false>), grid, dim3(256), 0, s, si, ri, mask, (uint32_t)npix, (int)C, keys, stride, nv);
  (void)who;
  return launched(kLaunchHist, "hist_keys_kernel launch", kHistKeys + planar);
}

template <int PASS>
static int hist_sort_pass(const uint32_t* in, uint32_t* out, int64_t stride, uint32_t npix, uint32_t ntiles, int32_t P, uint32_t* counters,
                          hipStream_t s) {
  const dim3 grid(ntiles, (unsigned)P);
  hipLaunchKernelGGL((hist_count_kernel<PASS>), grid, dim3(kSortThreads), 0, s, in, stride, npix, ntiles, counters);
  int rc = launched(kLaunchHist, "hist_count_kernel launch", kHistCount + PASS);
  if (rc != HSR_OK) return rc;
  hipLaunchKernelGGL(hist_scan_kernel, dim3(1, (unsigned)P), dim3(kScanThreads), 0, s, counters, ntiles);
  rc = launched(kLaunchHist, "hist_scan_kernel launch", kHistScan);
  if (rc != HSR_OK) return rc;
  hipLaunchKernelGGL((hist_scatter_kernel<PASS>), grid, dim3(kSortThreads), 0, s, in, out, stride, npix, ntiles, counters);
  return launched(kLaunchHist, "hist_scatter_kernel launch", kHistScatter + PASS);
}

static int hist_sort_launch(uint32_t* keys, uint32_t* tmp, int64_t stride, int64_t npix, int32_t P, uint32_t* counters, hipStream_t s) {
  const uint32_t n = (uint32_t)npix, ntiles = (n + kHistTile - 1) / kHistTile;
  int rc = hist_sort_pass<0>(keys, tmp, stride, n, ntiles, P, counters, s);
  if (rc == HSR_OK) rc = hist_sort_pass<1>(tmp, keys, stride, n, ntiles, P, counters, s);
  if (rc == HSR_OK) rc = hist_sort_pass<2>(keys, tmp, stride, n, ntiles, P, counters, s);
  if (rc == HSR_OK) rc = hist_sort_pass<3>(tmp, keys, stride, n, ntiles, P, counters, s);
  return rc;
}

static int hist_lookup_launch(const uint32_t* sorted, int64_t stride, const int64_t* n_valid, uint32_t* pivots, const float* src, int64_t scs,
                              int64_t sps, const float* ref, int64_t rcs, int64_t rps, const uint8_t* mask, int64_t npix, int32_t C,
                              int planar, float* out, int64_t ocs, int64_t ops, hipStream_t s) {
  const HistCaps hc = hist_caps((uint32_t)npix);
  const uint64_t entries = (uint64_t)hc.cap[1] + hc.cap[2] + hc.cap[3];
  const long long* nv = reinterpret_cast<const long long*>(n_valid);
  hipLaunchKernelGGL(hist_pivots_kernel, dim3((unsigned)((entries + 255) / 256), (unsigned)(2 * C)), dim3(256), 0, s, sorted, stride, nv,
                     (int)C, (uint32_t)npix, pivots);
  int rc = launched(kLaunchHist, "hist_pivots_kernel launch", kHistPivots);
  if (rc != HSR_OK) return rc;
  const HistImage si{src, scs, sps}, ri{ref, rcs, rps};
  const dim3 grid((unsigned)((npix + kLookThreads * kLookPer - 1) / (kLookThreads * kLookPer)), (unsigned)C);
  if (planar)
    hipLaunchKernelGGL((hist_lookup_kernel<true>), grid, dim3(kLookThreads), 0, s, sorted, stride, nv, pivots, si, ri, mask, (uint32_t)npix,
                       (int)C, out, ocs, ops);
  else
    hipLaunchKernelGGL((hist_lookup_kernel<false>), grid, dim3(kLookThreads), 0, s, sorted, stride, nv, pivots, si, ri, mask, (uint32_t)npix,
                       (int)C, out, ocs, ops);
  return launched(kLaunchHist, "hist_lookup_kernel launch", kHistLookup + planar);
}

static size_t hist_round256(size_t b) { return (b + 255u) & ~(size_t)255u; }

}  // namespace hsr

using namespace hsr;

extern "C" int64_t hsr_hist_plane_stride(int64_t npix) {
  return npix >= 1 && npix <= HSR_HIST_MAX_NPIX ? (npix + 63) & ~(int64_t)63 : 0;
}

extern "C" size_t hsr_hist_sort_bytes(int64_t npix, int32_t P) {
  if (npix < 1 || npix > HSR_HIST_MAX_NPIX || P < 1 || P > 2 * HSR_HIST_MAX_CHANNELS) return 0;
  return (size_t)P * kHistBins * (size_t)((npix + kHistTile - 1) / kHistTile) * sizeof(uint32_t);
}

extern "C" size_t hsr_hist_pivot_bytes(int64_t npix, int32_t C) {
  if (npix < 1 || npix > HSR_HIST_MAX_NPIX || C < 1 || C > HSR_HIST_MAX_CHANNELS) return 0;
  return (size_t)(2 * C) * hist_caps((uint32_t)npix).total * sizeof(uint32_t);
}

extern "C" size_t hsr_hist_scratch_bytes(int64_t npix, int32_t C) {
  if (npix < 1 || npix > HSR_HIST_MAX_NPIX || C < 1 || C > HSR_HIST_MAX_CHANNELS) return 0;
  const size_t planes = hist_round256((size_t)(2 * C) * (size_t)hsr_hist_plane_stride(npix) * sizeof(uint32_t));
  return 2 * planes + hist_round256(hsr_hist_sort_bytes(npix, 2 * C)) + hist_round256(hsr_hist_pivot_bytes(npix, C));
}

extern "C" uint32_t hsr_hist_key_host(float v) { return hist_finite(v) ? hist_key(v) : kSentinel; }

extern "C" int hsr_hist_keys(const float* src_dev, int64_t src_cs, int64_t src_ps, const float* ref_dev, int64_t ref_cs, int64_t ref_ps,
                             const uint8_t* mask_dev, int64_t npix, int32_t C, uint32_t* keys_dev, int64_t key_stride,
                             int64_t* n_valid_dev, hsr_stream_t stream) {
  const char* who = "hsr_hist_keys";
  HistImages im{};
  int rc = hist_images_ok(who, src_dev, src_cs, src_ps, ref_dev, ref_cs, ref_ps, mask_dev, npix, C, nullptr, 0, 0, false, &im);
  if (rc != HSR_OK) return rc;
  HSR_REQUIRE(keys_dev && n_valid_dev, HSR_ERR_INVALID, "%s: NULL pointer (keys or counts)", who);
  HSR_REQUIRE(key_stride >= npix, HSR_ERR_INVALID, "%s: key_stride=%lld below npix=%lld", who, (long long)key_stride, (long long)npix);
  const uint64_t kb = hist_planes_bytes(key_stride, npix, 2 * C);
  HSR_REQUIRE(!hist_overlap(keys_dev, kb, src_dev, im.src_bytes) && !hist_overlap(keys_dev, kb, ref_dev, im.ref_bytes) &&
                  !hist_overlap(keys_dev, kb, mask_dev, (uint64_t)npix) && !hist_overlap(keys_dev, kb, n_valid_dev, (uint64_t)C * 8u),
              HSR_ERR_INVALID, "%s: the keys overlap an input or the counts", who);
  HSR_REQUIRE(!hist_overlap(n_valid_dev, (uint64_t)C * 8u, src_dev, im.src_bytes) && !hist_overlap(n_valid_dev, (uint64_t)C * 8u, ref_dev, im.ref_bytes) &&
                  !hist_overlap(n_valid_dev, (uint64_t)C * 8u, mask_dev, (uint64_t)npix), HSR_ERR_INVALID, "%s: the counts overlap an input", who);
  return hist_keys_launch(who, src_dev, src_cs, src_ps, ref_dev, ref_cs, ref_ps, mask_dev, npix, C, im.planar, keys_dev, key_stride,
                          n_valid_dev, (hipStream_t)stream);
}

static int hist_sort_args(const char* who, const uint32_t* keys_dev, const uint32_t* tmp_dev, int64_t key_stride, int64_t npix, int32_t P,
                          const void* counters_dev, size_t counters_bytes) {
  HSR_REQUIRE(keys_dev && tmp_dev && counters_dev, HSR_ERR_INVALID, "%s: NULL pointer", who);
  const int rc = hist_size_ok(who, npix, P, 2 * HSR_HIST_MAX_CHANNELS);
  if (rc != HSR_OK) return rc;
  HSR_REQUIRE(key_stride >= npix, HSR_ERR_INVALID, "%s: key_stride=%lld below npix=%lld", who, (long long)key_stride, (long long)npix);
  const size_t need = hsr_hist_sort_bytes(npix, P);
  HSR_REQUIRE(counters_bytes >= need, HSR_ERR_INVALID, "%s: %zu bytes of counters, %zu needed", who, counters_bytes, need);
  HSR_REQUIRE(((uintptr_t)counters_dev & 3u) == 0, HSR_ERR_INVALID, "%s: the counters are not 4-byte aligned", who);
  const uint64_t kb = hist_planes_bytes(key_stride, npix, P);
  HSR_REQUIRE(!hist_overlap(keys_dev, kb, tmp_dev, kb) && !hist_overlap(keys_dev, kb, counters_dev, need) &&
                  !hist_overlap(tmp_dev, kb, counters_dev, need), HSR_ERR_INVALID, "%s: the two key buffers and the counters overlap", who);
  return HSR_OK;
}

extern "C" int hsr_hist_sort(uint32_t* keys_dev, uint32_t* tmp_dev, int64_t key_stride, int64_t npix, int32_t P, void* counters_dev,
                             size_t counters_bytes, hsr_stream_t stream) {
  const int rc = hist_sort_args("hsr_hist_sort", keys_dev, tmp_dev, key_stride, npix, P, counters_dev, counters_bytes);
  if (rc != HSR_OK) return rc;
  return hist_sort_launch(keys_dev, tmp_dev, key_stride, npix, P, static_cast<uint32_t*>(counters_dev), (hipStream_t)stream);
}

extern "C" int hsr_hist_sort_pass(const uint32_t* in_dev, uint32_t* out_dev, int64_t key_stride, int64_t npix, int32_t P, int32_t pass,
                                  void* counters_dev, size_t counters_bytes, hsr_stream_t stream) {
  const int rc = hist_sort_args("hsr_hist_sort_pass", in_dev, out_dev, key_stride, npix, P, counters_dev, counters_bytes);
  if (rc != HSR_OK) return rc;
  HSR_REQUIRE(pass >= 0 && pass < kHistPasses, HSR_ERR_INVALID, "hsr_hist_sort_pass: pass=%d outside [0,%d]", pass, kHistPasses - 1);
  const uint32_t n = (uint32_t)npix, ntiles = (n + kHistTile - 1) / kHistTile;
  uint32_t* counters = static_cast<uint32_t*>(counters_dev);
  hipStream_t s = (hipStream_t)stream;
  switch (pass) {
    case 0: return hist_sort_pass<0>(in_dev, out_dev, key_stride, n, ntiles, P, counters, s);
    case 1: return hist_sort_pass<1>(in_dev, out_dev, key_stride, n, ntiles, P, counters, s);
    case 2: return hist_sort_pass<2>(in_dev, out_dev, key_stride, n, ntiles, P, counters, s);
    default: return hist_sort_pass<3>(in_dev, out_dev, key_stride, n, ntiles, P, counters, s);
  }
}

extern "C" int hsr_hist_lookup(const uint32_t* sorted_dev, int64_t key_stride, const int64_t* n_valid_dev, void* pivots_dev,
                               size_t pivots_bytes, const float* src_dev, int64_t src_cs, int64_t src_ps, const float* ref_dev,
                               int64_t ref_cs, int64_t ref_ps, const uint8_t* mask_dev, int64_t npix, int32_t C, float* out_dev,
                               int64_t out_cs, int64_t out_ps, hsr_stream_t stream) {
  const char* who = "hsr_hist_lookup";
  HistImages im{};
  const int rc = hist_images_ok(who, src_dev, src_cs, src_ps, ref_dev, ref_cs, ref_ps, mask_dev, npix, C, out_dev, out_cs, out_ps, true, &im);
  if (rc != HSR_OK) return rc;
  HSR_REQUIRE(sorted_dev && n_valid_dev && pivots_dev, HSR_ERR_INVALID, "%s: NULL pointer (sorted planes, counts or pivots)", who);
  HSR_REQUIRE(key_stride >= npix, HSR_ERR_INVALID, "%s: key_stride=%lld below npix=%lld", who, (long long)key_stride, (long long)npix);
  const size_t need = hsr_hist_pivot_bytes(npix, C);
  HSR_REQUIRE(pivots_bytes >= need, HSR_ERR_INVALID, "%s: %zu bytes of pivots, %zu needed", who, pivots_bytes, need);
  HSR_REQUIRE(((uintptr_t)pivots_dev & 3u) == 0, HSR_ERR_INVALID, "%s: the pivots are not 4-byte aligned", who);
  const uint64_t kb = hist_planes_bytes(key_stride, npix, 2 * C);
  HSR_REQUIRE(!hist_overlap(out_dev, im.out_bytes, sorted_dev, kb) && !hist_overlap(out_dev, im.out_bytes, pivots_dev, need) &&
                  !hist_overlap(out_dev, im.out_bytes, n_valid_dev, (uint64_t)C * 8u), HSR_ERR_INVALID,
              "%s: the output overlaps a sorted plane, the pivots or the counts", who);
  HSR_REQUIRE(!hist_overlap(pivots_dev, need, sorted_dev, kb), HSR_ERR_INVALID, "%s: the pivots overlap the sorted planes", who);
  return hist_lookup_launch(sorted_dev, key_stride, n_valid_dev, static_cast<uint32_t*>(pivots_dev), src_dev, src_cs, src_ps, ref_dev,
                            ref_cs, ref_ps, mask_dev, npix, C, im.planar, out_dev, out_cs, out_ps, (hipStream_t)stream);
}

extern "C" int hsr_hist_match(const float* src_dev, int64_t src_cs, int64_t src_ps, const float* ref_dev, int64_t ref_cs, int64_t ref_ps,
                              const uint8_t* mask_dev, int64_t npix, int32_t C, float* out_dev, int64_t out_cs, int64_t out_ps,
                              int64_t* n_valid_dev, void* work_dev, size_t work_bytes, hsr_stream_t stream) {
  const char* who = "hsr_hist_match";
  HistImages im{};
  int rc = hist_images_ok(who, src_dev, src_cs, src_ps, ref_dev, ref_cs, ref_ps, mask_dev, npix, C, out_dev, out_cs, out_ps, true, &im);
  if (rc != HSR_OK) return rc;
  HSR_REQUIRE(n_valid_dev && work_dev, HSR_ERR_INVALID, "%s: NULL pointer (counts or workspace)", who);
  const size_t need = hsr_hist_scratch_bytes(npix, C);
  HSR_REQUIRE(work_bytes >= need, HSR_ERR_INVALID, "%s: a workspace of %zu bytes, %zu needed", who, work_bytes, need);
  HSR_REQUIRE(((uintptr_t)work_dev & 255u) == 0, HSR_ERR_INVALID, "%s: the workspace is not 256-byte aligned", who);
  HSR_REQUIRE(!hist_overlap(work_dev, need, out_dev, im.out_bytes) && !hist_overlap(work_dev, need, src_dev, im.src_bytes) &&
                  !hist_overlap(work_dev, need, ref_dev, im.ref_bytes) && !hist_overlap(work_dev, need, mask_dev, (uint64_t)npix) &&
                  !hist_overlap(work_dev, need, n_valid_dev, (uint64_t)C * 8u), HSR_ERR_INVALID,
              "%s: the workspace overlaps an image, the mask or the counts", who);
  HSR_REQUIRE(!hist_overlap(out_dev, im.out_bytes, n_valid_dev, (uint64_t)C * 8u), HSR_ERR_INVALID, "%s: the output overlaps the counts", who);
  HSR_REQUIRE(!hist_overlap(n_valid_dev, (uint64_t)C * 8u, src_dev, im.src_bytes) && !hist_overlap(n_valid_dev, (uint64_t)C * 8u, ref_dev, im.ref_bytes) &&
                  !hist_overlap(n_valid_dev, (uint64_t)C * 8u, mask_dev, (uint64_t)npix), HSR_ERR_INVALID, "%s: the counts overlap an input", who);
  const int64_t stride = hsr_hist_plane_stride(npix);
  const size_t planes = hist_round256((size_t)(2 * C) * (size_t)stride * sizeof(uint32_t));
  char* w = static_cast<char*>(work_dev);
  uint32_t* keys = reinterpret_cast<uint32_t*>(w);
  uint32_t* tmp = reinterpret_cast<uint32_t*>(w + planes);
  uint32_t* counters = reinterpret_cast<uint32_t*>(w + 2 * planes);
  uint32_t* pivots = reinterpret_cast<uint32_t*>(w + 2 * planes + hist_round256(hsr_hist_sort_bytes(npix, 2 * C)));
  hipStream_t s = (hipStream_t)stream;
  rc = hist_keys_launch(who, src_dev, src_cs, src_ps, ref_dev, ref_cs, ref_ps, mask_dev, npix, C, im.planar, keys, stride, n_valid_dev, s);
  if (rc == HSR_OK) rc = hist_sort_launch(keys, tmp, stride, npix, 2 * C, counters, s);
  if (rc == HSR_OK)
    rc = hist_lookup_launch(keys, stride, n_valid_dev, pivots, src_dev, src_cs, src_ps, ref_dev, ref_cs, ref_ps, mask_dev, npix, C, im.planar,
                            out_dev, out_cs, out_ps, s);
  return rc;
}

extern "C" int hsr_hist_match_host(const float* src, int64_t src_cs, int64_t src_ps, const float* ref, int64_t ref_cs, int64_t ref_ps,
                                   const uint8_t* mask, int64_t npix, int32_t C, float* out, int64_t out_cs, int64_t out_ps,
                                   int64_t* n_valid) {
  HistImages im{};
  const int rc = hist_images_ok("hsr_hist_match_host", src, src_cs, src_ps, ref, ref_cs, ref_ps, mask, npix, C, out, out_cs, out_ps, true, &im);
  if (rc != HSR_OK) return rc;
  const HistCaps hc = hist_caps((uint32_t)npix);
  const uint32_t entries = hc.cap[1] + hc.cap[2] + hc.cap[3];
  std::vector<uint32_t> ks((size_t)npix), kr((size_t)npix), ps(hc.total), pr(hc.total);
  auto at = [&](const float* p, int64_t cs, int64_t pst, int c, int64_t i) { return im.planar ? p[(int64_t)c * cs + i] : p[i * pst + c]; };
  for (int c = 0; c < C; ++c) {
    uint32_t n = 0;
    for (int64_t i = 0; i < npix; ++i) {
      const float s = at(src, src_cs, src_ps, c, i), r = at(ref, ref_cs, ref_ps, c, i);
      const bool valid = mask[i] != 0 && hist_finite(s) && hist_finite(r);
      ks[(size_t)i] = valid ? hist_key(s) : kSentinel;
      kr[(size_t)i] = valid ? hist_key(r) : kSentinel;
      n += valid ? 1u : 0u;
    }
    std::sort(ks.begin(), ks.end());
    std::sort(kr.begin(), kr.end());
    for (uint32_t e = 0; e < entries; ++e) {
      hist_pivot_entry(ks.data(), ps.data(), hc, n, e);
      hist_pivot_entry(kr.data(), pr.data(), hc, n, e);
    }
    const HistTab S = hist_tab(ks.data(), ps.data(), hc, n), R = hist_tab(kr.data(), pr.data(), hc, n);
    for (int64_t i = 0; i < npix; ++i) {
      const float v = at(src, src_cs, src_ps, c, i);
      const bool valid = mask[i] != 0 && hist_finite(v) && hist_finite(at(ref, ref_cs, ref_ps, c, i));
      out[im.planar ? (int64_t)c * out_cs + i : i * out_ps + c] = hist_pixel(S, S.lvl[S.top], R, R.lvl[R.top], v, valid);
    }
    if (n_valid) n_valid[c] = (int64_t)n;
  }
  return HSR_OK;
}
