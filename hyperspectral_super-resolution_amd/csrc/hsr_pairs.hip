// Tile pairs (s2_emit.fuse_tile_pairs): the front of the notebook's per-pair flow (legacy_notebooks/Spectral_matching.ipynb)
// for a batch of pairs, before the batched ridge fit of hsr_ridge.hip / hsr_chol.hip:
//   pair prep  one pass over a pair: S2 (nb, H f, W f) -> its f x f block mean on the EMIT grid (float64 sum of the f^2 samples,
//              float32 store: the bits of hsr_block_mean; a block holding a non-finite or nodata sample is NaN), the T selected
//              EMIT bands gathered and decoded (uint16: 65535 -> NaN, else u * 1e-4f), and flatten_pixels' training mask
//              (:108-126): all inputs and all selected targets finite and none close to its side's nodata value;
//   pair stats StandardScaler's statistics over the masked pixels (count, mean, then the centred sum of squares: two passes in a
//              fixed order, one workgroup per pair).
// blockIdx.y / blockIdx.x is the pair; nothing a pair computes depends on the other pairs of its batch.
// GDAL's bilinear `reproject` of S2 onto the EMIT grid (notebook raw line 377) is NOT reproduced: the block mean is the exact
// mean of the aligned 6 x 6 windows the tiles are cut as; callers with S2 already on the EMIT grid pass it as `s2_coarse`.
#include "hsr_common.h"

namespace hsr {

constexpr int kPairMaxIn = 16;

// predict_cube_logit's closeness test in float32, as pred_bad_input evaluates it (|x - nd| <= 1e-8 + 1e-5 |nd|, NaN never close)
__device__ __forceinline__ bool pair_close(float x, float nd) { return x == nd || fabsf(x - nd) <= 1e-8f + 1e-5f * fabsf(nd); }

__device__ __forceinline__ float pair_load(const void* p, int dtype, int64_t i) {
  return dtype == 2 ? (float)static_cast<const uint16_t*>(p)[i] : static_cast<const float*>(p)[i];
}

struct PairPrepArgs {
  const void* emit;          // (P, emit_bands, H, W): uint16 (dtype 2) or float32 (0)
  const void* s2;            // (P, nb, H f, W f): uint16 or float32; with f == 0 the (P, nb, H, W) float32 coarse image
  const int32_t* bands;      // [T] selected EMIT bands
  float* x;                  // (P, nb, H W) block mean
  float* y;                  // (P, T, H W) selected reflectance
  uint8_t* mask;             // (P, H W)
  int64_t pair_emit, pair_s2;
  int32_t emit_dtype, s2_dtype, nb, T, H, W, f;
  int32_t use_emit_nodata, use_s2_nodata;
  float emit_nodata, s2_nodata;
};

__global__ __launch_bounds__(256) void pair_prep_kernel(const PairPrepArgs a) {
  const int64_t pr = blockIdx.y;
  const int64_t npix = (int64_t)a.H * a.W;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npix) return;
  const int yy = (int)(p / a.W), xx = (int)(p - (int64_t)yy * a.W);
  float* x = a.x + pr * a.nb * npix;
  bool ok = true;
  for (int c = 0; c < a.nb; ++c) {
    float m;
    if (a.f == 0) {
      m = static_cast<const float*>(a.s2)[pr * a.pair_s2 + c * npix + p];
    } else {
      // hsr_block_mean's sum: float64, (dy, dx) order, divided by f^2 and stored as float32
      const int64_t Wf = (int64_t)a.W * a.f;
      const int64_t base = pr * a.pair_s2 + (int64_t)c * npix * a.f * a.f + (int64_t)yy * a.f * Wf + (int64_t)xx * a.f;
      double s = 0.0;
      bool bad = false;
      for (int dy = 0; dy < a.f; ++dy)
        for (int dx = 0; dx < a.f; ++dx) {
          const float v = pair_load(a.s2, a.s2_dtype, base + (int64_t)dy * Wf + dx);
          bad |= !finite_f32(v) || (a.use_s2_nodata && pair_close(v, a.s2_nodata));
          s += (double)v;
        }
      m = bad ? __builtin_nanf("") : (float)(s / (double)(a.f * a.f));
    }
    ok = ok && finite_f32(m) && !(a.use_s2_nodata && pair_close(m, a.s2_nodata));
    x[c * npix + p] = m;
  }
  float* y = a.y + pr * a.T * npix;
  for (int t = 0; t < a.T; ++t) {
    float v = pair_load(a.emit, a.emit_dtype, pr * a.pair_emit + (int64_t)a.bands[t] * npix + p);
    if (a.emit_dtype == 2) v = v == 65535.0f ? __builtin_nanf("") : v * 1e-4f;   // hsr_tile_decode_u16's rule
    ok = ok && finite_f32(v) && !(a.use_emit_nodata && pair_close(v, a.emit_nodata));
    y[t * npix + p] = v;
  }
  a.mask[pr * npix + p] = ok ? 1 : 0;
}

// One workgroup per pair: n = the mask's count, mean = sum / n, M2 = sum (x - mean)^2 over the masked pixels (float64; every
// thread walks the pixels p = tid + 1024 k in order, waves are joined by the xor butterfly, the 16 waves in wave order).
// stats (P, 1 + 2 nb) = [n, mean.., M2..] (PolyRidge.local_stats' layout), mean / scale (P, nb) = StandardScaler's (zero
// variance -> 1; a pair without training pixels: mean 0, scale 1), n_train (P) int64.
constexpr int kPairStatsThreads = 1024;

__device__ double pair_block_sum(double v, double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_sum(v);
  __syncthreads();                                 // red is reused by consecutive calls
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < kPairStatsThreads / 64; ++w) s += red[w];
  return s;
}

__global__ __launch_bounds__(kPairStatsThreads) void pair_stats_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask,
                                                                       int64_t npix, int nb, double* __restrict__ stats,
                                                                       double* __restrict__ mean_out, double* __restrict__ scale_out,
                                                                       int64_t* __restrict__ n_train) {
  __shared__ double red[kPairStatsThreads / 64];
  const int64_t pr = blockIdx.x;
  x += pr * nb * npix;
  mask += pr * npix;
  stats += pr * (1 + 2 * nb);
  mean_out += pr * nb;
  scale_out += pr * nb;
  double cnt = 0.0;
  for (int64_t p = threadIdx.x; p < npix; p += kPairStatsThreads) cnt += mask[p] ? 1.0 : 0.0;
  const double n = pair_block_sum(cnt, red);
  for (int c = 0; c < nb; ++c) {
    const float* xc = x + c * npix;
    double s1 = 0.0;
    for (int64_t p = threadIdx.x; p < npix; p += kPairStatsThreads)
      if (mask[p]) s1 += (double)xc[p];
    const double sum = pair_block_sum(s1, red);
    const double mean = n > 0.0 ? sum / n : 0.0;
    double s2 = 0.0;
    for (int64_t p = threadIdx.x; p < npix; p += kPairStatsThreads)
      if (mask[p]) {
        const double d = (double)xc[p] - mean;
        s2 += d * d;
      }
    const double m2 = pair_block_sum(s2, red);
    if (threadIdx.x == 0) {
      stats[1 + c] = mean;
      stats[1 + nb + c] = m2;
      mean_out[c] = mean;
      const double sc = n > 0.0 ? sqrt(m2 / n) : 0.0;
      scale_out[c] = sc == 0.0 ? 1.0 : sc;
    }
  }
  if (threadIdx.x == 0) {
    stats[0] = n;
    n_train[pr] = (int64_t)n;
  }
}

}  // namespace hsr

using namespace hsr;

extern "C" int hsr_pair_prep(const void* emit_dev, int32_t emit_dtype, int64_t pair_emit, int32_t emit_bands,
                             const int32_t* bands_dev, int32_t T, const void* s2_dev, int32_t s2_dtype, int64_t pair_s2,
                             int32_t nb, int32_t H, int32_t W, int32_t factor, float emit_nodata, int32_t use_emit_nodata,
                             float s2_nodata, int32_t use_s2_nodata, float* x_dev, float* y_dev, uint8_t* mask_dev,
                             int32_t npairs, hsr_stream_t stream) {
  HSR_REQUIRE(emit_dev && bands_dev && s2_dev && x_dev && y_dev && mask_dev, HSR_ERR_INVALID, "hsr_pair_prep: NULL pointer");
  HSR_REQUIRE(H >= 1 && W >= 1 && nb >= 1 && nb <= kPairMaxIn && T >= 1 && T <= emit_bands && factor >= 0 && factor <= 64 &&
              npairs >= 1 && npairs <= 65535, HSR_ERR_INVALID,
              "hsr_pair_prep: bad shape (nb=%d T=%d emit_bands=%d H=%d W=%d factor=%d P=%d)", nb, T, emit_bands, H, W, factor, npairs);
  HSR_REQUIRE((emit_dtype == 0 || emit_dtype == 2) && (s2_dtype == 0 || s2_dtype == 2) && (factor > 0 || s2_dtype == 0),
              HSR_ERR_UNSUPPORTED, "hsr_pair_prep: dtypes emit=%d s2=%d (0 float32, 2 uint16; a coarse S2 is float32)", emit_dtype,
              s2_dtype);
  const int64_t npix = (int64_t)H * W;
  HSR_REQUIRE(npairs == 1 || (pair_emit >= (int64_t)emit_bands * npix && pair_s2 >= (int64_t)nb * npix * factor * factor &&
                              pair_s2 >= (factor == 0 ? (int64_t)nb * npix : 0)),
              HSR_ERR_INVALID, "hsr_pair_prep: pair strides overlap");
  // the band indices are read on the device; their range is the caller's (s2_emit.pairs checks it on the host)
  PairPrepArgs a{emit_dev, s2_dev, bands_dev, x_dev, y_dev, mask_dev, pair_emit, pair_s2, emit_dtype, s2_dtype, nb, T, H, W,
                 factor, use_emit_nodata, use_s2_nodata, emit_nodata, s2_nodata};
  hipLaunchKernelGGL(pair_prep_kernel, dim3((unsigned)((npix + 255) / 256), (unsigned)npairs), dim3(256), 0, (hipStream_t)stream, a);
  HSR_LAUNCH_CHECK("pair_prep_kernel");
  return HSR_OK;
}

extern "C" int hsr_pair_stats(const float* x_dev, const uint8_t* mask_dev, int64_t npix, int32_t nb, double* stats_dev,
                              double* mean_dev, double* scale_dev, int64_t* n_train_dev, int32_t npairs, hsr_stream_t stream) {
  HSR_REQUIRE(x_dev && mask_dev && stats_dev && mean_dev && scale_dev && n_train_dev, HSR_ERR_INVALID,
              "hsr_pair_stats: NULL pointer");
  HSR_REQUIRE(npix >= 1 && nb >= 1 && nb <= kPairMaxIn && npairs >= 1 && npairs <= 65535, HSR_ERR_INVALID,
              "hsr_pair_stats: bad shape (npix=%lld nb=%d P=%d)", (long long)npix, nb, npairs);
  hipLaunchKernelGGL(pair_stats_kernel, dim3((unsigned)npairs), dim3(kPairStatsThreads), 0, (hipStream_t)stream, x_dev, mask_dev,
                     npix, nb, stats_dev, mean_dev, scale_dev, n_train_dev);
  HSR_LAUNCH_CHECK("pair_stats_kernel");
  return HSR_OK;
}
