// Tile pairs (s2_emit.fuse_tile_pairs): the front of the notebook's per-pair flow (legacy_notebooks/Spectral_matching.ipynb)
// for a batch of pairs, before the batched ridge fit of hsr_ridge.hip / hsr_gram.hip / hsr_chol.hip:
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
#include "hsr_tree_dev.h"

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

// Fit report (fuse_tile_pairs(report=True)): the notebook's cell 26 - predict the training pixels with the fitted model, sigmoid,
// per-band R^2 and RMSE against the decoded targets - on the expanded rows Q the fit has just read.  Columns 0 .. na-1 of a row of
// Q are [1 | phi | 0] (all zero for an untrained pixel), so the in-sample logit is Q[:, :na] . [b64; Bp[:nf]; 0], a
// (npix x na) . (na x T) product per pair on v_mfma_f64_16x16x4_f64; the cast, sigmoid, residual and masking run in the MFMA
// epilogue, in registers.
//   partial  grid (chunks, ceil(T / 32), P): a workgroup owns kRepRows rows (a plan that depends on npix only) and 32 bands;
//            each wave 4 strips of 16 rows x 2 band tiles.  The coefficient panel is staged in LDS kRepKc features at a time.
//            k order: MFMA step u of k-tile kt contracts features kt + 4 kk + u (kk = lane >> 4), so a lane reads 4
//            consecutive doubles of its row as two 16-byte loads and takes the coefficients of the same 4 features.
//            Per (pair, chunk, band) partial: [sum d^2, n, mean(yt), M2(yt)], every lane in a fixed order, lanes and waves
//            joined in a fixed order (Chan's merge).
//   finish   one workgroup per pair: the chunks merged in index order; r2 = 1 - ss_res / (M2 + 1e-8), rmse = sqrt(ss_res / n),
//            NaN for a pair whose status is not 0.
// A pair's numbers therefore depend on neither the batch size nor its position in the batch.
constexpr int kRepRows = 256;          // rows per chunk: 4 waves x 4 strips x 16
constexpr int kRepKc = 96;             // features per LDS coefficient panel (6 k-tiles)
constexpr int kRepLd = 36;             // panel row pitch in doubles: the kk = 0 / 1 halves of a wave read disjoint banks

typedef double rep_f64x4 __attribute__((ext_vector_type(4)));

struct PairReportArgs {
  const double* q;                     // (P, npix, ldq): [1 | phi | 0-pad] in columns 0 .. na-1
  const double* b64;                   // (P, T) intercepts
  const double* bp;                    // (P, >= nf, ldbp) coefficients on phi
  const float* y;                      // (P, T, npix) decoded targets
  const uint8_t* mask;                 // (P, npix) training mask
  double* work;                        // (P, pair_work): [chunk][T][4]
  int64_t ldq, pair_q, pair_b, ldbp, pair_bp, pair_y, pair_m, pair_work, npix;
  int32_t na, nf, T;
};

struct RepStat {
  double sd, n, mu, m2;
};

__device__ __forceinline__ RepStat rep_merge(RepStat a, RepStat b) {   // Chan et al.: a then b
  if (b.n == 0.0) {
    a.sd += b.sd;
    return a;
  }
  if (a.n == 0.0) {
    b.sd += a.sd;
    return b;
  }
  const double n = a.n + b.n, delta = b.mu - a.mu;
  return RepStat{a.sd + b.sd, n, a.mu + delta * (b.n / n), a.m2 + b.m2 + delta * delta * (a.n * b.n / n)};
}

__global__ __launch_bounds__(256) void pair_report_partial_kernel(const PairReportArgs a) {
  __shared__ __attribute__((aligned(16))) double lds[kRepKc * kRepLd];
  const int64_t pr = blockIdx.z;
  const int chunk = blockIdx.x, j0 = blockIdx.y * 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, kk = lane >> 4;
  const double* q = a.q + pr * a.pair_q;
  const double* b64 = a.b64 + pr * a.pair_b;
  const double* bp = a.bp + pr * a.pair_bp;
  const int64_t row_w = (int64_t)chunk * kRepRows + wave * 64;
  // A operand row of this lane in strip s: row_w + 16 s + c (clamped to row 0 past the end: its results are never used)
  const double* qrow[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int64_t r = row_w + 16 * s + c;
    qrow[s] = q + (r < a.npix ? r : 0) * a.ldq + 4 * kk;
  }
  rep_f64x4 acc[4][2];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[s][b] = rep_f64x4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < a.na; k0 += kRepKc) {
    const int kc = min(kRepKc, a.na - k0);
    __syncthreads();                                   // the previous panel is consumed
    for (int e = threadIdx.x; e < kc * 32; e += 256) {
      const int kr = e >> 5, jb = e & 31, k = k0 + kr, j = j0 + jb;
      double v = 0.0;
      if (j < a.T) v = k == 0 ? b64[j] : (k <= a.nf ? bp[(int64_t)(k - 1) * a.ldbp + j] : 0.0);
      lds[kr * kRepLd + jb] = v;
    }
    __syncthreads();
    for (int kt = 0; kt < kc; kt += 16) {
      double2 qa[4][2];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const double2* p = reinterpret_cast<const double2*>(qrow[s] + k0 + kt);
        qa[s][0] = p[0];
        qa[s][1] = p[1];
      }
      const double* pan = lds + (kt + 4 * kk) * kRepLd + c;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double b0 = pan[u * kRepLd], b1 = pan[u * kRepLd + 16];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double av = u == 0 ? qa[s][0].x : u == 1 ? qa[s][0].y : u == 2 ? qa[s][1].x : qa[s][1].y;
          acc[s][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b0, acc[s][0], 0, 0, 0);
          acc[s][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b1, acc[s][1], 0, 0, 0);
        }
      }
    }
  }
  // epilogue: D[row = kk + 4 g][col = c] (the f64 map) = pixel row_w + 16 s + kk + 4 g, band j0 + 16 b + c
  const float* y = a.y + pr * a.pair_y;
  const uint8_t* mask = a.mask + pr * a.pair_m;
  RepStat st[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t pix = row_w + 16 * s + kk + 4 * g;
      if (pix >= a.npix || !mask[pix]) continue;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int j = j0 + 16 * b + c;
        if (j >= a.T) continue;
        const float z = (float)acc[s][b][g];
        const float zc = z < -50.0f ? -50.0f : (z > 50.0f ? 50.0f : z);   // np.clip: NaN stays NaN
        const float yp = 1.0f / (1.0f + expf(-zc));
        const float yt = y[(int64_t)j * a.npix + pix];
        const float d = yt - yp;
        RepStat& r = st[b];
        r.sd += (double)d * (double)d;
        r.n += 1.0;
        const double delta = (double)yt - r.mu;
        r.mu += delta / r.n;
        r.m2 += delta * ((double)yt - r.mu);
      }
    }
  __syncthreads();                                     // the panel is free: it holds the 16 lane sets of 32 bands now
  RepStat* red = reinterpret_cast<RepStat*>(lds);      // [wave * 4 + kk][32]
#pragma unroll
  for (int b = 0; b < 2; ++b) red[(wave * 4 + kk) * 32 + 16 * b + c] = st[b];
  __syncthreads();
  if (threadIdx.x < 32 && j0 + (int)threadIdx.x < a.T) {
    RepStat r = red[threadIdx.x];
    for (int i = 1; i < 16; ++i) r = rep_merge(r, red[i * 32 + threadIdx.x]);
    double* out = a.work + pr * a.pair_work + ((int64_t)chunk * a.T + j0 + threadIdx.x) * 4;
    out[0] = r.sd;
    out[1] = r.n;
    out[2] = r.mu;
    out[3] = r.m2;
  }
}

__global__ __launch_bounds__(256) void pair_report_finish_kernel(const double* __restrict__ work, int64_t pair_work, int chunks,
                                                                 int T, const int32_t* __restrict__ status, double* __restrict__ r2,
                                                                 double* __restrict__ rmse, int64_t pair_out) {
  const int64_t pr = blockIdx.x;
  work += pr * pair_work;
  const bool ok = status[pr] == 0;
  for (int j = threadIdx.x; j < T; j += 256) {
    RepStat r{0.0, 0.0, 0.0, 0.0};
    for (int ch = 0; ch < chunks; ++ch) {
      const double* p = work + ((int64_t)ch * T + j) * 4;
      r = rep_merge(r, RepStat{p[0], p[1], p[2], p[3]});
    }
    const double nan = __builtin_nan("");
    r2[pr * pair_out + j] = ok ? 1.0 - r.sd / (r.m2 + 1e-8) : nan;
    rmse[pr * pair_out + j] = ok ? sqrt(r.sd / r.n) : nan;
  }
}

// Hold-out (fuse_tile_pairs(train_mask=...)): the fit's mask = the flatten rule's mask & the caller's, and the group code of every
// pixel for the validation score: 1 fit, 2 held out (valid but kept from the fit), 0 neither.
__global__ __launch_bounds__(256) void pair_holdout_kernel(const uint8_t* __restrict__ valid, const uint8_t* __restrict__ train,
                                                           int64_t pair_train, int64_t npix, uint8_t* __restrict__ mask,
                                                           uint8_t* __restrict__ group) {
  const int64_t pr = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npix) return;
  const bool v = valid[pr * npix + p] != 0, t = train[pr * pair_train + p] != 0;
  mask[pr * npix + p] = v && t ? 1 : 0;
  group[pr * npix + p] = v ? (t ? 1 : 2) : 0;
}

// Validation score (fuse_tile_pairs(validate=True)): one view of the prediction on the EMIT grid, pred (P, T, npix), against the
// decoded targets y (P, T, npix), for the two pixel groups of group (P, npix) at once.  Two reductions cross on the band-major
// layout - per band along the pixels (error statistics), per pixel along the bands (spectral angle) - and both are fed from ONE
// pass over pred and y:
//   partial  grid (chunks, P), one wave per workgroup.  A wave owns kScorePix consecutive pixels (a plan that depends on npix
//            only), a lane 4 kScoreVec of them as kScoreVec 16-byte loads per array and band (the vectorised instance; the plain
//            one loads the same pixels one by one with bounds checks: same lanes, same order, same bits).  The lane walks the
//            bands in order with its pixels' dot / |y|^2 / |p|^2 sums in registers (float64), and forms per band and group the
//            statistics of its own pixels: n, sum d^2, mean = sum / n and M2 = sum (y - mean)^2 - two passes over <= 8 values in
//            registers, so equal targets give M2 == 0 exactly.  A chunk without held-out pixels (always, without a train_mask)
//            takes an instance of the walk that computes the fit group only.  The 64 lane partials of kScoreBands bands are joined through LDS:
//            lane (band b, group g, segment s) merges lanes 8 s .. 8 s + 7 in lane order (Chan), three shuffle-down steps merge
//            the segments left to right, and the segment-0 lanes store the chunk's partial [sum d^2, n, mean, M2].  Angles: per
//            pixel at the end, float32 into sam_map, their float64 sum and count per group into the chunk's partial.
//   finish   one workgroup per pair, a thread per band: chunks merged in index order (their partials loaded four chunks ahead of
//            the merge chain); n, rmse, r2, mean_ref per band and group, ERGAS over the bands (a lane adds its bands in order,
//            lanes by the xor butterfly, waves in wave order), the mean angle.
// Every order depends on (npix, T) only: a pair's numbers depend on neither the batch size nor its position in the batch.
constexpr int kScoreVec = 2;                         // 16-byte loads per lane, array and band
constexpr int kScoreLanePix = 4 * kScoreVec;         // pixels of a lane
constexpr int kScorePix = 64 * kScoreLanePix;        // pixels of a chunk
constexpr int kScoreBands = 4;                       // bands per LDS join: 4 bands x 2 groups x 8 segments = 64 lanes
constexpr int kScoreHalf = 2;                        // bands per group of loads (kept one group ahead of the arithmetic)
constexpr int kScorePitch = 72;                      // 64 lane partials + one pad per 8: the 8 segments start on disjoint banks

struct PairScoreArgs {
  const float* pred;                   // (P, T, npix)
  const float* y;                      // (P, T, npix)
  const uint8_t* group;                // (P, npix): 0 skip, 1 fit, 2 held out
  double* work;                        // (P, pair_work): [chunk][T][2][4] then [chunk][2][2]
  float* sam_map;                      // (P, npix)
  int64_t pair_pred, pair_y, pair_group, pair_work, pair_map, npix;
  int32_t T, chunks;
};

// Chan's merge without branches: an empty side has mean 0 and M2 0, so its terms vanish (frac = 0, or delta * 1 from mean 0), and
// delta == 0 leaves mean and M2 + M2 untouched: equal targets keep M2 == 0 exactly.
__device__ __forceinline__ RepStat score_merge(const RepStat& a, const RepStat& b) {
  const double n = a.n + b.n, delta = b.mu - a.mu;
  const double frac = n > 0.0 ? b.n / n : 0.0;
  return RepStat{a.sd + b.sd, n, a.mu + delta * frac, a.m2 + b.m2 + delta * delta * (a.n * frac)};
}

struct ScoreLane {                     // what a lane keeps across the bands
  int64_t p0[kScoreVec];               // first pixel of each of its vectors
  int grp[kScoreLanePix];              // group code of each pixel (0 past the end)
  double dot[kScoreLanePix], sa[kScoreLanePix], sb[kScoreLanePix];
};

// Bands j0 and j0 + 1 of this lane's pixels (zeros past T and past npix).
template <bool kVec>
__device__ __forceinline__ void score_load(const PairScoreArgs& a, const float* __restrict__ pred, const float* __restrict__ y,
                                           const ScoreLane& L, int j0, float (&pv)[kScoreHalf][kScoreLanePix],
                                           float (&yv)[kScoreHalf][kScoreLanePix]) {
#pragma unroll
  for (int jj = 0; jj < kScoreHalf; ++jj) {
    const int j = j0 + jj;
#pragma unroll
    for (int v = 0; v < kScoreVec; ++v) {
      const int64_t off = (int64_t)j * a.npix + L.p0[v];
      if (kVec) {
        float4 p4 = make_float4(0.f, 0.f, 0.f, 0.f), y4 = p4;
        if (j < a.T && L.p0[v] < a.npix) {
          p4 = *reinterpret_cast<const float4*>(pred + off);
          y4 = *reinterpret_cast<const float4*>(y + off);
        }
        pv[jj][4 * v] = p4.x, pv[jj][4 * v + 1] = p4.y, pv[jj][4 * v + 2] = p4.z, pv[jj][4 * v + 3] = p4.w;
        yv[jj][4 * v] = y4.x, yv[jj][4 * v + 1] = y4.y, yv[jj][4 * v + 2] = y4.z, yv[jj][4 * v + 3] = y4.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool in = j < a.T && L.p0[v] + e < a.npix;
          pv[jj][4 * v + e] = in ? pred[off + e] : 0.f;
          yv[jj][4 * v + e] = in ? y[off + e] : 0.f;
        }
      }
    }
  }
}

// One band of this lane's pixels: the angle sums, and the lane's partial of each group into slot `slot` of the join.
// Products of two float32 values are exact in float64, so fma(x, y, s) below carries the bits of s + x * y.
template <int kGroups>
__device__ __forceinline__ void score_band(const float (&pv)[kScoreLanePix], const float (&yv)[kScoreLanePix], bool live, ScoreLane& L,
                                           RepStat* part, int slot) {
  const int lane = threadIdx.x;
  int n[kGroups];
  double sy[kGroups], sd[kGroups];
  bool in[kGroups][kScoreLanePix];
#pragma unroll
  for (int g = 0; g < kGroups; ++g) n[g] = 0, sy[g] = 0.0, sd[g] = 0.0;
#pragma unroll
  for (int e = 0; e < kScoreLanePix; ++e) {
    const float pe = pv[e], ye = yv[e];
    const bool f = live && __builtin_isfinite(pe) && __builtin_isfinite(ye);   // a band past T: empty partials
    const float d = ye - pe;
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
      const bool s = f && L.grp[e] == g + 1;
      in[g][e] = s;
      const float ds = s ? d : 0.f, ys = s ? ye : 0.f;
      n[g] += s ? 1 : 0;
      sy[g] += (double)ys;
      sd[g] = fma((double)ds, (double)ds, sd[g]);
    }
    const double y64 = ye, p64 = pe;                   // a band past T adds exact zeros
    L.dot[e] = fma(y64, p64, L.dot[e]);
    L.sa[e] = fma(y64, y64, L.sa[e]);
    L.sb[e] = fma(p64, p64, L.sb[e]);
  }
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    RepStat r{0.0, 0.0, 0.0, 0.0};
    if (g < kGroups) {
      const int gi = g < kGroups ? g : 0;
      const double nn = (double)n[gi];
      const double mu = nn > 0.0 ? sy[gi] / nn : 0.0;
      double m2 = 0.0;
#pragma unroll
      for (int e = 0; e < kScoreLanePix; ++e) {
        const double c = in[gi][e] ? (double)yv[e] - mu : 0.0;
        m2 = fma(c, c, m2);
      }
      r = RepStat{sd[gi], nn, mu, m2};
    }
    part[(slot * 2 + g) * kScorePitch + lane + (lane >> 3)] = r;
  }
}

// The walk over the bands for kGroups = 1 (no held-out pixel in the chunk: group 2's partials are empty without being computed)
// or 2.  Bands are loaded two at a time, one pair of bands ahead of the arithmetic, and joined four at a time.
template <bool kVec, int kGroups>
__device__ __forceinline__ void score_walk(const PairScoreArgs& a, const float* __restrict__ pred, const float* __restrict__ y,
                                           double* __restrict__ work, RepStat* part, ScoreLane& L) {
  const int chunk = blockIdx.x, lane = threadIdx.x;
  const int jb = lane >> 4, jg = (lane >> 3) & 1, seg = lane & 7;
  float pa[kScoreHalf][kScoreLanePix], ya[kScoreHalf][kScoreLanePix], pb[kScoreHalf][kScoreLanePix], yb[kScoreHalf][kScoreLanePix];
  score_load<kVec>(a, pred, y, L, 0, pa, ya);
  for (int j0 = 0; j0 < a.T; j0 += kScoreBands) {
    score_load<kVec>(a, pred, y, L, j0 + 2, pb, yb);
    __syncthreads();                                   // the previous join has read its partials
    score_band<kGroups>(pa[0], ya[0], j0 < a.T, L, part, 0);
    score_band<kGroups>(pa[1], ya[1], j0 + 1 < a.T, L, part, 1);
    score_load<kVec>(a, pred, y, L, j0 + 4, pa, ya);
    score_band<kGroups>(pb[0], yb[0], j0 + 2 < a.T, L, part, 2);
    score_band<kGroups>(pb[1], yb[1], j0 + 3 < a.T, L, part, 3);
    __syncthreads();
    const RepStat* src = part + (jb * 2 + jg) * kScorePitch + 9 * seg;
    RepStat r = src[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) r = score_merge(r, src[i]);
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) {            // segment 0 ends with ((0 1)(2 3))((4 5)(6 7))
      const RepStat o{__shfl_down(r.sd, off, 64), __shfl_down(r.n, off, 64), __shfl_down(r.mu, off, 64), __shfl_down(r.m2, off, 64)};
      r = score_merge(r, o);
    }
    if (seg == 0 && j0 + jb < a.T) {
      double* out = work + (((int64_t)chunk * a.T + j0 + jb) * 2 + jg) * 4;
      out[0] = r.sd;
      out[1] = r.n;
      out[2] = r.mu;
      out[3] = r.m2;
    }
  }
}

template <bool kVec>
__global__ __launch_bounds__(64) void pair_score_partial_kernel(const PairScoreArgs a) {
  __shared__ __attribute__((aligned(16))) RepStat part[kScoreBands * 2 * kScorePitch];
  const int64_t pr = blockIdx.y;
  const int chunk = blockIdx.x, lane = threadIdx.x;
  const float* pred = a.pred + pr * a.pair_pred;
  const float* y = a.y + pr * a.pair_y;
  const uint8_t* group = a.group + pr * a.pair_group;
  double* work = a.work + pr * a.pair_work;
  // pixel e of vector v of this lane: chunk kScorePix + 256 v + 4 lane + e
  ScoreLane L;
#pragma unroll
  for (int v = 0; v < kScoreVec; ++v) {
    L.p0[v] = (int64_t)chunk * kScorePix + 256 * v + 4 * lane;
    if (kVec) {                                        // npix % 4 == 0: a vector is inside or outside as a whole
      uchar4 g4 = make_uchar4(0, 0, 0, 0);
      if (L.p0[v] < a.npix) g4 = *reinterpret_cast<const uchar4*>(group + L.p0[v]);
      L.grp[4 * v] = g4.x;
      L.grp[4 * v + 1] = g4.y;
      L.grp[4 * v + 2] = g4.z;
      L.grp[4 * v + 3] = g4.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) L.grp[4 * v + e] = L.p0[v] + e < a.npix ? group[L.p0[v] + e] : 0;
    }
  }
  bool held = false;
#pragma unroll
  for (int e = 0; e < kScoreLanePix; ++e) {
    L.grp[e] = L.grp[e] == 1 || L.grp[e] == 2 ? L.grp[e] : 0;
    held = held || L.grp[e] == 2;
    L.dot[e] = L.sa[e] = L.sb[e] = 0.0;
  }
  if (__ballot(held) != 0)                             // the same for the whole wave
    score_walk<kVec, 2>(a, pred, y, work, part, L);
  else
    score_walk<kVec, 1>(a, pred, y, work, part, L);
  // spectral angles of this lane's pixels: a non-finite value in any band has made sa or sb non-finite
  double asum[2] = {0.0, 0.0}, acnt[2] = {0.0, 0.0};
  float ang32[kScoreLanePix];
#pragma unroll
  for (int e = 0; e < kScoreLanePix; ++e) {
    ang32[e] = __builtin_nanf("");
    if (L.grp[e] != 0 && __builtin_isfinite(L.sa[e]) && __builtin_isfinite(L.sb[e]) && L.sa[e] > 0.0 && L.sb[e] > 0.0) {
      double c = L.dot[e] / sqrt(L.sa[e] * L.sb[e]);
      c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
      const double ang = acos(c) * (180.0 / 3.14159265358979323846);
      ang32[e] = (float)ang;
      asum[L.grp[e] - 1] += ang;
      acnt[L.grp[e] - 1] += 1.0;
    }
  }
  float* map = a.sam_map + pr * a.pair_map;
#pragma unroll
  for (int v = 0; v < kScoreVec; ++v) {
    if (kVec) {
      if (L.p0[v] < a.npix)
        *reinterpret_cast<float4*>(map + L.p0[v]) = make_float4(ang32[4 * v], ang32[4 * v + 1], ang32[4 * v + 2], ang32[4 * v + 3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (L.p0[v] + e < a.npix) map[L.p0[v] + e] = ang32[4 * v + e];
    }
  }
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    asum[g] = wave_sum(asum[g]);
    acnt[g] = wave_sum(acnt[g]);
  }
  if (lane == 0) {
    double* out = work + (int64_t)a.chunks * a.T * 8 + (int64_t)chunk * 4;
    out[0] = asum[0];
    out[1] = acnt[0];
    out[2] = asum[1];
    out[3] = acnt[1];
  }
}

struct PairScoreOut {
  int64_t* n;                          // (P, pair_out): [group][T]
  double* rmse;
  double* r2;
  double* mean_ref;
  double* sam;                         // (P, pair_sam): [group]
  int64_t* n_sam;
  double* ergas;
  int64_t pair_out, pair_sam;
};

constexpr int kScoreFinishThreads = 512;
constexpr int kScoreFinishAhead = 4;   // chunks whose partials are loaded before their merges: the loads do not wait for the chain

__global__ __launch_bounds__(kScoreFinishThreads) void pair_score_finish_kernel(const double* __restrict__ work, int64_t pair_work,
                                                                                 int chunks, int T, double ergas_scale,
                                                                                 const PairScoreOut o) {
  __shared__ double red[2][2][kScoreFinishThreads / 64];
  const int64_t pr = blockIdx.x;
  work += pr * pair_work;
  const double nan = __builtin_nan("");
  double es[2] = {0.0, 0.0}, ec[2] = {0.0, 0.0};
  for (int j = threadIdx.x; j < T; j += kScoreFinishThreads) {
    RepStat r[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    for (int c0 = 0; c0 < chunks; c0 += kScoreFinishAhead) {
      double2 buf[kScoreFinishAhead][4];                 // [chunk][group 0: sd n | mu m2 | group 1: sd n | mu m2]
#pragma unroll
      for (int u = 0; u < kScoreFinishAhead; ++u)
        if (c0 + u < chunks) {
          const double2* p = reinterpret_cast<const double2*>(work + ((int64_t)(c0 + u) * T + j) * 8);
#pragma unroll
          for (int q = 0; q < 4; ++q) buf[u][q] = p[q];
        }
#pragma unroll
      for (int u = 0; u < kScoreFinishAhead; ++u)
        if (c0 + u < chunks) {
#pragma unroll
          for (int g = 0; g < 2; ++g)
            r[g] = score_merge(r[g], RepStat{buf[u][2 * g].x, buf[u][2 * g].y, buf[u][2 * g + 1].x, buf[u][2 * g + 1].y});
        }
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const bool ok = r[g].n > 0.0;
      const double rm = ok ? sqrt(r[g].sd / r[g].n) : nan;
      const int64_t at = pr * o.pair_out + (int64_t)g * T + j;
      o.n[at] = (int64_t)r[g].n;
      o.rmse[at] = rm;
      o.r2[at] = ok ? 1.0 - r[g].sd / (r[g].m2 + 1e-8) : nan;
      o.mean_ref[at] = ok ? r[g].mu : nan;
      if (ok && r[g].mu != 0.0) {
        const double q = rm / r[g].mu;
        es[g] += q * q;
        ec[g] += 1.0;
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int g = 0; g < 2; ++g) {
    const double s = wave_sum(es[g]), c = wave_sum(ec[g]);
    if (lane == 0) {
      red[g][0][wave] = s;
      red[g][1][wave] = c;
    }
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int g = threadIdx.x;
    double s = 0.0, c = 0.0;
    for (int w = 0; w < kScoreFinishThreads / 64; ++w) {
      s += red[g][0][w];
      c += red[g][1][w];
    }
    o.ergas[pr * o.pair_sam + g] = c > 0.0 ? ergas_scale * sqrt(s / c) : nan;
    const double* ap = work + (int64_t)chunks * T * 8;
    double as = 0.0, an = 0.0;
    for (int ch = 0; ch < chunks; ++ch) {
      as += ap[(int64_t)ch * 4 + 2 * g];
      an += ap[(int64_t)ch * 4 + 2 * g + 1];
    }
    o.sam[pr * o.pair_sam + g] = an > 0.0 ? as / an : nan;
    o.n_sam[pr * o.pair_sam + g] = (int64_t)an;
  }
}

// Pooled models (fuse_tile_pairs(pool=...)): M groups of pairs share one model each.  Membership is two small arrays the host
// builds: order (P) = the pairs sorted by (group, pair index), start (M + 1) = each group's slice of order; group_of (P) is the
// inverse map.  Every merge walks a group's members in pair-index order, skips a member whose stats[0] (its training pixels) is 0
// and COPIES the first non-empty member, so a singleton group, and a group with empty members, carries the bits of the group
// without them.  A pair index outside [0, P), a group id outside [0, M) or a slice outside [0, P] is skipped, never dereferenced.
//   pool stats   one wave per group, lane c owns band c: [n, mean.., M2..] of the members merged by Chan's update (as
//                PolyRidge.combine_stats / rep_merge write it); the group's mean and scale go to the group (M, nb) arrays and to
//                every member's row of the pair (P, nb) arrays, which hsr_pair_expand_f64 then reads as it reads hsr_pair_stats'.
//   pool gram    grid (chunks of elements, M): a thread owns its elements for the whole walk and adds the members' values in
//                order (float64), four members' loads in flight ahead of the adds; 16-byte loads in the vector instance.
//   pool models  grid (chunks, P): pair p gets its group's fitted model - Bp rows [0, nf) (zero rows up to npad), b64, W32, b32,
//                mean32, inv32 - its status word and the report's (non-zero for a failed group or a pair without training pixels).
constexpr int kPoolAhead = 4;                      // members whose loads are issued before their adds
constexpr int kPoolGramThreads = 256;

__device__ __forceinline__ void pool_slice(const int32_t* __restrict__ start, int g, int P, int& k0, int& k1) {
  k0 = start[g];
  k1 = start[g + 1];
  k0 = k0 < 0 ? 0 : (k0 > P ? P : k0);
  k1 = k1 < k0 ? k0 : (k1 > P ? P : k1);
}

__global__ __launch_bounds__(64) void pool_stats_kernel(const double* __restrict__ stats, int nb, int P,
                                                        const int32_t* __restrict__ order, const int32_t* __restrict__ start,
                                                        double* __restrict__ gstats, int64_t* __restrict__ n_pool,
                                                        double* __restrict__ gmean, double* __restrict__ gscale,
                                                        double* __restrict__ mean_out, double* __restrict__ scale_out) {
  const int g = blockIdx.x, c = threadIdx.x;
  if (c >= nb) return;
  const int ls = 1 + 2 * nb;
  int k0, k1;
  pool_slice(start, g, P, k0, k1);
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int k = k0; k < k1; ++k) {
    const int p = order[k];
    if (p < 0 || p >= P) continue;
    const double* s = stats + (int64_t)p * ls;
    const double nb_ = s[0];
    if (nb_ == 0.0) continue;
    const double mb = s[1 + c], m2b = s[1 + nb + c];
    if (n == 0.0) {
      n = nb_, mean = mb, m2 = m2b;
      continue;
    }
    const double tot = n + nb_, delta = mb - mean;
    mean += delta * (nb_ / tot);
    m2 = m2 + m2b + delta * delta * (n * nb_ / tot);
    n = tot;
  }
  const double sc = n > 0.0 ? sqrt(m2 / n) : 0.0;
  const double scale = sc == 0.0 ? 1.0 : sc;
  gstats[(int64_t)g * ls + 1 + c] = mean;
  gstats[(int64_t)g * ls + 1 + nb + c] = m2;
  gmean[(int64_t)g * nb + c] = mean;
  gscale[(int64_t)g * nb + c] = scale;
  if (c == 0) {
    gstats[(int64_t)g * ls] = n;
    n_pool[g] = (int64_t)n;
  }
  for (int k = k0; k < k1; ++k) {
    const int p = order[k];
    if (p < 0 || p >= P) continue;
    mean_out[(int64_t)p * nb + c] = mean;
    scale_out[(int64_t)p * nb + c] = scale;
  }
}

template <bool kVec>
__global__ __launch_bounds__(kPoolGramThreads) void pool_gram_kernel(const double* __restrict__ gsrc, int64_t pair_g, int64_t n_elems,
                                                                     const double* __restrict__ cnt, int64_t pair_n, int P,
                                                                     const int32_t* __restrict__ order,
                                                                     const int32_t* __restrict__ start, double* __restrict__ out,
                                                                     int64_t group_out) {
  const int g = blockIdx.y;
  const int64_t e0 = ((int64_t)blockIdx.x * kPoolGramThreads + threadIdx.x) * 2;   // this thread's elements: e0, e0 + 1
  if (e0 >= n_elems) return;
  const bool two = e0 + 1 < n_elems;               // always, in the vector instance (n_elems is even there)
  int k0, k1;
  pool_slice(start, g, P, k0, k1);
  double ax = 0.0, ay = 0.0;
  bool first = true;
  for (int k = k0; k < k1; k += kPoolAhead) {
    double vx[kPoolAhead], vy[kPoolAhead];
    bool use[kPoolAhead];
#pragma unroll
    for (int u = 0; u < kPoolAhead; ++u) {
      use[u] = false;
      vx[u] = vy[u] = 0.0;
      if (k + u >= k1) continue;
      const int p = order[k + u];
      if (p < 0 || p >= P || cnt[(int64_t)p * pair_n] == 0.0) continue;
      use[u] = true;
      const double* src = gsrc + (int64_t)p * pair_g + e0;
      if (kVec) {
        const double2 v = *reinterpret_cast<const double2*>(src);
        vx[u] = v.x, vy[u] = v.y;
      } else {
        vx[u] = src[0];
        if (two) vy[u] = src[1];
      }
    }
#pragma unroll
    for (int u = 0; u < kPoolAhead; ++u) {
      if (!use[u]) continue;
      ax = first ? vx[u] : ax + vx[u];
      ay = first ? vy[u] : ay + vy[u];
      first = false;
    }
  }
  double* dst = out + (int64_t)g * group_out + e0;
  if (kVec) {
    *reinterpret_cast<double2*>(dst) = make_double2(ax, ay);
  } else {
    dst[0] = ax;
    if (two) dst[1] = ay;
  }
}

struct PoolModelArgs {
  const double* g_bp;                  // (M, >= nf rows, T) group models; group strides below
  const double* g_b64;                 // (M, T)
  const float* g_w32;                  // (M, kpad, T)
  const float* g_b32;                  // (M, T)
  const float* g_mean32;               // (M, nb)
  const float* g_inv32;                // (M, nb)
  const int32_t* pool_status;          // (M)
  const int64_t* n_train;              // (P)
  const int32_t* group_of;             // (P)
  double* bp;                          // (P, npad, T) and the rest per pair, contiguous
  double* b64;
  float* w32;
  float* b32;
  float* mean32;
  float* inv32;
  int32_t* status;                     // (P)
  int32_t* report_status;              // (P)
  int64_t group_bp, group_w32;         // element strides between groups of g_bp and g_w32
  int32_t nf, npad, kpad, T, nb, M;
};

__global__ __launch_bounds__(256) void pool_models_kernel(const PoolModelArgs a) {
  const int64_t pr = blockIdx.y;
  const int g = a.group_of[pr];
  if (g < 0 || g >= a.M) return;
  const int64_t nbp = (int64_t)a.npad * a.T, nw = (int64_t)a.kpad * a.T;
  const int64_t o_b64 = nbp, o_w = o_b64 + a.T, o_b32 = o_w + nw, o_mean = o_b32 + a.T, o_inv = o_mean + a.nb, total = o_inv + a.nb;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    if (e < o_b64) {
      a.bp[pr * nbp + e] = e < (int64_t)a.nf * a.T ? a.g_bp[g * a.group_bp + e] : 0.0;
    } else if (e < o_w) {
      a.b64[pr * a.T + (e - o_b64)] = a.g_b64[(int64_t)g * a.T + (e - o_b64)];
    } else if (e < o_b32) {
      a.w32[pr * nw + (e - o_w)] = a.g_w32[g * a.group_w32 + (e - o_w)];
    } else if (e < o_mean) {
      a.b32[pr * a.T + (e - o_b32)] = a.g_b32[(int64_t)g * a.T + (e - o_b32)];
    } else if (e < o_inv) {
      a.mean32[pr * a.nb + (e - o_mean)] = a.g_mean32[(int64_t)g * a.nb + (e - o_mean)];
    } else {
      a.inv32[pr * a.nb + (e - o_inv)] = a.g_inv32[(int64_t)g * a.nb + (e - o_inv)];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int32_t s = a.pool_status[g];
    a.status[pr] = s;
    a.report_status[pr] = s != 0 ? s : (a.n_train[pr] == 0 ? 1 : 0);
  }
}

}  // namespace hsr

using namespace hsr;

// HSR_LAUNCH_CHECK that also appends the instance to the calling thread's record (hsr_pairs_last_launch) on success
#define HSR_PAIRS_LAUNCHED(name, instance)                                    \
  do {                                                                        \
    int rc_ = hsr::launched(hsr::kLaunchPairs, name " launch", (instance));   \
    if (rc_ != HSR_OK) return rc_;                                            \
  } while (0)

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
  HSR_PAIRS_LAUNCHED("pair_prep_kernel", kPairsPrep);
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
  HSR_PAIRS_LAUNCHED("pair_stats_kernel", kPairsStats);
  return HSR_OK;
}

extern "C" size_t hsr_pair_report_work_bytes(int64_t npix, int32_t T) {
  if (npix < 1 || T < 1) return 0;
  return (size_t)((npix + kRepRows - 1) / kRepRows) * (size_t)T * 4 * sizeof(double);
}

extern "C" int hsr_pair_report_f64(const double* q_dev, int64_t ldq, int64_t pair_q, int32_t na, int64_t npix, const double* b64_dev,
                                   int64_t pair_b, const double* bp_dev, int64_t ldbp, int64_t pair_bp, int32_t nf,
                                   const float* y_dev, int64_t pair_y, const uint8_t* mask_dev, int64_t pair_m, int32_t T,
                                   const int32_t* status_dev, double* work_dev, int64_t pair_work, double* r2_dev,
                                   double* rmse_dev, int64_t pair_out, int32_t npairs, hsr_stream_t stream) {
  HSR_REQUIRE(q_dev && b64_dev && bp_dev && y_dev && mask_dev && status_dev && work_dev && r2_dev && rmse_dev, HSR_ERR_INVALID,
              "hsr_pair_report_f64: NULL pointer");
  HSR_REQUIRE(npix >= 1 && T >= 1 && nf >= 1 && na >= nf + 1 && na % 16 == 0 && ldq >= na && ldbp >= T && npairs >= 1 &&
              npairs <= 65535, HSR_ERR_INVALID, "hsr_pair_report_f64: bad shape (npix=%lld na=%d nf=%d T=%d ldq=%lld P=%d)",
              (long long)npix, na, nf, T, (long long)ldq, npairs);
  const int64_t chunks = (npix + kRepRows - 1) / kRepRows;
  HSR_REQUIRE(chunks <= 0x7fffffff, HSR_ERR_UNSUPPORTED, "hsr_pair_report_f64: npix=%lld too large", (long long)npix);
  HSR_REQUIRE(pair_work >= chunks * T * 4, HSR_ERR_INVALID, "hsr_pair_report_f64: pair_work below hsr_pair_report_work_bytes / 8");
  HSR_REQUIRE(npairs == 1 || (pair_q >= npix * ldq && pair_b >= T && pair_bp >= (int64_t)nf * ldbp && pair_y >= (int64_t)T * npix &&
                              pair_m >= npix && pair_out >= T),
              HSR_ERR_INVALID, "hsr_pair_report_f64: pair strides overlap");
  // two 16-byte loads per lane and k-tile: rows and pairs of Q on 16-byte boundaries
  HSR_REQUIRE(((uintptr_t)q_dev & 15) == 0 && ldq % 2 == 0 && pair_q % 2 == 0, HSR_ERR_UNSUPPORTED,
              "hsr_pair_report_f64: needs 16-byte aligned rows of Q");
  PairReportArgs a{q_dev, b64_dev, bp_dev, y_dev, mask_dev, work_dev, ldq, pair_q, pair_b, ldbp, pair_bp, pair_y, pair_m,
                   pair_work, npix, na, nf, T};
  hipLaunchKernelGGL(pair_report_partial_kernel, dim3((unsigned)chunks, (unsigned)((T + 31) / 32), (unsigned)npairs), dim3(256), 0,
                     (hipStream_t)stream, a);
  HSR_PAIRS_LAUNCHED("pair_report_partial_kernel", kPairsReportPartial);
  hipLaunchKernelGGL(pair_report_finish_kernel, dim3((unsigned)npairs), dim3(256), 0, (hipStream_t)stream, work_dev,
                     pair_work, (int)chunks, T, status_dev, r2_dev, rmse_dev, pair_out);
  HSR_PAIRS_LAUNCHED("pair_report_finish_kernel", kPairsReportFinish);
  return HSR_OK;
}

extern "C" int hsr_pair_holdout(const uint8_t* valid_dev, const uint8_t* train_dev, int64_t pair_train, int64_t npix,
                                uint8_t* mask_dev, uint8_t* group_dev, int32_t npairs, hsr_stream_t stream) {
  HSR_REQUIRE(valid_dev && train_dev && mask_dev && group_dev, HSR_ERR_INVALID, "hsr_pair_holdout: NULL pointer");
  HSR_REQUIRE(npix >= 1 && npix <= (int64_t)0x7fffffff * 256 && npairs >= 1 && npairs <= 65535 && (npairs == 1 || pair_train >= npix),
              HSR_ERR_INVALID, "hsr_pair_holdout: bad shape (npix=%lld pair_train=%lld P=%d)", (long long)npix, (long long)pair_train,
              npairs);
  hipLaunchKernelGGL(pair_holdout_kernel, dim3((unsigned)((npix + 255) / 256), (unsigned)npairs), dim3(256), 0, (hipStream_t)stream,
                     valid_dev, train_dev, pair_train, npix, mask_dev, group_dev);
  HSR_PAIRS_LAUNCHED("pair_holdout_kernel", kPairsHoldout);
  return HSR_OK;
}

extern "C" size_t hsr_pair_score_work_bytes(int64_t npix, int32_t T) {
  if (npix < 1 || T < 1) return 0;
  return (size_t)((npix + kScorePix - 1) / kScorePix) * ((size_t)T * 8 + 4) * sizeof(double);
}

extern "C" int hsr_pair_score_f64(const float* pred_dev, int64_t pair_pred, const float* y_dev, int64_t pair_y,
                                  const uint8_t* group_dev, int64_t pair_group, int64_t npix, int32_t T, double ergas_scale,
                                  double* work_dev, int64_t pair_work, int64_t* n_dev, double* rmse_dev, double* r2_dev,
                                  double* mean_ref_dev, int64_t pair_out, double* sam_dev, int64_t* n_sam_dev, double* ergas_dev,
                                  int64_t pair_sam, float* sam_map_dev, int64_t pair_map, int32_t npairs, hsr_stream_t stream) {
  HSR_REQUIRE(pred_dev && y_dev && group_dev && work_dev && n_dev && rmse_dev && r2_dev && mean_ref_dev && sam_dev && n_sam_dev &&
              ergas_dev && sam_map_dev, HSR_ERR_INVALID, "hsr_pair_score_f64: NULL pointer");
  HSR_REQUIRE(npix >= 1 && T >= 1 && npairs >= 1 && npairs <= 65535, HSR_ERR_INVALID,
              "hsr_pair_score_f64: bad shape (npix=%lld T=%d P=%d)", (long long)npix, T, npairs);
  const int64_t chunks = (npix + kScorePix - 1) / kScorePix;
  HSR_REQUIRE(chunks <= 0x7fffffff, HSR_ERR_UNSUPPORTED, "hsr_pair_score_f64: npix=%lld too large", (long long)npix);
  HSR_REQUIRE(pair_work >= chunks * ((int64_t)T * 8 + 4), HSR_ERR_INVALID,
              "hsr_pair_score_f64: pair_work below hsr_pair_score_work_bytes / 8");
  HSR_REQUIRE(((uintptr_t)work_dev & 15) == 0 && pair_work % 2 == 0, HSR_ERR_UNSUPPORTED,
              "hsr_pair_score_f64: needs a 16-byte aligned workspace and an even pair_work");
  HSR_REQUIRE(npairs == 1 || (pair_pred >= (int64_t)T * npix && pair_y >= (int64_t)T * npix && pair_group >= npix &&
                              pair_out >= 2 * (int64_t)T && pair_sam >= 2 && pair_map >= npix),
              HSR_ERR_INVALID, "hsr_pair_score_f64: pair strides overlap");
  PairScoreArgs a{pred_dev, y_dev, group_dev, work_dev, sam_map_dev, pair_pred, pair_y, pair_group, pair_work, pair_map, npix, T,
                  (int32_t)chunks};
  // 16-byte loads and stores need band rows that start 16-byte aligned in every array; anything else takes the plain instance
  const bool vec = npix % 4 == 0 && pair_pred % 4 == 0 && pair_y % 4 == 0 && pair_group % 4 == 0 && pair_map % 4 == 0 &&
                   ((uintptr_t)pred_dev & 15) == 0 && ((uintptr_t)y_dev & 15) == 0 && ((uintptr_t)group_dev & 3) == 0 &&
                   ((uintptr_t)sam_map_dev & 15) == 0;
  const dim3 grid((unsigned)chunks, (unsigned)npairs);
  if (vec)
    hipLaunchKernelGGL(pair_score_partial_kernel<true>, grid, dim3(64), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(pair_score_partial_kernel<false>, grid, dim3(64), 0, (hipStream_t)stream, a);
  HSR_PAIRS_LAUNCHED("pair_score_partial_kernel", kPairsScorePartial + (vec ? 1 : 0));
  const PairScoreOut o{n_dev, rmse_dev, r2_dev, mean_ref_dev, sam_dev, n_sam_dev, ergas_dev, pair_out, pair_sam};
  hipLaunchKernelGGL(pair_score_finish_kernel, dim3((unsigned)npairs), dim3(kScoreFinishThreads), 0, (hipStream_t)stream, work_dev, pair_work,
                     (int)chunks, T, ergas_scale, o);
  HSR_PAIRS_LAUNCHED("pair_score_finish_kernel", kPairsScoreFinish);
  return HSR_OK;
}

extern "C" int hsr_pool_stats(const double* stats_dev, int32_t nb, int32_t npairs, const int32_t* order_dev, const int32_t* start_dev,
                              int32_t ngroups, double* gstats_dev, int64_t* n_pool_dev, double* gmean_dev, double* gscale_dev,
                              double* mean_dev, double* scale_dev, hsr_stream_t stream) {
  HSR_REQUIRE(stats_dev && order_dev && start_dev && gstats_dev && n_pool_dev && gmean_dev && gscale_dev && mean_dev && scale_dev,
              HSR_ERR_INVALID, "hsr_pool_stats: NULL pointer");
  HSR_REQUIRE(nb >= 1 && nb <= kPairMaxIn && npairs >= 1 && npairs <= 65535 && ngroups >= 1 && ngroups <= npairs, HSR_ERR_INVALID,
              "hsr_pool_stats: bad shape (nb=%d P=%d M=%d)", nb, npairs, ngroups);
  hipLaunchKernelGGL(pool_stats_kernel, dim3((unsigned)ngroups), dim3(64), 0, (hipStream_t)stream, stats_dev, nb, npairs, order_dev,
                     start_dev, gstats_dev, n_pool_dev, gmean_dev, gscale_dev, mean_dev, scale_dev);
  HSR_PAIRS_LAUNCHED("pool_stats_kernel", kPairsPoolStats);
  return HSR_OK;
}

extern "C" int hsr_pool_gram(const double* g_dev, int64_t pair_g, int64_t n_elems, const double* count_dev, int64_t pair_count,
                             int32_t npairs, const int32_t* order_dev, const int32_t* start_dev, int32_t ngroups, double* out_dev,
                             int64_t group_out, hsr_stream_t stream) {
  HSR_REQUIRE(g_dev && count_dev && order_dev && start_dev && out_dev, HSR_ERR_INVALID, "hsr_pool_gram: NULL pointer");
  HSR_REQUIRE(n_elems >= 1 && npairs >= 1 && npairs <= 65535 && ngroups >= 1 && ngroups <= npairs && pair_count >= 1,
              HSR_ERR_INVALID, "hsr_pool_gram: bad shape (n_elems=%lld P=%d M=%d)", (long long)n_elems, npairs, ngroups);
  HSR_REQUIRE((npairs == 1 || pair_g >= n_elems) && (ngroups == 1 || group_out >= n_elems), HSR_ERR_INVALID,
              "hsr_pool_gram: strides overlap");
  const int64_t chunks = (n_elems + 2 * kPoolGramThreads - 1) / (2 * kPoolGramThreads);
  HSR_REQUIRE(chunks <= 0x7fffffff, HSR_ERR_UNSUPPORTED, "hsr_pool_gram: n_elems=%lld too large", (long long)n_elems);
  // a 16-byte load per thread and member needs even sizes and strides and aligned bases; anything else takes the plain instance
  const bool vec = n_elems % 2 == 0 && pair_g % 2 == 0 && group_out % 2 == 0 && ((uintptr_t)g_dev & 15) == 0 &&
                   ((uintptr_t)out_dev & 15) == 0;
  const dim3 grid((unsigned)chunks, (unsigned)ngroups);
  if (vec)
    hipLaunchKernelGGL(pool_gram_kernel<true>, grid, dim3(kPoolGramThreads), 0, (hipStream_t)stream, g_dev, pair_g, n_elems,
                       count_dev, pair_count, npairs, order_dev, start_dev, out_dev, group_out);
  else
    hipLaunchKernelGGL(pool_gram_kernel<false>, grid, dim3(kPoolGramThreads), 0, (hipStream_t)stream, g_dev, pair_g, n_elems,
                       count_dev, pair_count, npairs, order_dev, start_dev, out_dev, group_out);
  HSR_PAIRS_LAUNCHED("pool_gram_kernel", kPairsPoolGram + (vec ? 1 : 0));
  return HSR_OK;
}

extern "C" int hsr_pool_models(const double* gbp_dev, int64_t group_bp, const double* gb64_dev, const float* gw32_dev,
                               int64_t group_w32, const float* gb32_dev, const float* gmean32_dev, const float* ginv32_dev,
                               const int32_t* pool_status_dev, const int64_t* n_train_dev, const int32_t* group_of_dev, int32_t nf,
                               int32_t npad, int32_t kpad, int32_t T, int32_t nb, double* bp_dev, double* b64_dev, float* w32_dev,
                               float* b32_dev, float* mean32_dev, float* inv32_dev, int32_t* status_dev, int32_t* report_status_dev,
                               int32_t npairs, int32_t ngroups, hsr_stream_t stream) {
  HSR_REQUIRE(gbp_dev && gb64_dev && gw32_dev && gb32_dev && gmean32_dev && ginv32_dev && pool_status_dev && n_train_dev &&
              group_of_dev && bp_dev && b64_dev && w32_dev && b32_dev && mean32_dev && inv32_dev && status_dev && report_status_dev,
              HSR_ERR_INVALID, "hsr_pool_models: NULL pointer");
  HSR_REQUIRE(nf >= 1 && npad >= nf && kpad >= nf && T >= 1 && nb >= 1 && nb <= kPairMaxIn && npairs >= 1 && npairs <= 65535 &&
              ngroups >= 1 && ngroups <= npairs, HSR_ERR_INVALID,
              "hsr_pool_models: bad shape (nf=%d npad=%d kpad=%d T=%d nb=%d P=%d M=%d)", nf, npad, kpad, T, nb, npairs, ngroups);
  HSR_REQUIRE(ngroups == 1 || (group_bp >= (int64_t)nf * T && group_w32 >= (int64_t)kpad * T), HSR_ERR_INVALID,
              "hsr_pool_models: group strides overlap");
  const PoolModelArgs a{gbp_dev, gb64_dev, gw32_dev, gb32_dev, gmean32_dev, ginv32_dev, pool_status_dev, n_train_dev, group_of_dev,
                        bp_dev, b64_dev, w32_dev, b32_dev, mean32_dev, inv32_dev, status_dev, report_status_dev, group_bp, group_w32,
                        nf, npad, kpad, T, nb, ngroups};
  const int64_t total = (int64_t)npad * T + (int64_t)kpad * T + 2 * (int64_t)T + 2 * nb;
  const int64_t blocks = (total + 1023) / 1024;              // 4 elements per thread, at most 64 blocks per pair
  hipLaunchKernelGGL(pool_models_kernel, dim3((unsigned)(blocks < 64 ? blocks : 64), (unsigned)npairs), dim3(256), 0,
                     (hipStream_t)stream, a);
  HSR_PAIRS_LAUNCHED("pool_models_kernel", kPairsPoolModels);
  return HSR_OK;
}
