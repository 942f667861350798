// Scene pairs (s2_emit.scenes): the front and the back of the tile-pair flow, on whole co-registered scenes.
//   black counts  tiles_helpers/utils.py:201-220 (is_black_mask) over every window of the regular grid that
//                 find_valid_paired_tiles (:223-305) walks: the number of black pixels per window.  A pixel is black when ONE of
//                 three predicates holds in EVERY band (all close to nodata | all close to masked_val | all |v| < zero_atol),
//                 so a lane carries three live flags and a valid pixel is decided by its first band: the band loop ends for the
//                 wave as soon as no lane has a live flag.
//   gather        the windows of a scene -> the (P, bands, th, tw) stack that fuse_tile_pairs takes, optionally quantised by
//                 save_tile_pair's rule (:362-374, encode_sample of hsr_common.h: the bits of hsr_tile_encode_u16).
//   mosaic        (P, T, th, tw) tile cubes -> the (T, H, W) scene grid in one pass over the output: every byte is written once.
//   blend         the same for windows that overlap on a lattice: a pixel is the tent-weighted mean of the cubes over it, still
//                 one pass over the output (nothing in the reference: its tiles never go back onto the scene grid).
// A scene is band-sequential (bands, H, W); dtype codes as hsr_pair_prep: 0 float32, 2 uint16.
#include "hsr_common.h"

#include <math.h>

namespace hsr {

// ---- black counts ----------------------------------------------------------------------------------------------------------
// np.isclose(arr, v, atol=a) with v a Python float, as NumPy 2 evaluates it: (|x - v| <= a + 1e-5 |v|) & isfinite(v) | (x == v).
// float32 scenes stay float32 (v and the tolerance are rounded to float32 once, on the host); integer scenes promote to float64.
// A non-finite v has tol = -1: only x == v is left.
template <typename T>
struct BlackRule;

template <>
struct BlackRule<float> {
  float nd, nd_tol, mk, mk_tol, zero;
  __device__ __forceinline__ void apply(float x, bool& f_nd, bool& f_mk, bool& f_zr) const {
    f_nd &= (fabsf(x - nd) <= nd_tol) | (x == nd);     // bitwise on purpose: no branches in the band loop
    f_mk &= (fabsf(x - mk) <= mk_tol) | (x == mk);
    f_zr &= fabsf(x) < zero;
  }
};

template <>
struct BlackRule<uint16_t> {
  double nd, nd_tol, mk, mk_tol, zero;
  __device__ __forceinline__ void apply(uint16_t u, bool& f_nd, bool& f_mk, bool& f_zr) const {
    const double x = (double)u;
    f_nd &= (fabs(x - nd) <= nd_tol) | (x == nd);
    f_mk &= (fabs(x - mk) <= mk_tol) | (x == mk);
    f_zr &= x < zero;
  }
};

constexpr int kScanAhead = 8;          // bands whose loads are in flight between two checks of the live flags

template <typename T>
struct SceneScanArgs {
  const T* scene;                      // (bands, H, W)
  int32_t* counts;                     // (ny, nx), zeroed before the launch
  BlackRule<T> rule;
  int64_t plane;                       // H W
  int32_t bands, W, tile_h, tile_w, ny, nx, use_nodata, rows;
};

// grid (ceil(nx tile_w / 256), ceil(covered rows / rows)): a wave owns 64 consecutive x (256 B per band for float32) of `rows`
// consecutive covered rows; pixels right of and below the last window are never read.  Band 0 is tested alone - it decides
// every valid pixel - and the others kScanAhead at a time, so a black region is not a chain of dependent round trips.  The
// black lanes of a wave are counted per window by ballot + popcount, and the wave keeps the counts of the two windows it met
// last in registers across its rows: one integer atomic per wave and window it leaves, however many windows it touches -
// same-word atomics from many waves serialise, and a wave that walks down one 600-row window would otherwise add per row.
template <typename T>
__global__ __launch_bounds__(256) void scene_black_kernel(const SceneScanArgs<T> a) {
  const int wc = a.nx * a.tile_w, hc = a.ny * a.tile_h;
  const int x = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const bool in = x < wc;
  const int y0 = blockIdx.y * a.rows, y1 = min(hc, y0 + a.rows);
  int held_w[2] = {-1, -1}, held_n[2] = {0, 0};       // wave-uniform: the two windows met last and their counts so far
  for (int y = y0; y < y1; ++y) {
    const T* p = a.scene + (int64_t)y * a.W + (in ? x : 0);
    bool f_nd = in && a.use_nodata != 0, f_mk = in, f_zr = in;
    if (in) a.rule.apply(p[0], f_nd, f_mk, f_zr);
    for (int b = 1; b < a.bands && __any(f_nd || f_mk || f_zr); b += kScanAhead) {
      if (f_nd || f_mk || f_zr) {
        T v[kScanAhead];
#pragma unroll
        for (int j = 0; j < kScanAhead; ++j) v[j] = p[(int64_t)min(b + j, a.bands - 1) * a.plane];   // past the end: the last band again
#pragma unroll
        for (int j = 0; j < kScanAhead; ++j) a.rule.apply(v[j], f_nd, f_mk, f_zr);
      }
    }
    const bool black = f_nd || f_mk || f_zr;
    uint64_t rest = __ballot(black);
    if (rest == 0) continue;
    const int w = (y / a.tile_h) * a.nx + (in ? x / a.tile_w : 0);
    while (rest != 0) {
      const int leader = __ffsll((long long)rest) - 1;
      const int wl = __shfl(w, leader, 64);
      const uint64_t same = __ballot(black && w == wl);
      const int n = (int)__popcll(same);
      rest &= ~same;
      if (wl == held_w[0]) {
        held_n[0] += n;
      } else if (wl == held_w[1]) {
        held_n[1] += n;
      } else {                                         // a third window: the older one leaves
        if (lane == 0 && held_n[0] > 0) atomicAdd(a.counts + held_w[0], held_n[0]);
        held_w[0] = held_w[1], held_n[0] = held_n[1];
        held_w[1] = wl, held_n[1] = n;
      }
    }
  }
  if (lane == 0) {
    if (held_n[0] > 0) atomicAdd(a.counts + held_w[0], held_n[0]);
    if (held_n[1] > 0) atomicAdd(a.counts + held_w[1], held_n[1]);
  }
}

template <typename T>
static int launch_scan(const SceneScanArgs<T>& a, hipStream_t s) {
  const int wc = a.nx * a.tile_w, hc = a.ny * a.tile_h;
  hipLaunchKernelGGL(scene_black_kernel<T>, dim3((unsigned)((wc + 255) / 256), (unsigned)((hc + a.rows - 1) / a.rows)), dim3(256), 0, s, a);
  return launched(kLaunchScene, "scene_black_kernel launch", kSceneBlack + (sizeof(T) == 2 ? 1 : 0));
}

// ---- gather ----------------------------------------------------------------------------------------------------------------
struct SceneGatherArgs {
  const void* scene;                   // (bands, H, W)
  const int32_t* origins;              // (P, 2): row, col
  void* out;                           // (P, bands, th, tw)
  int64_t plane;
  int32_t bands, H, W, th, tw;
  float scale, src_nodata;
  int32_t has_src_nodata, nodata_u16;
};

template <typename T>
using scene_vec4 = T __attribute__((ext_vector_type(4)));

// grid (chunks of a tile plane, bands, P).  A window outside the scene is skipped, never dereferenced.  kVec (tw % 4 == 0 and
// an aligned stack): a thread owns four consecutive samples of a row and stores them as one vector; the scene side of a row
// starts at an arbitrary byte offset (the origin's), so it is read as one vector only where the address allows it.
template <typename TI, typename TO, bool kEncode, bool kVec>
__global__ __launch_bounds__(256) void scene_gather_kernel(const SceneGatherArgs a) {
  const int64_t pr = blockIdx.z, b = blockIdx.y;
  const int r0 = a.origins[2 * pr], c0 = a.origins[2 * pr + 1];
  if (r0 < 0 || c0 < 0 || r0 > a.H - a.th || c0 > a.W - a.tw) return;
  constexpr int E = kVec ? 4 : 1;
  const uint32_t rowq = (uint32_t)a.tw / E, n = (uint32_t)a.th * rowq;
  const TI* src = static_cast<const TI*>(a.scene) + b * a.plane + (int64_t)r0 * a.W + c0;
  TO* dst = static_cast<TO*>(a.out) + (pr * a.bands + b) * ((int64_t)a.th * a.tw);
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const uint32_t r = i / rowq, q = i - r * rowq;
    const TI* s = src + (int64_t)r * a.W + q * E;
    TI v[E];
    if (kVec && ((uintptr_t)s & (4 * sizeof(TI) - 1)) == 0) {
      const scene_vec4<TI> v4 = *reinterpret_cast<const scene_vec4<TI>*>(s);
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = v4[e];
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = s[e];
    }
    TO o[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if constexpr (kEncode) o[e] = encode_sample(v[e], a.scale, a.has_src_nodata != 0, a.src_nodata, a.nodata_u16);
      else o[e] = v[e];
    }
    TO* d = dst + (int64_t)i * E;        // row r, column q E: the stack's rows are dense
    if (kVec) {
      scene_vec4<TO> o4;
#pragma unroll
      for (int e = 0; e < E; ++e) o4[e] = o[e];
      *reinterpret_cast<scene_vec4<TO>*>(d) = o4;
    } else {
      d[0] = o[0];
    }
  }
}

template <typename TI, typename TO, bool kEncode>
static int launch_gather(const SceneGatherArgs& a, int ntiles, hipStream_t s) {
  constexpr int pair = kEncode ? 2 : (sizeof(TI) == 2 ? 1 : 0);
  const int64_t n = (int64_t)a.th * a.tw;
  const bool vec = a.tw % 4 == 0 && ((uintptr_t)a.out & (4 * sizeof(TO) - 1)) == 0;
  const int64_t chunks = ((vec ? n / 4 : n) + 255) / 256;
  const dim3 grid((unsigned)(chunks < 1024 ? chunks : 1024), (unsigned)a.bands, (unsigned)ntiles);
  if (vec)
    hipLaunchKernelGGL((scene_gather_kernel<TI, TO, kEncode, true>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((scene_gather_kernel<TI, TO, kEncode, false>), grid, dim3(256), 0, s, a);
  return launched(kLaunchScene, "scene_gather_kernel launch", kSceneGather + 2 * pair + (vec ? 1 : 0));
}

// ---- mosaic ----------------------------------------------------------------------------------------------------------------
struct SceneMosaicArgs {
  const float* cubes;                  // (P, T, th, tw)
  float* out;                          // (T, H, W)
  const int32_t* slot;                 // (ny, nx): >= 0 the cube of the window, -1 fill, -2 (and anything else) leave untouched
  int64_t plane, tile_plane;
  int32_t P, T, H, W, th, tw, ny, nx, fill_rest;
  float fill;
};

// grid (ceil(W / E / 256), rows, T).  A thread keeps its column(s) and walks rows; the window row is the same for the whole
// workgroup.  kVec (W % 4 == 0, tw % 4 == 0, aligned bases): four columns per thread - they share one window, and the
// remainder strip starts on a multiple of four - moved as 16-byte loads and stores.
template <bool kVec>
__global__ __launch_bounds__(256) void scene_mosaic_kernel(const SceneMosaicArgs a) {
  constexpr int E = kVec ? 4 : 1;
  const int x = (blockIdx.x * 256 + threadIdx.x) * E;
  if (x >= a.W) return;
  const int64_t t = blockIdx.z;
  const int wx = (int)((uint32_t)x / (uint32_t)a.tw), cx = x - wx * a.tw;
  float* out = a.out + t * a.plane + x;
  for (int y = blockIdx.y; y < a.H; y += gridDim.y) {
    const int wy = y / a.th;
    float* d = out + (int64_t)y * a.W;
    const float* s = nullptr;
    bool fill = false;
    if (wy < a.ny && wx < a.nx) {
      const int sl = a.slot[wy * a.nx + wx];
      if (sl >= 0 && sl < a.P) s = a.cubes + (sl * (int64_t)a.T + t) * a.tile_plane + (int64_t)(y - wy * a.th) * a.tw + cx;
      fill = sl == -1;
    } else {
      fill = a.fill_rest != 0;
    }
    if (kVec) {
      if (s) *reinterpret_cast<float4*>(d) = *reinterpret_cast<const float4*>(s);
      else if (fill) *reinterpret_cast<float4*>(d) = make_float4(a.fill, a.fill, a.fill, a.fill);
    } else {
      if (s) d[0] = s[0];
      else if (fill) d[0] = a.fill;
    }
  }
}

// ---- feathered mosaic -------------------------------------------------------------------------------------------------------
constexpr int kBlendMax = 16;          // contributors of one output pixel, at most

struct SceneBlendArgs {
  const float* cubes;                  // (P, T, th, tw)
  float* out;                          // (T, H, W)
  const int32_t* start;                // (ny, nx): the cube whose window starts at lattice cell (j, i), -1 none
  int64_t plane, tile_plane;
  int32_t P, T, H, W, th, tw, sy, sx, K, nx;
  int32_t ly, lx;                      // rows and columns of `start` whose cells lie in the table AND whose window stays in (H, W)
  float fill;
  uint8_t dj[kBlendMax], di[kBlendMax];   // contributor k starts dj[k] cells above and di[k] cells left of the pixel's cell:
};                                        // ascending start row, then ascending start column

// The tent weight of local position p of a window of n samples: min(p + 1, n - p), an integer.
__device__ __forceinline__ float tent(int p, int n) { return (float)min(p + 1, n - p); }

// grid (ceil(W / E / 256), rows, T), as scene_mosaic_kernel: a thread keeps its column(s) and walks rows; the lattice row, the
// local rows and wy are the same for the whole workgroup, the lattice column, the local columns and wx are fixed per thread.
// kVec (W, tw and sx multiples of 4, aligned bases): four columns per thread - they share one lattice cell, hence one
// contributor set - moved as 16-byte loads and stores.  KMAX >= K is the unrolled contributor count.  Every one of the KMAX
// table reads and then every one of the KMAX cube loads is issued, unconditionally, before the arithmetic, so a row's loads are
// in flight together and none sits behind a branch: a slot without a contributor reads entry 0 of the table, which it ignores,
// and the first samples of the stack, which it masks out.
template <bool kVec, int KMAX>
__global__ __launch_bounds__(256) void scene_blend_kernel(const SceneBlendArgs a) {
  constexpr int E = kVec ? 4 : 1;
  const int x = (blockIdx.x * 256 + threadIdx.x) * E;
  if (x >= a.W) return;
  const int64_t t = blockIdx.z;
  const int cx = (int)((uint32_t)x / (uint32_t)a.sx);
  float* out = a.out + t * a.plane + x;
  const float* cubes_t = a.cubes + t * a.tile_plane;
  const int64_t cube_pitch = (int64_t)a.T * a.tile_plane;
  for (int y = blockIdx.y; y < a.H; y += gridDim.y) {
    const int cy = y / a.sy;
    bool on[KMAX];
    int ent[KMAX], row[KMAX], col[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int sj = cy - a.dj[k], si = cx - a.di[k];                  // the start cell
      on[k] = k < a.K && (uint32_t)sj < (uint32_t)a.ly && (uint32_t)si < (uint32_t)a.lx;
      ent[k] = a.start[on[k] ? sj * a.nx + si : 0];
      row[k] = y - sj * a.sy;
      col[k] = x - si * a.sx;
    }
    const float* src[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      on[k] = on[k] && ent[k] >= 0 && ent[k] < a.P;
      src[k] = on[k] ? cubes_t + ent[k] * cube_pitch + ((int64_t)row[k] * a.tw + col[k]) : a.cubes;
    }
    float v[KMAX][E];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if constexpr (kVec) {
        const float4 q = *reinterpret_cast<const float4*>(src[k]);
        v[k][0] = q.x, v[k][1] = q.y, v[k][2] = q.z, v[k][3] = q.w;
      } else {
        v[k][0] = src[k][0];
      }
    }
    // `one` is what an element with n <= 1 gets: `fill` while no cube covers it; then, while nothing is taken, the value of the
    // contributor visited last (a NaN, with its bits); then the first value taken.
    float num[E], den[E], one[E];
    int n[E];
#pragma unroll
    for (int e = 0; e < E; ++e) num[e] = 0.0f, den[e] = 0.0f, one[e] = a.fill, n[e] = 0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const float wy = tent(row[k], a.th);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float val = v[k][e], w = wy * tent(col[k] + e, a.tw);   // integers whose product is below 2^24: exact
        const bool take = on[k] && val == val;
        one[e] = (take || (on[k] && n[e] == 0)) ? val : one[e];
        num[e] = take ? fmaf(w, val, num[e]) : num[e];
        den[e] = take ? den[e] + w : den[e];
        n[e] += take ? 1 : 0;
      }
    }
    float* d = out + (int64_t)y * a.W;
    if constexpr (kVec) {
      float4 q;
      q.x = n[0] <= 1 ? one[0] : __fdiv_rn(num[0], den[0]);
      q.y = n[1] <= 1 ? one[1] : __fdiv_rn(num[1], den[1]);
      q.z = n[2] <= 1 ? one[2] : __fdiv_rn(num[2], den[2]);
      q.w = n[3] <= 1 ? one[3] : __fdiv_rn(num[3], den[3]);
      *reinterpret_cast<float4*>(d) = q;
    } else {
      d[0] = n[0] <= 1 ? one[0] : __fdiv_rn(num[0], den[0]);
    }
  }
}

template <bool kVec>
static void launch_blend(const SceneBlendArgs& a, dim3 grid, hipStream_t s) {
  if (a.K <= 1) hipLaunchKernelGGL((scene_blend_kernel<kVec, 1>), grid, dim3(256), 0, s, a);
  else if (a.K <= 2) hipLaunchKernelGGL((scene_blend_kernel<kVec, 2>), grid, dim3(256), 0, s, a);
  else if (a.K <= 4) hipLaunchKernelGGL((scene_blend_kernel<kVec, 4>), grid, dim3(256), 0, s, a);
  else if (a.K <= 8) hipLaunchKernelGGL((scene_blend_kernel<kVec, 8>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((scene_blend_kernel<kVec, kBlendMax>), grid, dim3(256), 0, s, a);
}

// atol + 1e-5 |v| in double, as Python adds it; -1 (never reached by |x - v|) for a non-finite v
static double close_tol(double v, double atol) { return isfinite(v) ? atol + 1e-5 * fabs(v) : -1.0; }

}  // namespace hsr

using namespace hsr;

extern "C" int hsr_scene_black_counts(const void* scene_dev, int32_t dtype, int32_t bands, int32_t H, int32_t W, int32_t tile_h,
                                      int32_t tile_w, int32_t use_nodata, double nodata, double masked_val, double nodata_atol,
                                      double zero_atol, int32_t* counts_dev, hsr_stream_t stream) {
  HSR_REQUIRE(scene_dev && counts_dev, HSR_ERR_INVALID, "hsr_scene_black_counts: NULL pointer");
  HSR_REQUIRE(dtype == 0 || dtype == 2, HSR_ERR_UNSUPPORTED, "hsr_scene_black_counts: dtype=%d (0 float32, 2 uint16)", dtype);
  HSR_REQUIRE(bands >= 1 && H >= 1 && W >= 1 && tile_h >= 1 && tile_h <= H && tile_w >= 1 && tile_w <= W, HSR_ERR_INVALID,
              "hsr_scene_black_counts: bad shape (bands=%d H=%d W=%d tile=%d x %d)", bands, H, W, tile_h, tile_w);
  const int ny = H / tile_h, nx = W / tile_w;
  HSR_REQUIRE((int64_t)ny * nx <= 0x7fffffff, HSR_ERR_UNSUPPORTED, "hsr_scene_black_counts: %d x %d windows", ny, nx);
  hipStream_t s = (hipStream_t)stream;
  int rc = check_hip(hipMemsetAsync(counts_dev, 0, (size_t)ny * nx * sizeof(int32_t), s), "hsr_scene_black_counts: hipMemsetAsync");
  if (rc != HSR_OK) return rc;
  // rows per wave: as many as leave about 16 Ki waves (two per wave slot of the chip) to keep the loads of a black region in
  // flight, at most 64, and few enough for the grid's y extent
  const int64_t waves = (int64_t)((nx * (int64_t)tile_w + 63) / 64) * ((int64_t)ny * tile_h);
  int64_t rows = waves / 16384;
  rows = rows < 1 ? 1 : (rows > 64 ? 64 : rows);
  while (((int64_t)ny * tile_h + rows - 1) / rows > 65535) rows *= 2;
  const double nd_tol = close_tol(nodata, nodata_atol), mk_tol = close_tol(masked_val, nodata_atol);
  if (dtype == 0) {
    const SceneScanArgs<float> a{static_cast<const float*>(scene_dev), counts_dev,
                                 BlackRule<float>{(float)nodata, (float)nd_tol, (float)masked_val, (float)mk_tol, (float)zero_atol},
                                 (int64_t)H * W, bands, W, tile_h, tile_w, ny, nx, use_nodata, (int32_t)rows};
    return launch_scan(a, s);
  }
  const SceneScanArgs<uint16_t> a{static_cast<const uint16_t*>(scene_dev), counts_dev,
                                  BlackRule<uint16_t>{nodata, nd_tol, masked_val, mk_tol, zero_atol},
                                  (int64_t)H * W, bands, W, tile_h, tile_w, ny, nx, use_nodata, (int32_t)rows};
  return launch_scan(a, s);
}

extern "C" int hsr_scene_gather_tiles(const void* scene_dev, int32_t dtype, int32_t bands, int32_t H, int32_t W,
                                      const int32_t* origins_dev, int32_t ntiles, int32_t th, int32_t tw, int32_t encode,
                                      float scale, int32_t has_src_nodata, float src_nodata, int32_t nodata_u16, void* out_dev,
                                      hsr_stream_t stream) {
  HSR_REQUIRE(scene_dev && origins_dev && out_dev, HSR_ERR_INVALID, "hsr_scene_gather_tiles: NULL pointer");
  HSR_REQUIRE(dtype == 0 || dtype == 2, HSR_ERR_UNSUPPORTED, "hsr_scene_gather_tiles: dtype=%d (0 float32, 2 uint16)", dtype);
  HSR_REQUIRE(!encode || dtype == 0, HSR_ERR_UNSUPPORTED, "hsr_scene_gather_tiles: encode quantises float32 scenes, dtype=%d", dtype);
  HSR_REQUIRE(!encode || (nodata_u16 >= 1 && nodata_u16 <= 0xffff), HSR_ERR_INVALID,
              "hsr_scene_gather_tiles: nodata_u16=%d outside [1,65535]", nodata_u16);
  HSR_REQUIRE(bands >= 1 && bands <= 65535 && H >= 1 && W >= 1 && th >= 1 && th <= H && tw >= 1 && tw <= W && ntiles >= 1 &&
              ntiles <= 65535 && (int64_t)th * tw <= 0x7fffffff, HSR_ERR_INVALID,
              "hsr_scene_gather_tiles: bad shape (bands=%d H=%d W=%d tile=%d x %d P=%d)", bands, H, W, th, tw, ntiles);
  const SceneGatherArgs a{scene_dev, origins_dev, out_dev, (int64_t)H * W, bands, H, W, th, tw, scale, src_nodata, has_src_nodata,
                          nodata_u16};
  hipStream_t s = (hipStream_t)stream;
  if (encode) return launch_gather<float, uint16_t, true>(a, ntiles, s);
  if (dtype == 0) return launch_gather<float, float, false>(a, ntiles, s);
  return launch_gather<uint16_t, uint16_t, false>(a, ntiles, s);
}

extern "C" int hsr_scene_mosaic(const float* cubes_dev, int32_t ncubes, int32_t T, int32_t th, int32_t tw, float* out_dev, int32_t H,
                                int32_t W, const int32_t* slot_dev, int32_t ny, int32_t nx, float fill, int32_t fill_rest,
                                hsr_stream_t stream) {
  HSR_REQUIRE(out_dev && slot_dev && (cubes_dev || ncubes == 0), HSR_ERR_INVALID, "hsr_scene_mosaic: NULL pointer");
  HSR_REQUIRE(ncubes >= 0 && T >= 1 && T <= 65535 && H >= 1 && W >= 1 && th >= 1 && tw >= 1 && ny >= 1 && nx >= 1 &&
              (int64_t)ny * th <= H && (int64_t)nx * tw <= W && (int64_t)ny * nx <= 0x7fffffff, HSR_ERR_INVALID,
              "hsr_scene_mosaic: bad shape (P=%d T=%d H=%d W=%d tile=%d x %d windows=%d x %d)", ncubes, T, H, W, th, tw, ny, nx);
  const SceneMosaicArgs a{cubes_dev, out_dev, slot_dev, (int64_t)H * W, (int64_t)th * tw, ncubes, T, H, W, th, tw, ny, nx, fill_rest,
                          fill};
  const bool vec = W % 4 == 0 && tw % 4 == 0 && ((uintptr_t)out_dev & 15) == 0 && ((uintptr_t)cubes_dev & 15) == 0;
  const int64_t gx = ((vec ? W / 4 : W) + 255) / 256;
  int64_t gy = 65536 / (gx * T);                     // about 64 Ki workgroups: the rows are strided over them
  gy = gy < 1 ? 1 : (gy > H ? H : gy);
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)T);
  if (vec)
    hipLaunchKernelGGL(scene_mosaic_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(scene_mosaic_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
  return launched(kLaunchScene, "scene_mosaic_kernel launch", kSceneMosaic + (vec ? 1 : 0));
}

extern "C" int hsr_scene_mosaic_blend(const float* cubes_dev, int32_t ncubes, int32_t T, int32_t th, int32_t tw, int32_t sy, int32_t sx,
                                      const int32_t* start_dev, int32_t ny, int32_t nx, float* out_dev, int32_t H, int32_t W,
                                      float fill, hsr_stream_t stream) {
  HSR_REQUIRE(cubes_dev && start_dev && out_dev, HSR_ERR_INVALID, "hsr_scene_mosaic_blend: NULL pointer");
  HSR_REQUIRE(ncubes >= 1 && T >= 1 && th >= 1 && tw >= 1 && sy >= 1 && sx >= 1 && ny >= 1 && nx >= 1 && H >= 1 && W >= 1,
              HSR_ERR_INVALID, "hsr_scene_mosaic_blend: bad shape (P=%d T=%d H=%d W=%d tile=%d x %d pitch=%d x %d cells=%d x %d)",
              ncubes, T, H, W, th, tw, sy, sx, ny, nx);
  HSR_REQUIRE(th % sy == 0 && tw % sx == 0, HSR_ERR_INVALID,
              "hsr_scene_mosaic_blend: the lattice pitch %d x %d does not divide the tile %d x %d", sy, sx, th, tw);
  const int64_t ky = th / sy, kx = tw / sx, K = ky * kx;
  HSR_REQUIRE(K <= kBlendMax, HSR_ERR_UNSUPPORTED, "hsr_scene_mosaic_blend: %lld x %lld = %lld windows over a pixel, at most %d",
              (long long)ky, (long long)kx, (long long)K, kBlendMax);
  const int64_t wsum = K * ((th + 1) / 2) * (int64_t)((tw + 1) / 2);   // what the weights of one pixel can add up to
  HSR_REQUIRE(wsum <= (1 << 24), HSR_ERR_UNSUPPORTED,
              "hsr_scene_mosaic_blend: weight sum %lld = %lld x ceil(%d / 2) x ceil(%d / 2) above 2^24 is no exact float32 integer",
              (long long)wsum, (long long)K, th, tw);
  HSR_REQUIRE(T <= 65535, HSR_ERR_UNSUPPORTED, "hsr_scene_mosaic_blend: T=%d above 65535", T);
  HSR_REQUIRE((int64_t)ny * nx <= 0x7fffffff, HSR_ERR_UNSUPPORTED, "hsr_scene_mosaic_blend: %d x %d lattice cells", ny, nx);
  // the start cells whose window stays inside the output: rows 0 .. (H - th) / sy, none when the tile is larger than the output
  const int64_t fy = H >= th ? (int64_t)(H - th) / sy + 1 : 0, fx = W >= tw ? (int64_t)(W - tw) / sx + 1 : 0;
  SceneBlendArgs a{cubes_dev, out_dev, start_dev, (int64_t)H * W, (int64_t)th * tw, ncubes, T, H, W, th, tw, sy, sx, (int32_t)K, nx,
                   (int32_t)(fy < ny ? fy : ny), (int32_t)(fx < nx ? fx : nx), fill, {}, {}};
  for (int k = 0; k < (int)K; ++k) {                  // ascending start row, then ascending start column
    a.dj[k] = (uint8_t)(ky - 1 - k / kx);
    a.di[k] = (uint8_t)(kx - 1 - k % kx);
  }
  const bool vec = W % 4 == 0 && tw % 4 == 0 && sx % 4 == 0 && ((uintptr_t)out_dev & 15) == 0 && ((uintptr_t)cubes_dev & 15) == 0;
  const int64_t gx = ((vec ? W / 4 : W) + 255) / 256;
  int64_t gy = 65536 / (gx * T);                     // about 64 Ki workgroups: the rows are strided over them
  gy = gy < 1 ? 1 : (gy > H ? H : gy);
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)T);
  if (vec) launch_blend<true>(a, grid, (hipStream_t)stream);
  else launch_blend<false>(a, grid, (hipStream_t)stream);
  const int lg = K <= 1 ? 0 : K <= 2 ? 1 : K <= 4 ? 2 : K <= 8 ? 3 : 4;        // launch_blend's KMAX
  return launched(kLaunchScene, "scene_blend_kernel launch", kSceneBlend + (vec ? 5 : 0) + lg);
}
