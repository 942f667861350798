// EMIT swath -> orthorectified scene (s2_emit.ortho): the geometry-lookup-table gather of the reference's
//   EMIT_data/emit_tools.py  apply_glt (:153-181) under ortho_xr (:184-268), with the quality and band masks that emit_xarray
//                            (:115-119) writes into the swath first (quality_mask :271-298, band_mask :301-321), and
//   EMIT_data/emit_proj.py   nc_to_envi's in-bounds rule (:691-717) and band-chunked gather (:947-987),
// as ONE launch over the output: fill, index, mask and (for a band-sequential scene) transpose in the same pass, every output
// byte written once.  The contract is the comment above hsr_ortho_glt in include/hsr.h.
//
// A workgroup (bip: 256 threads, bsq: 512) owns kOrthoPx = 64 consecutive pixels of one output row.  Wave 0 reads their 64 GLT entries (512
// contiguous bytes), decides each pixel - fill (no data, or out of bounds: dropped), masked (quality mask == 1: every band is
// `masked`, the spectrum is not read) or copy - and leaves the source pixel index in LDS; the dropped entries are counted by
// ballot and added with at most one integer atomic per workgroup.  Then each wave takes kOrthoPxWave = 16 (bsq: 8) of the pixels,
// kOrthoAhead = 4 (bsq: 8) at a time: a pixel's spectrum is one contiguous run of `bands` floats read by the lanes side by side as bands / 4
// float4 (1 KiB per wave instruction) and bands % 4 single floats behind them, and the spectra of kOrthoAhead pixels are in
// flight per wave before the first is stored.  A pixel base lies on 16 bytes only when (pixel index x bands) % 4 == 0, so the
// float4 are dword-aligned accesses, which gfx950's global loads and stores take as they are.
//   bip  (h, w, bands): the spectrum goes straight back out, one contiguous run per pixel (streaming stores).  kVec - bands % 4
//        == 0 and both bases on 16 bytes, so that every pixel base is - declares the float4 16-byte aligned.
//   bsq  (bands, h, w): the spectra land in an LDS tile [64 pixels][bands | 1 floats] (the odd pitch keeps the transposed read off
//        shared banks); after a barrier wave w stores bands w, w + 8, ...: 64 lanes = 64 consecutive x = one 256-byte segment
//        of the band's plane per instruction.  Fill and masked pixels never touch the tile: their lane stores the constant.
#include "hsr_ortho_dev.h"                // the workgroup geometry, ortho_entry, OrthoVec and ortho_value: shared with hsr_merge.hip

namespace hsr {

static_assert(kOrthoPx * ((kOrthoMaxBands | 1) * 4) + 1024 <= 160 * 1024, "the bsq tile fits the LDS of a CU");

struct OrthoArgs {
  const float* swath;                  // (rows, cols, bands)
  const int32_t* glt;                  // (glt_h, glt_w, 2): one-based column, row
  const uint8_t* qmask;                // (rows, cols) or NULL
  const uint8_t* bmask;                // (rows, cols, bmask_bytes) or NULL
  float* out;                          // bip (out_h, out_w, bands) or bsq (bands, out_h, out_w)
  unsigned long long* dropped;         // zeroed before the launch, or NULL
  int64_t plane;                       // out_h out_w
  int32_t rows, cols, bands, glt_w, glt_nodata, row0, col0, out_w, bmask_bytes;
  float fill, masked;
};

// Wave 0: the GLT entries of the workgroup's pixels -> s_src (source pixel index sy cols + sx), s_kind and s_const (what a pixel
// that is not copied holds in every band: `masked` or `fill`, selected on the bits); ends with a barrier.
// The decision on an entry is ortho_entry (hsr_ortho_dev.h).
__device__ __forceinline__ void ortho_resolve(const OrthoArgs& a, int y, int x0, int* s_src, int* s_kind, float* s_const) {
  const int t = threadIdx.x;
  if (t < kOrthoPx) {
    const int x = x0 + t;
    int kind = kOrthoFill, src = 0;
    bool drop = false;
    if (x < a.out_w) {
      const int64_t g = ((int64_t)(a.row0 + y) * a.glt_w + (a.col0 + x)) * 2;
      kind = ortho_entry(a.glt[g], a.glt[g + 1], a.glt_nodata, a.rows, a.cols, a.qmask, src, drop);
    }
    s_src[t] = src;
    s_kind[t] = kind;
    const uint32_t fb = __float_as_uint(a.fill), mb = __float_as_uint(a.masked);
    s_const[t] = __uint_as_float(fb ^ ((fb ^ mb) & (kind == kOrthoMasked ? 0xffffffffu : 0u)));
    if (a.dropped) {
      const int n = (int)__popcll(__ballot(drop));
      if (t == 0 && n > 0) atomicAdd(a.dropped, (unsigned long long)n);
    }
  }
  __syncthreads();
}

// Pixels [p0, p0 + kAhead) of the workgroup (those below pend), bands [b, b + E) of each: all loads, then `sink(j, p, value)`.
template <bool kMask, int E, bool kAligned, int kAhead, typename Sink>
__device__ __forceinline__ void ortho_group(const OrthoArgs& a, const int* s_src, const int* s_kind, const float* s_const, int p0,
                                            int pend, int b, Sink sink) {
  OrthoVec<E, kAligned> v[kAhead];
#pragma unroll
  for (int j = 0; j < kAhead; ++j) {
    const int p = min(p0 + j, pend - 1);                               // past the end: the last pixel again, not passed on
    ortho_value<kMask>(a, s_kind[p], s_const[p], s_src[p], b, v[j]);
  }
#pragma unroll
  for (int j = 0; j < kAhead; ++j)
    if (p0 + j < pend) sink(p0 + j, v[j]);
}

// grid: out_h ceil(out_w / 64) workgroups, row-major over (y, chunk of x).  A pixel is bands / 4 quads, lane after lane, and
// bands % 4 single floats behind them.
template <bool kMask, bool kVec>
__global__ __launch_bounds__(256) void ortho_bip_kernel(const OrthoArgs a) {
  __shared__ int s_src[kOrthoPx], s_kind[kOrthoPx];
  __shared__ float s_const[kOrthoPx];
  const int nbx = (a.out_w + kOrthoPx - 1) / kOrthoPx;
  const int y = (int)(blockIdx.x / (uint32_t)nbx), x0 = (int)(blockIdx.x - (uint32_t)y * (uint32_t)nbx) * kOrthoPx;
  ortho_resolve(a, y, x0, s_src, s_kind, s_const);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int pend = min(min(kOrthoPx, a.out_w - x0), (wave + 1) * kOrthoPxWave);
  const int quads = a.bands >> 2, rest = a.bands & 3;
  float* row = a.out + ((int64_t)y * a.out_w + x0) * a.bands;
  for (int p0 = wave * kOrthoPxWave; p0 < pend; p0 += kOrthoAhead) {
    for (int q = lane; q < quads; q += 64)
      ortho_group<kMask, 4, kVec, kOrthoAhead>(a, s_src, s_kind, s_const, p0, pend, 4 * q,
                                               [&](int p, const OrthoVec<4, kVec>& v) { v.store(row + (int64_t)p * a.bands + 4 * q); });
    if (!kVec && lane < rest)
      ortho_group<kMask, 1, false, kOrthoAhead>(a, s_src, s_kind, s_const, p0, pend, 4 * quads + lane, [&](int p, const OrthoVec<1, false>& v) {
        v.store(row + (int64_t)p * a.bands + 4 * quads + lane);
      });
  }
}

// 512 threads.  The tile row of a pixel holds its quads element by element - float e of quad q at word e quads + q, the bands %
// 4 floats of the tail behind them at their own index - so that the four LDS writes of a float4 go to consecutive words lane
// after lane (no bank is hit twice); band b is read back from word (b & 3) quads + (b >> 2).
template <bool kMask>
__global__ __launch_bounds__(64 * kOrthoBsqWaves) void ortho_bsq_kernel(const OrthoArgs a) {
  extern __shared__ float s_tile[];                                    // [kOrthoPx][pitch]
  __shared__ int s_src[kOrthoPx], s_kind[kOrthoPx];
  __shared__ float s_const[kOrthoPx];
  const int pitch = a.bands | 1;
  const int nbx = (a.out_w + kOrthoPx - 1) / kOrthoPx;
  const int y = (int)(blockIdx.x / (uint32_t)nbx), x0 = (int)(blockIdx.x - (uint32_t)y * (uint32_t)nbx) * kOrthoPx;
  ortho_resolve(a, y, x0, s_src, s_kind, s_const);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int pend = min(min(kOrthoPx, a.out_w - x0), (wave + 1) * kOrthoPxWaveBsq);
  const int quads = a.bands >> 2, rest = a.bands & 3;
  // a constant pixel's tile row is neither written nor read: its lane stores the constant
  for (int p0 = wave * kOrthoPxWaveBsq; p0 < pend; p0 += kOrthoAheadBsq) {
    for (int q = lane; q < quads; q += 64)
      ortho_group<kMask, 4, false, kOrthoAheadBsq>(a, s_src, s_kind, s_const, p0, pend, 4 * q, [&](int p, const OrthoVec<4, false>& v) {
        if (s_kind[p] == kOrthoCopy) {
          float* t = s_tile + p * pitch + q;
          t[0] = v.v[0], t[quads] = v.v[1], t[2 * quads] = v.v[2], t[3 * quads] = v.v[3];
        }
      });
    if (lane < rest)
      ortho_group<kMask, 1, false, kOrthoAheadBsq>(a, s_src, s_kind, s_const, p0, pend, 4 * quads + lane, [&](int p, const OrthoVec<1, false>& v) {
        if (s_kind[p] == kOrthoCopy) s_tile[p * pitch + 4 * quads + lane] = v.v[0];
      });
  }
  __syncthreads();
  const int x = x0 + lane;
  if (x >= a.out_w) return;
  const bool copy = s_kind[lane] == kOrthoCopy;
  const float constant = s_const[lane];
  const float* mine = s_tile + lane * pitch;
  float* o = a.out + (int64_t)y * a.out_w + x;
#pragma unroll 4
  for (int b = wave; b < a.bands; b += kOrthoBsqWaves) {
    const int word = b < 4 * quads ? (b & 3) * quads + (b >> 2) : b;
    st_stream(o + (int64_t)b * a.plane, copy ? mine[word] : constant);
  }
}

}  // namespace hsr

using namespace hsr;

extern "C" int hsr_ortho_glt(const float* swath_dev, int32_t rows, int32_t cols, int32_t bands, const int32_t* glt_dev,
                             int32_t glt_h, int32_t glt_w, int32_t glt_nodata, int32_t row0, int32_t col0, int32_t out_h,
                             int32_t out_w, const uint8_t* qmask_dev, const uint8_t* bmask_dev, int32_t bmask_bytes, float fill,
                             float masked, int32_t layout, float* out_dev, int64_t* dropped_dev, hsr_stream_t stream) {
  HSR_REQUIRE(swath_dev && glt_dev && out_dev, HSR_ERR_INVALID, "hsr_ortho_glt: NULL pointer");
  HSR_REQUIRE(rows >= 1 && cols >= 1 && bands >= 1 && glt_h >= 1 && glt_w >= 1 && out_h >= 1 && out_w >= 1, HSR_ERR_INVALID,
              "hsr_ortho_glt: bad shape (swath %d x %d x %d, GLT %d x %d, window %d x %d)", rows, cols, bands, glt_h, glt_w, out_h,
              out_w);
  HSR_REQUIRE(row0 >= 0 && col0 >= 0 && (int64_t)row0 + out_h <= glt_h && (int64_t)col0 + out_w <= glt_w, HSR_ERR_INVALID,
              "hsr_ortho_glt: the window of %d x %d at row %d, col %d leaves the %d x %d GLT grid", out_h, out_w, row0, col0, glt_h,
              glt_w);
  HSR_REQUIRE(!bmask_dev || bmask_bytes >= (bands + 7) / 8, HSR_ERR_INVALID,
              "hsr_ortho_glt: bmask_bytes=%d, %d bands need %d", bmask_bytes, bands, (bands + 7) / 8);
  HSR_REQUIRE(layout == 0 || layout == 1, HSR_ERR_INVALID, "hsr_ortho_glt: layout=%d (0 bip, 1 bsq)", layout);
  HSR_REQUIRE(bands <= kOrthoMaxBands, HSR_ERR_UNSUPPORTED, "hsr_ortho_glt: bands=%d above %d", bands, kOrthoMaxBands);
  HSR_REQUIRE((int64_t)rows * cols <= 0x7fffffff, HSR_ERR_UNSUPPORTED, "hsr_ortho_glt: a swath of %d x %d pixels, at most 2^31 - 1",
              rows, cols);
  HSR_REQUIRE((int64_t)out_h * out_w <= 0x7fffffff, HSR_ERR_UNSUPPORTED, "hsr_ortho_glt: a window of %d x %d pixels, at most 2^31 - 1",
              out_h, out_w);
  hipStream_t s = (hipStream_t)stream;
  if (dropped_dev) {
    const int rc = check_hip(hipMemsetAsync(dropped_dev, 0, sizeof(int64_t), s), "hsr_ortho_glt: hipMemsetAsync");
    if (rc != HSR_OK) return rc;
  }
  const OrthoArgs a{swath_dev, glt_dev, qmask_dev, bmask_dev, out_dev, reinterpret_cast<unsigned long long*>(dropped_dev),
                    (int64_t)out_h * out_w, rows, cols, bands, glt_w, glt_nodata, row0, col0, out_w, bmask_dev ? bmask_bytes : 0,
                    fill, masked};
  const bool mask = qmask_dev || bmask_dev;
  const dim3 grid((unsigned)((int64_t)out_h * ((out_w + kOrthoPx - 1) / kOrthoPx)));       // <= out_h out_w <= INT32_MAX
  if (layout == 0) {
    const bool vec = bands % 4 == 0 && ((uintptr_t)swath_dev & 15) == 0 && ((uintptr_t)out_dev & 15) == 0;
    if (mask && vec) hipLaunchKernelGGL((ortho_bip_kernel<true, true>), grid, dim3(256), 0, s, a);
    else if (mask) hipLaunchKernelGGL((ortho_bip_kernel<true, false>), grid, dim3(256), 0, s, a);
    else if (vec) hipLaunchKernelGGL((ortho_bip_kernel<false, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((ortho_bip_kernel<false, false>), grid, dim3(256), 0, s, a);
    return launched(kLaunchOrtho, "ortho_bip_kernel launch", kOrthoBip + 2 * (mask ? 1 : 0) + (vec ? 1 : 0));
  }
  const size_t lds = (size_t)kOrthoPx * (size_t)(bands | 1) * sizeof(float);
  static thread_local size_t configured[2] = {};     // per kernel: ortho_bsq_kernel<false>, <true>
  if (mask) {
    raise_lds_limit(reinterpret_cast<const void*>(ortho_bsq_kernel<true>), lds, configured[1]);
    hipLaunchKernelGGL(ortho_bsq_kernel<true>, grid, dim3(64 * kOrthoBsqWaves), lds, s, a);
  } else {
    raise_lds_limit(reinterpret_cast<const void*>(ortho_bsq_kernel<false>), lds, configured[0]);
    hipLaunchKernelGGL(ortho_bsq_kernel<false>, grid, dim3(64 * kOrthoBsqWaves), lds, s, a);
  }
  return launched(kLaunchOrtho, "ortho_bsq_kernel launch", kOrthoBsq + (mask ? 1 : 0));
}
