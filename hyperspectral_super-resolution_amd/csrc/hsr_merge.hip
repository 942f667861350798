// Adjacent EMIT scenes of one orbit onto one grid (s2_emit.merge): the reference's merge_emit (EMIT_data/emit_tools.py:631-704),
// which orthorectifies every granule and hands the results to rioxarray's merge_arrays(..., nodata=-9999) - rasterio's "first"
// rule.  The definition - the grid, the nearest-cell placement, the per-element first rule - is the comment at the top of
// include/hsr_merge.h; every entry point's contract stands above its declaration there.
//
// hsr_merge_scenes   merge_scenes_kernel: a streaming select.  The rule is per element, so a layout is only strides: an output row
//     is a run of L = W (bsq, one row per band and y) or L = W bands (bip, one row per y) floats.  A workgroup of 256 threads owns
//     HSR_MERGE_RUN = 1024 elements of one row; a thread owns the four that share a 16-byte line of the OUTPUT (the row's first and
//     last line may be cut), so that every whole line leaves as one 16-byte streaming store whatever the row's length is.  The
//     sources are walked in order; a wave skips one that none of its lanes needs (ballot) and stops when nothing is empty any more.
//     merge_source_kernel (only with a source plane): a thread per cell.
// hsr_ortho_merge    ortho_merge_bip_kernel / ortho_merge_bsq_kernel: the kernels of csrc/hsr_ortho.hip with N lookup tables
//     instead of one.  Wave 0 resolves the workgroup's 64 pixels against every table (ortho_entry of hsr_ortho_dev.h) and leaves a
//     candidate list per pixel in LDS; the copying waves read the first candidate as before and a later one only where a ballot
//     shows an element that is still empty.
// Both element rules are __host__ __device__: hsr_merge_scenes_host runs them on the CPU.
#include "hsr_ortho_dev.h"

#include <math.h>

#include "../../include/hsr_merge.h"

namespace hsr {

constexpr int kMergeMax = HSR_MERGE_MAX_SOURCES;
constexpr int kMergeThreads = 256;
constexpr int kMergeLine = 4;          // floats of a 16-byte line
static_assert(kMergeThreads * kMergeLine == HSR_MERGE_RUN, "a thread owns one line of the run");
static_assert(kMergeMax <= 16, "a candidate's code keeps the source index in four bits");
static_assert(kOrthoPx * ((kOrthoMaxBands | 1) * 4) + 2 * kMergeMax * kOrthoPx * 4 + 1536 <= 160 * 1024,
              "the bsq tile and the candidate lists fit the LDS of a CU");
static_assert(HSR_MERGE_MAX_BANDS == kOrthoMaxBands, "the band limit is hsr_ortho_glt's");

__host__ __device__ inline bool merge_empty(float v, float nodata, bool nan_is_nodata) {
  return v == nodata || (nan_is_nodata && v != v);
}

// =====================================================================================================================================
// merge_scenes
// =====================================================================================================================================
struct MergeSrc {
  const float* p;
  int64_t ps, rs;                      // plane and row stride in elements (bip: one plane)
  int64_t x0, lx;                      // the scene's rows are elements [x0, x0 + lx) of the output's rows ...
  int32_t y0, h;                       // ... y0 .. y0 + h - 1
};

struct MergeArgs {
  MergeSrc s[kMergeMax];
  float* out;
  uint8_t* source;                     // (H, W) or NULL
  int64_t L;                           // elements of an output row
  int32_t n, H, W, bands, bsq, nchunk, nan;
  float nodata;
};

// Element i of row y of plane p under the first rule; who: the source that supplied it, -1: none (the value is `nodata`).
__host__ __device__ inline float merge_element(const MergeArgs& a, int p, int y, int64_t i, int& who) {
  who = -1;
  for (int k = 0; k < a.n; ++k) {
    const MergeSrc& s = a.s[k];
    const int64_t yy = (int64_t)y - s.y0, j = i - s.x0;
    if (yy < 0 || yy >= s.h || j < 0 || j >= s.lx) continue;
    const float v = s.p[(int64_t)p * s.ps + yy * s.rs + j];
    if (!merge_empty(v, a.nodata, a.nan != 0)) {
      who = k;
      return v;
    }
  }
  return a.nodata;
}

// The first source that supplies any band of cell (y, x), HSR_MERGE_NO_SOURCE: none.
__host__ __device__ inline uint8_t merge_first_source(const MergeArgs& a, int y, int x) {
  for (int k = 0; k < a.n; ++k) {
    const MergeSrc& s = a.s[k];
    const int64_t yy = (int64_t)y - s.y0;
    const int64_t j0 = (a.bsq ? (int64_t)x : (int64_t)x * a.bands) - s.x0;
    if (yy < 0 || yy >= s.h || j0 < 0 || j0 >= s.lx) continue;
    for (int b = 0; b < a.bands; ++b) {
      const float v = a.bsq ? s.p[(int64_t)b * s.ps + yy * s.rs + j0] : s.p[yy * s.rs + j0 + b];
      if (!merge_empty(v, a.nodata, a.nan != 0)) return (uint8_t)k;
    }
  }
  return HSR_MERGE_NO_SOURCE;
}

// grid: rows x nchunk workgroups, rows = H (bip) or bands H (bsq).
__global__ __launch_bounds__(kMergeThreads) void merge_scenes_kernel(const MergeArgs a) {
  const uint32_t r = blockIdx.x / (uint32_t)a.nchunk, c = blockIdx.x - r * (uint32_t)a.nchunk;
  const int p = a.bsq ? (int)(r / (uint32_t)a.H) : 0, y = (int)(r - (uint32_t)p * (uint32_t)a.H);
  float* orow = a.out + (int64_t)r * a.L;
  const int ph = (int)(((uintptr_t)orow >> 2) & 3);                    // floats by which the row starts past a 16-byte line
  const int64_t i0 = ((int64_t)c * kMergeThreads + threadIdx.x) * kMergeLine - ph;     // the thread's line: elements i0 .. i0 + 3
  if (i0 >= a.L) return;
  const int lo = i0 < 0 ? (int)-i0 : 0, hi = a.L - i0 < kMergeLine ? (int)(a.L - i0) : kMergeLine;   // of them, [lo, hi) exist
  const bool nan = a.nan != 0;
  float v[kMergeLine];
#pragma unroll
  for (int e = 0; e < kMergeLine; ++e) v[e] = a.nodata;
  unsigned empty = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
  for (int k = 0; k < a.n; ++k) {
    if (__ballot(empty != 0) == 0) break;
    const MergeSrc& s = a.s[k];
    const int64_t yy = (int64_t)y - s.y0;
    if (yy < 0 || yy >= s.h) continue;                                 // the same for the whole workgroup
    const int64_t j = i0 - s.x0;                                       // the line starts at element j of the scene's row
    const bool need = empty != 0 && j + hi > 0 && j + lo < s.lx;
    if (__ballot(need) == 0) continue;
    if (!need) continue;
    const float* q = s.p + ((int64_t)p * s.ps + yy * s.rs + j);
    if (j >= 0 && j + kMergeLine <= s.lx && ((uintptr_t)q & 15) == 0) {
      const ortho_f4a w = __builtin_nontemporal_load(reinterpret_cast<const ortho_f4a*>(q));
      const float we[kMergeLine] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int e = 0; e < kMergeLine; ++e)
        if (((empty >> e) & 1u) && !merge_empty(we[e], a.nodata, nan)) {
          v[e] = we[e];
          empty &= ~(1u << e);
        }
    } else {
#pragma unroll
      for (int e = 0; e < kMergeLine; ++e)
        if (((empty >> e) & 1u) && j + e >= 0 && j + e < s.lx) {
          const float w = ld_stream(q + e);
          if (!merge_empty(w, a.nodata, nan)) {
            v[e] = w;
            empty &= ~(1u << e);
          }
        }
    }
  }
  float* o = orow + i0;
  if (lo == 0 && hi == kMergeLine) {
    const ortho_f4a w = {v[0], v[1], v[2], v[3]};
    __builtin_nontemporal_store(w, reinterpret_cast<ortho_f4a*>(o));
  } else {
#pragma unroll
    for (int e = 0; e < kMergeLine; ++e)
      if (e >= lo && e < hi) st_stream(o + e, v[e]);
  }
}

__global__ __launch_bounds__(kMergeThreads) void merge_source_kernel(const MergeArgs a) {
  const int64_t cell = (int64_t)blockIdx.x * kMergeThreads + threadIdx.x;
  if (cell >= (int64_t)a.H * a.W) return;
  const int y = (int)(cell / a.W), x = (int)(cell - (int64_t)y * a.W);
  a.source[cell] = merge_first_source(a, y, x);
}

static void merge_scenes_host(const MergeArgs& a) {
  const int planes = a.bsq ? a.bands : 1;
  for (int p = 0; p < planes; ++p)
    for (int y = 0; y < a.H; ++y) {
      float* orow = a.out + ((int64_t)p * a.H + y) * a.L;
      for (int64_t i = 0; i < a.L; ++i) {
        int who;
        orow[i] = merge_element(a, p, y, i, who);
      }
    }
  if (a.source)
    for (int y = 0; y < a.H; ++y)
      for (int x = 0; x < a.W; ++x) a.source[(int64_t)y * a.W + x] = merge_first_source(a, y, x);
}

static bool ranges_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && na > 0 && nb > 0 && a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

// The argument checks of hsr_merge_scenes and its host twin -> the kernel's arguments.
static int merge_scenes_args(const char* fn, const hsr_merge_scene* scenes, int32_t n, int32_t layout, int32_t out_h, int32_t out_w,
                             float nodata, int32_t nan_is_nodata, float* out, uint8_t* source, MergeArgs& a) {
  HSR_REQUIRE(n >= 1 && n <= kMergeMax, HSR_ERR_INVALID, "%s: %d sources, 1 to %d", fn, n, kMergeMax);
  HSR_REQUIRE(scenes && out, HSR_ERR_INVALID, "%s: NULL pointer", fn);
  HSR_REQUIRE(layout == 0 || layout == 1, HSR_ERR_INVALID, "%s: layout=%d (0 bip, 1 bsq)", fn, layout);
  HSR_REQUIRE(out_h >= 1 && out_w >= 1, HSR_ERR_INVALID, "%s: an output of %d x %d", fn, out_h, out_w);
  const int32_t bands = scenes[0].bands;
  HSR_REQUIRE(bands >= 1, HSR_ERR_INVALID, "%s: bands=%d", fn, bands);
  HSR_REQUIRE(bands <= kOrthoMaxBands, HSR_ERR_UNSUPPORTED, "%s: bands=%d above %d", fn, bands, kOrthoMaxBands);
  HSR_REQUIRE((int64_t)out_h * out_w <= 0x7fffffff, HSR_ERR_UNSUPPORTED, "%s: an output of %d x %d pixels, at most 2^31 - 1", fn, out_h,
              out_w);
  HSR_REQUIRE(((uintptr_t)out & 3) == 0, HSR_ERR_INVALID, "%s: the output is not on 4 bytes", fn);
  const int64_t out_bytes = (int64_t)out_h * out_w * bands * 4;
  a = MergeArgs{};
  for (int k = 0; k < n; ++k) {
    const hsr_merge_scene& s = scenes[k];
    HSR_REQUIRE(s.scene_dev, HSR_ERR_INVALID, "%s: source %d is NULL", fn, k);
    HSR_REQUIRE(((uintptr_t)s.scene_dev & 3) == 0, HSR_ERR_INVALID, "%s: source %d is not on 4 bytes", fn, k);
    HSR_REQUIRE(s.h >= 1 && s.w >= 1, HSR_ERR_INVALID, "%s: source %d is %d x %d", fn, k, s.h, s.w);
    HSR_REQUIRE(s.bands == bands, HSR_ERR_INVALID, "%s: source %d has %d bands, source 0 has %d", fn, k, s.bands, bands);
    HSR_REQUIRE((int64_t)s.h * s.w <= 0x7fffffff, HSR_ERR_UNSUPPORTED, "%s: source %d has %d x %d pixels, at most 2^31 - 1", fn, k, s.h, s.w);
    const int64_t bytes = (int64_t)s.h * s.w * bands * 4;
    HSR_REQUIRE(!ranges_overlap(out, out_bytes, s.scene_dev, bytes) && !ranges_overlap(source, (int64_t)out_h * out_w, s.scene_dev, bytes),
                HSR_ERR_INVALID, "%s: the output overlaps source %d", fn, k);
    const int64_t epp = layout == 1 ? 1 : bands;
    a.s[k] = MergeSrc{s.scene_dev, layout == 1 ? (int64_t)s.h * s.w : 0, (int64_t)s.w * epp, (int64_t)s.off_x * epp, (int64_t)s.w * epp,
                      s.off_y, s.h};
  }
  HSR_REQUIRE(!ranges_overlap(out, out_bytes, source, (int64_t)out_h * out_w), HSR_ERR_INVALID, "%s: the source plane overlaps the output", fn);
  a.out = out;
  a.source = source;
  a.L = (int64_t)out_w * (layout == 1 ? 1 : bands);
  a.n = n, a.H = out_h, a.W = out_w, a.bands = bands, a.bsq = layout, a.nan = nan_is_nodata != 0;
  a.nodata = nodata;
  const int64_t nchunk = (a.L + (kMergeLine - 1) + HSR_MERGE_RUN - 1) / HSR_MERGE_RUN;       // a row may start up to 3 floats into a line
  HSR_REQUIRE(nchunk * out_h * (layout == 1 ? bands : 1) <= 0x7fffffff, HSR_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 workgroups", fn);
  a.nchunk = (int32_t)nchunk;
  return HSR_OK;
}

// =====================================================================================================================================
// ortho_merge
// =====================================================================================================================================
struct OrthoMergeSrc {
  const float* swath;
  const int32_t* glt;
  const uint8_t* qmask;
  const uint8_t* bmask;
  int32_t rows, cols, glt_h, glt_w, off_y, off_x, bmask_bytes, pad;
};

struct OrthoMergeArgs {
  OrthoMergeSrc s[kMergeMax];
  float* out;                          // bip (out_h, out_w, bands) or bsq (bands, out_h, out_w)
  unsigned long long* dropped;         // [n], zeroed before the launch, or NULL
  uint8_t* source;                     // (out_h, out_w) or NULL
  int64_t plane;                       // out_h out_w
  int32_t n, bands, glt_nodata, out_w;
  int32_t fill_empty, masked_empty;    // `nodata` (what a fill pixel holds) and `masked` are empty under the first rule
  float nodata, masked;
};

// What ortho_value needs of one source.
struct OrthoMergeView {
  const float* swath;
  const uint8_t* bmask;
  int32_t bands, bmask_bytes;
  float masked;
};

// The candidate lists of a workgroup's pixels: per pixel cnt candidates in source order, each a swath pixel index and a code
// (source index | kind << 4).  A candidate that is a constant (kOrthoMasked, kOrthoFill) is listed only when the constant is not
// empty, and then ends the list: every band of it wins.  use_tile / constant: what the bsq store pass does with the pixel.
struct MergeLds {
  int src[kMergeMax][kOrthoPx];
  int code[kMergeMax][kOrthoPx];
  int cnt[kOrthoPx];
  int win[kOrthoPx];                   // the source that supplied the pixel's first band, HSR_MERGE_NO_SOURCE: none
  int use_tile[kOrthoPx];
  float constant[kOrthoPx];
};

__device__ __forceinline__ float merge_constant(const OrthoMergeArgs& a, int kind) { return kind == kOrthoMasked ? a.masked : a.nodata; }

// Wave 0: the workgroup's pixels against the n tables; ends with a barrier.
__device__ __forceinline__ void merge_resolve(const OrthoMergeArgs& a, int y, int x0, MergeLds& l) {
  const int t = threadIdx.x;
  if (t < kOrthoPx) {
    const int x = x0 + t;
    int cnt = 0, first_kind = kOrthoFill;
    bool open = true;
    for (int k = 0; k < a.n; ++k) {
      const OrthoMergeSrc& s = a.s[k];
      const int64_t gy = (int64_t)y - s.off_y, gx = (int64_t)x - s.off_x;
      if (gy < 0 || gy >= s.glt_h) continue;                           // the same for the whole workgroup
      int kind = kOrthoFill, src = 0;
      bool drop = false;
      const bool covered = x < a.out_w && gx >= 0 && gx < s.glt_w;
      if (covered) {
        const int64_t g = (gy * s.glt_w + gx) * 2;
        kind = ortho_entry(s.glt[g], s.glt[g + 1], a.glt_nodata, s.rows, s.cols, s.qmask, src, drop);
      }
      const bool listed = covered && open &&
                          (kind == kOrthoCopy || (kind == kOrthoMasked && !a.masked_empty) || (kind == kOrthoFill && !a.fill_empty));
      if (listed) {
        if (cnt == 0) first_kind = kind;
        l.src[cnt][t] = src;
        l.code[cnt][t] = k | (kind << 4);
        ++cnt;
        open = kind == kOrthoCopy;
      }
      if (a.dropped) {
        const int n = (int)__popcll(__ballot(drop));
        if (t == 0 && n > 0) atomicAdd(a.dropped + k, (unsigned long long)n);
      }
    }
    l.cnt[t] = cnt;
    l.win[t] = HSR_MERGE_NO_SOURCE;
    l.use_tile[t] = cnt > 0 && first_kind == kOrthoCopy;
    l.constant[t] = cnt > 0 ? merge_constant(a, first_kind) : a.nodata;
  }
  __syncthreads();
}

// Candidate c of pixel p, bands [b, b + E).
template <bool kMask, int E, bool kAligned>
__device__ __forceinline__ void merge_candidate(const OrthoMergeArgs& a, const MergeLds& l, int p, int c, int b, OrthoVec<E, kAligned>& o) {
  const int code = __builtin_amdgcn_readfirstlane(l.code[c][p]), src = __builtin_amdgcn_readfirstlane(l.src[c][p]);
  const OrthoMergeSrc& s = a.s[code & 15];
  const OrthoMergeView view{s.swath, s.bmask, a.bands, s.bmask_bytes, a.masked};
  ortho_value<kMask>(view, code >> 4, merge_constant(a, code >> 4), src, b, o);
}

// Pixels [p0, p0 + kAhead) of the workgroup (those below pend), bands [b, b + E) of each: the first candidates of all of them are
// loaded before the first is looked at; then, pixel by pixel, the later candidates where an element is still empty, and
// `sink(p, value)`.  first[j]: the lowest candidate that supplied an element of pixel p0 + j (over the calls of one pixel group).
// p0, pend and with them the pixel, its candidates and every ballot are uniform over the lanes that run this.
template <bool kMask, int E, bool kAligned, int kAhead, typename Sink>
__device__ __forceinline__ void merge_group(const OrthoMergeArgs& a, const MergeLds& l, int p0, int pend, int b, int (&first)[kAhead],
                                            Sink sink) {
  OrthoVec<E, kAligned> v[kAhead];
#pragma unroll
  for (int j = 0; j < kAhead; ++j) {
    const int p = min(p0 + j, pend - 1);                               // past the end: the last pixel again, not passed on
    if (__builtin_amdgcn_readfirstlane(l.cnt[p]) > 0) {
      merge_candidate<kMask>(a, l, p, 0, b, v[j]);
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) v[j].v[e] = a.nodata;
    }
  }
#pragma unroll
  for (int j = 0; j < kAhead; ++j) {
    if (p0 + j >= pend) continue;
    const int p = p0 + j, cnt = __builtin_amdgcn_readfirstlane(l.cnt[p]);
    unsigned empty = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) empty |= (merge_empty(v[j].v[e], a.nodata, false) ? 1u : 0u) << e;
    if (cnt > 0 && __ballot(empty != (1u << E) - 1u) != 0) first[j] = 0;
    for (int c = 1; c < cnt && __ballot(empty != 0) != 0; ++c) {
      bool took = false;
      if (empty != 0) {
        OrthoVec<E, kAligned> w;
        merge_candidate<kMask>(a, l, p, c, b, w);
#pragma unroll
        for (int e = 0; e < E; ++e)
          if (((empty >> e) & 1u) && !merge_empty(w.v[e], a.nodata, false)) {
            v[j].v[e] = w.v[e];
            empty &= ~(1u << e);
            took = true;
          }
      }
      if (__ballot(took) != 0) first[j] = min(first[j], c);
    }
#pragma unroll
    for (int e = 0; e < E; ++e)
      if ((empty >> e) & 1u) v[j].v[e] = a.nodata;                      // the bits of nodata, whatever bits compared equal to it
    sink(p, v[j]);
  }
}

// Lane 0 has run every call of a pixel group (it owns quad 0 and tail band 0): its first[] is the group's.
template <int kAhead>
__device__ __forceinline__ void merge_note_winners(const OrthoMergeArgs& a, MergeLds& l, int lane, int p0, int pend, const int (&first)[kAhead]) {
  if (!a.source || lane != 0) return;
#pragma unroll
  for (int j = 0; j < kAhead; ++j)
    if (p0 + j < pend && first[j] < kMergeMax) l.win[p0 + j] = l.code[first[j]][p0 + j] & 15;
}

// After a barrier: the 64 bytes of the source plane, one store instruction.
__device__ __forceinline__ void merge_store_winners(const OrthoMergeArgs& a, const MergeLds& l, int y, int x0) {
  const int t = threadIdx.x;
  if (a.source && t < kOrthoPx && x0 + t < a.out_w) a.source[(int64_t)y * a.out_w + x0 + t] = (uint8_t)l.win[t];
}

// grid: out_h ceil(out_w / 64) workgroups, row-major over (y, chunk of x), as ortho_bip_kernel.
template <bool kMask, bool kVec>
__global__ __launch_bounds__(256) void ortho_merge_bip_kernel(const OrthoMergeArgs a) {
  __shared__ MergeLds l;
  const int nbx = (a.out_w + kOrthoPx - 1) / kOrthoPx;
  const int y = (int)(blockIdx.x / (uint32_t)nbx), x0 = (int)(blockIdx.x - (uint32_t)y * (uint32_t)nbx) * kOrthoPx;
  merge_resolve(a, y, x0, l);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int pend = min(min(kOrthoPx, a.out_w - x0), (wave + 1) * kOrthoPxWave);
  const int quads = a.bands >> 2, rest = a.bands & 3;
  float* row = a.out + ((int64_t)y * a.out_w + x0) * a.bands;
  for (int p0 = wave * kOrthoPxWave; p0 < pend; p0 += kOrthoAhead) {
    int first[kOrthoAhead];
#pragma unroll
    for (int j = 0; j < kOrthoAhead; ++j) first[j] = kMergeMax;
    for (int q = lane; q < quads; q += 64)
      merge_group<kMask, 4, kVec, kOrthoAhead>(a, l, p0, pend, 4 * q, first,
                                               [&](int p, const OrthoVec<4, kVec>& v) { v.store(row + (int64_t)p * a.bands + 4 * q); });
    if (!kVec && lane < rest)
      merge_group<kMask, 1, false, kOrthoAhead>(a, l, p0, pend, 4 * quads + lane, first, [&](int p, const OrthoVec<1, false>& v) {
        v.store(row + (int64_t)p * a.bands + 4 * quads + lane);
      });
    merge_note_winners<kOrthoAhead>(a, l, lane, p0, pend, first);
  }
  if (a.source) {
    __syncthreads();
    merge_store_winners(a, l, y, x0);
  }
}

// 512 threads and the tile of ortho_bsq_kernel: float e of quad q at word e quads + q of the pixel's tile row, the tail behind.
template <bool kMask>
__global__ __launch_bounds__(64 * kOrthoBsqWaves) void ortho_merge_bsq_kernel(const OrthoMergeArgs a) {
  extern __shared__ float s_tile[];                                    // [kOrthoPx][pitch]
  __shared__ MergeLds l;
  const int pitch = a.bands | 1;
  const int nbx = (a.out_w + kOrthoPx - 1) / kOrthoPx;
  const int y = (int)(blockIdx.x / (uint32_t)nbx), x0 = (int)(blockIdx.x - (uint32_t)y * (uint32_t)nbx) * kOrthoPx;
  merge_resolve(a, y, x0, l);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int pend = min(min(kOrthoPx, a.out_w - x0), (wave + 1) * kOrthoPxWaveBsq);
  const int quads = a.bands >> 2, rest = a.bands & 3;
  // a pixel whose first candidate is no spectrum (or that has none) is a constant: its tile row is neither written nor read
  for (int p0 = wave * kOrthoPxWaveBsq; p0 < pend; p0 += kOrthoAheadBsq) {
    int first[kOrthoAheadBsq];
#pragma unroll
    for (int j = 0; j < kOrthoAheadBsq; ++j) first[j] = kMergeMax;
    for (int q = lane; q < quads; q += 64)
      merge_group<kMask, 4, false, kOrthoAheadBsq>(a, l, p0, pend, 4 * q, first, [&](int p, const OrthoVec<4, false>& v) {
        if (l.use_tile[p]) {
          float* t = s_tile + p * pitch + q;
          t[0] = v.v[0], t[quads] = v.v[1], t[2 * quads] = v.v[2], t[3 * quads] = v.v[3];
        }
      });
    if (lane < rest)
      merge_group<kMask, 1, false, kOrthoAheadBsq>(a, l, p0, pend, 4 * quads + lane, first, [&](int p, const OrthoVec<1, false>& v) {
        if (l.use_tile[p]) s_tile[p * pitch + 4 * quads + lane] = v.v[0];
      });
    merge_note_winners<kOrthoAheadBsq>(a, l, lane, p0, pend, first);
  }
  __syncthreads();
  merge_store_winners(a, l, y, x0);
  const int x = x0 + lane;
  if (x >= a.out_w) return;
  const bool copy = l.use_tile[lane] != 0;
  const float constant = l.constant[lane];
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

extern "C" int hsr_merge_scenes(const hsr_merge_scene* scenes, int32_t n, int32_t layout, int32_t out_h, int32_t out_w, float nodata,
                                int32_t nan_is_nodata, float* out_dev, uint8_t* source_dev, hsr_stream_t stream) {
  MergeArgs a;
  const int rc = merge_scenes_args("hsr_merge_scenes", scenes, n, layout, out_h, out_w, nodata, nan_is_nodata, out_dev, source_dev, a);
  if (rc != HSR_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)out_h * (layout == 1 ? a.bands : 1);
  hipLaunchKernelGGL(merge_scenes_kernel, dim3((unsigned)(rows * a.nchunk)), dim3(kMergeThreads), 0, s, a);
  if (!source_dev) return launched(kLaunchMerge, "merge_scenes_kernel launch", kMergeScenes);
  const int64_t cells = (int64_t)out_h * out_w;
  hipLaunchKernelGGL(merge_source_kernel, dim3((unsigned)((cells + kMergeThreads - 1) / kMergeThreads)), dim3(kMergeThreads), 0, s, a);
  return launched(kLaunchMerge, "merge_scenes_kernel / merge_source_kernel launch", kMergeScenes, kMergeSource);
}

extern "C" int hsr_merge_scenes_host(const hsr_merge_scene* scenes, int32_t n, int32_t layout, int32_t out_h, int32_t out_w, float nodata,
                                     int32_t nan_is_nodata, float* out, uint8_t* source) {
  MergeArgs a;
  const int rc = merge_scenes_args("hsr_merge_scenes_host", scenes, n, layout, out_h, out_w, nodata, nan_is_nodata, out, source, a);
  if (rc != HSR_OK) return rc;
  merge_scenes_host(a);
  return HSR_OK;
}

extern "C" int hsr_ortho_merge(const hsr_merge_swath* swaths, int32_t n, int32_t glt_nodata, int32_t layout, int32_t out_h, int32_t out_w,
                               float nodata, float masked, float* out_dev, int64_t* dropped_dev, uint8_t* source_dev, hsr_stream_t stream) {
  const char* fn = "hsr_ortho_merge";
  HSR_REQUIRE(n >= 1 && n <= kMergeMax, HSR_ERR_INVALID, "%s: %d sources, 1 to %d", fn, n, kMergeMax);
  HSR_REQUIRE(swaths && out_dev, HSR_ERR_INVALID, "%s: NULL pointer", fn);
  HSR_REQUIRE(layout == 0 || layout == 1, HSR_ERR_INVALID, "%s: layout=%d (0 bip, 1 bsq)", fn, layout);
  HSR_REQUIRE(out_h >= 1 && out_w >= 1, HSR_ERR_INVALID, "%s: an output of %d x %d", fn, out_h, out_w);
  const int32_t bands = swaths[0].bands;
  HSR_REQUIRE(bands >= 1, HSR_ERR_INVALID, "%s: bands=%d", fn, bands);
  HSR_REQUIRE(bands <= kOrthoMaxBands, HSR_ERR_UNSUPPORTED, "%s: bands=%d above %d", fn, bands, kOrthoMaxBands);
  HSR_REQUIRE((int64_t)out_h * out_w <= 0x7fffffff, HSR_ERR_UNSUPPORTED, "%s: an output of %d x %d pixels, at most 2^31 - 1", fn, out_h,
              out_w);
  const int64_t cells = (int64_t)out_h * out_w, out_bytes = cells * bands * 4;
  const void* outs[3] = {out_dev, dropped_dev, source_dev};
  const int64_t out_sizes[3] = {out_bytes, (int64_t)n * 8, cells};
  OrthoMergeArgs a{};
  bool mask = false, vec = bands % 4 == 0 && ((uintptr_t)out_dev & 15) == 0;
  for (int k = 0; k < n; ++k) {
    const hsr_merge_swath& s = swaths[k];
    HSR_REQUIRE(s.swath_dev && s.glt_dev, HSR_ERR_INVALID, "%s: source %d has a NULL swath or GLT", fn, k);
    HSR_REQUIRE(s.rows >= 1 && s.cols >= 1 && s.glt_h >= 1 && s.glt_w >= 1, HSR_ERR_INVALID, "%s: source %d: swath %d x %d, GLT %d x %d", fn,
                k, s.rows, s.cols, s.glt_h, s.glt_w);
    HSR_REQUIRE(s.bands == bands, HSR_ERR_INVALID, "%s: source %d has %d bands, source 0 has %d", fn, k, s.bands, bands);
    HSR_REQUIRE(!s.bmask_dev || s.bmask_bytes >= (bands + 7) / 8, HSR_ERR_INVALID, "%s: source %d: bmask_bytes=%d, %d bands need %d", fn, k,
                s.bmask_bytes, bands, (bands + 7) / 8);
    HSR_REQUIRE((int64_t)s.rows * s.cols <= 0x7fffffff, HSR_ERR_UNSUPPORTED, "%s: source %d: a swath of %d x %d pixels, at most 2^31 - 1", fn,
                k, s.rows, s.cols);
    const int64_t px = (int64_t)s.rows * s.cols;
    const void* ins[4] = {s.swath_dev, s.glt_dev, s.qmask_dev, s.bmask_dev};
    const int64_t in_sizes[4] = {px * bands * 4, (int64_t)s.glt_h * s.glt_w * 8, px, px * s.bmask_bytes};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 4; ++j)
        HSR_REQUIRE(!ranges_overlap(outs[i], out_sizes[i], ins[j], in_sizes[j]), HSR_ERR_INVALID, "%s: an output overlaps an input of source %d",
                    fn, k);
    a.s[k] = OrthoMergeSrc{s.swath_dev, s.glt_dev, s.qmask_dev, s.bmask_dev, s.rows, s.cols, s.glt_h, s.glt_w, s.off_y, s.off_x,
                           s.bmask_dev ? s.bmask_bytes : 0, 0};
    mask = mask || s.qmask_dev || s.bmask_dev;
    vec = vec && ((uintptr_t)s.swath_dev & 15) == 0;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = i + 1; j < 3; ++j)
      HSR_REQUIRE(!ranges_overlap(outs[i], out_sizes[i], outs[j], out_sizes[j]), HSR_ERR_INVALID, "%s: two outputs overlap", fn);
  hipStream_t st = (hipStream_t)stream;
  if (dropped_dev) {
    const int rc = check_hip(hipMemsetAsync(dropped_dev, 0, sizeof(int64_t) * n, st), "hsr_ortho_merge: hipMemsetAsync");
    if (rc != HSR_OK) return rc;
  }
  a.out = out_dev;
  a.dropped = reinterpret_cast<unsigned long long*>(dropped_dev);
  a.source = source_dev;
  a.plane = cells;
  a.n = n, a.bands = bands, a.glt_nodata = glt_nodata, a.out_w = out_w;
  a.fill_empty = merge_empty(nodata, nodata, false), a.masked_empty = merge_empty(masked, nodata, false);
  a.nodata = nodata, a.masked = masked;
  const dim3 grid((unsigned)((int64_t)out_h * ((out_w + kOrthoPx - 1) / kOrthoPx)));       // <= out_h out_w <= INT32_MAX
  if (layout == 0) {
    if (mask && vec) hipLaunchKernelGGL((ortho_merge_bip_kernel<true, true>), grid, dim3(256), 0, st, a);
    else if (mask) hipLaunchKernelGGL((ortho_merge_bip_kernel<true, false>), grid, dim3(256), 0, st, a);
    else if (vec) hipLaunchKernelGGL((ortho_merge_bip_kernel<false, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((ortho_merge_bip_kernel<false, false>), grid, dim3(256), 0, st, a);
    return launched(kLaunchMerge, "ortho_merge_bip_kernel launch", kOrthoMergeBip + 2 * (mask ? 1 : 0) + (vec ? 1 : 0));
  }
  const size_t lds = (size_t)kOrthoPx * (size_t)(bands | 1) * sizeof(float);
  static thread_local size_t configured[2] = {};     // per kernel: ortho_merge_bsq_kernel<false>, <true>
  if (mask) {
    raise_lds_limit(reinterpret_cast<const void*>(ortho_merge_bsq_kernel<true>), lds, configured[1]);
    hipLaunchKernelGGL(ortho_merge_bsq_kernel<true>, grid, dim3(64 * kOrthoBsqWaves), lds, st, a);
  } else {
    raise_lds_limit(reinterpret_cast<const void*>(ortho_merge_bsq_kernel<false>), lds, configured[0]);
    hipLaunchKernelGGL(ortho_merge_bsq_kernel<false>, grid, dim3(64 * kOrthoBsqWaves), lds, st, a);
  }
  return launched(kLaunchMerge, "ortho_merge_bsq_kernel launch", kOrthoMergeBsq + (mask ? 1 : 0));
}

// ---- the grid (host only, float64; built with -ffp-contract=off: every operation is rounded on its own) --------------------------------
extern "C" int hsr_merge_grid(const double* geotransforms, const int32_t* shapes, int32_t n, const double* bounds, double* grid_gt,
                              int32_t* grid_shape, int32_t* offsets, double* residuals) {
  const char* fn = "hsr_merge_grid";
  const double kLimit = 1073741824.0;                                  // 2^30
  HSR_REQUIRE(n >= 1 && n <= kMergeMax, HSR_ERR_INVALID, "%s: %d sources, 1 to %d", fn, n, kMergeMax);
  HSR_REQUIRE(geotransforms && shapes && grid_gt && grid_shape && offsets && residuals, HSR_ERR_INVALID, "%s: NULL pointer", fn);
  for (int k = 0; k < n; ++k) {
    const double* g = geotransforms + 6 * k;
    for (int i = 0; i < 6; ++i) HSR_REQUIRE(isfinite(g[i]), HSR_ERR_INVALID, "%s: source %d: term %d of the geotransform is not finite", fn, k, i);
    HSR_REQUIRE(shapes[2 * k] >= 1 && shapes[2 * k + 1] >= 1, HSR_ERR_INVALID, "%s: source %d is %d x %d", fn, k, shapes[2 * k], shapes[2 * k + 1]);
    HSR_REQUIRE(g[2] == 0.0 && g[4] == 0.0, HSR_ERR_UNSUPPORTED, "%s: source %d has rotation terms (%g, %g)", fn, k, g[2], g[4]);
  }
  const double dx = geotransforms[1], dy = geotransforms[5];
  HSR_REQUIRE(dx > 0.0 && dy != 0.0, HSR_ERR_INVALID, "%s: a pixel size of (%g, %g): dx > 0 and dy != 0", fn, dx, dy);
  for (int k = 1; k < n; ++k) {
    const double* g = geotransforms + 6 * k;
    const double ex = fabs(g[1] / dx - 1.0) * shapes[2 * k + 1], ey = fabs(g[5] / dy - 1.0) * shapes[2 * k];
    HSR_REQUIRE(ex <= 0.01 && ey <= 0.01, HSR_ERR_UNSUPPORTED,
                "%s: the pixel size of source %d (%.17g, %.17g) differs from source 0's (%.17g, %.17g) by (%g, %g) pixels over its extent, at most 0.01",
                fn, k, g[1], g[5], dx, dy, ex, ey);
  }
  double X0, Y0;
  if (bounds) {
    for (int i = 0; i < 4; ++i) HSR_REQUIRE(isfinite(bounds[i]), HSR_ERR_INVALID, "%s: bounds[%d] is not finite", fn, i);
    HSR_REQUIRE(bounds[0] < bounds[2] && bounds[1] < bounds[3], HSR_ERR_INVALID, "%s: bounds (%g, %g, %g, %g): left < right and bottom < top", fn,
                bounds[0], bounds[1], bounds[2], bounds[3]);
    X0 = bounds[0];
    Y0 = dy < 0.0 ? bounds[3] : bounds[1];
  } else {
    X0 = geotransforms[0], Y0 = geotransforms[3];
    for (int k = 1; k < n; ++k) {
      const double* g = geotransforms + 6 * k;
      X0 = g[0] < X0 ? g[0] : X0;
      Y0 = dy < 0.0 ? (g[3] > Y0 ? g[3] : Y0) : (g[3] < Y0 ? g[3] : Y0);
    }
  }
  double W = 0.0, H = 0.0;
  for (int k = 0; k < n; ++k) {
    const double* g = geotransforms + 6 * k;
    const double fx = (g[0] - X0) / dx, fy = (g[3] - Y0) / dy;
    const double ox = floor(fx + 0.5), oy = floor(fy + 0.5);
    HSR_REQUIRE(fabs(ox) <= kLimit && fabs(oy) <= kLimit, HSR_ERR_INVALID, "%s: source %d lies (%g, %g) cells from the origin, at most 2^30", fn, k,
                oy, ox);
    offsets[2 * k] = (int32_t)oy, offsets[2 * k + 1] = (int32_t)ox;
    residuals[2 * k] = fy - oy, residuals[2 * k + 1] = fx - ox;
    W = ox + shapes[2 * k + 1] > W ? ox + shapes[2 * k + 1] : W;
    H = oy + shapes[2 * k] > H ? oy + shapes[2 * k] : H;
  }
  if (bounds) {
    W = floor((bounds[2] - bounds[0]) / dx + 0.5);
    H = floor((bounds[3] - bounds[1]) / fabs(dy) + 0.5);
    W = W < 1.0 ? 1.0 : W, H = H < 1.0 ? 1.0 : H;
  }
  HSR_REQUIRE(W <= kLimit && H <= kLimit, HSR_ERR_INVALID, "%s: a grid of %g x %g cells, at most 2^30 a side", fn, H, W);
  grid_gt[0] = X0, grid_gt[1] = dx, grid_gt[2] = 0.0, grid_gt[3] = Y0, grid_gt[4] = 0.0, grid_gt[5] = dy;
  grid_shape[0] = (int32_t)H, grid_shape[1] = (int32_t)W;
  return HSR_OK;
}
