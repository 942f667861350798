// What the swath -> scene gather (csrc/hsr_ortho.hip, hsr_ortho_glt) and the merging gather of N swaths (csrc/hsr_merge.hip,
// hsr_ortho_merge) share, so that a cell of one source means the same thing in both: the geometry of a workgroup, the decision
// on one lookup-table entry, the E floats a lane moves and the masked value of a swath pixel.  Device code only; the contract is
// the comment above hsr_ortho_glt in include/hsr.h.
#pragma once
#include "hsr_common.h"

#include <type_traits>

namespace hsr {

constexpr int kOrthoPx = 64;           // output pixels of a workgroup, consecutive in x
constexpr int kOrthoPxWave = 16;       // ... of one wave
constexpr int kOrthoAhead = 4;         // spectra a wave has in flight: bip (up to 8 wave slots a SIMD)
constexpr int kOrthoBsqWaves = 8;      // bsq: 512 threads share the workgroup's pixels, the tile leaves room for two workgroups
constexpr int kOrthoPxWaveBsq = 8;     // a CU at 285 bands, so a wave takes 8 pixels and has all 8 spectra in flight
constexpr int kOrthoAheadBsq = 8;
constexpr int kOrthoMaxBands = 512;    // the bsq tile: 64 x 513 floats = 128.25 KiB of the CU's 160 KiB of LDS
static_assert(kOrthoPx == 4 * kOrthoPxWave && kOrthoPxWave % kOrthoAhead == 0, "bip: four waves share the workgroup's pixels");
static_assert(kOrthoPx == kOrthoBsqWaves * kOrthoPxWaveBsq && kOrthoPxWaveBsq % kOrthoAheadBsq == 0, "bsq: eight waves share them");

enum OrthoKind : int { kOrthoFill = 0, kOrthoCopy = 1, kOrthoMasked = 2 };

// One entry (xv, yv) of a lookup table against a swath of rows x cols pixels: kOrthoFill (no data; or outside the swath: `drop`),
// kOrthoMasked (quality mask == 1) or kOrthoCopy, and the swath pixel index sy cols + sx in `src`.
// xv - 1 and yv - 1 are formed in 64 bits, so INT32_MIN stays negative; an entry outside the swath is never used as an index.
__device__ __forceinline__ int ortho_entry(int32_t xv, int32_t yv, int32_t glt_nodata, int32_t rows, int32_t cols, const uint8_t* qmask,
                                           int& src, bool& drop) {
  int kind = kOrthoFill;
  if (xv != glt_nodata && yv != glt_nodata) {
    const int64_t sx = (int64_t)xv - 1, sy = (int64_t)yv - 1;
    if (sx >= 0 && sx < cols && sy >= 0 && sy < rows) {
      src = (int)(sy * cols + sx);                                     // rows cols <= INT32_MAX (checked on the host)
      kind = (qmask && qmask[src] == 1) ? kOrthoMasked : kOrthoCopy;
    } else {
      drop = true;
    }
  }
  return kind;
}

// E floats of one lane.  E == 4 moves them as ONE 16-byte access: kAligned says the address lies on 16 bytes; without it the
// vector type is only dword-aligned, which global loads and stores of gfx950 take as they are (a pixel base is bands * 4 bytes
// times the pixel index: on 16 bytes for every fourth pixel only when bands % 4 != 0).
typedef float ortho_f4a __attribute__((ext_vector_type(4)));
typedef float ortho_f4u __attribute__((ext_vector_type(4), aligned(4)));
template <int E, bool kAligned>
struct OrthoVec;
template <bool kAligned>
struct OrthoVec<1, kAligned> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = p[0]; }
  __device__ __forceinline__ void store(float* p) const { st_stream(p, v[0]); }
};
template <bool kAligned>
struct OrthoVec<4, kAligned> {
  using T = std::conditional_t<kAligned, ortho_f4a, ortho_f4u>;
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const T q = *reinterpret_cast<const T*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  }
  __device__ __forceinline__ void store(float* p) const {
    const T q = {v[0], v[1], v[2], v[3]};
    __builtin_nontemporal_store(q, reinterpret_cast<T*>(p));
  }
};

// Bands b .. b + E - 1 (b % E == 0, so they share one byte of the band mask) of pixel `src`: the constant of a fill or masked
// pixel; else the bits of the swath, `masked` where the band's bit - np.unpackbits' order, the highest bit first - is set.
// A: anything with swath, bands, bmask, bmask_bytes and masked (OrthoArgs; one source of a merge).
template <bool kMask, int E, bool kAligned, typename A>
__device__ __forceinline__ void ortho_value(const A& a, int kind, float constant, int src, int b, OrthoVec<E, kAligned>& o) {
  if (kind != kOrthoCopy) {
#pragma unroll
    for (int e = 0; e < E; ++e) o.v[e] = constant;
    return;
  }
  o.load(a.swath + (int64_t)src * a.bands + b);
  if constexpr (kMask) {
    if (a.bmask) {
      const uint32_t byte = a.bmask[(int64_t)src * a.bmask_bytes + (b >> 3)];
#pragma unroll
      for (int e = 0; e < E; ++e) o.v[e] = ((byte >> (7 - ((b + e) & 7))) & 1u) ? a.masked : o.v[e];
    }
  }
}

}  // namespace hsr
