// Shared helpers of libhsr_mi355x (gfx950 only; no portability layer on purpose).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/hsr.h"

namespace hsr {

void set_error(const char* fmt, ...);

inline int check_hip(hipError_t e, const char* what) {
  if (e == hipSuccess) return HSR_OK;
  set_error("%s: %s", what, hipGetErrorString(e));
  return HSR_ERR_HIP;
}

#define HSR_REQUIRE(cond, code, ...)  \
  do {                                \
    if (!(cond)) {                    \
      hsr::set_error(__VA_ARGS__);    \
      return (code);                  \
    }                                 \
  } while (0)

#define HSR_LAUNCH_CHECK(name)                                   \
  do {                                                           \
    int rc_ = hsr::check_hip(hipGetLastError(), name " launch"); \
    if (rc_ != HSR_OK) return rc_;                               \
  } while (0)

// Kernel instances of hsr_select.hip, hsr_resample.hip and hsr_tile.hip, the index of the name table behind hsr_aux_last_launch /
// hsr_aux_instance_name (csrc/hsr_lib.hip).  A family's instances are consecutive: base + template-argument offset.
enum AuxInstance : int {
  kAuxSelectHist = 0,                      // + (PASS - 1) * 2 + MODE
  kAuxSelectRows4 = kAuxSelectHist + 6,    // + PASS - 1
  kAuxSelectScan = kAuxSelectRows4 + 3,    // + PASS - 1
  kAuxSelectTiny = kAuxSelectScan + 3,
  kAuxBlockMeanTile = kAuxSelectTiny + 1,  // + in_dtype (0 float, 1 uint8_t, 2 uint16_t)
  kAuxBlockMean = kAuxBlockMeanTile + 3,   // + in_dtype
  kAuxBilinearUp = kAuxBlockMean + 3,      // + VEC4 + IN4: <false, false>, <true, false>, <true, true>
  kAuxBilinearUpHist = kAuxBilinearUp + 3, // + IN4
  kAuxTileEncode = kAuxBilinearUpHist + 2, // + vec
  kAuxTileDecode = kAuxTileEncode + 2,     // + vec
  kAuxTranspose = kAuxTileDecode + 2,      // + 0 <float, float>, 1 <uint16_t, uint16_t>, 2 <uint16_t, float>, 3 <int16_t, float>
  kAuxInstances = kAuxTranspose + 4
};

// Kernel instances of hsr_scene.hip, the index of the name table behind hsr_scene_last_launch / hsr_scene_instance_name
// (csrc/hsr_lib.hip): a table of its own, so the auxiliary one keeps its 32 names.  base + template-argument offset, as above.
enum SceneInstance : int {
  kSceneBlack = 0,                         // + 0 <float>, 1 <uint16_t>
  kSceneGather = kSceneBlack + 2,          // + 2 * (0 <float, float, false>, 1 <uint16_t, uint16_t, false>, 2 <float, uint16_t, true>) + kVec
  kSceneMosaic = kSceneGather + 6,         // + kVec
  kSceneBlend = kSceneMosaic + 2,          // + 5 * kVec + log2(KMAX): KMAX 1, 2, 4, 8, 16
  kSceneInstances = kSceneBlend + 10
};

// Kernel instances of hsr_ridge.hip, hsr_gram.hip and hsr_chol.hip (K4), the index of the name table behind hsr_k4_last_launch /
// hsr_k4_instance_name (csrc/hsr_lib.hip).  A family's instances are consecutive: base + offset.
enum K4Instance : int {
  kK4Expand = 0,
  kK4PairExpand,
  kK4StatsPartial,
  kK4StatsFinish,
  kK4Assemble,
  kK4Finish,
  kK4Predict,                              // + 0 <1>, 1 <2>, 2 <4>
  kK4PredictX16 = kK4Predict + 3,          // + arm of pred_load10 (0 x2, 1 scalar)
  kK4PredictSlice = kK4PredictX16 + 2,     // + (TT - 1) * 2 + arm
  kK4GramLds = kK4PredictSlice + 6,        // + kinds - 1 (bit 0 wide, bit 1 diag, bit 2 narrow)
  kK4GramReg = kK4GramLds + 7,             // + 0 sym, 1 full
  kK4GramReduce = kK4GramReg + 2,
  kK4CholFactorRes,
  kK4CholFactor,
  kK4CholSolve,                            // + 0 block inverses in LDS, 1 in global memory
  kK4Instances = kK4CholSolve + 2
};

// Kernel instances of hsr_pairs.hip, the index of the name table behind hsr_pairs_last_launch / hsr_pairs_instance_name
// (csrc/hsr_lib.hip): a table of its own, so the K4 one keeps its 31 names (pair_expand_f64_kernel stays there).
enum PairsInstance : int {
  kPairsPrep = 0,
  kPairsStats,
  kPairsReportPartial,
  kPairsReportFinish,
  kPairsHoldout,
  kPairsScorePartial,                      // + kVec
  kPairsScoreFinish = kPairsScorePartial + 2,
  kPairsPoolStats,
  kPairsPoolGram,                          // + kVec
  kPairsPoolModels = kPairsPoolGram + 2,
  kPairsInstances
};

// Kernel instances of hsr_ortho.hip, the index of the name table behind hsr_ortho_last_launch / hsr_ortho_instance_name
// (csrc/hsr_lib.hip): a table of its own, so the scene one keeps its 20 names.
enum OrthoInstance : int {
  kOrthoBip = 0,                           // + 2 * kMask + kVec
  kOrthoBsq = kOrthoBip + 4,               // + kMask
  kOrthoInstances = kOrthoBsq + 2
};

// Kernel instances of hsr_color.hip, the index of the name table behind hsr_color_last_launch / hsr_color_instance_name
// (csrc/hsr_lib.hip, include/hsr_color.h): a table of its own, so the five others keep their sizes.
enum ColorInstance : int {
  kColorMoments = 0,                       // + 3 * LX + LY (load modes of x and y: 0 dword, 1 padded rows, 2 packed rows)
  kColorMomentsF64 = kColorMoments + 9,
  kColorReduceSolve,
  kColorApply,                             // + 3 * LIN + LOUT
  kColorInstances = kColorApply + 9
};

// Kernel instances of hsr_coreg.hip, the index of the name table behind hsr_coreg_last_launch / hsr_coreg_instance_name
// (csrc/hsr_lib.hip, include/hsr_coreg.h): a table of its own, so the six others keep their sizes.
enum CoregInstance : int {
  kCoregSurface = 0,                       // + 0 <float>, 1 <uint16_t>
  kCoregPeaks = kCoregSurface + 2,
  kCoregFitModel,
  kCoregWarp,                              // + 2 * (0 <float>, 1 <uint16_t>) + (0 LDS, 1 DIRECT)
  kCoregInstances = kCoregWarp + 4
};

// Kernel instances of hsr_reproject.hip, the index of the name table behind hsr_reproject_last_launch / hsr_reproject_instance_name
// (csrc/hsr_lib.hip, include/hsr_reproject.h): a table of its own, so the seven others keep their sizes.
enum ReprojectInstance : int {
  kReprojectCoords = 0,
  kReprojectWarp,                          // + 2 * (0 LDS, 1 DIRECT) + (0 STRICT, 1 RENORM)
  kReprojectInstances = kReprojectWarp + 4
};

// Kernel instances of hsr_scl.hip, the index of the name table behind hsr_scl_last_launch / hsr_scl_instance_name
// (csrc/hsr_lib.hip, include/hsr_scl.h): a table of its own, so the eight others keep their sizes.
enum SclInstance : int {
  kSclCounts = 0,
  kSclMask,                                // + 0 LOOKUP, 1 DISC, 2 SQUARE
  kSclCoarse = kSclMask + 3,
  kSclGather,
  kSclApply,                               // + 0 UP1, 1 UP2
  kSclInstances = kSclApply + 2
};

// Kernel instances of hsr_s2stack.hip, the index of the name table behind hsr_s2stack_last_launch / hsr_s2stack_instance_name
// (csrc/hsr_lib.hip, include/hsr_s2stack.h): a table of its own, so the nine others keep their sizes.
enum S2StackInstance : int {
  kS2Stack = 0,                            // + 2 * (0 U16, 1 F32) + (0 STRICT, 1 RENORM)
  kS2Expand = kS2Stack + 4,                // + 0 UP1, 1 UP2
  kS2StackInstances = kS2Expand + 2
};

// Kernel instances of hsr_hist.hip, the index of the name table behind hsr_hist_last_launch / hsr_hist_instance_name
// (csrc/hsr_lib.hip, include/hsr_hist.h): a table of its own, so the ten others keep their sizes.
enum HistInstance : int {
  kHistKeys = 0,                           // + 0 PIXMAJOR, 1 PLANAR
  kHistCount = kHistKeys + 2,              // + pass (digit 0..3)
  kHistScan = kHistCount + 4,
  kHistScatter,                            // + pass
  kHistPivots = kHistScatter + 4,
  kHistLookup,                             // + 0 PIXMAJOR, 1 PLANAR
  kHistInstances = kHistLookup + 2
};

// Kernel instances of hsr_resize.hip, the index of the name table behind hsr_resize_last_launch / hsr_resize_instance_name
// (csrc/hsr_lib.hip, include/hsr_resize.h): a table of its own, so the eleven others keep their sizes.
enum ResizeInstance : int {
  kAreaStaged = 0,                         // + 5 * (0 PLANAR, 1 PIXMAJOR) + pair: 0 <F32, F32>, 1 <U8, U8>, 2 <U8, F32>, 3 <U16, U16>, 4 <U16, F32>
  kAreaGather = kAreaStaged + 10,          // + pair
  kResizeInstances = kAreaGather + 5
};

// Kernel instances of hsr_merge.hip, the index of the name table behind hsr_merge_last_launch / hsr_merge_instance_name
// (csrc/hsr_lib.hip, include/hsr_merge.h): a table of its own, so the twelve others keep their sizes.
enum MergeInstance : int {
  kOrthoMergeBip = 0,                      // + 2 * kMask + kVec
  kOrthoMergeBsq = kOrthoMergeBip + 4,     // + kMask
  kMergeScenes = kOrthoMergeBsq + 2,
  kMergeSource,
  kMergeInstances
};

// Kernel instances of hsr_roi.hip, the index of the name table behind hsr_roi_last_launch / hsr_roi_instance_name
// (csrc/hsr_lib.hip, include/hsr_roi.h): a table of its own, so the thirteen others keep their sizes.
enum RoiInstance : int {
  kRoiRaster = 0,                          // + rule (0 CENTER, 1 TOUCHED)
  kRoiCounts = kRoiRaster + 2,             // + rule
  kRoiRecordInit = kRoiCounts + 2,
  kRoiGltClip,
  kRoiGltReindex,
  kRoiInstances
};

// HSR_LAUNCH_CHECK of an entry point's one or two launches (second < 0: one) that also appends their instances, in launch order,
// to the calling thread's record of family f on success (hsr_{aux,scene,k4,pairs,ortho,color,coreg,reproject,scl,s2stack,hist,resize,merge,roi}_last_launch,
// csrc/hsr_lib.hip).
enum LaunchFamily : int { kLaunchAux, kLaunchScene, kLaunchK4, kLaunchPairs, kLaunchOrtho, kLaunchColor, kLaunchCoreg, kLaunchReproject, kLaunchScl,
                          kLaunchS2Stack, kLaunchHist, kLaunchResize, kLaunchMerge, kLaunchRoi, kLaunchFamilies };
int launched(LaunchFamily f, const char* what, int first, int second = -1);

// Raises a kernel's dynamic-LDS limit when a launch needs more than `configured` (the caller's cache slot, one per kernel)
// records, and clears the error a refused request leaves: the launch itself then reports it.
inline void raise_lds_limit(const void* kernel, size_t bytes, size_t& configured) {
  if (bytes <= configured) return;
  (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  (void)hipGetLastError();
  configured = bytes;
}

// Internal entry of hsr_srf.hip for the step executor (hsr_exec.hip); not part of the C ABI.
// srf_bind_launch_events: the next K1 launch of this thread (hsr_srf_integrate_moments* and their _apply forms) goes out with
// these timing events bound to its dispatch (hipExtLaunchKernelGGL) instead of two marker packets round it; either may be NULL.
// The record is consumed by that launch; a caller whose launch call failed early clears it with (NULL, NULL).
void srf_bind_launch_events(hipEvent_t start, hipEvent_t stop);

constexpr int kWave = 64;

// Number of moments for a degree.
__host__ __device__ constexpr int moment_count(int deg) { return 3 * deg + 2; }

// Partial slots: fixed function of the pixel count only, so that the summation tree (and with it
// every bit of the fitted coefficients) does not depend on the device or the launch environment.
inline int partial_slots(int64_t npix) {
  int64_t tiles = (npix + HSR_TILE_PIXELS - 1) / HSR_TILE_PIXELS;
  if (tiles < 1) tiles = 1;
  return (int)(tiles < 512 ? tiles : 512);  // 256 CUs x 2 resident workgroups
}

// Streaming (non-temporal) accesses: everything on this path is touched exactly once, and letting
// the 1.2 GB cube stream allocate in the 4 MB L2s evicts the dirty output lines early - measured on
// K1: 0.2285 ms with plain loads, 0.2002 ms with `nt` on the LDS-DMA, 0.1957 ms with `nt` stores too.
typedef float native_f32x4 __attribute__((ext_vector_type(4)));
template <typename T>
__device__ __forceinline__ T ld_stream(const T* p) { return __builtin_nontemporal_load(p); }
template <typename T>
__device__ __forceinline__ void st_stream(T* p, T v) { __builtin_nontemporal_store(v, p); }
// HIP's float4 is a struct; the builtins want the native vector type (same size and alignment)
__device__ __forceinline__ float4 ld_stream(const float4* p) {
  const native_f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const native_f32x4*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st_stream(float4* p, float4 v) {
  native_f32x4 n = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(n, reinterpret_cast<native_f32x4*>(p));
}
constexpr int kGldsStream = 2;  // aux/cpol bits of global_load_lds: 2 = nt

__device__ __forceinline__ bool finite_f32(float v) {
  return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u;
}

// One sample of the uint16 tile format, the reference writer's rule (tiles_helpers/utils.py:362-374; the statements are spelled
// out in hsr_tile.hip): used by hsr_tile_encode_u16 and by the encoding gather of hsr_scene.hip, which must give the same bits.
__device__ __forceinline__ uint16_t encode_sample(float x, float scale, bool has_src_nodata, float src_nodata,
                                                  int32_t nodata_u16) {
  const bool valid = finite_f32(x) && !(has_src_nodata && x == src_nodata);
  if (!valid) return (uint16_t)nodata_u16;
  const float r = rintf(x * scale);   // -ffp-contract=off: the product is rounded to float32 first
  int32_t q;
  if (!(r >= -2147483648.0f && r < 2147483648.0f)) q = INT32_MIN;   // x86 "integer indefinite"
  else q = (int32_t)r;
  q = q < 0 ? 0 : (q > nodata_u16 - 1 ? nodata_u16 - 1 : q);
  return (uint16_t)q;
}

// float32(clip((v - lo) / (hi - lo + 1e-12), 0, 1)) in float64, as s2_emit/color.py:33 evaluates it
// (np.percentile returns float64 limits, so the whole expression is float64 before the store).
__device__ __forceinline__ float stretch_f64(float v, double lo, double hi) {
  double r = ((double)v - lo) / (hi - lo + 1e-12);
  r = r < 0.0 ? 0.0 : (r > 1.0 ? 1.0 : r);  // NaN falls through both compares, like np.clip
  return (float)r;
}

}  // namespace hsr
