// Library-level entry points of libhsr_mi355x: error state, sizing helpers, and a pure-read
// bandwidth probe used by bench.py to put the HBM roofline of THIS box next to the vendor peak.
#include <string.h>

#include "hsr_common.h"
#include "../../include/hsr_color.h"
#include "../../include/hsr_coreg.h"
#include "../../include/hsr_reproject.h"
#include "../../include/hsr_scl.h"
#include "../../include/hsr_s2stack.h"
#include "../../include/hsr_hist.h"
#include "../../include/hsr_resize.h"
#include "../../include/hsr_merge.h"
#include "../../include/hsr_roi.h"

namespace hsr {

static thread_local char g_error[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}

// Streams `n16` 16-byte words once and folds them into one float per workgroup (kept so the loads
// cannot be eliminated).  Same access shape and cache policy as the cube stream of K1: 16 B per lane,
// coalesced, non-temporal.
__global__ __launch_bounds__(256) void probe_read_kernel(const float4* __restrict__ src, int64_t n16,
                                                         float* __restrict__ sink) {
  float acc = 0.0f;
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n16; i += 4 * stride) {
    const float4 a = hsr::ld_stream(src + i), b = hsr::ld_stream(src + i + stride), c = hsr::ld_stream(src + i + 2 * stride),
                 d = hsr::ld_stream(src + i + 3 * stride);
    acc += (a.x + a.y + a.z + a.w) + (b.x + b.y + b.z + b.w) + (c.x + c.y + c.z + c.w) + (d.x + d.y + d.z + d.w);
  }
  for (; i < n16; i += stride) {
    const float4 a = hsr::ld_stream(src + i);
    acc += a.x + a.y + a.z + a.w;
  }
  acc += __shfl_xor(acc, 32, 64);
  acc += __shfl_xor(acc, 16, 64);
  acc += __shfl_xor(acc, 8, 64);
  acc += __shfl_xor(acc, 4, 64);
  acc += __shfl_xor(acc, 2, 64);
  acc += __shfl_xor(acc, 1, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(&sink[blockIdx.x & 63], acc);
}

// The load shape of K1 with nothing else: 512 persistent workgroups of 512 threads (2 per CU), each streaming
// 72 KiB slabs (workgroup b takes slabs b, b + grid, ...) HBM -> LDS with non-temporal global_load_lds_dwordx4,
// one barrier per slab, nothing read back.  What this kernel reaches is the ceiling of K1's staging structure on
// this box (round 1 lab: 6.9 TB/s); a plain global_load stream (mode 1) reads 5.6 TB/s.
constexpr int kProbeSlab = 72 * 1024;
// SLAB bytes per barrier: 72 KiB = a float32 group of K1 (modes 0), 36 KiB = a uint16 group (modes 2, 3).
template <int SLAB>
__global__ __launch_bounds__(512, 4) void probe_lds_dma_kernel(const char* __restrict__ src, int64_t n16, float* __restrict__ sink) {
  extern __shared__ __attribute__((aligned(16))) unsigned char psmem[];
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr int kChunks = SLAB / 16;
  const int64_t nslabs = (n16 + kChunks - 1) / kChunks;
  for (int64_t sl = blockIdx.x; sl < nslabs; sl += gridDim.x) {
    const int64_t base = sl * kChunks;
    const int64_t left = n16 - base;
    const int nch = left < kChunks ? (int)left : kChunks;
    for (int c0 = wave * 64; c0 < nch; c0 += 512) {
      const int c = c0 + lane;
      if (c < nch)
        __builtin_amdgcn_global_load_lds((gptr_t)(src + (base + c) * 16), (lptr_t)(psmem + (size_t)c0 * 16), 16, 0, kGldsStream);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && blockIdx.x == 0) sink[0] = reinterpret_cast<const float*>(psmem)[0];   // keeps the LDS image observable
}

template <int SLAB>
static int launch_probe_lds(const void* buf, int64_t bytes, int lds_bytes, int grid_cap, float* sink, hipStream_t stream) {
  auto kern = probe_lds_dma_kernel<SLAB>;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  (void)hipGetLastError();
  const int64_t nslabs = (bytes + SLAB - 1) / SLAB;
  hipLaunchKernelGGL(kern, dim3((unsigned)(nslabs < grid_cap ? nslabs : grid_cap)), dim3(512), lds_bytes, stream,
                     (const char*)buf, bytes / 16, sink);
  HSR_LAUNCH_CHECK("probe_lds_dma_kernel");
  return HSR_OK;
}

// Launch records (hsr_{aux,scene,k4,pairs,ortho,color,coreg,reproject,scl,s2stack,hist,resize,merge,roi}_last_launch): per family and thread, the kernels launched successfully since the last
// read, as indices of the family's name table (the instance enums of hsr_common.h) in launch order; the oldest is dropped when
// the list is full.  Indices turn into names only when read.
static const char* const kAuxNames[] = {
    "select_hist_kernel<1, 0>", "select_hist_kernel<1, 1>", "select_hist_kernel<2, 0>", "select_hist_kernel<2, 1>",
    "select_hist_kernel<3, 0>", "select_hist_kernel<3, 1>",
    "select_hist_rows4_kernel<1>", "select_hist_rows4_kernel<2>", "select_hist_rows4_kernel<3>",
    "select_scan_kernel<1>", "select_scan_kernel<2>", "select_scan_kernel<3>",
    "select_tiny_kernel",
    "block_mean_tile_kernel<float>", "block_mean_tile_kernel<uint8_t>", "block_mean_tile_kernel<uint16_t>",
    "block_mean_kernel<float>", "block_mean_kernel<uint8_t>", "block_mean_kernel<uint16_t>",
    "bilinear_up_kernel<false, false>", "bilinear_up_kernel<true, false>", "bilinear_up_kernel<true, true>",
    "bilinear_up_hist_kernel<false>", "bilinear_up_hist_kernel<true>",
    "tile_encode_kernel scalar", "tile_encode_kernel vec",
    "tile_decode_kernel scalar", "tile_decode_kernel vec",
    "transpose_rc_kernel<float, float>", "transpose_rc_kernel<uint16_t, uint16_t>", "transpose_rc_kernel<uint16_t, float>",
    "transpose_rc_kernel<int16_t, float>",
};
static const char* const kSceneNames[] = {
    "scene_black_kernel<float>", "scene_black_kernel<uint16_t>",
    "scene_gather_kernel<float, float, false, false>", "scene_gather_kernel<float, float, false, true>",
    "scene_gather_kernel<uint16_t, uint16_t, false, false>", "scene_gather_kernel<uint16_t, uint16_t, false, true>",
    "scene_gather_kernel<float, uint16_t, true, false>", "scene_gather_kernel<float, uint16_t, true, true>",
    "scene_mosaic_kernel<false>", "scene_mosaic_kernel<true>",
    "scene_blend_kernel<false, 1>", "scene_blend_kernel<false, 2>", "scene_blend_kernel<false, 4>", "scene_blend_kernel<false, 8>",
    "scene_blend_kernel<false, 16>",
    "scene_blend_kernel<true, 1>", "scene_blend_kernel<true, 2>", "scene_blend_kernel<true, 4>", "scene_blend_kernel<true, 8>",
    "scene_blend_kernel<true, 16>",
};
static const char* const kK4Names[] = {
    "expand_f64_kernel", "pair_expand_f64_kernel", "ridge_stats_partial_kernel", "ridge_stats_finish_kernel",
    "ridge_assemble_kernel", "ridge_finish_kernel",
    "predict_kernel<1>", "predict_kernel<2>", "predict_kernel<4>",
    "predict103_x16_kernel x2", "predict103_x16_kernel scalar",
    "predict103_slice_kernel<1> x2", "predict103_slice_kernel<1> scalar",
    "predict103_slice_kernel<2> x2", "predict103_slice_kernel<2> scalar",
    "predict103_slice_kernel<3> x2", "predict103_slice_kernel<3> scalar",
    "gram_f64_lds_kernel wide", "gram_f64_lds_kernel diag", "gram_f64_lds_kernel wide+diag", "gram_f64_lds_kernel narrow",
    "gram_f64_lds_kernel wide+narrow", "gram_f64_lds_kernel diag+narrow", "gram_f64_lds_kernel wide+diag+narrow",
    "gram_f64_kernel sym", "gram_f64_kernel full",
    "gram_reduce_kernel",
    "chol_factor_res_kernel", "chol_factor_kernel",
    "chol_solve_kernel lds", "chol_solve_kernel global",
};
static const char* const kPairsNames[] = {
    "pair_prep_kernel", "pair_stats_kernel", "pair_report_partial_kernel", "pair_report_finish_kernel", "pair_holdout_kernel",
    "pair_score_partial_kernel<false>", "pair_score_partial_kernel<true>", "pair_score_finish_kernel",
    "pool_stats_kernel", "pool_gram_kernel<false>", "pool_gram_kernel<true>", "pool_models_kernel",
};
static const char* const kOrthoNames[] = {
    "ortho_bip_kernel<false, false>", "ortho_bip_kernel<false, true>", "ortho_bip_kernel<true, false>", "ortho_bip_kernel<true, true>",
    "ortho_bsq_kernel<false>", "ortho_bsq_kernel<true>",
};
static const char* const kColorNames[] = {
    "affine_moments_kernel<0, 0>", "affine_moments_kernel<0, 1>", "affine_moments_kernel<0, 2>",
    "affine_moments_kernel<1, 0>", "affine_moments_kernel<1, 1>", "affine_moments_kernel<1, 2>",
    "affine_moments_kernel<2, 0>", "affine_moments_kernel<2, 1>", "affine_moments_kernel<2, 2>",
    "affine_moments_f64_kernel", "affine_reduce_solve_kernel",
    "affine_apply_kernel<0, 0>", "affine_apply_kernel<0, 1>", "affine_apply_kernel<0, 2>",
    "affine_apply_kernel<1, 0>", "affine_apply_kernel<1, 1>", "affine_apply_kernel<1, 2>",
    "affine_apply_kernel<2, 0>", "affine_apply_kernel<2, 1>", "affine_apply_kernel<2, 2>",
};
static const char* const kCoregNames[] = {
    "coreg_surface_kernel<float>", "coreg_surface_kernel<uint16_t>", "coreg_peaks_kernel", "coreg_fit_model_kernel",
    "coreg_warp_kernel<float, LDS>", "coreg_warp_kernel<float, DIRECT>",
    "coreg_warp_kernel<uint16_t, LDS>", "coreg_warp_kernel<uint16_t, DIRECT>",
};
static const char* const kReprojectNames[] = {
    "reproject_coords_kernel",
    "reproject_warp_kernel<LDS, STRICT>", "reproject_warp_kernel<LDS, RENORM>",
    "reproject_warp_kernel<DIRECT, STRICT>", "reproject_warp_kernel<DIRECT, RENORM>",
};
static const char* const kSclNames[] = {
    "scl_counts_kernel", "scl_mask_kernel<LOOKUP>", "scl_mask_kernel<DISC>", "scl_mask_kernel<SQUARE>", "scl_coarse_kernel",
    "scl_gather_kernel", "scl_apply_kernel<UP1>", "scl_apply_kernel<UP2>",
};
static const char* const kS2StackNames[] = {
    "s2_stack_kernel<U16, STRICT>", "s2_stack_kernel<U16, RENORM>", "s2_stack_kernel<F32, STRICT>", "s2_stack_kernel<F32, RENORM>",
    "s2_expand_kernel<UP1>", "s2_expand_kernel<UP2>",
};
static const char* const kHistNames[] = {
    "hist_keys_kernel<PIXMAJOR>", "hist_keys_kernel<PLANAR>",
    "hist_count_kernel<0>", "hist_count_kernel<1>", "hist_count_kernel<2>", "hist_count_kernel<3>",
    "hist_scan_kernel",
    "hist_scatter_kernel<0>", "hist_scatter_kernel<1>", "hist_scatter_kernel<2>", "hist_scatter_kernel<3>",
    "hist_pivots_kernel",
    "hist_lookup_kernel<PIXMAJOR>", "hist_lookup_kernel<PLANAR>",
};
static const char* const kResizeNames[] = {
    "area_staged_kernel<F32, F32, PLANAR>", "area_staged_kernel<U8, U8, PLANAR>", "area_staged_kernel<U8, F32, PLANAR>",
    "area_staged_kernel<U16, U16, PLANAR>", "area_staged_kernel<U16, F32, PLANAR>",
    "area_staged_kernel<F32, F32, PIXMAJOR>", "area_staged_kernel<U8, U8, PIXMAJOR>", "area_staged_kernel<U8, F32, PIXMAJOR>",
    "area_staged_kernel<U16, U16, PIXMAJOR>", "area_staged_kernel<U16, F32, PIXMAJOR>",
    "area_gather_kernel<F32, F32>", "area_gather_kernel<U8, U8>", "area_gather_kernel<U8, F32>", "area_gather_kernel<U16, U16>",
    "area_gather_kernel<U16, F32>",
};
static const char* const kMergeNames[] = {
    "ortho_merge_bip_kernel<false, false>", "ortho_merge_bip_kernel<false, true>", "ortho_merge_bip_kernel<true, false>",
    "ortho_merge_bip_kernel<true, true>", "ortho_merge_bsq_kernel<false>", "ortho_merge_bsq_kernel<true>",
    "merge_scenes_kernel", "merge_source_kernel",
};
static const char* const kRoiNames[] = {
    "roi_raster_kernel<CENTER>", "roi_raster_kernel<TOUCHED>", "roi_counts_kernel<CENTER>", "roi_counts_kernel<TOUCHED>",
    "roi_record_init_kernel", "roi_glt_clip_kernel", "roi_glt_reindex_kernel",
};
template <int N>
constexpr int length(const char* const (&)[N]) { return N; }
static_assert(length(kOrthoNames) == kOrthoInstances, "kOrthoNames: one name per OrthoInstance");
static_assert(length(kColorNames) == kColorInstances, "kColorNames: one name per ColorInstance");
static_assert(length(kCoregNames) == kCoregInstances, "kCoregNames: one name per CoregInstance");
static_assert(length(kReprojectNames) == kReprojectInstances, "kReprojectNames: one name per ReprojectInstance");
static_assert(length(kSclNames) == kSclInstances, "kSclNames: one name per SclInstance");
static_assert(length(kS2StackNames) == kS2StackInstances, "kS2StackNames: one name per S2StackInstance");
static_assert(length(kHistNames) == kHistInstances, "kHistNames: one name per HistInstance");
static_assert(length(kResizeNames) == kResizeInstances, "kResizeNames: one name per ResizeInstance");
static_assert(length(kMergeNames) == kMergeInstances, "kMergeNames: one name per MergeInstance");
static_assert(length(kRoiNames) == kRoiInstances, "kRoiNames: one name per RoiInstance");
static_assert(length(kAuxNames) == kAuxInstances, "kAuxNames: one name per AuxInstance");
static_assert(length(kSceneNames) == kSceneInstances, "kSceneNames: one name per SceneInstance");
static_assert(length(kK4Names) == kK4Instances, "kK4Names: one name per K4Instance");
static_assert(length(kPairsNames) == kPairsInstances, "kPairsNames: one name per PairsInstance");

// Aux, scene and ortho entry points launch one kernel each, so their record keeps the last launch only; K4 and pairs entry points
// launch up to two, and a caller may read after several calls; a colour fit is a chain of three entry points and a
// co-registration one of four, read after the chain; a reprojection is two; the SCL chain mask -> coarse -> gather -> apply is four;
// the S2 stack and the SCL under its window are two; a histogram match is keys, four passes of count, scan and scatter, the pivots
// and the lookup: fifteen; an area resampling is one; a merge is one, two with its source plane; a polygon
// clip is the record's start values, the clip and the re-index: three.
constexpr int kRecordCap = 32;
constexpr int kColorRecordCap = 8;
constexpr int kHistRecordCap = 16;
struct Family {
  const char* const* names;
  int count;
  int cap;              // launches the record keeps, <= kRecordCap
  const char* name_fn;  // for the out-of-range error text
};
static const Family kFamilies[] = {
    {kAuxNames, kAuxInstances, 1, "hsr_aux_instance_name"},        // kLaunchAux
    {kSceneNames, kSceneInstances, 1, "hsr_scene_instance_name"},  // kLaunchScene
    {kK4Names, kK4Instances, kRecordCap, "hsr_k4_instance_name"},  // kLaunchK4
    {kPairsNames, kPairsInstances, kRecordCap, "hsr_pairs_instance_name"},  // kLaunchPairs
    {kOrthoNames, kOrthoInstances, 1, "hsr_ortho_instance_name"},  // kLaunchOrtho
    {kColorNames, kColorInstances, kColorRecordCap, "hsr_color_instance_name"},  // kLaunchColor
    {kCoregNames, kCoregInstances, kColorRecordCap, "hsr_coreg_instance_name"},  // kLaunchCoreg
    {kReprojectNames, kReprojectInstances, kColorRecordCap, "hsr_reproject_instance_name"},  // kLaunchReproject
    {kSclNames, kSclInstances, kColorRecordCap, "hsr_scl_instance_name"},  // kLaunchScl
    {kS2StackNames, kS2StackInstances, kColorRecordCap, "hsr_s2stack_instance_name"},  // kLaunchS2Stack
    {kHistNames, kHistInstances, kHistRecordCap, "hsr_hist_instance_name"},  // kLaunchHist
    {kResizeNames, kResizeInstances, kColorRecordCap, "hsr_resize_instance_name"},  // kLaunchResize
    {kMergeNames, kMergeInstances, kColorRecordCap, "hsr_merge_instance_name"},  // kLaunchMerge
    {kRoiNames, kRoiInstances, kColorRecordCap, "hsr_roi_instance_name"},  // kLaunchRoi
};
static_assert(sizeof(kFamilies) / sizeof(kFamilies[0]) == kLaunchFamilies, "kFamilies: one row per LaunchFamily");
struct Record {
  int seq[kRecordCap];
  int count;
};
static thread_local Record g_records[kLaunchFamilies];

static void record_append(LaunchFamily f, int instance) {
  Record& r = g_records[f];
  if (r.count == kFamilies[f].cap) {
    for (int i = 1; i < r.count; ++i) r.seq[i - 1] = r.seq[i];
    --r.count;
  }
  r.seq[r.count++] = instance;
}

int launched(LaunchFamily f, const char* what, int first, int second) {
  const int rc = check_hip(hipGetLastError(), what);
  if (rc == HSR_OK) {
    record_append(f, first);
    if (second >= 0) record_append(f, second);
  }
  return rc;
}

// Always clears the record; writes the names joined by "; ", cut to capacity - 1 characters, unless there is no buffer.
static int record_read(LaunchFamily f, char* names, int32_t capacity) {
  Record& r = g_records[f];
  const int count = r.count;
  r.count = 0;
  if (!names || capacity < 1) return count > 0 ? 1 : 0;
  names[0] = 0;
  size_t used = 0;
  for (int i = 0; i < count && used + 1 < (size_t)capacity; ++i) {
    const int w = snprintf(names + used, (size_t)capacity - used, "%s%s", i ? "; " : "", kFamilies[f].names[r.seq[i]]);
    if (w < 0) break;
    used += (size_t)w < (size_t)capacity - used ? (size_t)w : (size_t)capacity - used - 1;
  }
  return count > 0 ? 1 : 0;
}

static const char* instance_name(LaunchFamily f, int32_t i) {
  if (i < 0 || i >= kFamilies[f].count) {
    set_error("%s: i=%d outside [0,%d)", kFamilies[f].name_fn, i, kFamilies[f].count);
    return nullptr;
  }
  return kFamilies[f].names[i];
}

}  // namespace hsr

extern "C" int hsr_aux_last_launch(char* name, int32_t capacity) { return hsr::record_read(hsr::kLaunchAux, name, capacity); }
extern "C" int hsr_aux_instance_count(void) { return hsr::kAuxInstances; }
extern "C" const char* hsr_aux_instance_name(int32_t i) { return hsr::instance_name(hsr::kLaunchAux, i); }
extern "C" int hsr_scene_last_launch(char* name, int32_t capacity) { return hsr::record_read(hsr::kLaunchScene, name, capacity); }
extern "C" int hsr_scene_instance_count(void) { return hsr::kSceneInstances; }
extern "C" const char* hsr_scene_instance_name(int32_t i) { return hsr::instance_name(hsr::kLaunchScene, i); }
extern "C" int hsr_k4_last_launch(char* names, int32_t capacity) { return hsr::record_read(hsr::kLaunchK4, names, capacity); }
extern "C" int hsr_k4_instance_count(void) { return hsr::kK4Instances; }
extern "C" const char* hsr_k4_instance_name(int32_t i) { return hsr::instance_name(hsr::kLaunchK4, i); }
extern "C" int hsr_pairs_last_launch(char* names, int32_t capacity) { return hsr::record_read(hsr::kLaunchPairs, names, capacity); }
extern "C" int hsr_pairs_instance_count(void) { return hsr::kPairsInstances; }
extern "C" const char* hsr_pairs_instance_name(int32_t i) { return hsr::instance_name(hsr::kLaunchPairs, i); }
extern "C" int hsr_ortho_last_launch(char* name, int32_t capacity) { return hsr::record_read(hsr::kLaunchOrtho, name, capacity); }
extern "C" int hsr_ortho_instance_count(void) { return hsr::kOrthoInstances; }
extern "C" const char* hsr_ortho_instance_name(int32_t i) { return hsr::instance_name(hsr::kLaunchOrtho, i); }

extern "C" int hsr_color_last_launch(char* names, int32_t capacity) { return hsr::record_read(hsr::kLaunchColor, names, capacity); }
extern "C" int hsr_color_instance_count(void) { return hsr::kColorInstances; }
extern "C" const char* hsr_color_instance_name(int32_t i) { return hsr::instance_name(hsr::kLaunchColor, i); }

extern "C" int hsr_coreg_last_launch(char* names, int32_t capacity) { return hsr::record_read(hsr::kLaunchCoreg, names, capacity); }
extern "C" int hsr_coreg_instance_count(void) { return hsr::kCoregInstances; }
extern "C" const char* hsr_coreg_instance_name(int32_t i) { return hsr::instance_name(hsr::kLaunchCoreg, i); }

extern "C" int hsr_reproject_last_launch(char* names, int32_t capacity) { return hsr::record_read(hsr::kLaunchReproject, names, capacity); }
extern "C" int hsr_reproject_instance_count(void) { return hsr::kReprojectInstances; }
extern "C" const char* hsr_reproject_instance_name(int32_t i) { return hsr::instance_name(hsr::kLaunchReproject, i); }

extern "C" int hsr_scl_last_launch(char* names, int32_t capacity) { return hsr::record_read(hsr::kLaunchScl, names, capacity); }
extern "C" int hsr_scl_instance_count(void) { return hsr::kSclInstances; }
extern "C" const char* hsr_scl_instance_name(int32_t i) { return hsr::instance_name(hsr::kLaunchScl, i); }

extern "C" int hsr_s2stack_last_launch(char* names, int32_t capacity) { return hsr::record_read(hsr::kLaunchS2Stack, names, capacity); }
extern "C" int hsr_s2stack_instance_count(void) { return hsr::kS2StackInstances; }
extern "C" const char* hsr_s2stack_instance_name(int32_t i) { return hsr::instance_name(hsr::kLaunchS2Stack, i); }

extern "C" int hsr_hist_last_launch(char* names, int32_t capacity) { return hsr::record_read(hsr::kLaunchHist, names, capacity); }
extern "C" int hsr_hist_instance_count(void) { return hsr::kHistInstances; }
extern "C" const char* hsr_hist_instance_name(int32_t i) { return hsr::instance_name(hsr::kLaunchHist, i); }

extern "C" int hsr_resize_last_launch(char* names, int32_t capacity) { return hsr::record_read(hsr::kLaunchResize, names, capacity); }
extern "C" int hsr_resize_instance_count(void) { return hsr::kResizeInstances; }
extern "C" const char* hsr_resize_instance_name(int32_t i) { return hsr::instance_name(hsr::kLaunchResize, i); }

extern "C" int hsr_merge_last_launch(char* names, int32_t capacity) { return hsr::record_read(hsr::kLaunchMerge, names, capacity); }
extern "C" int hsr_merge_instance_count(void) { return hsr::kMergeInstances; }
extern "C" const char* hsr_merge_instance_name(int32_t i) { return hsr::instance_name(hsr::kLaunchMerge, i); }

extern "C" int hsr_roi_last_launch(char* names, int32_t capacity) { return hsr::record_read(hsr::kLaunchRoi, names, capacity); }
extern "C" int hsr_roi_instance_count(void) { return hsr::kRoiInstances; }
extern "C" const char* hsr_roi_instance_name(int32_t i) { return hsr::instance_name(hsr::kLaunchRoi, i); }

extern "C" int hsr_abi_version(void) { return HSR_ABI_VERSION; }

extern "C" const char* hsr_last_error(void) { return hsr::g_error; }

extern "C" int hsr_moment_count(int32_t deg) { return deg >= 1 && deg <= HSR_MAX_DEG ? hsr::moment_count(deg) : -1; }

extern "C" size_t hsr_partials_bytes(int32_t nb, int32_t deg) {
  if (nb < 1 || nb > HSR_MAX_BANDS || deg < 1 || deg > HSR_MAX_DEG) return 0;
  return (size_t)nb * hsr::moment_count(deg) * HSR_MAX_PARTIALS * sizeof(double);
}

extern "C" int hsr_probe_read(const void* buf_dev, int64_t bytes, int32_t mode, float* sink_dev, hsr_stream_t stream) {
  HSR_REQUIRE(buf_dev && sink_dev && bytes >= 16, HSR_ERR_INVALID, "hsr_probe_read: bad argument");
  HSR_REQUIRE(((uintptr_t)buf_dev & 15) == 0, HSR_ERR_INVALID, "hsr_probe_read: buffer not 16-byte aligned");
  HSR_REQUIRE(mode >= 0 && mode <= 3, HSR_ERR_INVALID, "hsr_probe_read: mode must be 0..3");
  if (mode == 1) {
    hipLaunchKernelGGL(hsr::probe_read_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)buf_dev, bytes / 16, sink_dev);
    HSR_LAUNCH_CHECK("probe_read_kernel");
    return HSR_OK;
  }
  // LDS footprint decides how many workgroups share a CU (160 KiB): 72 KiB -> 2, 36 KiB -> 4
  if (mode == 0) return hsr::launch_probe_lds<hsr::kProbeSlab>(buf_dev, bytes, hsr::kProbeSlab, 512, sink_dev, (hipStream_t)stream);
  if (mode == 2) return hsr::launch_probe_lds<hsr::kProbeSlab / 2>(buf_dev, bytes, hsr::kProbeSlab, 512, sink_dev, (hipStream_t)stream);
  return hsr::launch_probe_lds<hsr::kProbeSlab / 2>(buf_dev, bytes, hsr::kProbeSlab / 2, 1024, sink_dev, (hipStream_t)stream);
}
