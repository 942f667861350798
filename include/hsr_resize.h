/* libhsr_mi355x: area resampling at any ratio and origin on the device - the area-weighted mean of the source pixels under each
 * destination cell, with fractional coverage at the cell's edges.  What resize_s2_rgb_to (reference s2_emit/viz.py:19-24,
 * cv2.resize(..., INTER_AREA)) and the notebook's downsample_s2_to_grid(resampling="average") between two grids of one CRS do,
 * beyond the exactly aligned integer factors of hsr_block_mean (include/hsr.h, f1): a 7455-wide S2 crop onto a 1242-wide EMIT grid,
 * two grids whose origins differ by a fraction of a pixel, a preview of a 10980^2 granule at 1024^2.  cv2's bits and GDAL's are
 * NOT claimed (cv2 works in float32 and drops slivers below 1e-3): the resampling is DEFINED here, exactly.
 *
 * A family of its own beside include/hsr.h, like include/hsr_s2stack.h: it adds exports only, changes no entry point of hsr.h and
 * leaves the ABI version where it is.  Status codes, hsr_last_error() and hsr_stream_t are those of hsr.h.  The launch-path entry
 * takes the stream last, allocates nothing, synchronises nothing, can be captured in a graph, records its kernel name and refuses
 * bad arguments with an error text and no launch; an entry marked "host only" touches no device.  Every output depends on the
 * inputs and parameters only - never on the device, the launch geometry or the arrival order of atomics (the only ones are
 * integer sums).
 *
 * THE FRAME.  The source is (h, w) per plane and the destination (H, W).  Each axis has a real origin and a scale in source
 * pixels, float64: (y0, sy) for the rows, (x0, sx) for the columns.  A scale outside [1, HSR_AREA_MAX_SCALE] is refused with
 * HSR_ERR_UNSUPPORTED: enlarging is the bilinear kernels' job.  INTER_AREA's frame is x0 = 0, sx = (double)w / (double)W.
 *   edge(j) = x0 + (double)j * sx      one multiply and one add, each rounded (the library is built with -ffp-contract=off).
 *   Cell j covers [lo, hi] with lo = max(edge(j), 0) and hi = min(edge(j + 1), w).  edge(j + 1) of a cell is the same expression
 *   as edge of its neighbour, so the cells tile the axis exactly.  hi <= lo: the cell is outside.
 * TAPS.  i = floor(lo) ... ceil(hi) - 1, at most ceil(sx) + 1 per axis, with the weight wx(i) = min(hi, i + 1) - max(lo, i).
 *   The rows are the same with (y0, sy, h): r and wy(r).
 * VALIDITY of a sample v.  float32: isfinite(v) && !(has_nodata && (double)v == nodata); uint8 / uint16:
 *   !(has_nodata && (double)v == nodata).  An invalid sample is skipped, never multiplied: a NaN never enters a sum.
 * SUMS.  All float64; each product is rounded, then added, in ascending order of the tap.
 *   Row pass, for every source row r of the footprint:   R(r) = sum_i wx(i) v(r, i) over the valid samples,
 *                                                        M(r) = sum_i wx(i) over the valid samples,   F(r) = sum_i wx(i).
 *   Column pass:   S = sum_r wy(r) R(r),   A = sum_r wy(r) M(r),   Full = sum_r wy(r) F(r).
 *   Horizontal, then vertical: the separable evaluation IS the definition, not an approximation of one.
 * RULES.
 *   STRICT   the output is invalid when any tap is invalid.
 *   RENORM   the output is invalid when A == 0 or A < min_valid_frac * Full (one float64 product); min_valid_frac in [0, 1].
 *   A cell outside the source (in either axis) is invalid under both rules; a cell only clipped by the source's edge is not.
 * VALUES.  q = S / A.
 *   float32 output   (float)q * post_scale, multiplied in float32 as hsr_block_mean does; invalid -> fill, which may be NaN.
 *   uint8 / uint16   nearbyint(q) (half to even), saturated to the type; invalid -> nodata_out.  post_scale and fill are unused.
 *   The output dtype is the input's, or float32.
 *   invalid_dev      NULL, or one int64 per plane / channel, zeroed by the call: the number of invalid outputs.
 * LAYOUTS.  Source and destination each have a channel (plane), a row and a pixel stride in elements: planar (C, H, W) is
 *   (H * W, W, 1), pixel-major (H, W, C) is (1, W * C, C); padded rows and a channel slice of a wider image are strides too.
 *   C <= HSR_AREA_MAX_CHANNELS.
 * CONSEQUENCES.  sx = sy = 1 at origin 0 returns the valid samples bit for bit.  An aligned integer factor f on uint8 / uint16 with
 *   a float32 output gives (float)(sum / (f * f)) * post_scale: hsr_block_mean's bits.  A constant float32 image returns the constant.
 */
#ifndef HSR_RESIZE_H_
#define HSR_RESIZE_H_

#include "hsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_AREA_MAX_SCALE 64       /* source pixels per destination pixel, per axis */
#define HSR_AREA_MAX_CHANNELS 16
#define HSR_AREA_F32 0              /* in_dtype / out_dtype: the codes of hsr_block_mean's in_dtype */
#define HSR_AREA_U8 1
#define HSR_AREA_U16 2
#define HSR_AREA_STRICT 0           /* rule */
#define HSR_AREA_RENORM 1
#define HSR_AREA_TILE_H 8           /* the output tile of a workgroup */
#define HSR_AREA_TILE_W 32
#define HSR_AREA_LDS_BYTES 81920    /* what a staged workgroup may hold (two workgroups share a CU's 160 KiB): see
                                       hsr_area_resample_instance */

/* hsr_area_resample: dst (C, H, W) = the area resampling of src (C, h, w) under the definition above; both images in device
 * memory with (channel, row, pixel) strides in elements.  ONE launch for all planes; the tap geometry is computed in the kernel
 * from (y0, x0, sy, sx): no device table, no host-to-device copy, so the call captures.
 * The kernels.  A workgroup of 256 threads makes a tile of 8 x 32 outputs.
 *   area_staged_kernel<IN, OUT, PLANAR>     src_ps == 1: a workgroup per (plane, tile).  The tile's source rectangle goes to LDS
 *       once, with 16-byte loads between a row's first and last 16-byte boundary; the row pass writes R, M and an "any tap
 *       invalid" flag for (source row, tile column) into an LDS intermediate; the column pass reads that and stores a row of the
 *       tile per 32 lanes.
 *   area_staged_kernel<IN, OUT, PIXMAJOR>   src_cs == 1 and src_ps >= C: a workgroup per tile; the rectangle is staged once with
 *       all its channels, then the two passes run channel by channel over the same intermediate.
 *   area_gather_kernel<IN, OUT>             every other layout, and every scale whose rectangle and intermediate exceed
 *       HSR_AREA_LDS_BYTES: a thread per output reads its taps from global memory.  The same sums in the same order.
 *   The choice is made on the host from (layout, dtype, C, sy, sx) alone - hsr_area_resample_instance - and recorded in the name.
 * Refused (HSR_ERR_INVALID): NULL pointers, a pointer that is no multiple of its element size, an extent < 1, C outside [1, 16],
 * strides < 1 or under which elements of one image overlap, a non-finite origin or scale, rule, in_dtype or out_dtype out of
 * range, an out_dtype that is neither in_dtype nor float32, min_valid_frac outside [0, 1], a nodata_out that the integer output type
 * cannot hold, an output that overlaps the input; (HSR_ERR_UNSUPPORTED): sy or sx outside [1, 64], more than 2^31 - 1 tiles. */
int hsr_area_resample(const void* src_dev, int32_t in_dtype, int32_t C, int32_t h, int32_t w, int64_t src_cs, int64_t src_rs,
                      int64_t src_ps, double y0, double x0, double sy, double sx, int32_t has_nodata, double nodata, int32_t rule,
                      double min_valid_frac, void* dst_dev, int32_t out_dtype, int32_t H, int32_t W, int64_t dst_cs, int64_t dst_rs,
                      int64_t dst_ps, float post_scale, float fill, int32_t nodata_out, int64_t* invalid_dev, hsr_stream_t stream);

/* hsr_area_resample_host.  Host only: the tile code of hsr_area_resample - the same instance, every thread of every workgroup in
 * turn - compiled for the CPU, on images and counts in host memory; the same refusals. */
int hsr_area_resample_host(const void* src, int32_t in_dtype, int32_t C, int32_t h, int32_t w, int64_t src_cs, int64_t src_rs,
                           int64_t src_ps, double y0, double x0, double sy, double sx, int32_t has_nodata, double nodata, int32_t rule,
                           double min_valid_frac, void* dst, int32_t out_dtype, int32_t H, int32_t W, int64_t dst_cs, int64_t dst_rs,
                           int64_t dst_ps, float post_scale, float fill, int32_t nodata_out, int64_t* invalid);

/* hsr_area_resample_instance.  Host only: the index (hsr_resize_instance_name) of the kernel that hsr_area_resample launches for
 * this layout, dtype pair and scale, or a negative status with an error text.  Staged when the layout allows it and
 *   rows = ceil(8 sy) + 3, cols = ceil(32 sx) + 3, pitch = round16(((cols - 1) ps + c) esize) + 16   (ps = 1, c = 1 planar;
 *   src_ps, C pixel-major),   rows * pitch + rows * 32 * 16 + round16(rows * 32) <= HSR_AREA_LDS_BYTES. */
int hsr_area_resample_instance(int32_t in_dtype, int32_t out_dtype, int32_t C, int64_t src_cs, int64_t src_ps, double sy, double sx);

/* hsr_area_grid_from_geotransforms.  Host only: two GDAL geotransforms (x0, dx, rx, y0, ry, dy) of ONE CRS -> grid[4] =
 * (y0, x0, sy, sx) of the destination grid in source pixels: x0 = (dst[0] - src[0]) / src[1], sx = dst[1] / src[1],
 * y0 = (dst[3] - src[3]) / src[5], sy = dst[5] / src[5].
 * Refused (HSR_ERR_INVALID): NULL pointers, non-finite terms, a pixel size of 0; (HSR_ERR_UNSUPPORTED): rotation terms, pixel sizes
 * of differing sign, sx or sy below 1. */
int hsr_area_grid_from_geotransforms(const double* src_gt, const double* dst_gt, double* grid);

/* resize (hsr_resize_last_launch; hsr_resize_instance_count = 15, hsr_resize_instance_name; the 8 most recent launches): the launch
 * record of csrc/hsr_resize.hip, under the contract written above hsr_aux_last_launch in hsr.h.  Host only.  The names:
 * area_staged_kernel<I, O, L> with L PLANAR or PIXMAJOR, and area_gather_kernel<I, O>; <I, O> is <F32, F32>, <U8, U8>, <U8, F32>,
 * <U16, U16> or <U16, F32>. */
int hsr_resize_last_launch(char* names, int32_t capacity);
int hsr_resize_instance_count(void);
const char* hsr_resize_instance_name(int32_t i);

#ifdef __cplusplus
}
#endif
#endif /* HSR_RESIZE_H_ */
