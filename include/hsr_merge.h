/* libhsr_mi355x: adjacent EMIT scenes of one orbit onto one grid on the device.  An EMIT scene is about 75 km of an orbit and a
 * Sentinel-2 granule 110 km on a side, so a granule is normally covered by two or three consecutive scenes.  The reference merges
 * them with merge_emit / is_adjacent (EMIT_data/emit_tools.py:622-704): every granule is orthorectified and the results go to
 * rioxarray.merge.merge_arrays(..., nodata=-9999), rasterio's "first" rule on a common grid.  Here that is
 *   hsr_merge_grid     the common grid and every source's integer offset on it (host only, float64);
 *   hsr_merge_scenes   the "first" rule over N orthorectified scenes, one streaming launch;
 *   hsr_ortho_merge    N swaths with their lookup tables straight onto the merged grid in ONE launch: the N intermediate
 *                      scenes of hsr_ortho_glt per source + hsr_merge_scenes are never written; the same bits.
 *
 * A family of its own beside include/hsr.h, like include/hsr_resize.h: it adds exports only, changes no entry point of hsr.h and
 * leaves the ABI version where it is.  Status codes, hsr_last_error() and hsr_stream_t are those of hsr.h.  A launch-path entry
 * takes the stream last, allocates nothing, synchronises nothing, can be captured in a graph, records its kernel names and refuses
 * bad arguments with an error text and no launch; an entry marked "host only" touches no device.  The sources are at most
 * HSR_MERGE_MAX_SOURCES small structs in HOST memory: they travel by value in the kernel arguments, so there is no device-side
 * table and no host-to-device copy.  Every output depends on the inputs and parameters only - never on the device, the launch
 * geometry or the arrival order of atomics (the only ones are integer sums).  All byte offsets are 64-bit.
 *
 * THE GRID.  Source k has a north-up GDAL geotransform (x0_k, dx_k, 0, y0_k, 0, dy_k) and a shape (h_k, w_k).  The merged grid has
 * the pixel size (dx, dy) of source 0, dx > 0, dy of either sign (dy < 0: y0 is the northern edge).
 *   No bounds:  X0 = min_k x0_k (the westmost origin); Y0 = max_k y0_k when dy < 0 (the northmost), min_k y0_k when dy > 0.
 *   bounds = (l, b, r, t), l < r and b < t:  X0 = l; Y0 = t when dy < 0, b when dy > 0;
 *               W = max(1, floor((r - l) / dx + 0.5)), H = max(1, floor((t - b) / |dy| + 0.5)).
 *   Source k sits at the INTEGER offset off_x_k = floor((x0_k - X0) / dx + 0.5), off_y_k = floor((y0_k - Y0) / dy + 0.5): each
 *   of the subtraction, the division and the addition rounded on its own in float64.  This is a nearest-cell placement: nothing is
 *   resampled.  The sub-pixel remainder res_x_k = (x0_k - X0) / dx - off_x_k (res_y_k alike), in pixels, in [-0.5, 0.5], is
 *   returned so that the caller sees it; a source offset by exactly half a pixel moves to the next cell (remainder -0.5).
 *   No bounds:  W = max_k (off_x_k + w_k), H = max_k (off_y_k + h_k): the extent reaches the farthest source edge.
 *   Refused: rotation terms; a pixel size of source k that differs from source 0's by more than 0.01 pixel over the source's
 *   extent, |dx_k / dx - 1| w_k > 0.01 or |dy_k / dy - 1| h_k > 0.01 - a different sign included - (HSR_ERR_UNSUPPORTED);
 *   non-finite terms, dx <= 0, dy == 0, shapes < 1, an offset or extent beyond 2^30 (HSR_ERR_INVALID).
 *   rasterio's own window rounding (rasterio.merge, reached through rioxarray) is NOT claimed: it is version-dependent, and neither
 *   package was at hand.  On grids that are aligned - every remainder 0, which consecutive scenes of one orbit's GLT grid are -
 *   any rounding gives these offsets.
 *
 * THE FIRST RULE (rasterio's copy_first), PER ELEMENT.  Output element (b, y, x) starts as `nodata`.  The sources are visited in
 * the caller's order.  Source k covers the cell when 0 <= y - off_y_k < h_k and 0 <= x - off_x_k < w_k.  The first source that
 * covers the cell and whose value v there is not empty supplies the BITS of the output: a NaN payload, -0.0 or a denormal that
 * wins is copied bit for bit.  v is empty when v == nodata in float32 comparison (so -0.0 is empty under nodata = 0, and a NaN
 * nodata makes nothing empty); with nan_is_nodata != 0 a NaN v is empty too - off in the reference, which tests equality with
 * -9999 only.  An element that no source supplies holds the bits of `nodata`.
 *   The rule is per ELEMENT, not per pixel: a band of a cell that one scene's band mask blanked, or a cell that its quality mask
 *   blanked, is filled from the next scene in the overlap, band by band.  That is what the reference does.
 *   source_dev (optional): uint8 (H, W), the index of the first source that supplies ANY band of the cell, 255 when none does.
 *
 * LAYOUTS.  layout 0 (bip): scenes and output (h, w, bands); layout 1 (bsq): (bands, h, w); contiguous; the same bits either way.
 */
#ifndef HSR_MERGE_H_
#define HSR_MERGE_H_

#include "hsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_MERGE_MAX_SOURCES 8
#define HSR_MERGE_MAX_BANDS 512     /* hsr_ortho_glt's limit */
#define HSR_MERGE_RUN 1024          /* elements of one output row that a workgroup of hsr_merge_scenes owns */
#define HSR_MERGE_NO_SOURCE 255

/* One orthorectified scene of hsr_merge_scenes (32 bytes): float32, contiguous in the call's layout, at (off_y, off_x) on the
 * merged grid; the offsets may be negative and the scene may lie wholly outside the output (it then contributes nothing).
 * reserved is 0. */
typedef struct hsr_merge_scene {
  const float* scene_dev;
  int32_t h, w;
  int32_t off_y, off_x;
  int32_t bands, reserved;
} hsr_merge_scene;

/* One swath of hsr_ortho_merge (64 bytes): the arguments of hsr_ortho_glt - swath (rows, cols, bands) float32, glt (glt_h, glt_w, 2)
 * int32, qmask (rows, cols) uint8 or NULL, bmask (rows, cols, bmask_bytes) uint8 or NULL - with the whole GLT grid as the window,
 * placed at (off_y, off_x) on the merged grid. */
typedef struct hsr_merge_swath {
  const float* swath_dev;
  const int32_t* glt_dev;
  const uint8_t* qmask_dev;
  const uint8_t* bmask_dev;
  int32_t rows, cols;
  int32_t glt_h, glt_w;
  int32_t off_y, off_x;
  int32_t bmask_bytes, bands;
} hsr_merge_swath;

/* hsr_merge_grid.  Host only: n geotransforms (6 doubles each) and shapes (h, w each) -> the merged grid of THE GRID above:
 * grid_gt[6], grid_shape[2] = (H, W), offsets[2 n] = (off_y_k, off_x_k), residuals[2 n] = (res_y_k, res_x_k).  bounds: NULL or
 * (l, b, r, t).  n in [1, HSR_MERGE_MAX_SOURCES]. */
int hsr_merge_grid(const double* geotransforms, const int32_t* shapes, int32_t n, const double* bounds, double* grid_gt,
                   int32_t* grid_shape, int32_t* offsets, double* residuals);

/* hsr_merge_scenes: out (H, W) x bands = THE FIRST RULE over the n scenes.  A streaming select; the rule is per element, so a
 * layout is only strides: an output row is H rows of W elements per band (bsq) or of W bands elements (bip).
 *   merge_scenes_kernel   a workgroup of 256 threads owns a run of HSR_MERGE_RUN elements of one row; a thread owns the
 *       four that share a 16-byte line of the OUTPUT, which it stores as one 16-byte store (single floats where the row's ends cut
 *       the line).  A source is read only inside its own rectangle, and a later source only where an element is still empty (a
 *       wave skips a source that none of its lanes needs: ballot); the four elements of a thread come as one 16-byte load where
 *       they lie inside the source's rectangle and on 16 bytes there, as single floats otherwise: the same bits.  Every output
 *       byte is written exactly once; there is no memset of the output.
 *   merge_source_kernel   only when source_dev is given: a thread per cell walks the sources and bands until an element
 *       that is not empty turns up (in the common case the first one it reads).
 * Refused (HSR_ERR_INVALID): n outside [1, HSR_MERGE_MAX_SOURCES], NULL pointers, non-positive sizes, layout outside {0, 1}, scenes
 * that differ in `bands`, a pointer off 4 bytes, an output (or source plane) that overlaps an input; (HSR_ERR_UNSUPPORTED): bands > HSR_MERGE_MAX_BANDS, an
 * output or a scene of more than 2^31 - 1 pixels, more than 2^31 - 1 workgroups. */
int hsr_merge_scenes(const hsr_merge_scene* scenes, int32_t n, int32_t layout /* 0 bip, 1 bsq */, int32_t out_h, int32_t out_w,
                     float nodata, int32_t nan_is_nodata, float* out_dev, uint8_t* source_dev, hsr_stream_t stream);

/* hsr_merge_scenes_host.  Host only: the per-element function of the kernels compiled for the CPU, on scenes and outputs in host
 * memory; the same refusals. */
int hsr_merge_scenes_host(const hsr_merge_scene* scenes, int32_t n, int32_t layout, int32_t out_h, int32_t out_w,
                          float nodata, int32_t nan_is_nodata, float* out, uint8_t* source);

/* hsr_ortho_merge: n swaths -> the merged scene in ONE launch.  For source k the value of cell (y, x) that it covers (0 <= y -
 * off_y_k < glt_h_k, 0 <= x - off_x_k < glt_w_k) is exactly what hsr_ortho_glt (include/hsr.h) defines for GLT entry (y - off_y_k,
 * x - off_x_k) with fill = nodata: the no-data entry, the entry outside the swath (fill, counted as dropped), `masked` under the
 * quality and band masks, the swath's bits.  THE FIRST RULE (nan_is_nodata = 0) then runs over those values.  The result is
 * bit-equal to hsr_ortho_glt per source followed by hsr_merge_scenes; with one source at offset (0, 0) on a grid of the GLT's
 * shape the scene and the count are hsr_ortho_glt's.
 *   dropped_dev   NULL or int64[n], zeroed by the call: per source, the entries inside the output that point outside the swath.
 *   source_dev    NULL or uint8 (out_h, out_w), as above.
 * The kernels keep hsr_ortho_glt's shape: 64 consecutive output pixels per workgroup.
 *   ortho_merge_bip_kernel<kMask, kVec> (256 threads), ortho_merge_bsq_kernel<kMask> (512 threads, the [64][bands | 1] LDS tile).
 *   Wave 0 walks the n tables for its 64 pixels and leaves in LDS, per pixel, the list of candidates in source order - source
 *   index, swath pixel index, kind - without those that are empty in every band (fill; `masked` when masked == nodata), and
 *   counts the dropped entries per source by ballot, at most one integer atomic per source and workgroup.  A wave that copies a
 *   pixel reads the first candidate's spectrum as hsr_ortho_glt does - float4 runs and a tail, four (bsq: eight) spectra in flight
 *   - and only where a ballot shows an empty element and another candidate exists reads the next one and selects per element; the
 *   loop is uniform over the wave, which holds one pixel's spectrum across its lanes.  A pixel with one fully valid candidate
 *   costs what it costs in hsr_ortho_glt; a pixel without candidates reads no spectrum.
 *   kMask: some source has a quality or band mask; kVec: bands % 4 == 0 and the output and every swath start on 16 bytes.
 * Refused (HSR_ERR_INVALID): n outside [1, HSR_MERGE_MAX_SOURCES], NULL swath / glt / out, non-positive sizes, swaths that
 * differ in `bands`, bmask_dev with bmask_bytes < ceil(bands / 8), layout outside {0, 1}, an output (scene, counts or source plane) that overlaps an input;
 * (HSR_ERR_UNSUPPORTED): bands > HSR_MERGE_MAX_BANDS, rows cols > 2^31 - 1, out_h out_w > 2^31 - 1. */
int hsr_ortho_merge(const hsr_merge_swath* swaths, int32_t n, int32_t glt_nodata, int32_t layout, int32_t out_h,
                    int32_t out_w, float nodata, float masked, float* out_dev, int64_t* dropped_dev, uint8_t* source_dev,
                    hsr_stream_t stream);

/* merge (hsr_merge_last_launch; hsr_merge_instance_count = 8, hsr_merge_instance_name; the 8 most recent launches): the launch
 * record of csrc/hsr_merge.hip, under the contract written above hsr_aux_last_launch in hsr.h.  Host only.  The names:
 * ortho_merge_bip_kernel<kMask, kVec>, ortho_merge_bsq_kernel<kMask>, merge_scenes_kernel, merge_source_kernel.
 * hsr_merge_scenes with a source plane records "merge_scenes_kernel; merge_source_kernel". */
int hsr_merge_last_launch(char* names, int32_t capacity);
int hsr_merge_instance_count(void);
const char* hsr_merge_instance_name(int32_t i);

#ifdef __cplusplus
}
#endif
#endif /* HSR_MERGE_H_ */
