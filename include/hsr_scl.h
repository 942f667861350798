/* libhsr_mi355x: the Sentinel-2 scene classification layer (SCL) on the device - the class statistics of a plane, the buffered
 * class mask, that mask reduced to the EMIT grid, the byte tile gather and the blanking of a 10 m cube under a mask.  What stands
 * between an SCL raster and a cloud-aware scene fusion (s2_emit.clouds, fuse_scene_clear).  The reference reads the SCL only to
 * choose a granule (s2_data/cloud_utils.py: count_cloud_pixels :33-53, scl_metrics :82-101); its statistics are reproduced count for
 * count, the mask, its buffer and the coarse grid are defined here.
 *
 * A family of its own beside include/hsr.h, like include/hsr_coreg.h and include/hsr_reproject.h: it adds exports only, changes no
 * entry point of hsr.h and leaves the ABI version where it is.  Status codes, hsr_last_error() and hsr_stream_t are those of hsr.h.
 * Every launch-path entry takes the stream last, allocates nothing, synchronises nothing, can be captured in a graph, records its
 * kernel name and refuses bad arguments with an error text and no launch; an entry marked "host only" touches no device.  Every
 * output is an integer or a copied bit pattern and depends on the inputs and parameters only - never on the device, the launch
 * geometry or the arrival order of atomics (the only ones are integer sums, whose order cannot change the result).
 *
 * An SCL plane is (H, W) uint8 with a row stride in elements.  It may be at 10 m or at 20 m: `up` is the number of S2 pixels per
 * SCL pixel, 1 or 2.  Sen2Cor's classes are taken as given: there is no cloud detection here and no reprojection of the SCL, which
 * shares the S2 grid.
 */
#ifndef HSR_SCL_H_
#define HSR_SCL_H_

#include "hsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_SCL_BINS 16         /* bins of a window's histogram: the classes 0 .. 11, bin 12 for every other value, 13 .. 15 stay 0 */
#define HSR_SCL_MAX_RADIUS 32   /* the largest buffer, in SCL pixels: 320 m at 10 m, 640 m at 20 m */
#define HSR_SCL_DISC 0          /* shape: dy^2 + dx^2 <= r^2 */
#define HSR_SCL_SQUARE 1        /* shape: max(|dy|, |dx|) <= r */
#define HSR_SCL_MAX_K 16        /* the largest block of hsr_scl_coarse */

/* hsr_scl_class_counts: counts_dev (H / tile_h, W / tile_w, 16) int32 (floor; zeroed by the call) = the histogram of the class
 * values of every window of the regular tile_h x tile_w grid; the strips right of and below the last window belong to no window
 * and are not read (the convention of hsr_scene_black_counts).  The bin of a value v is v < 12 ? v : 12; bins 13 .. 15 stay 0.
 * One window the size of the plane gives np.unique(scl, return_counts=True) of scl_metrics (cloud_utils.py:87-89) and, summed over
 * class sets, the two sums of count_cloud_pixels (cloud_utils.py:49-53) and cloud_px / valid_px of scl_metrics (:90-93).
 * The kernel: a wave walks rows of its window with 16-byte loads where the row address allows them and single bytes before and
 * after; every thread counts into 13 bins of its own; a workgroup that leaves the window adds its sums with one integer atomic per
 * non-zero bin.
 * Refused: NULL pointers, H, W, tile_h or tile_w < 1, a tile larger than the plane, rs < W, a window of more than 2^31 - 1 pixels.
 * Records "scl_counts_kernel". */
int hsr_scl_class_counts(const uint8_t* scl_dev, int32_t H, int32_t W, int64_t rs, int32_t tile_h, int32_t tile_w, int32_t* counts_dev,
                         hsr_stream_t stream);

/* hsr_scl_mask: mask_dev (H, W) uint8 0 / 1 with a row stride of its own, every byte written once: the pixels of the classes to
 * leave out, the classes of grow_bits buffered by a structuring element.  Replaces the class tests of cloud_utils.py:91-92
 * (np.isin(scl, cloud_set)) for a per-pixel use; the buffer has no counterpart in the reference.
 *   grow_bits   bit v set: class v is bad and is buffered (dilated);
 *   flat_bits   bit v set: class v is bad and is not buffered (nodata, defective).  A value v >= 32 is in neither set.
 *   g[y][x]    = (grow_bits >> v) & 1 for v = scl[y][x] < 32, else 0; 0 outside the plane - no wrap and no clamp;
 *   mask[y][x] = flat(v) | OR over the structuring element of g[y + dy][x + dx];
 *   shape 0     the disc dy^2 + dx^2 <= r^2;  shape 1 the square max(|dy|, |dx|) <= r;  r an integer, 0 <= r <= 32.
 * r == 0 launches a plain lookup instance.  Otherwise, exactly and in O(r) per pixel: a 64 x 32 output tile with a halo of r is
 * staged as one bit per pixel (a wave's ballot is a row of 64 flags); every staged pixel of the tile's columns gets the
 * horizontal distance to the nearest set flag of its row, capped at r + 1, from two bit scans; the output is the OR over
 * dy = -r .. r of rowdist[y + dy][x] <= hw(|dy|), with hw(d) = floor(sqrt(r^2 - d^2)) for the disc, from an integer table built
 * on the host, and hw = r for the square.  A workgroup whose whole staged box holds no grow flag skips the sweep: clear sky is the
 * common case.
 * Refused: NULL pointers, H or W < 1, a row stride below W, r outside [0, 32], shape outside {0, 1}, mask overlapping scl
 * (HSR_ERR_INVALID); a plane of more than 2^31 - 1 tiles (HSR_ERR_UNSUPPORTED).
 * Records "scl_mask_kernel<LOOKUP>", "scl_mask_kernel<DISC>" or "scl_mask_kernel<SQUARE>". */
int hsr_scl_mask(const uint8_t* scl_dev, int32_t H, int32_t W, int64_t rs, uint32_t grow_bits, uint32_t flat_bits, int32_t r,
                 int32_t shape, uint8_t* mask_dev, int64_t mask_rs, hsr_stream_t stream);

/* hsr_scl_mask_host.  Host only: the tile code of hsr_scl_mask compiled for the CPU, on planes in host memory; the same refusals. */
int hsr_scl_mask_host(const uint8_t* scl, int32_t H, int32_t W, int64_t rs, uint32_t grow_bits, uint32_t flat_bits, int32_t r,
                      int32_t shape, uint8_t* mask, int64_t mask_rs);

/* hsr_scl_coarse: a mask reduced to the EMIT grid.  k is the number of mask pixels per EMIT pixel (factor / up), 1 <= k <= 16; the
 * grid is (hc, wc) = (H / k, W / k), floor: the leftover strips are not read.  No counterpart in the reference, which trains on
 * every pixel that is not black (tiles_helpers/utils.py:285-302 select by black fraction only; cloud_utils.py:91-92 names the
 * classes).
 *   clear_dev     (hc, wc) uint8, contiguous: 1 when the cell's k x k block holds at most max_bad non-zero mask pixels, else 0;
 *   cell_bad_dev  NULL or (hc, wc) uint8: min(count, 255) - a block of 16 x 16 can hold 256;
 *   win_counts_dev NULL or (hc / ce_h, wc / ce_w) int32, zeroed by the call: the number of not-clear cells in every cell-window
 *                 of ce_h x ce_w EMIT cells (floor; the cells right of and below the last window are not counted).  The count grid
 *                 s2_emit.scenes.select_tiles sums: the cell-window is the tile, or the stride.  ce_h, ce_w are ignored when NULL.
 * Refused: NULL mask or clear, H or W < 1, rs < W, k outside [1, 16] or larger than the plane, max_bad < 0, with win_counts ce_h or
 * ce_w < 1 or larger than the grid.
 * Records "scl_coarse_kernel". */
int hsr_scl_coarse(const uint8_t* mask_dev, int32_t H, int32_t W, int64_t rs, int32_t k, int32_t max_bad, uint8_t* clear_dev,
                   uint8_t* cell_bad_dev, int32_t ce_h, int32_t ce_w, int32_t* win_counts_dev, hsr_stream_t stream);

/* hsr_scl_gather_tiles: out_dev (ntiles, th, tw) uint8 = the windows of a uint8 plane at origins_dev (ntiles, 2) int32 (row, col):
 * hsr_scene_gather_tiles' contract (save_tile_pair, tiles_helpers/utils.py:308-440) for bytes - arbitrary origins, duplicates
 * allowed; a window that leaves the plane is skipped, never dereferenced, and its output left untouched.
 * Refused: NULL pointers, H, W, th, tw or ntiles < 1, rs < W.
 * Records "scl_gather_kernel". */
int hsr_scl_gather_tiles(const uint8_t* plane_dev, int32_t H, int32_t W, int64_t rs, const int32_t* origins_dev, int32_t ntiles,
                         int32_t th, int32_t tw, uint8_t* out_dev, hsr_stream_t stream);

/* hsr_scl_apply: in place on a cube (T, H, W) float32 with band and row strides in elements: element (t, y, x) becomes `fill`
 * where mask[y / up][x / up] != 0; no other byte is written.  mask is (Hm, Wm) uint8 with a row stride of its own, up 1 or 2.
 * The per-pixel use of the class tests of cloud_utils.py:91-92, which the reference applies to no cube.
 *   count_dev   NULL or one int64, set by the call: the number of (y, x) pixels filled.
 * The mask is read once per pixel and shared by all bands, and stores are issued only under the mask: the cost follows the cloud
 * cover, not the size of the cube.
 * Refused: NULL cube or mask, an extent < 1, up outside {1, 2}, H > Hm up or W > Wm up, rs < W, bs below (H - 1) rs + W,
 * mask_rs < Wm.
 * Records "scl_apply_kernel<UP1>" or "scl_apply_kernel<UP2>". */
int hsr_scl_apply(float* cube_dev, int32_t T, int32_t H, int32_t W, int64_t bs, int64_t rs, const uint8_t* mask_dev, int32_t Hm,
                  int32_t Wm, int64_t mask_rs, int32_t up, float fill, int64_t* count_dev, hsr_stream_t stream);

/* scl (hsr_scl_last_launch; hsr_scl_instance_count = 8, hsr_scl_instance_name; the 8 most recent launches): the launch record of
 * csrc/hsr_scl.hip, under the contract written above hsr_aux_last_launch in hsr.h.  Host only.  The names: scl_counts_kernel,
 * scl_mask_kernel<M> with M LOOKUP, DISC or SQUARE, scl_coarse_kernel, scl_gather_kernel and scl_apply_kernel<U> with U UP1 or
 * UP2. */
int hsr_scl_last_launch(char* names, int32_t capacity);
int hsr_scl_instance_count(void);
const char* hsr_scl_instance_name(int32_t i);

#ifdef __cplusplus
}
#endif
#endif /* HSR_SCL_H_ */
