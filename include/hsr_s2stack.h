/* libhsr_mi355x: the Sentinel-2 band planes of a granule to the cropped, model-ready 10 m stack on the device - the resampling of
 * the 20 m bands, the stacking and the crop in ONE launch - and the SCL plane under the same window.  What stands between the band
 * planes as the granule delivers them (uint16, at 10 m and 20 m) and the S2 scene that find_valid_paired_tiles, coregister_scene
 * and fuse_scene take.  The reference makes that scene on the host with rasterio: download_s2_spectral_stack
 * (s2_data/s2_utils.py:505-614: band_order :567-586, Resampling.nearest for the 10 m bands, Resampling.bilinear for the 20 m
 * bands, 9 bands without a distinct nir08 :560-590) and crop_s2_stack_to_te (s2_utils.py:617-783: the snap :649-672, the covering
 * window :677-683, the clip :692-696).  The download and the decoding are I/O and stay on the host; GDAL's bits are not claimed:
 * the resampling is DEFINED here, exactly.
 *
 * A family of its own beside include/hsr.h, like include/hsr_scl.h: it adds exports only, changes no entry point of hsr.h and
 * leaves the ABI version where it is.  Status codes, hsr_last_error() and hsr_stream_t are those of hsr.h.  Every launch-path
 * entry takes the stream last, allocates nothing, synchronises nothing, can be captured in a graph, records its kernel name and
 * refuses bad arguments with an error text and no launch; an entry marked "host only" touches no device.  Every output is an
 * integer or the float32 rounding of one float64 expression and depends on the inputs and parameters only - never on the device,
 * the launch geometry or the arrival order of atomics (the only ones are integer sums).
 *
 * THE FRAME.  The granule's 10 m grid is (H10, W10).  A band plane is uint16 with a row stride `rs` in elements; `up` is the number
 * of 10 m pixels per plane pixel, 1 or 2, and the plane has (H, W) = (ceil(H10 / up), ceil(W10 / up)).  The window is
 * (row0, col0, h, w) in 10 m pixels and lies inside the grid.  Output element (b, y, x) belongs to the granule pixel
 * (Y, X) = (row0 + y, col0 + x): all geometry uses (Y, X), never (y, x), so the result of a window IS that window cut out of the
 * full-granule result.
 *
 * TAPS.
 *   up == 1 (either method)   one tap, DN[Y][X], weight 1.
 *   up == 2, NEAREST          one tap, DN[Y >> 1][X >> 1], weight 1.
 *   up == 2, BILINEAR         pixel-centre aligned, source coordinate (Y + 0.5) / 2 - 0.5: i0 = (Y - 1) >> 1 (floor: -1 at Y = 0);
 *                             the row i0 + 1 has quarter-weight 1 when Y is odd and 3 when Y is even, the row i0 the rest of 4; the
 *                             same in X.  Rows and columns are clamped to the plane and a clamped duplicate stays a tap of its
 *                             own: four taps with integer weights wy wx in {1, 3, 9} whose sum is 16.  Exactly one has weight 9:
 *                             the source pixel that contains the output pixel.
 * VALIDITY.  A tap is valid unless has_nodata is set and its DN equals nodata_in.
 *   STRICT   the output is invalid when any tap is invalid.
 *   RENORM   the output is invalid when the weight-9 tap (for one tap: that tap) is invalid; otherwise the invalid taps drop out:
 *            the nodata footprint of a 20 m band is exactly its own pixels, neither eroded nor extrapolated into.
 *   N = sum w DN and Wt = sum w, both over the taps that are used.
 * VALUES.
 *   uint16   q = (2 N + Wt) / (2 Wt) in integer arithmetic (round half up); v = q + add_offset, clamped into the 65535 values that
 *            are not nodata_out (0 or 65535), so a valid sample never becomes nodata; invalid -> nodata_out.
 *   float32  (float)(((double)N / (double)Wt + (double)add_offset) / quantification), both divisions in float64 and correctly
 *            rounded (N / 16 and N / 1 are exact, so the kernel scales there); invalid -> fill, which may be NaN.
 *   invalid_dev  NULL or nbands int64, zeroed by the call: the number of invalid outputs per band.
 */
#ifndef HSR_S2STACK_H_
#define HSR_S2STACK_H_

#include "hsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_S2_MAX_BANDS 16     /* entries of a band table */
#define HSR_S2_NEAREST 0        /* method */
#define HSR_S2_BILINEAR 1
#define HSR_S2_STRICT 0         /* rule */
#define HSR_S2_RENORM 1
#define HSR_S2_U16 0            /* out_dtype */
#define HSR_S2_F32 1
#define HSR_S2_TILE_H 16        /* the output tile of a workgroup, in 10 m pixels */
#define HSR_S2_TILE_W 512

/* One band of the table: its plane (device memory for hsr_s2_stack, host memory for hsr_s2_stack_host), the row stride in
 * elements, the plane's extents, `up`, the method and the offset added to the resampled DN (BOA_ADD_OFFSET of processing baseline
 * 04.00 and later: -1000).  reserved must be 0. */
typedef struct { const void* plane_dev; int64_t rs; int32_t H, W; int32_t up; int32_t method; int32_t add_offset; int32_t reserved; } hsr_s2_band;

/* hsr_s2_stack: out_dev (nbands, h, w) uint16 or float32 with band and row strides in elements = the window of the stack that
 * download_s2_spectral_stack (s2_utils.py:505-614) builds and crop_s2_stack_to_te (s2_utils.py:617-783) cuts, under the definition
 * above.  `bands` is an array in HOST memory of nbands <= 16 entries, passed to the kernel by value in its arguments: no device
 * table is made and no host-to-device copy is issued, so the call captures.  ONE launch for all bands.
 * The kernel: a workgroup per (band, tile) of 16 x 512 output pixels; the source rectangle of the tile - with a one-pixel halo for
 * a bilinear band - is fetched once, with 16-byte loads where a row's address allows them, into LDS; a thread makes eight
 * neighbouring outputs of a row from twelve staged taps (two rows of six) and stores them with 16-byte stores between the row's
 * first and last 16-byte boundary, single elements before and after.  The uint16 path is integer only.
 * Refused (HSR_ERR_INVALID): NULL pointers, nbands outside [1, 16], an extent < 1, a window that leaves the grid, a plane whose
 * (H, W) is not (ceil(H10 / up), ceil(W10 / up)), rs < W, out_rs < w, out_bs < (h - 1) out_rs + w, method, rule or out_dtype out
 * of range, nodata_out not in {0, 65535}, quantification not finite or <= 0, an output that overlaps an input;
 * (HSR_ERR_UNSUPPORTED): up outside {1, 2} - the 60 m bands are not part of the reference's stack - and more than 2^31 - 1 tiles.
 * Records "s2_stack_kernel<U16, STRICT>", "s2_stack_kernel<U16, RENORM>", "s2_stack_kernel<F32, STRICT>" or
 * "s2_stack_kernel<F32, RENORM>". */
int hsr_s2_stack(const hsr_s2_band* bands, int32_t nbands, int32_t H10, int32_t W10, int32_t row0, int32_t col0, int32_t h, int32_t w,
                 int32_t has_nodata, int32_t nodata_in, int32_t rule, int32_t out_dtype, void* out_dev, int64_t out_bs, int64_t out_rs,
                 int32_t nodata_out, float fill, double quantification, int64_t* invalid_dev, hsr_stream_t stream);

/* hsr_s2_stack_host.  Host only: the tile code of hsr_s2_stack compiled for the CPU, on planes, output and counts in host memory;
 * the same refusals. */
int hsr_s2_stack_host(const hsr_s2_band* bands, int32_t nbands, int32_t H10, int32_t W10, int32_t row0, int32_t col0, int32_t h,
                      int32_t w, int32_t has_nodata, int32_t nodata_in, int32_t rule, int32_t out_dtype, void* out, int64_t out_bs,
                      int64_t out_rs, int32_t nodata_out, float fill, double quantification, int64_t* invalid);

/* hsr_s2_expand_u8: out_dev (h, w) uint8 with a row stride, out[y][x] = plane[(row0 + y) / up][(col0 + x) / up]: a byte plane at
 * 10 m or 20 m - the SCL - under the window of crop_s2_stack_to_te (s2_utils.py:677-696) at 10 m, so that fuse_scene_clear takes it
 * at up = 1 whatever the parity of the window's origin.  16-byte stores where a row's address allows them.
 * Refused (HSR_ERR_INVALID): NULL pointers, an extent < 1, a window that leaves the grid, (H, W) not (ceil(H10 / up),
 * ceil(W10 / up)), rs < W, out_rs < w, an output that overlaps the input; (HSR_ERR_UNSUPPORTED): up outside {1, 2}.
 * Records "s2_expand_kernel<UP1>" or "s2_expand_kernel<UP2>". */
int hsr_s2_expand_u8(const uint8_t* plane_dev, int32_t H, int32_t W, int64_t rs, int32_t up, int32_t H10, int32_t W10, int32_t row0,
                     int32_t col0, int32_t h, int32_t w, uint8_t* out_dev, int64_t out_rs, hsr_stream_t stream);

/* s2stack (hsr_s2stack_last_launch; hsr_s2stack_instance_count = 6, hsr_s2stack_instance_name; the 8 most recent launches): the
 * launch record of csrc/hsr_s2stack.hip, under the contract written above hsr_aux_last_launch in hsr.h.  Host only.  The names:
 * s2_stack_kernel<D, R> with D U16 or F32 and R STRICT or RENORM, and s2_expand_kernel<U> with U UP1 or UP2. */
int hsr_s2stack_last_launch(char* names, int32_t capacity);
int hsr_s2stack_instance_count(void);
const char* hsr_s2stack_instance_name(int32_t i);

#ifdef __cplusplus
}
#endif
#endif /* HSR_S2STACK_H_ */
