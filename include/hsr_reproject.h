/* libhsr_mi355x: an EMIT scene on its geographic grid -> the Sentinel-2 UTM grid - the source index of every output cell by the
 * inverse transverse Mercator projection, and a cubic remap under any such field.  The stage between ortho_scene and
 * coregister_scene / the tile-pair drivers; the reference does it with `gdalwarp -r cubic` (emit_proj.py:876-940, for data, loc and
 * obs alike: emit_proj.py:1035,1135,1227), which is a program call and not reproduced: the algorithm is defined here, and neither
 * the geometry nor the resampling claims GDAL's bits.
 *
 * A family of its own beside include/hsr.h, like include/hsr_coreg.h: it adds exports only, changes no entry point of hsr.h and
 * leaves the ABI version where it is.  Status codes, hsr_last_error() and hsr_stream_t are those of hsr.h.  Every launch-path
 * entry takes the stream last, allocates nothing, synchronises nothing, can be captured in a graph, records its kernel name and
 * refuses bad arguments with an error text and no launch; an entry marked "host only" touches no device.  Results depend on the
 * inputs and parameters only - never on the device, the launch geometry or the arrival order of atomics (the only ones are
 * integer sums and an integer or, whose order cannot change the result).
 *
 * Two stages because the reference warps three rasters with one geometry: the field is computed once and the remap runs on any
 * field, not only this one.
 */
#ifndef HSR_REPROJECT_H_
#define HSR_REPROJECT_H_

#include "hsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_REPROJECT_STRICT 0    /* rule: an invalid consulted tap makes the output fill (hsr_coreg_warp's rule) */
#define HSR_REPROJECT_RENORM 1    /* rule: the valid consulted taps are renormalised when the nearest pixel is valid */
#define HSR_REPROJECT_TILE_W 64   /* the output tile of a workgroup, for the reading of max_footprint below */
#define HSR_REPROJECT_TILE_H 8

/* hsr_reproject_coords: coords_dev[h][w][2] float64 (sy, sx), every element written once: for every cell of a north-up output grid
 * in a transverse Mercator CRS the fractional source index in a north-up geographic grid.  Replaces the coordinate transformer of
 * gdalwarp (emit_proj.py:876-940).
 *   e0, n0           the outer corner of the top-left cell; dx, dy > 0 the cell size; h, w the grid.
 *   lon0_deg, k0, false_easting, false_northing, a, inv_f   the projection on an ellipsoid with f = 1 / inv_f.
 *   g0, g1, g3, g5   the source geotransform, g1 > 0, g5 < 0: lon = g0 + g1 * col, lat = g3 + g5 * row at a cell's outer
 *                    corner.  Rotation terms are not taken.
 * Per cell (r, c), in float64, every product and sum rounded on its own (the library is built with -ffp-contract=off):
 *   1. E = e0 + ((double)c + 0.5) * dx,  N = n0 - ((double)r + 0.5) * dy.
 *   2. The inverse by the Krueger series to n^6 (Karney 2011, the form PROJ's etmerc uses):  n = f / (2 - f),
 *      A = a / (1 + n) * (1 + n^2 / 4 + n^4 / 64 + n^6 / 256),  xi = (N - FN) / (k0 A),  eta = (E - FE) / (k0 A),
 *      xi' = xi - sum_{j = 1..6} beta_j sin(2 j xi) cosh(2 j eta),  eta' = eta - sum beta_j cos(2 j xi) sinh(2 j eta),
 *      tau' = sin xi' / sqrt(sinh^2 eta' + cos^2 xi'),  lambda = atan2(sinh eta', cos xi'), with
 *        beta1 = n/2 - 2/3 n^2 + 37/96 n^3 - 1/360 n^4 - 81/512 n^5 + 96199/604800 n^6
 *        beta2 = 1/48 n^2 + 1/15 n^3 - 437/1440 n^4 + 46/105 n^5 - 1118711/3870720 n^6
 *        beta3 = 17/480 n^3 - 37/840 n^4 - 209/4480 n^5 + 5569/90720 n^6
 *        beta4 = 4397/161280 n^4 - 11/504 n^5 - 830251/7257600 n^6
 *        beta5 = 4583/161280 n^5 - 108847/3991680 n^6
 *        beta6 = 20648693/638668800 n^6.
 *   3. tau from tau' by exactly 3 Newton steps from tau = tau', with e^2 = f (2 - f):
 *        sigma = sinh(e atanh(e tau / sqrt(1 + tau^2))),  tau'_i = tau sqrt(1 + sigma^2) - sigma sqrt(1 + tau^2),
 *        tau += (tau' - tau'_i) / sqrt(1 + tau'_i^2) * (1 + (1 - e^2) tau^2) / ((1 - e^2) sqrt(1 + tau^2)).
 *   4. lat = atan tau, lon = lon0 + lambda, both in degrees.  There is no antimeridian wrap: a grid whose longitudes pass +-180
 *      gets indices off the source, which the warp fills.
 *   5. sx = (lon - g0) / g1 - 0.5,  sy = (lat - g3) / g5 - 0.5.
 * The bits of coords are not specified (device and host libm differ); tests/reproject_cases.py states the accuracy.
 * Refused: NULL coords, h or w < 1, a non-finite geometry parameter, dx, dy, g1, -g5, a or k0 <= 0, inv_f <= 1.
 * Records "reproject_coords_kernel". */
int hsr_reproject_coords(double e0, double n0, double dx, double dy, int32_t h, int32_t w, double lon0_deg, double k0,
                         double false_easting, double false_northing, double a, double inv_f, double g0, double g1, double g3,
                         double g5, double* coords_dev, hsr_stream_t stream);

/* hsr_reproject_coords_host.  Host only: the code of hsr_reproject_coords compiled for the CPU, on a field in host memory. */
int hsr_reproject_coords_host(double e0, double n0, double dx, double dy, int32_t h, int32_t w, double lon0_deg, double k0,
                              double false_easting, double false_northing, double a, double inv_f, double g0, double g1,
                              double g3, double g5, double* coords);

/* hsr_reproject_warp: out[b, y, x] = cubic(src[b])(sy, sx) with (sy, sx) = coords[y][x].  Replaces the resampling of
 * `gdalwarp -r cubic` (emit_proj.py:876-940; GDAL's cubic is the Keys kernel with a = -0.5).
 *   src_dev       (bands, hs, ws) float32, band-sequential, band and row strides in elements.
 *   coords_dev    (h, w, 2) float64, contiguous: ANY field, not only hsr_reproject_coords'.
 *   out_dev       (bands, h, w) float32 with band and row strides of its own; every element is written once.
 * A coordinate outside [0, hs - 1] x [0, ws - 1], NaN or infinite gives fill in every band: no tap is read and no unbounded
 * double is converted to an integer.  Otherwise iy = floor(sy), t = sy - iy, the weights w0 .. w3 of hsr_coreg_warp
 * (include/hsr_coreg.h) on the taps iy - 1 .. iy + 2 clamped to the plane, columns alike; a tap whose weight is exactly 0
 * contributes 0 and is not consulted; r_k = ((wx0 v0 + wx1 v1) + wx2 v2) + wx3 v3 per row and ((wy0 r0 + wy1 r1) + wy2 r2) +
 * wy3 r3 in float64, stored as float32.  So an integer translation is a bit-exact shifted copy.
 * A sample is valid when it is finite and, with has_nodata != 0, not equal to nodata.
 *   rule 0, STRICT   an invalid consulted tap makes the output fill.
 *   rule 1, RENORM   all consulted taps valid: STRICT's value, bit for bit.  Otherwise fill when the nearest source pixel
 *                    (iy + (t_y >= 0.5), ix + (t_x >= 0.5)), clamped, is invalid; otherwise acc / wsum, both formed in the order
 *                    above over the valid consulted taps only: roww_k = sum_c wx_c, wsum = sum_k wy_k roww_k (wsum > 0.03: the
 *                    nearest tap weighs at least 0.316 and the negative lobes at most 0.282).  What a quality-masked scene
 *                    needs: under STRICT every nodata pixel erases a 4 x 4 neighbourhood and the swath edge loses two cells.
 * Neither rule claims GDAL's bits (GDAL renormalises too, but by its own mask thresholds).  The kernel is NOT scaled for
 * minification: GDAL widens it when it downsamples, here the four taps stay; EMIT's 0.000542 degree cell against 60 m is a ratio
 * near 1.
 *   max_footprint the caller's bound of the field in source pixels per output pixel.  The host sizes the staged LDS box of a
 *                 64 x 8 tile as (ceil(64 m) + 5) x (ceil(8 m) + 5) samples and launches the direct-gather instance when that
 *                 exceeds 32 KiB.
 *   status_dev    one int32, set by the call: 0, or 1 when some tile's own footprint (min / max over its inside pixels' taps) is
 *                 wider or taller than that box.  A tile whose footprint does not fit the staged capacity gathers directly;
 *                 nothing out of range is ever read and the output is the same either way.
 *   counts_dev    NULL or 2 int64, set by the call: [0] pixels whose coordinate is outside or non-finite, [1] (band, pixel)
 *                 samples inside the plane that became fill by the sample rule.
 * status and counts are cleared by memset nodes on the stream ahead of the one kernel.
 * Refused: NULL src / coords / out / status, rule outside {0, 1}, extents < 1, a row stride below its width, a band stride below
 * (rows - 1) rs + width, negative or NaN max_footprint, out overlapping src or coords.
 * Records "reproject_warp_kernel<LDS|DIRECT, STRICT|RENORM>". */
int hsr_reproject_warp(const float* src_dev, int32_t bands, int32_t hs, int32_t ws, int64_t src_bs, int64_t src_rs,
                       const double* coords_dev, int32_t h, int32_t w, int32_t has_nodata, double nodata, double fill, int32_t rule,
                       double max_footprint, float* out_dev, int64_t out_bs, int64_t out_rs, int64_t* counts_dev,
                       int32_t* status_dev, hsr_stream_t stream);

/* reproject (hsr_reproject_last_launch; hsr_reproject_instance_count = 5, hsr_reproject_instance_name; the 8 most recent
 * launches): the launch record of csrc/hsr_reproject.hip, under the contract written above hsr_aux_last_launch in hsr.h.  Host
 * only.  The names: reproject_coords_kernel and reproject_warp_kernel<I, R> with I LDS or DIRECT and R STRICT or RENORM. */
int hsr_reproject_last_launch(char* names, int32_t capacity);
int hsr_reproject_instance_count(void);
const char* hsr_reproject_instance_name(int32_t i);

#ifdef __cplusplus
}
#endif
#endif /* HSR_REPROJECT_H_ */
