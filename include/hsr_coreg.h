/* libhsr_mi355x: co-registration of a Sentinel-2 scene to an EMIT scene - tie-point score surfaces, peaks, a shift model and the
 * cubic warp.  The stage between ortho_scene and the tile-pair drivers; the reference does it with AROSICS and rasterio
 * (s2_emit/arosics_coreg.py, coregister_s2_granule_to_emit_granule), which is a library call and not reproduced: the algorithm is
 * defined here, on the sensor model of the rest of the project (an EMIT pixel is the factor x factor block mean of S2 pixels).
 *
 * A family of its own beside include/hsr.h, like include/hsr_color.h: it adds exports only, changes no entry point of hsr.h and
 * leaves the ABI version where it is.  Status codes, hsr_last_error() and hsr_stream_t are those of hsr.h.  Every launch-path
 * entry takes the stream last, allocates nothing, synchronises nothing, can be captured in a graph, records its kernel name and
 * refuses bad arguments with an error text and no launch; an entry marked "host only" touches no device.  Results depend on the
 * inputs and parameters only - never on the device, the launch geometry or the arrival order of atomics (there are none).
 *
 * Shared definitions.  Coordinates are array indices.  f = factor, 1 .. 8.  The shift (dy, dx) says: EMIT pixel (i, j) ~ the mean
 * of S2[f i + dy + 0 .. f - 1, f j + dx + 0 .. f - 1]; the corrected scene is S2'[y, x] = S2[y + dy, x + dx].  An S2 sample is
 * valid when it is finite and, with has_nodata != 0, not equal to nodata; a box is valid when its f * f samples are.  An EMIT
 * pixel is valid when it is finite and its mask byte, if a mask is given, is non-zero.  Planes are a base and a row stride in
 * elements, so a band of a (bands, H, W) scene passes without a copy.  s2_dtype: 0 float32, 1 uint16.
 *
 * Tie-point record, HSR_COREG_RECORD = 8 doubles: [cy, cx, dy, dx, score, sharpness, n_valid, status].
 * Shift model, HSR_COREG_MODEL = 10 doubles: [dy0, dy_x, dy_y, dx0, dx_x, dx_y, xc, yc, n_used, kind_used], with
 *     dy(y, x) = (dy0 + dy_x * (x - xc)) + dy_y * (y - yc)          and dx the same way,
 * every product and sum rounded on its own in float64.
 */
#ifndef HSR_COREG_H_
#define HSR_COREG_H_

#include "hsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_COREG_RECORD 8        /* doubles of a tie-point record                     */
#define HSR_COREG_MODEL 10        /* doubles of a shift model                          */
#define HSR_COREG_MAX_FACTOR 8    /* f in [1, 8]                                       */
#define HSR_COREG_MIN_WINDOW 4    /* w in [4, 64]                                      */
#define HSR_COREG_MAX_WINDOW 64
#define HSR_COREG_MAX_SHIFT 24    /* R in [1, 24]                                      */

#define HSR_COREG_OK 0            /* usable                                            */
#define HSR_COREG_OUTSIDE 1       /* the search region leaves a plane                  */
#define HSR_COREG_NO_SCORE 2      /* no finite entry                                   */
#define HSR_COREG_BORDER 3        /* the peak lies on the edge of the search window, or one of its four neighbours is NaN */
#define HSR_COREG_LOW_SCORE 4     /* score < min_score                                 */
#define HSR_COREG_OUTLIER 5       /* written by hsr_coreg_fit_model                    */

/* hsr_coreg_surface: the score surface of every tie point, surface_dev[npoints][2R+1][2R+1] float64, every entry written once.
 * Replaces the per-window matching of AROSICS' COREG_LOCAL (s2_emit/arosics_coreg.py, coregister_s2_granule_to_emit_granule).
 *   emit_dev       float32 plane (he, we), row stride emit_rs; emit_mask_dev NULL or bytes with row stride mask_rs.
 *   s2_dev         float32 or uint16 plane (hs, ws), row stride s2_rs.
 *   origins_dev    npoints x 2 int32 (i0, j0): the EMIT origin of a window x window window.
 * Entry (dy + R, dx + R) of a point is the zero-mean normalised cross-correlation, in float64, between the window's EMIT values
 * e and the S2 box sums m at (f (i0 + i) + dy, f (j0 + j) + dx), over the n pairs where both are valid:
 *     S_ee = sum e e - (sum e)(sum e) / n,  S_mm and S_em alike,  score = S_em / sqrt(S_ee * S_mm).
 * NaN when n < min_valid, when all e or all m of the pairs are equal (zero variance), or when S_ee or S_mm is not positive.
 * A box sum adds its rows top to bottom, each row left to right; a pair sum is formed per lane over the pairs lane, lane + 64,
 * ... in row-major order of the window and then by the xor butterfly over the 64 lanes: a function of `window` alone.
 * A point whose search region is not inside both planes - f i0 - R >= 0, f (i0 + w - 1) + R + f - 1 <= hs - 1, 0 <= i0,
 * i0 + w <= he, and the same for columns - gets an all-NaN surface; nothing outside a plane is read.
 * Refused: NULL emit / s2 / origins / surface, s2_dtype outside {0, 1}, window outside [4, 64], factor outside [1, 8], max_shift
 * outside [1, 24], min_valid < 1, npoints < 0, a plane extent < 1 or a row stride below its width.  npoints == 0 succeeds and
 * launches nothing.  Records "coreg_surface_kernel<float>" or "coreg_surface_kernel<uint16_t>". */
int hsr_coreg_surface(const float* emit_dev, int64_t emit_rs, int32_t he, int32_t we, const uint8_t* emit_mask_dev, int64_t mask_rs,
                      const void* s2_dev, int32_t s2_dtype, int64_t s2_rs, int32_t hs, int32_t ws, int32_t has_nodata, double nodata,
                      const int32_t* origins_dev, int32_t npoints, int32_t window, int32_t factor, int32_t max_shift,
                      int32_t min_valid, double* surface_dev, hsr_stream_t stream);

/* hsr_coreg_peaks: surface -> one record per point, table_dev[npoints][8], every double written.  Replaces the tie-point table
 * of AROSICS (CoRegPoints_table; s2_emit/arosics_coreg.py keeps its reliable rows).
 *   cy = f (i0 + w / 2) - 0.5 (w / 2 not truncated), cx alike: the window centre in S2 index coordinates.
 *   The peak is the largest finite entry; among equal maxima the first in row-major order.  score = its value c.
 *   Per axis, with l, r its two neighbours and den = l - 2 c + r:  offset = den < 0 ? 0.5 * (l - r) / den : 0, clipped to
 *   [-0.5, 0.5];  dy = (row - R) + offset_y,  dx = (column - R) + offset_x.
 *   sharpness = c minus the largest finite entry outside the peak's 3 x 3 neighbourhood, NaN if there is none.  Reported only.
 *   n_valid = the number of finite entries of the surface.
 *   status: OUTSIDE by the region test of hsr_coreg_surface; else NO_SCORE; else BORDER; else LOW_SCORE; else OK.
 *   For status != OK dy and dx are written as 0; score and sharpness are NaN for OUTSIDE and NO_SCORE.
 * Refused: NULL pointers and the ranges of hsr_coreg_surface.  npoints == 0 launches nothing.  Records "coreg_peaks_kernel". */
int hsr_coreg_peaks(const double* surface_dev, const int32_t* origins_dev, int32_t npoints, int32_t window, int32_t factor,
                    int32_t max_shift, int32_t he, int32_t we, int32_t hs, int32_t ws, double min_score, double* table_dev,
                    hsr_stream_t stream);

/* hsr_coreg_fit_model: records -> shift model, in one workgroup; the records are updated in place.  Replaces the filtering of
 * tie points and the warp transform AROSICS derives from them (s2_emit/arosics_coreg.py, correct_shifts).
 *   kind 0 translation: the mean of the OK records' shifts.  kind 1 affine: least squares of both shift components on
 *   [1, u, v], u = (cx - xc) / max(xc, 1), v = (cy - yc) / max(yc, 1), xc = (ws - 1) / 2, yc = (hs - 1) / 2 (the scene centre);
 *   sums in float64 in record order; the 3 x 3 Gram is eigen-decomposed (cyclic Jacobi) and inverted through its eigenvalues.
 *   Affine falls back to translation with fewer than 3 OK records or when the Gram's smallest eigenvalue is below 1e-10 of its
 *   largest (collinear points); kind_used says which was fitted.  With fewer than max(min_points, 1) OK records the model is
 *   all zeros with kind_used = -1 (the warp is then the identity).
 *   One rejection pass: an OK record whose residual hypot(dy - dy(cy, cx), dx - dx(cy, cx)) exceeds reject_px gets status
 *   OUTLIER and zero shifts; if any did, the model is fitted once more on the rest.  No third pass.
 * Refused: NULL pointers, npoints < 0, kind outside {0, 1}, min_points < 0, reject_px not > 0, hs or ws < 1.
 * Records "coreg_fit_model_kernel". */
int hsr_coreg_fit_model(double* table_dev, int32_t npoints, int32_t kind, int32_t min_points, double reject_px, int32_t hs,
                        int32_t ws, double* model_dev, hsr_stream_t stream);

/* hsr_coreg_fit_model_host.  Host only: the code of hsr_coreg_fit_model compiled for the CPU, on records and a model in host
 * memory. */
int hsr_coreg_fit_model_host(double* table, int32_t npoints, int32_t kind, int32_t min_points, double reject_px, int32_t hs,
                             int32_t ws, double* model);

/* hsr_coreg_warp: the corrected scene, out[b, y, x] = cubic(S2[b])(y + dy(y, x), x + dx(y, x)).  Replaces the cubic resampling
 * of the granule (s2_emit/arosics_coreg.py: resamp_alg_calc = 'cubic'; GDAL's cubic is the Keys kernel with a = -0.5).
 *   s2_dev / out_dev   (bands, h, w) float32 or uint16 (s2_dtype, the same on both sides), band and row strides in elements.
 *   model_dev          10 doubles as above, read on the device.
 * Per output pixel, in float64 and without contraction: sy = y + dy(y, x), sx = x + dx(y, x).  Outside [0, h - 1] x [0, w - 1]
 * (or NaN) the output is fill.  Otherwise iy = floor(sy), t = sy - iy,
 *     w0 = ((-0.5 t + 1.0) t - 0.5) t      w1 = ((1.5 t - 2.5) t) t + 1.0
 *     w2 = ((-1.5 t + 2.0) t + 0.5) t      w3 = ((0.5 t - 0.5) t) t
 * on the taps iy - 1 .. iy + 2 clamped to the plane; columns alike.  A tap whose weight is exactly 0 contributes 0 and is not
 * consulted.  If a tap with non-zero wy and wx is invalid the output is fill.  Otherwise r_k = ((wx0 v0 + wx1 v1) + wx2 v2) +
 * wx3 v3 per row and ((wy0 r0 + wy1 r1) + wy2 r2) + wy3 r3, stored as float32, or as uint16 by round-half-even clamped to
 * [0, 65535] (fill the same way).  So an integer translation is a bit-exact shifted copy, and every output element is written once.
 *   max_abs_shift, max_abs_slope   the caller's bound of the model over the scene: |dy|, |dx| <= max_abs_shift and the four
 *                      slopes <= max_abs_slope.  The host sizes the LDS footprint of a 64 x 16 output tile from the slope bound
 *                      and launches the direct-gather instance when it would exceed 32 KiB.
 *   status_dev         one int32, written by every launch: 0, or 1 when the model on the device exceeds the bound.  A tile
 *                      whose actual footprint does not fit the staged one gathers directly; nothing out of range is ever read
 *                      and the output is the same either way.
 * Refused: NULL pointers, s2_dtype outside {0, 1}, extents < 1, a row stride below w, a band stride below (h - 1) rs + w,
 * negative or NaN bounds, out overlapping s2.  Records "coreg_warp_kernel<float|uint16_t, LDS|DIRECT>". */
int hsr_coreg_warp(const void* s2_dev, int32_t s2_dtype, int32_t bands, int32_t h, int32_t w, int64_t in_bs, int64_t in_rs,
                   const double* model_dev, int32_t has_nodata, double nodata, double fill, double max_abs_shift,
                   double max_abs_slope, void* out_dev, int64_t out_bs, int64_t out_rs, int32_t* status_dev, hsr_stream_t stream);

/* coreg (hsr_coreg_last_launch; hsr_coreg_instance_count = 8, hsr_coreg_instance_name; the 8 most recent launches): the launch
 * record of csrc/hsr_coreg.hip, under the contract written above hsr_aux_last_launch in hsr.h.  Host only.  The names:
 * coreg_surface_kernel<T> with T float or uint16_t, coreg_peaks_kernel, coreg_fit_model_kernel, coreg_warp_kernel<T, LDS> and
 * coreg_warp_kernel<T, DIRECT>. */
int hsr_coreg_last_launch(char* names, int32_t capacity);
int hsr_coreg_instance_count(void);
const char* hsr_coreg_instance_name(int32_t i);

#ifdef __cplusplus
}
#endif
#endif /* HSR_COREG_H_ */
