/* libhsr_mi355x: the cross-channel (3 -> 3) affine colour transfer, out = x @ A + t.
 *
 * A family of its own beside include/hsr.h: it adds exports only, changes no entry point of hsr.h and leaves
 * HSR_ABI_VERSION where it is.  Status codes, hsr_last_error(), hsr_stream_t and the stride convention (a band stride and a
 * pixel stride, in elements) are those of hsr.h.  Every launch-path entry takes the stream last, allocates nothing and
 * synchronises nothing; an entry marked "host only" touches no device.
 *
 * Images are three float32 channels per pixel in one of the layouts that the stride pair describes:
 *   packed rows  (npix, 3): band_stride 1, pixel_stride 3         (the reference API's (H, W, 3))
 *   padded rows  (npix, 4): band_stride 1, pixel_stride 4         (how match_pair holds its images; any pixel_stride >= 3 works)
 *   planar       (3, npix): band_stride >= npix, pixel_stride 1
 * Anything else - strides under which rows overlap - is refused with HSR_ERR_INVALID.
 * Load / store mode of an image, computed on the host and part of the recorded kernel name: 1 = padded rows with
 * pixel_stride 4 and a 16-byte aligned base (one 16-byte access per pixel), 2 = packed rows with a 16-byte aligned base (three
 * 16-byte accesses per four pixels), 0 = everything else (dword accesses).
 *
 * Moments of a fit: 22 doubles.  With z = (x0, x1, x2, 1) the source channels of a row and y = (y0, y1, y2) its reference
 * channels, first the upper triangle of G = sum z z^T, row-major (G00 G01 G02 G03 G11 G12 G13 G22 G23 G33; G33 is the row
 * count), then R = sum z y^T, row-major (R[i][c], i = 0..3, c = 0..2).
 */
#ifndef HSR_COLOR_H_
#define HSR_COLOR_H_

#include "hsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_AFFINE_MOMENTS 22        /* doubles per fit, the order above                        */
#define HSR_AFFINE_MAX_SLOTS 512     /* upper bound of hsr_affine_partial_slots                 */
#define HSR_AFFINE_SLOT_PIXELS 2048  /* pixels of a partial slot until the slot count saturates */

/* hsr_affine_partial_slots.  Host only.  Partial slots of a moments launch over npix rows: ceil(npix / HSR_AFFINE_SLOT_PIXELS) in
 * [1, HSR_AFFINE_MAX_SLOTS], a function of npix alone, so that the summation tree - and with it every bit of (A, t) - does not
 * depend on the device or the launch.  npix == 0 gives 1; npix < 0 gives -1 and the error text. */
int hsr_affine_partial_slots(int64_t npix);
/* hsr_affine_partials_bytes.  Host only.  Bytes of a partials workspace that serves every npix: HSR_AFFINE_MAX_SLOTS *
 * HSR_AFFINE_MOMENTS doubles. */
size_t hsr_affine_partials_bytes(void);

/* hsr_affine_moments: the 22 moment sums of all usable rows of a float32 image pair, one partial per slot:
 * partials_dev[slot][22].  Replaces the row selection and the normal-equation side of the reference's least squares - `Xv = X[mask]`, the isfinite filter and
 * np.linalg.lstsq(X_aug, Y) of fit_ot_affine_rgb (Pairs_EMIT_S2_demo-2.ipynb, the cell after reproject_stack_to_grid) and of
 * s2_emit/color.py:96-109 - for the all-valid-pixels fit, and the stretch of s2_emit/color.py:33 in front of it.
 *   x_dev, y_dev   float32 images, strides as above; both are only read.
 *   mask_dev       npix bytes or NULL: a row counts when its byte is non-zero (NULL: every row) AND its six RAW values are finite.
 *   lohi_x_dev / lohi_y_dev   NULL or 3 x 2 doubles (lo, hi per channel): every value is first stretched as hsr_poly_moments
 *                  does, float32(clip((v - lo) / (hi - lo + 1e-12), 0, 1)) evaluated in float64; hi == lo is allowed.
 *   partials_dev   hsr_affine_partial_slots(npix) * 22 doubles, every one written.  Slot s sums the contiguous rows
 *                  [s * per, (s + 1) * per), per = ceil(npix / slots) rounded up to a multiple of 4, in float64, in an order
 *                  that depends on (npix, slots) only - not on the layout, the alignment or the device.
 *   slots_out      NULL or where the slot count goes.
 * npix == 0 succeeds and writes one slot of zeros (the solve then yields the identity).  Refused: NULL x / y / partials,
 * npix < 0, overlapping strides.  Records "affine_moments_kernel<LX, LY>" (the two load modes). */
int hsr_affine_moments(const float* x_dev, int64_t x_bs, int64_t x_ps, const float* y_dev, int64_t y_bs, int64_t y_ps,
                       const uint8_t* mask_dev, int64_t npix, const double* lohi_x_dev, const double* lohi_y_dev,
                       double* partials_dev, int32_t* slots_out, hsr_stream_t stream);

/* hsr_affine_moments_f64: the same sums for float64 sample rows, the OT path: x_dev (n, 3) the drawn source samples, y_dev
 * (n, 3) their barycentric targets, row strides x_rs, y_rs >= 3 doubles.  Replaces the normal-equation side of `np.linalg.lstsq(X_aug, Ybar, rcond=None)`
 * (s2_emit/color.py:106-109; fit_ot_affine_rgb in the notebook).  No mask and no stretch.  A row with a non-finite value is
 * SKIPPED; np.linalg.lstsq would raise LinAlgError for it (the reference never hands it one: its samples are filtered and the
 * Sinkhorn targets of finite samples are finite or the fit is useless anyway).  Slots, partials and npix == 0 as above.
 * Records "affine_moments_f64_kernel". */
int hsr_affine_moments_f64(const double* x_dev, int64_t x_rs, const double* y_dev, int64_t y_rs, int64_t npix,
                           double* partials_dev, int32_t* slots_out, hsr_stream_t stream);

/* hsr_affine_reduce_solve: fixed-order reduction of the slots (lane l adds slots l, l + 64, ... in order, then the xor
 * butterfly over the 64 lane sums: the scheme of hsr_moments_reduce) and the solve, in one workgroup.  Replaces np.linalg.lstsq(X_aug, Y, rcond=None) and
 * `A, t = W[:3, :], W[3, :]` (s2_emit/color.py:106-110) and the notebook's fallback `return np.eye(3), np.zeros(3)`.
 *   moments_dev   22 doubles out: the reduced sums.
 *   At_dev        12 doubles out: A row-major (out = x @ A + t, so A[i][c] weighs source channel i in output channel c), then t.
 * Semantics of the solve: unscaled least squares from the moments; the 4 x 4 Gram is eigen-decomposed (cyclic Jacobi), the
 * eigenvalues above max((eps * max(count, 4))^2, 4 eps) * largest are kept - np.linalg.lstsq's singular-value cut with
 * rcond=None, floored where rounded moments stop resolving - and the pseudo-inverse is applied to the three right-hand sides,
 * which is the minimum-norm solution under rank loss.  count < min_count (or count < 1) gives the identity, A = I, t = 0.
 * Refused: NULL pointers, slots outside [1, HSR_AFFINE_MAX_SLOTS].  Records "affine_reduce_solve_kernel". */
int hsr_affine_reduce_solve(const double* partials_dev, int32_t slots, int64_t min_count, double* moments_dev, double* At_dev,
                            hsr_stream_t stream);

/* hsr_affine_solve_host.  Host only: the solve of hsr_affine_reduce_solve, the same code compiled for the CPU, on 22 reduced
 * moments in host memory. */
int hsr_affine_solve_host(const double* moments, int64_t min_count, double* At);

/* hsr_affine_apply: out = x @ A + t, streaming.  Replaces apply_affine_rgb of the notebook and s2_emit/color.py:112-115
 * (`out[mask] = np.clip(Xm @ A + t, 0, 1)`), with the stretch of color.py:33 fused in front.
 * Per pixel: v_c = float32(x_c), stretched first when lohi_dev (3 x 2 doubles) is given.  Where the mask byte is non-zero (or
 * mask_dev is NULL), in float64 and without contraction, exactly
 *     o_c = ((v0 * A[0][c] + v1 * A[1][c]) + v2 * A[2][c]) + t[c]
 * stored as float32; elsewhere the pixel passes through as v_c.
 *   clip_mode  0 no clip; 1 clip the transformed pixels to [0, 1] (the notebook, color.py:114); 2 clip every pixel (the driver's
 *              convention, hsr_poly_apply(clip = 1)).  NaN stays NaN; a non-finite channel of a transformed pixel gives all three
 *              outputs what IEEE arithmetic gives (NaN for NaN and for inf * 0, as the reference's matmul).
 *   out_dev    float32 image with strides of its own; must not overlap x_dev unless it IS x_dev with x's strides.  Every output
 *              float is written once; the fourth float of an output row with band_stride 1 and pixel_stride >= 4 is written
 *              as 0, floats beyond it are left alone.
 * npix == 0 succeeds and launches nothing.  Refused: NULL x / At / out, npix < 0, overlapping strides, clip_mode outside
 * {0, 1, 2}.  Records "affine_apply_kernel<LIN, LOUT>" (the load mode of x, the store mode of out). */
int hsr_affine_apply(const float* x_dev, int64_t x_bs, int64_t x_ps, const uint8_t* mask_dev, const double* At_dev,
                     int64_t npix, const double* lohi_dev, int32_t clip_mode, float* out_dev, int64_t out_bs, int64_t out_ps,
                     hsr_stream_t stream);

/* color (hsr_color_last_launch; hsr_color_instance_count = 20, hsr_color_instance_name; the 8 most recent launches): the launch
 * record of csrc/hsr_color.hip, under the contract written above hsr_aux_last_launch in hsr.h.  Host only.  The names:
 * affine_moments_kernel<LX, LY> and affine_apply_kernel<LIN, LOUT> with each mode in 0 .. 2, affine_moments_f64_kernel,
 * affine_reduce_solve_kernel. */
int hsr_color_last_launch(char* names, int32_t capacity);
int hsr_color_instance_count(void);
const char* hsr_color_instance_name(int32_t i);

#ifdef __cplusplus
}
#endif
#endif /* HSR_COLOR_H_ */
