/* libhsr_mi355x: exact masked histogram (CDF) matching of float32 images on the device - histogram_match_rgb of the reference
 * (s2_emit/color.py:36-63: np.unique of the masked samples of both images, their empirical CDFs, np.interp between the reference's
 * distinct values) as a batched keys-only radix sort of every channel of both images and an exact rank lookup per pixel.
 *
 * A family of its own beside include/hsr.h, like include/hsr_s2stack.h: it adds exports only, changes no entry point of hsr.h and
 * leaves the ABI version where it is.  Status codes, hsr_last_error() and hsr_stream_t are those of hsr.h.  Every launch-path
 * entry takes the stream last, allocates nothing, synchronises nothing, works in the caller's workspace, can be captured in a
 * graph, records its kernel names and refuses bad arguments with an error text and no launch; an entry marked "host only" touches
 * no device.  No workgroup waits on another; the only atomics are integer sums, so every output depends on the inputs alone.
 *
 * THE DEFINITION.
 * Channels and layout.  C channels, 1 <= C <= 16.  An image is float32 with a channel stride `cs` and a pixel stride `ps`, both in
 * elements: PLANAR (C, npix) has ps == 1 and cs >= npix, PIXEL-MAJOR (npix, row) has cs == 1 and ps >= C.  The three images of a
 * call (src, ref, out) share the kind of layout; their strides are their own.  The mask is uint8 (npix,), nonzero = inside.
 * Validity.  For channel c: valid = mask && isfinite(src_c) && isfinite(ref_c); n = the number of valid pixels.
 * Key.  The radix key of csrc/hsr_select_dev.h (f32_key) with -0.0 taken as +0.0: bits with the sign bit set when the float is
 * >= 0, all bits inverted when it is < 0, so unsigned order of the keys is the order of the floats.  A pixel that is not valid
 * gets the key 0xFFFFFFFF, which no finite float has: there is no compaction, the sentinels sort to the end.
 * Sorted arrays.  S and R are the ascending valid keys of src_c and ref_c read back as floats; both have length n.
 * A valid pixel with value v, all arithmetic in float64, in this order, without contraction:
 *     cs = #{S <= v};  a = R[cs - 1];  hi = #{R <= a};  lo = #{R < a}
 *     hi == cs or lo == 0:  the result is a
 *     otherwise:            b = R[lo - 1];  the result is ((a - b) / (hi / n - lo / n)) * (cs / n - lo / n) + b
 *     rounded to float32, then clipped to [0, 1].
 * This is np.interp(s_quant, r_quant, r_values) of color.py:36-53 with comparisons of integers in place of comparisons of their
 * quotients by n: distinct integers below 2^53 over the same n stay distinct in float64.
 * Other pixels.  A pixel that is not valid gets clip(src, 0, 1), NaN stays NaN.  n == 0: the channel passes through (clipped).
 * n_valid_dev: C int64, the counts, written on the device.
 * Claimed against the reference: equality by value (-0 == +0), NaN at the same places, float32 - whenever every masked sample is
 * finite.  What np.unique does with NaN is not claimed.
 */
#ifndef HSR_HIST_H_
#define HSR_HIST_H_

#include "hsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_HIST_MAX_CHANNELS 16
#define HSR_HIST_SORT_TILE 8192       /* keys of a workgroup's tile in a sort pass */
#define HSR_HIST_SORT_BITS 8          /* a sort is 4 passes of 8 bits */
#define HSR_HIST_SCAN_STEP 4096       /* counters the offset scan takes in one step of its loop */
#define HSR_HIST_PIVOT 256            /* a pivot table keeps the last key of every 256 keys of the level below */
#define HSR_HIST_MAX_NPIX 2147483647  /* ranks and offsets are 32 bits */
#define HSR_HIST_SENTINEL 0xFFFFFFFFu

/* Workspace sizes.  Host only; 0 for arguments out of range.
 *   hsr_hist_plane_stride(npix)       elements between two key planes: npix rounded up to a multiple of 64.
 *   hsr_hist_sort_bytes(npix, P)      the block counters of a sort of P planes: P * 256 * ceil(npix / 8192) uint32.
 *   hsr_hist_pivot_bytes(npix, C)     the pivot tables of 2 C planes: per plane cap1 + cap2 + cap3 uint32 rounded up to a multiple
 *                                     of 64, cap1 = ceil(npix / 256), cap2 = ceil(cap1 / 256), cap3 = ceil(cap2 / 256).
 *   hsr_hist_scratch_bytes(npix, C)   the workspace of hsr_hist_match = two key buffers of 2 C planes each (16 C stride bytes),
 *                                     the counters and the pivot tables, in this order: at C = 3 and npix = 6144^2 1.82 GB. */
int64_t hsr_hist_plane_stride(int64_t npix);
size_t hsr_hist_sort_bytes(int64_t npix, int32_t P);
size_t hsr_hist_pivot_bytes(int64_t npix, int32_t C);
size_t hsr_hist_scratch_bytes(int64_t npix, int32_t C);

/* hsr_hist_keys: one pass over src, ref and mask.  keys_dev: 2 C planes of uint32 `key_stride` >= npix apart: plane c the keys of
 * src channel c, plane C + c those of ref channel c; n_valid_dev: C int64, zeroed by the call (a memset node) and summed with one
 * integer atomic per workgroup of 8192 pixels and channel.
 * Refused (HSR_ERR_INVALID): NULL pointers, C outside [1, 16], npix < 1, strides that fit neither layout or are too small,
 * key_stride < npix, keys that overlap an input, counts that overlap an input; (HSR_ERR_UNSUPPORTED): npix > HSR_HIST_MAX_NPIX.
 * Records "hist_keys_kernel<PIXMAJOR>" or "hist_keys_kernel<PLANAR>". */
int hsr_hist_keys(const float* src_dev, int64_t src_cs, int64_t src_ps, const float* ref_dev, int64_t ref_cs, int64_t ref_ps,
                  const uint8_t* mask_dev, int64_t npix, int32_t C, uint32_t* keys_dev, int64_t key_stride, int64_t* n_valid_dev,
                  hsr_stream_t stream);

/* hsr_hist_sort: P <= 32 planes of npix uint32 keys, `key_stride` apart, sorted ascending in place: a least-significant-digit
 * radix sort, 4 passes of 8 bits, every plane in the same launches (the plane in grid.y).  A pass is three launches: the digit
 * counts of every tile of 8192 keys (LDS integer atomics), an exclusive scan of the counters in (digit, tile) order by ONE
 * workgroup per plane in steps of 4096 counters - no look-back, no polling - and a stable scatter: each of a tile's 8 waves ranks
 * its 1024 keys in order with wave ballots against its own LDS counters, the tile is put in order in LDS and leaves in runs of
 * equal digits.  Keys only, so the result is THE sorted array whatever the arrival order.  tmp_dev: a second buffer of the same
 * shape; counters_dev: hsr_hist_sort_bytes(npix, P) bytes.  After the 4 passes the result is in keys_dev.
 * Refused (HSR_ERR_INVALID): NULL pointers, P outside [1, 32], npix < 1, key_stride < npix, counters too small, buffers that
 * overlap; (HSR_ERR_UNSUPPORTED): npix > HSR_HIST_MAX_NPIX.
 * Records hist_count_kernel<p>; hist_scan_kernel; hist_scatter_kernel<p> for p = 0, 1, 2, 3. */
int hsr_hist_sort(uint32_t* keys_dev, uint32_t* tmp_dev, int64_t key_stride, int64_t npix, int32_t P, void* counters_dev,
                  size_t counters_bytes, hsr_stream_t stream);

/* hsr_hist_sort_pass: ONE pass of hsr_hist_sort - count, scan, scatter on digit `pass` (bits 8 pass .. 8 pass + 7) - from in_dev to
 * out_dev: every plane of out_dev holds the keys of its plane of in_dev in ascending order of that digit, keys of equal digit in their
 * order in in_dev (the pass is stable).  hsr_hist_sort is passes 0, 1, 2, 3 between keys_dev and tmp_dev; the entry is for callers
 * that time or test a pass (tools/bench_histmatch.py).
 * Refused: as hsr_hist_sort, and pass outside [0, 3] (HSR_ERR_INVALID).
 * Records "hist_count_kernel<p>; hist_scan_kernel; hist_scatter_kernel<p>". */
int hsr_hist_sort_pass(const uint32_t* in_dev, uint32_t* out_dev, int64_t key_stride, int64_t npix, int32_t P, int32_t pass,
                       void* counters_dev, size_t counters_bytes, hsr_stream_t stream);

/* hsr_hist_lookup: the output image from the sorted planes (2 C planes as hsr_hist_keys lays them out, each: n valid keys
 * ascending, then sentinels), the counts, src, ref and mask, under the definition above.  ref is read for the validity alone.
 * Two launches.  The pivot tables: level l = 1, 2, 3 of a plane keeps the last key of every 256^l valid keys (of the first n),
 * made straight from the plane.  The lookup: a workgroup per (1024 pixels, channel) in pixel order; the top level - the first
 * with at most 256 entries, the keys themselves when n <= 256 - of S and of R goes to LDS; a rank is a binary search there and
 * one of at most 8 steps inside a window of 256 entries per level below.  #{S <= v} is always searched; a reference without ties
 * at a needs no further search (R[cs] > a gives hi == cs), a tied one searches hi and, unless R[cs - 2] < a, lo.  The rule of a
 * pixel is one __host__ __device__ function, shared with hsr_hist_match_host.  A pixel whose rank cs comes out 0 - possible only
 * when the planes are not those of src - passes through clipped.
 * out == src with the same strides is allowed (every element is read and written by the same thread); any other overlap is refused.
 * Refused (HSR_ERR_INVALID): NULL pointers, C outside [1, 16], npix < 1, strides that fit neither layout or are too small,
 * key_stride < npix, pivots too small, an output that overlaps ref, the mask, a sorted plane, the counts or the pivots;
 * (HSR_ERR_UNSUPPORTED): npix > HSR_HIST_MAX_NPIX.  Counts outside [0, npix] are read as npix (never an index out of a plane).
 * Records "hist_pivots_kernel; hist_lookup_kernel<PIXMAJOR>" or "...<PLANAR>". */
int hsr_hist_lookup(const uint32_t* sorted_dev, int64_t key_stride, const int64_t* n_valid_dev, void* pivots_dev, size_t pivots_bytes,
                    const float* src_dev, int64_t src_cs, int64_t src_ps, const float* ref_dev, int64_t ref_cs, int64_t ref_ps,
                    const uint8_t* mask_dev, int64_t npix, int32_t C, float* out_dev, int64_t out_cs, int64_t out_ps,
                    hsr_stream_t stream);

/* hsr_hist_match: keys, sort and lookup as one entry, in work_dev (hsr_hist_scratch_bytes(npix, C) bytes, 256-byte aligned).
 * The refusals of the three, a workspace that is too small, misaligned or overlaps an image, the mask or the counts, counts that overlap an input. */
int hsr_hist_match(const float* src_dev, int64_t src_cs, int64_t src_ps, const float* ref_dev, int64_t ref_cs, int64_t ref_ps,
                   const uint8_t* mask_dev, int64_t npix, int32_t C, float* out_dev, int64_t out_cs, int64_t out_ps,
                   int64_t* n_valid_dev, void* work_dev, size_t work_bytes, hsr_stream_t stream);

/* hsr_hist_match_host.  Host only: the key, pivot and pixel functions of the kernels compiled for the CPU, std::sort in the
 * middle, on host memory (it allocates its own planes).  The same refusals; n_valid may be NULL. */
int hsr_hist_match_host(const float* src, int64_t src_cs, int64_t src_ps, const float* ref, int64_t ref_cs, int64_t ref_ps,
                        const uint8_t* mask, int64_t npix, int32_t C, float* out, int64_t out_cs, int64_t out_ps, int64_t* n_valid);

/* hsr_hist_key_host.  Host only: the key of one float32 (the sentinel for a non-finite one). */
uint32_t hsr_hist_key_host(float v);

/* hist (hsr_hist_last_launch; hsr_hist_instance_count = 14, hsr_hist_instance_name; the 16 most recent launches): the launch
 * record of csrc/hsr_hist.hip, under the contract written above hsr_aux_last_launch in hsr.h.  Host only.  The names:
 * hist_keys_kernel<L> and hist_lookup_kernel<L> with L PIXMAJOR or PLANAR, hist_count_kernel<p> and hist_scatter_kernel<p> with
 * p 0..3, hist_scan_kernel, hist_pivots_kernel. */
int hsr_hist_last_launch(char* names, int32_t capacity);
int hsr_hist_instance_count(void);
const char* hsr_hist_instance_name(int32_t i);

#ifdef __cplusplus
}
#endif
#endif /* HSR_HIST_H_ */
