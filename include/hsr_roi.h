/* libhsr_mi355x: polygon regions of interest on the device - a polygon set rasterised onto a north-up grid, the class histogram
 * of the cells of a uint8 plane inside it, and the lookup table (GLT) of an EMIT granule clipped to it and re-indexed to the
 * swath rows and columns it still needs.  The reference takes a polygon in count_cloud_pixels (s2_data/cloud_utils.py:33-53) and
 * scl_metrics (:82-101) through rasterio.mask.mask, in _save_roi_from_asset (s2_data/s2_utils.py:361-383) and in spatial_subset
 * (EMIT_data/emit_tools.py:529-619) through rioxarray's clip.
 *
 * A family of its own beside include/hsr.h, like include/hsr_scl.h and include/hsr_merge.h: it adds exports only, changes no entry
 * point of hsr.h and leaves the ABI version where it is.  Status codes, hsr_last_error() and hsr_stream_t are those of hsr.h.
 * Every launch-path entry takes the stream last, allocates nothing, synchronises nothing, can be captured in a graph, records its
 * kernel names and refuses bad arguments with an error text and no launch; an entry marked "host only" touches no device.  Every
 * output is an integer; the only atomics are integer sums, minima and maxima, whose order cannot change the result.
 *
 * What is NOT claimed: the bits of GDAL's rasteriser (rasterio.features, rasterio.mask) and rasterio's window rounding.  rasterio,
 * shapely and GDAL are not available where this library is built and tested, so no fixture could be frozen from them; the rules
 * below are the DEFINITION, stated so that a NumPy restatement, the host twins and the kernels agree bit for bit.  In general
 * position (no edge through a cell centre, no edge along or through a lattice line) the centre rule is the even-odd point-in-polygon
 * test of the centre, which is what all_touched=False means, and the touched rule is "the boundary meets the cell or the centre is
 * inside", which is what all_touched=True means; tests/test_roi_host.py checks both against independent implementations.
 *
 * THE POLYGON SET.  nrings rings over one vertex array verts (nverts, 2) float64, (x, y) in the grid's coordinate system, with
 * ring_offsets (nrings + 1) int32: ring k is the vertices ring_offsets[k] .. ring_offsets[k + 1] - 1, closed implicitly (a repeated
 * closing vertex is allowed: it adds a zero-length edge, which crosses nothing and touches only the cell of its point).  Ring k
 * with n vertices has n edges a -> b, vertex i to vertex i + 1 and the last to the first; the set has nverts edges.  The EVEN-ODD
 * rule runs over all rings together: holes and multipolygons need no flag, and a cell covered by two overlapping parts is OUTSIDE.
 * This is not a union.  The vertex and offset arrays of the launch-path entries live in DEVICE memory; nrings and nverts travel by
 * value, so a captured graph can be replayed over another polygon set with the same counts.
 *   Refused (HSR_ERR_INVALID, with a text): NULL arrays, nrings < 1, a ring with fewer than 3 vertices, offsets that do not start at
 *   0, rise and end at nverts, a non-finite vertex, more than HSR_ROI_MAX_EDGES edges.  Nothing is truncated.  The host-only entries
 *   check all of this.  A launch-path entry cannot read device memory without a synchronisation: it refuses what the counts show
 *   (nrings < 1, nverts < 3 nrings, nverts > HSR_ROI_MAX_EDGES), and hsr_roi_check_host is the check of the contents, to be called on
 *   the host copy before the upload (s2_emit.roi always does).  Should the device arrays hold what the check refuses all the same,
 *   the kernels stay inside them and drop every edge they cannot place: an edge whose vertex index lies in no ring
 *   [ring_offsets[k], ring_offsets[k + 1]) within [0, nverts), and an edge with a non-finite vertex.
 *
 * THE GRID.  A GDAL geotransform gt = (x0, dx, 0, y0, 0, dy), six float64 in host memory read before the call returns, and H x W
 * cells.  The rotation terms must be 0 (HSR_ERR_UNSUPPORTED); every term finite and dx, dy not 0 (HSR_ERR_INVALID); dx and dy may
 * have either sign.  A vertex goes to pixel coordinates once, u = (x - gt[0]) / gt[1], v = (y - gt[3]) / gt[5], each then clamped to
 * [-1e300, 1e300] (a quotient can overflow; vertices at +-1e300 are legal input).  Cell (r, c) has its centre at (pu, pv) =
 * (c + 0.5, r + 0.5).  All arithmetic is float64, one rounding per operation (no contraction); every double -> int conversion is
 * bounded first, as in csrc/hsr_cubic_dev.h.
 *
 * THE CENTRE RULE (HSR_ROI_CENTER; all_touched=False, what rasterio.mask uses).  Cell (r, c) is inside iff an odd number of edges
 * a -> b satisfy both
 *     (va <= pv) != (vb <= pv)      and      pu < ua + (pv - va) * (ub - ua) / (vb - va)       evaluated in exactly this order.
 * Ties: a vertex or a horizontal edge exactly on pv counts as lying ABOVE the centre line's open side (<=), so a horizontal edge
 * never crosses and a vertex on the line is crossed by exactly one of its two edges when they continue to opposite sides; a
 * crossing exactly at pu is not to the right of the centre (strict <).
 *
 * THE TOUCHED RULE (HSR_ROI_TOUCHED; all_touched=True, what spatial_subset uses).  A cell is touched iff it is inside by the centre
 * rule, or some edge's span covers it.  An edge's span: with vmin = min(va, vb), vmax = max(va, vb), the rows floor(vmin) ..
 * floor(vmax).  In such a row r: a horizontal edge (va == vb) has u1 = ua, u2 = ub; any other edge is clipped to
 * lo = max(vmin, r), hi = min(vmax, r + 1) and u1 = U(lo), u2 = U(hi), where U(t) = ua if t == va, ub if t == vb, and
 * ua + (t - va) * (ub - ua) / (vb - va) otherwise.  The covered columns are floor(min(u1, u2)) .. floor(max(u1, u2)).
 * Ties, decided: a coordinate exactly on a lattice line belongs to the cell it opens (floor), never to the cell it closes.  So an
 * edge lying exactly on the line v = r touches row r and not row r - 1; a vertical edge exactly on u = c touches column c and not
 * c - 1; an edge that ends exactly on v = r touches, in row r, the one cell of its end point; a diagonal exactly through a lattice
 * corner (c, r) touches the cells it crosses and, in rows r - 1 and r, the column the corner's own u names: (r - 1, c) and (r, c).
 * GDAL's all_touched is a superset on such ties in some directions and not in others; none of its bits is claimed.
 *
 * A window (row_off, col_off, h, w) on the grid, 0 <= row_off, row_off + h <= H and the columns alike, h, w >= 1: only that part
 * is produced, and it IS the slice of the full result, whatever its origin.
 */
#ifndef HSR_ROI_H_
#define HSR_ROI_H_

#include "hsr.h"
#include "hsr_scl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_ROI_MAX_EDGES 8192   /* the most edges (= vertices) of a polygon set; the kernels stream them, none keeps them in LDS */
#define HSR_ROI_CENTER 0         /* rule: the centre rule */
#define HSR_ROI_TOUCHED 1        /* rule: the touched rule */
#define HSR_ROI_TILE_H 64        /* rows of a workgroup's tile */
#define HSR_ROI_TILE_W 256       /* columns of a workgroup's tile */
#define HSR_ROI_RUN 16           /* consecutive cells of one thread: one 16-byte store or load */
#define HSR_ROI_RECORD 8         /* int32 entries of the record of hsr_roi_glt_clip */

/* hsr_roi_check_host.  Host only: the refusals of THE POLYGON SET on arrays in host memory; HSR_OK when the set is legal. */
int hsr_roi_check_host(const double* verts, const int32_t* ring_offsets, int32_t nrings, int32_t nverts);

/* hsr_roi_rasterize: out_dev (h, w) uint8 with a row stride of its own, every byte of the window written once: inside_value where
 * the cell is inside (touched) by `rule`, outside_value elsewhere; 0 / 1 gives the "outside" mask that hsr_scl_apply takes.
 * The kernel: a workgroup of 256 threads owns a tile of 64 x 256 cells.  Its threads stream the edges from device memory, an edge
 * a thread; for every row of the tile the edge crosses, the crossing is evaluated ONCE (by edge and row, never by cell) and
 * reduced to the integer k = the number of columns left of it; the row's crossings are kept in LDS as one toggle bit per column
 * (bit k - 1), so a row holds any number of crossings in 256 bits, and the inside flags of the row are the suffix parity of its
 * toggle bits (crossings right of the tile toggle its last bit).  The touched rule ORs a second bit plane of column ranges.  A
 * thread then owns 16 consecutive cells and stores 16 bytes at once; the runs are anchored on the address row by row (the row
 * stride of a 10980-wide plane is no multiple of 16), with single bytes before a row's first 16-byte boundary and behind its last;
 * a tile no edge reaches is all zero bits and is stored the same way, uniformly.  With few edges up to 32 threads share an edge
 * and take its rows in turn.
 * Refused: THE POLYGON SET's and THE GRID's refusals, NULL out_dev, H, W, h or w < 1, a window that leaves the grid, out_rs < w, rule
 * outside {0, 1} (HSR_ERR_INVALID); a grid of more than 2^30 cells a side, a window of more than 2^31 - 1 tiles
 * (HSR_ERR_UNSUPPORTED).
 * Records "roi_raster_kernel<CENTER>" or "roi_raster_kernel<TOUCHED>". */
int hsr_roi_rasterize(const double* verts_dev, const int32_t* ring_offsets_dev, int32_t nrings, int32_t nverts, const double* gt,
                      int32_t H, int32_t W, int32_t rule, int32_t row_off, int32_t col_off, int32_t h, int32_t w,
                      uint8_t inside_value, uint8_t outside_value, uint8_t* out_dev, int64_t out_rs, hsr_stream_t stream);

/* hsr_roi_rasterize_host.  Host only: the element functions of the kernel compiled for the CPU, row by row, on arrays in host
 * memory; the same refusals and those of hsr_roi_check_host. */
int hsr_roi_rasterize_host(const double* verts, const int32_t* ring_offsets, int32_t nrings, int32_t nverts, const double* gt,
                           int32_t H, int32_t W, int32_t rule, int32_t row_off, int32_t col_off, int32_t h, int32_t w,
                           uint8_t inside_value, uint8_t outside_value, uint8_t* out, int64_t out_rs);

/* hsr_roi_class_counts: counts_dev 16 int32 (zeroed by the call) = hsr_scl_class_counts' histogram (bin v < 12 ? v : 12, bins 13 ..
 * 15 stay 0; HSR_SCL_BINS) of the cells of plane_dev (H, W) uint8, row stride rs, that lie in the window and are inside by `rule`;
 * inside_dev one int32 (zeroed by the call): the number of such cells.  One launch; the mask is never written; a run of 16 cells
 * without an inside cell is not read, so the plane is read at most once and the cost follows the polygon.  int32 suffices: a
 * window holds at most 2^31 - 1 cells (refused beyond), and a 10980 x 10980 plane has 120 560 400.  The sums are integer atomics,
 * one per non-zero bin and workgroup.
 * Refused: as hsr_roi_rasterize, NULL plane_dev, counts_dev or inside_dev, rs < W, a window of more than 2^31 - 1 cells.
 * Records "roi_counts_kernel<CENTER>" or "roi_counts_kernel<TOUCHED>". */
int hsr_roi_class_counts(const double* verts_dev, const int32_t* ring_offsets_dev, int32_t nrings, int32_t nverts, const double* gt,
                         int32_t H, int32_t W, int32_t rule, int32_t row_off, int32_t col_off, int32_t h, int32_t w,
                         const uint8_t* plane_dev, int64_t rs, int32_t* counts_dev, int32_t* inside_dev, hsr_stream_t stream);

/* hsr_roi_glt_clip: spatial_subset's clip (emit_tools.py:557-573) on a lookup table glt_dev (H, W, 2) int32 of ONE-based (column,
 * row) entries (s2_emit.glt_from_xy), under the touched rule.  out_glt_dev (h, w, 2) int32, contiguous, every element written
 * once: the window's entries, 0 in both components where the cell is not touched.  record_dev HSR_ROI_RECORD int32, set by the call:
 *   [0] down_lo  [1] down_hi    min - 1 and max - 1 of glt_y (component 1) over the touched cells with glt_y > 0;
 *   [2] cross_lo [3] cross_hi   the same of glt_x (component 0) over the touched cells with glt_x > 0;
 *   [4] n_valid                 the touched cells with glt_x > 0 and glt_y > 0;      [5] .. [7] 0.
 * The ranges are ZERO-based, like subset_down / subset_cross of the reference.  Without a cell the range is empty: lo = 2^31 - 1,
 * hi = -1 (lo > hi), where the reference raises.  Two launches: the record's start values, then the clip.
 * Refused: as hsr_roi_rasterize, NULL glt_dev, out_glt_dev or record_dev, out_glt_dev overlapping glt_dev.
 * Records "roi_record_init_kernel; roi_glt_clip_kernel". */
int hsr_roi_glt_clip(const double* verts_dev, const int32_t* ring_offsets_dev, int32_t nrings, int32_t nverts, const double* gt,
                     int32_t H, int32_t W, const int32_t* glt_dev, int32_t row_off, int32_t col_off, int32_t h, int32_t w,
                     int32_t* out_glt_dev, int32_t* record_dev, hsr_stream_t stream);

/* hsr_roi_glt_clip_host.  Host only: the same on arrays in host memory. */
int hsr_roi_glt_clip_host(const double* verts, const int32_t* ring_offsets, int32_t nrings, int32_t nverts, const double* gt,
                          int32_t H, int32_t W, const int32_t* glt, int32_t row_off, int32_t col_off, int32_t h, int32_t w,
                          int32_t* out_glt, int32_t* record);

/* hsr_roi_glt_reindex: in place on glt_dev (h, w, 2) int32: component 0 becomes max(glt_x - cross_lo, 0), component 1
 * max(glt_y - down_lo, 0) (emit_tools.py:594-595), the differences taken in 64 bits, with cross_lo = record_dev[2] and down_lo =
 * record_dev[0] READ FROM DEVICE MEMORY by the kernel: the table is one-based on the swath slice [down_lo, down_hi] x [cross_lo,
 * cross_hi].  With an empty range every entry becomes 0.
 * Refused: NULL pointers, h or w < 1, more than 2^31 - 1 cells.
 * Records "roi_glt_reindex_kernel". */
int hsr_roi_glt_reindex(int32_t* glt_dev, int32_t h, int32_t w, const int32_t* record_dev, hsr_stream_t stream);

/* hsr_roi_glt_reindex_host.  Host only: the same on arrays in host memory. */
int hsr_roi_glt_reindex_host(int32_t* glt, int32_t h, int32_t w, const int32_t* record);

/* roi (hsr_roi_last_launch; hsr_roi_instance_count = 7, hsr_roi_instance_name; the 8 most recent launches): the launch record of
 * csrc/hsr_roi.hip, under the contract written above hsr_aux_last_launch in hsr.h.  Host only.  The names: roi_raster_kernel<R> and
 * roi_counts_kernel<R> with R CENTER or TOUCHED, roi_record_init_kernel, roi_glt_clip_kernel and roi_glt_reindex_kernel. */
int hsr_roi_last_launch(char* names, int32_t capacity);
int hsr_roi_instance_count(void);
const char* hsr_roi_instance_name(int32_t i);

#ifdef __cplusplus
}
#endif
#endif /* HSR_ROI_H_ */
