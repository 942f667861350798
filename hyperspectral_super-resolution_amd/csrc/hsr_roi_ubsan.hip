// A stand-alone program for `make roi-ubsan`: the host twins of include/hsr_roi.h (hsr_roi_rasterize_host, hsr_roi_glt_clip_host,
// hsr_roi_glt_reindex_host, hsr_roi_check_host) over the extreme rows of tests/roi_cases.py - vertices at +-1e300, pixel sizes that
// overflow the quotient, a polygon wholly outside, zero-area rings, an over-limit edge count, a two-vertex ring, non-finite vertices -
// with hsr_roi.hip compiled host-only under AddressSanitizer and UndefinedBehaviorSanitizer.  A double -> int conversion out of
// range, a signed overflow or a store outside a buffer ends the program; it needs no device and no interpreter.
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/hsr_roi.h"

static int failures = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, hsr_last_error()); \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static int raster(const std::vector<double>& v, const std::vector<int32_t>& offs, const double* gt, int H, int W, int rule, int r0, int c0,
                  int h, int w, long* inside) {
  std::vector<uint8_t> out((size_t)h * w, 0xA5);                      // exactly the output: one byte more is an ASan report
  const int rc = hsr_roi_rasterize_host(v.data(), offs.data(), (int32_t)offs.size() - 1, (int32_t)(v.size() / 2), gt, H, W, rule, r0, c0, h, w, 1,
                                        0, out.data(), w);
  long n = 0;
  for (uint8_t b : out) n += b == 1;
  if (inside) *inside = n;
  if (rc == HSR_OK)
    for (uint8_t b : out) EXPECT(b <= 1);
  return rc;
}

int main() {
  const double big = 1e300;
  const double gt_utm[6] = {600000.0, 10.0, 0.0, 4100000.0, 0.0, -10.0}, gt_tiny[6] = {0.0, 1e-9, 0.0, 0.0, 0.0, -1e-9},
               gt_denorm[6] = {0.0, 5e-324, 0.0, 0.0, 0.0, 5e-324}, gt_px[6] = {0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  long n = 0;
  for (int rule = 0; rule < 2; ++rule) {
    EXPECT(raster({-big, -big, big, 4099800.0, 600250.0, big}, {0, 3}, gt_utm, 40, 60, rule, 0, 0, 40, 60, &n) == HSR_OK && n > 0);
    EXPECT(raster({-big, 4099895.0, big, 4099893.0, big, 4099701.0, -big, 4099707.0}, {0, 4}, gt_utm, 40, 60, rule, 3, 5, 30, 50, &n) == HSR_OK);
    EXPECT(raster({-big, big, big, big, 1.2e-8, -1.7e-8}, {0, 3}, gt_tiny, 20, 30, rule, 0, 0, 20, 30, &n) == HSR_OK && n > 0);
    EXPECT(raster({-big, big, big, -big, big, big, -big, -big}, {0, 4}, gt_denorm, 64, 257, rule, 0, 0, 64, 257, &n) == HSR_OK);
    EXPECT(raster({-big, -big, big, -big, big, big, -big, big}, {0, 4}, gt_px, 1 << 30, 1 << 30, rule, (1 << 30) - 3, (1 << 30) - 5, 3, 5, &n) ==
               HSR_OK && n == 15);                                    // the far corner of the largest grid, covered
    EXPECT(raster({1e6, 1e6, 1e6 + 5, 1e6, 1e6, 1e6 + 5}, {0, 3}, gt_px, 30, 40, rule, 0, 0, 30, 40, &n) == HSR_OK && n == 0);   // outside
    EXPECT(raster({3.2, 4.1, 30.7, 22.6, 3.2, 4.1, 30.7, 22.6}, {0, 4}, gt_px, 30, 40, rule, 0, 0, 30, 40, &n) == HSR_OK && (n > 0) == (rule == 1));
    EXPECT(raster({7.3, 9.6, 7.3, 9.6, 7.3, 9.6}, {0, 3}, gt_px, 30, 40, rule, 0, 0, 30, 40, &n) == HSR_OK && n == rule);
    // refused, nothing written past anything
    EXPECT(raster({1, 1, 9, 2, 4, 8, 2, 2, 3, 3}, {0, 3, 5}, gt_px, 10, 10, rule, 0, 0, 10, 10, nullptr) == HSR_ERR_INVALID);
    EXPECT(raster({1, 1, NAN, 2, 4, 8}, {0, 3}, gt_px, 10, 10, rule, 0, 0, 10, 10, nullptr) == HSR_ERR_INVALID);
    EXPECT(raster({1, 1, 9, INFINITY, 4, 8}, {0, 3}, gt_px, 10, 10, rule, 0, 0, 10, 10, nullptr) == HSR_ERR_INVALID);
    std::vector<double> many;
    for (int i = 0; i <= HSR_ROI_MAX_EDGES; ++i) {
      many.push_back(5 + 4 * cos(i * 1e-3));
      many.push_back(5 + 4 * sin(i * 1e-3));
    }
    EXPECT(raster(many, {0, HSR_ROI_MAX_EDGES + 1}, gt_px, 10, 10, rule, 0, 0, 10, 10, nullptr) == HSR_ERR_INVALID);
    many.resize(2 * HSR_ROI_MAX_EDGES);
    EXPECT(raster(many, {0, HSR_ROI_MAX_EDGES}, gt_px, 10, 10, rule, 0, 0, 10, 10, &n) == HSR_OK);
  }
  // the clip and the re-index: entries at both ends of int32, an empty range
  {
    const int H = 9, W = 11;
    std::vector<int32_t> glt((size_t)H * W * 2), out((size_t)H * W * 2, -7), rec(HSR_ROI_RECORD, -7);
    for (size_t i = 0; i < glt.size(); ++i) glt[i] = i % 7 == 0 ? INT_MIN : (i % 5 == 0 ? INT_MAX : (int32_t)(i % 13));
    const std::vector<double> v = {-big, -big, big, -big, big, big, -big, big};
    const std::vector<int32_t> offs = {0, 4};
    EXPECT(hsr_roi_glt_clip_host(v.data(), offs.data(), 1, 4, gt_px, H, W, glt.data(), 0, 0, H, W, out.data(), rec.data()) == HSR_OK);
    EXPECT(rec[0] == 0 && rec[1] == INT_MAX - 1 && rec[4] > 0);
    EXPECT(memcmp(glt.data(), out.data(), glt.size() * 4) == 0);
    EXPECT(hsr_roi_glt_reindex_host(out.data(), H, W, rec.data()) == HSR_OK);
    const int32_t empty[HSR_ROI_RECORD] = {INT_MAX, -1, INT_MAX, -1, 0, 0, 0, 0};
    EXPECT(hsr_roi_glt_reindex_host(glt.data(), H, W, empty) == HSR_OK);
    for (int32_t g : glt) EXPECT(g == 0);
    std::vector<int32_t> none((size_t)H * W * 2, 0);
    EXPECT(hsr_roi_glt_clip_host(v.data(), offs.data(), 1, 4, gt_px, H, W, none.data(), 2, 3, 4, 5, out.data(), rec.data()) == HSR_OK);
    EXPECT(rec[0] == INT_MAX && rec[1] == -1 && rec[2] == INT_MAX && rec[3] == -1 && rec[4] == 0);
  }
  EXPECT(hsr_roi_check_host(nullptr, nullptr, 1, 3) == HSR_ERR_INVALID);
  if (failures) return 1;
  printf("roi-ubsan ok\n");
  return 0;
}
