"""The reprojection drivers of s2_emit/reproject.py on an MI355X: reproject_scene against its two stages, the device's own field
through the NumPy statement of the remap, a planted scene of quadratic bands against fixture-grade coordinates, the reuse of a
field for a second raster, and the hand-over to find_valid_paired_tiles.

The scene is an EMIT-like geographic raster (0.000542 degree cells near 34.6 N, 119.9 W, 2.9 degrees from the central meridian) and the target a Sentinel-2 tile of UTM
zone 11 N whose extent covers part of it, so the output has cells outside the source and cells whose taps meet the masked
corner.  Bars: the remap bit-equal to reproject_cases.warp_ref; the planted scene within one float32 ulp of the float64 cubic of
the float32 samples at the reference coordinates plus |gradient| times the coordinate bar."""
import numpy as np
import pytest

import reproject_cases as rc
import s2_emit
from gpu_harness import same_bits, torch_gpu  # noqa: F401  (torch_gpu: the fixture)

pytestmark = pytest.mark.gpu

BANDS, HS, WS = 3, 150, 170
SRC_GT = (-119.9, rc.EMIT_CELL, 0.0, 34.65, 0.0, -rc.EMIT_CELL)
EPSG = 32611
S2_SHAPE = (4, 90 * 6, 96 * 6)                           # 10 m pixels: 90 x 96 cells of 60 m
MAX_EXCLUDED = 0.15


def _s2_geotransform():
    """An S2 raster whose origin lies 10 cells left of and above the source's projected top-left corner, on the 60 m lattice: the
    source's own bounds limit the grid there, and the meridian convergence (1.6 degrees) leaves cells outside the source."""
    E, N = s2_emit.tm_forward(SRC_GT[0], SRC_GT[3], s2_emit.utm_params(EPSG))
    return (60.0 * np.floor(float(E) / 60.0) - 600.0, 10.0, 0.0, 60.0 * np.ceil(float(N) / 60.0) + 600.0, 0.0, -10.0)


def _planted():
    """Bands that are quadratic polynomials of the source index (Keys' kernel reproduces quadratics), as float32."""
    yy, xx = np.meshgrid(np.arange(HS, dtype=np.float64), np.arange(WS, dtype=np.float64), indexing="ij")
    coef = [(0.2, 1e-3, -2e-3, 3e-6, -2e-6, 1e-6), (1.0, -3e-3, 1e-3, -1e-6, 4e-6, 2e-6), (-0.5, 2e-3, 2e-3, 2e-6, 1e-6, -3e-6)]
    return np.stack([c0 + cy * yy + cx * xx + cyy * yy * yy + cxx * xx * xx + cxy * yy * xx for c0, cy, cx, cyy, cxx, cxy in coef]), coef


@pytest.fixture(scope="module")
def scene(torch_gpu):
    torch = torch_gpu
    src = _planted()[0].astype(np.float32)
    masked = src.copy()
    masked[:, :30, :40] = -9999.0                         # a quality-masked corner
    masked[1, 100, 120] = np.nan
    out = s2_emit.reproject_scene(torch.from_numpy(masked).cuda(), SRC_GT, epsg=EPSG, s2_geotransform=_s2_geotransform(), s2_shape=S2_SHAPE)
    torch.cuda.synchronize()
    return dict(src=src, masked=masked, out=out)


def test_reproject_scene_is_its_two_stages(torch_gpu, scene):
    torch, out = torch_gpu, scene["out"]
    s2gt = _s2_geotransform()
    grid = s2_emit.utm_target_grid(SRC_GT, (BANDS, HS, WS), EPSG, s2gt, S2_SHAPE)
    assert out.grid == grid and out.geotransform == (grid[0], 60.0, 0.0, grid[3], 0.0, -60.0)
    rows, cols = grid[4:]
    assert tuple(out.scene.shape) == (BANDS, rows, cols) and out.scene.dtype == torch.float32 and out.scene.is_contiguous()
    assert tuple(out.coords.shape) == (rows, cols, 2) and out.coords.dtype == torch.float64 and 60 < rows <= 90 and 60 < cols <= 96
    coords = s2_emit.reproject_coords(grid, EPSG, SRC_GT)
    same_bits(coords.cpu().numpy(), out.coords.cpu().numpy(), "the field of reproject_scene")
    src = torch.from_numpy(scene["masked"]).cuda()
    for rule in ("renorm", "strict"):
        two, counts = s2_emit.remap_scene(src, coords, nodata=-9999.0, rule=rule)
        one = s2_emit.reproject_scene(src, SRC_GT, epsg=EPSG, s2_geotransform=s2gt, s2_shape=S2_SHAPE, rule=rule)
        same_bits(one.scene.cpu().numpy(), two.cpu().numpy(), f"reproject_scene, {rule}")
        assert np.array_equal(one.counts.cpu().numpy(), counts.cpu().numpy())
        # the device's own field through the NumPy statement of the remap
        ref, ref_counts, _ = rc.warp_ref(scene["masked"], coords.cpu().numpy(), -9999.0, -9999.0, rc.RENORM if rule == "renorm" else rc.STRICT)
        same_bits(two.cpu().numpy(), ref, f"remap_scene against the statement, {rule}")
        assert np.array_equal(counts.cpu().numpy(), ref_counts) and ref_counts[0] > 0 and ref_counts[1] > 0
    # out=: written in place, and a preallocated output with a row stride of its own
    back = torch.full((BANDS, rows, cols + 5), 7.0, dtype=torch.float32, device="cuda")
    got, _ = s2_emit.remap_scene(src, coords, nodata=-9999.0, out=back[:, :, :cols])
    assert got.data_ptr() == back.data_ptr() and (back[:, :, cols:] == 7.0).all()
    same_bits(back[:, :, :cols].cpu().numpy(), scene["out"].scene.cpu().numpy(), "out= with a row stride")


def test_planted_quadratics(torch_gpu, scene):
    """The unmasked planted scene at fixture-grade coordinates (the NumPy inverse, which tests/test_reproject_host.py holds within
    the coordinate bar of the mpmath fixture): |out - float64 cubic of the float32 samples| <= 1 float32 ulp + |gradient| x bar,
    and - Keys' kernel reproduces quadratics - the cubic is the polynomial itself up to the float32 rounding of the samples."""
    torch = torch_gpu
    s2gt = _s2_geotransform()
    out = s2_emit.reproject_scene(torch.from_numpy(scene["src"]).cuda(), SRC_GT, epsg=EPSG, s2_geotransform=s2gt, s2_shape=S2_SHAPE,
                                  rule="strict", coords=scene["out"].coords)
    got = out.scene.cpu().numpy()
    left, _, _, top, rows, cols = out.grid
    E, N = np.meshgrid(left + (np.arange(cols) + 0.5) * 60.0, top - (np.arange(rows) + 0.5) * 60.0)
    lon, lat = s2_emit.tm_inverse(E, N, s2_emit.utm_params(EPSG))
    sx, sy = (lon - SRC_GT[0]) / SRC_GT[1] - 0.5, (lat - SRC_GT[3]) / SRC_GT[5] - 0.5
    bar = rc.coord_bar(SRC_GT[1])
    dev = out.coords.cpu().numpy()
    assert np.abs(dev[..., 0] - sy).max() <= 2 * bar and np.abs(dev[..., 1] - sx).max() <= 2 * bar
    judged = (sy >= 2.0) & (sy <= HS - 3.0) & (sx >= 2.0) & (sx <= WS - 3.0)           # at least 2 source pixels inside
    excluded = 1.0 - judged.mean()
    print(f"planted scene: {rows} x {cols} cells, {100 * excluded:.1f} % excluded (cap {100 * MAX_EXCLUDED:.0f} %)")
    assert excluded <= MAX_EXCLUDED
    ref, _, _ = rc.warp_ref(scene["src"], np.stack([sy, sx], axis=-1), None, -9999.0, rc.STRICT)
    _, coef = _planted()
    worst = 0.0
    for b, (c0, cy, cx, cyy, cxx, cxy) in enumerate(coef):
        grad = np.abs(cy + 2 * cyy * sy + cxy * sx) + np.abs(cx + 2 * cxx * sx + cxy * sy)
        allowed = np.spacing(np.abs(ref[b]).astype(np.float32)).astype(np.float64) + grad * bar
        err = np.abs(got[b].astype(np.float64) - ref[b].astype(np.float64))
        worst = max(worst, float((err / allowed)[judged].max()))
        assert (err[judged] <= allowed[judged]).all(), (b, float((err / allowed)[judged].max()))
        poly = c0 + cy * sy + cx * sx + cyy * sy * sy + cxx * sx * sx + cxy * sy * sx
        # the samples are rounded to float32 (half an ulp each, weights summing to at most 1.27 in absolute value) before the cubic
        assert np.abs(ref[b].astype(np.float64) - poly)[judged].max() <= 2.0 * np.spacing(np.float32(np.abs(poly[judged]).max()))
    print(f"planted scene: worst |err| / allowed {worst:.3g}")


def test_coords_reuse_gives_the_same_bits(torch_gpu, scene):
    """The loc / obs case: a second raster of the same geometry under coords= - no first launch, the same field, the same bits."""
    torch = torch_gpu
    from gpu_harness import LaunchLog
    log = LaunchLog("hsr_reproject_last_launch", joined=True)
    src = torch.from_numpy(scene["masked"]).cuda()
    kw = dict(epsg=EPSG, s2_geotransform=_s2_geotransform(), s2_shape=S2_SHAPE)
    log.clear()
    first = s2_emit.reproject_scene(src, SRC_GT, **kw)
    assert log.read() == ["reproject_coords_kernel", "reproject_warp_kernel<LDS, RENORM>"]            # two launches
    again = s2_emit.reproject_scene(src, SRC_GT, coords=first.coords, **kw)
    assert log.read() == ["reproject_warp_kernel<LDS, RENORM>"] and again.coords is first.coords
    same_bits(again.scene.cpu().numpy(), first.scene.cpu().numpy(), "coords= reuse")
    same_bits(first.scene.cpu().numpy(), scene["out"].scene.cpu().numpy(), "a second call")
    loc = s2_emit.reproject_scene(src[:1] * 2.0, SRC_GT, coords=first.coords, nodata=-19998.0, **kw)    # another raster, one band
    ref, _, _ = rc.warp_ref(scene["masked"][:1] * np.float32(2.0), first.coords.cpu().numpy(), -19998.0, -9999.0, rc.RENORM)
    same_bits(loc.scene.cpu().numpy(), ref, "another raster under the same field")
    with pytest.raises(ValueError, match="coords"):
        s2_emit.reproject_scene(src, SRC_GT, coords=first.coords[:-1], **kw)


def test_result_feeds_find_valid_paired_tiles(torch_gpu, scene):
    """The output goes into find_valid_paired_tiles with emit_nodata=-9999 as it is: no copy, no conversion; the windows that the
    fill and the masked corner reach are dropped, and the device tensor selects what its host copy selects."""
    torch, out = torch_gpu, scene["out"]
    emit = out.scene
    assert emit.is_contiguous() and emit.dtype == torch.float32 and emit.is_cuda
    rows, cols = emit.shape[1:]
    rng = np.random.default_rng(5)
    s2 = torch.from_numpy(rng.uniform(0.1, 0.9, (2, rows * 6, cols * 6)).astype(np.float32)).cuda()
    ptr = emit.data_ptr()
    tiles = s2_emit.find_valid_paired_tiles(emit, s2, emit_tile_size=8, scale=6, emit_nodata=-9999.0)
    host = s2_emit.find_valid_paired_tiles(emit.cpu().numpy(), s2.cpu().numpy(), emit_tile_size=8, scale=6, emit_nodata=-9999.0)
    assert emit.data_ptr() == ptr and tiles == host
    total = (rows // 8) * (cols // 8)
    assert 0 < len(tiles) < total
    filled = (emit.cpu().numpy() == -9999.0).any(axis=0)
    for t in tiles:
        w = t["emit_window"]
        assert not filled[w.row_off:w.row_off + 8, w.col_off:w.col_off + 8].any()
