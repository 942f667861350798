"""s2_emit.roi on an MI355X: the polygon entry points against the reference's own lines restated in NumPy under the mask of
tests/roi_cases.py - scl_metrics_roi / count_cloud_pixels_roi against np.unique / np.isin of np.where(mask, scl, 0) over the window
(cloud_utils.py:47-53, :85-100), spatial_subset against emit_tools.py:557-600, the orthorectification of the subset against the
orthorectification of the whole swath under the clipped table (both sides the existing kernels), clip_cube against the slice and
mask_cube written by hand, and a window of rasterize_roi against the slice of the full plane.  Every comparison is an equality."""
import numpy as np
import pytest

import ortho_cases as oc
import roi_cases as rc
import s2_emit
from gpu_harness import torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from s2_emit import reproject
from test_gpu_roi_instances import scl_plane

pytestmark = pytest.mark.gpu

H, W = 150, 310
GT = rc.GT_UTM
FOOTPRINT = [rc.to_world([(40.3, 5.2), (290.7, 38.4), (262.1, 141.9), (12.6, 109.3)], GT)]           # a rotated quadrilateral
HOLED = [rc.to_world(r, GT) for r in rc.holed(H, W)]
CASES = {"footprint": FOOTPRINT, "holed": HOLED, "off-grid": [rc.to_world([(-40.5, -20.5), (200.2, 60.3), (90.1, 400.7)], GT)]}


def _ref_metrics(scl, mask, win, include_shadows):
    """cloud_utils.py:85-100 on what rio_mask(crop=True, filled=True) returns: the window with 0 outside the polygon."""
    r0, c0, h, w = win
    data = np.where(mask, scl[r0:r0 + h, c0:c0 + w], 0)
    vals, counts = np.unique(data, return_counts=True)
    by_class = {int(v): int(c) for v, c in zip(vals, counts)}
    valid = data != 0
    cloud_set = {8, 9, 10} | ({3} if include_shadows else set())
    cloud_px, valid_px = int(np.isin(data, list(cloud_set))[valid].sum()), int(valid.sum())
    names = {}
    for k, v in by_class.items():                                         # ours: the values above 11 share the key "other"
        key = s2_emit.SCL_NAMES.get(k, "other")
        names[key] = names.get(key, 0) + v
    return {"total_px": int(counts.sum()), "valid_px": valid_px, "nodata_px": by_class.get(0, 0), "cloud_px": cloud_px,
            "cloud_frac_valid": (cloud_px / valid_px) if valid_px else np.nan, "class_counts": names}, \
        (int(np.isin(data[valid], list(s2_emit.CLOUD_CLASSES)).sum()), valid_px)


@pytest.mark.parametrize("all_touched", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_scl_metrics_and_cloud_counts(torch_gpu, name, all_touched):
    rings = CASES[name]
    scl = scl_plane(H, W, 5)
    assert set(range(12)) <= set(np.unique(scl).tolist())
    win = rc.bbox_window(rings, GT, (H, W))
    mask = rc.rasterize_ref(rings, GT, (H, W), rc.TOUCHED if all_touched else rc.CENTER, win)
    for shadows in (False, True):
        want, cloud = _ref_metrics(scl, mask, win, shadows)
        for plane in (scl, torch_gpu.from_numpy(scl).cuda()):
            got = s2_emit.scl_metrics_roi(plane, rings, GT, shadows, all_touched=all_touched)
            assert got == want
        assert s2_emit.count_cloud_pixels_roi(scl, {"type": "Polygon", "coordinates": [r.tolist() for r in rings]}, GT, all_touched=all_touched) == cloud
    with pytest.raises(ValueError, match="do not overlap"):
        s2_emit.scl_metrics_roi(scl, [rings[0] + 1e7], GT)


def test_scl_metrics_without_a_valid_pixel(torch_gpu):
    got = s2_emit.scl_metrics_roi(np.zeros((H, W), np.uint8), FOOTPRINT, GT)
    assert got["valid_px"] == 0 and np.isnan(got["cloud_frac_valid"]) and got["class_counts"] == {"No data": got["total_px"]}


@pytest.mark.parametrize("window", [(0, 0, H, W), (1, 0, 64, 256), (0, 1, 65, 257), (17, 33, 100, 200), (149, 309, 1, 1)])
def test_rasterize_window_is_the_slice(torch_gpu, window):
    for rings, touched in ((FOOTPRINT, False), (HOLED, True)):
        full = s2_emit.rasterize_roi(rings, GT, (H, W), all_touched=touched).cpu().numpy()
        np.testing.assert_array_equal(full, rc.rasterize_ref(rings, GT, (H, W), rc.TOUCHED if touched else rc.CENTER).astype(np.uint8))
        r0, c0, h, w = window
        part = s2_emit.rasterize_roi(rings, GT, (H, W), all_touched=touched, window=window)
        np.testing.assert_array_equal(part.cpu().numpy(), full[r0:r0 + h, c0:c0 + w])
        out = torch_gpu.full((h, w + 5), 9, dtype=torch_gpu.uint8, device="cuda")
        inv = s2_emit.rasterize_roi(rings, GT, (H, W), all_touched=touched, window=window, invert=True, out=out[:, :w])
        assert inv.data_ptr() == out.data_ptr()
        np.testing.assert_array_equal(out.cpu().numpy()[:, :w], 1 - full[r0:r0 + h, c0:c0 + w])
        assert (out.cpu().numpy()[:, w:] == 9).all()


def test_rasterize_lon_lat(torch_gpu):
    lonlat = np.array([[-117.2, 34.1], [-117.0, 34.15], [-117.1, 34.3]])
    gt, shape = (470000.0, 100.0, 0.0, 3800000.0, 0.0, -100.0), (400, 300)
    e, n = reproject.tm_forward(lonlat[:, 0], lonlat[:, 1], reproject.utm_params(32611))
    got = s2_emit.rasterize_roi([lonlat], gt, shape, crs="wgs84", utm=32611).cpu().numpy()
    want = rc.rasterize_ref([np.stack([e, n], axis=1)], gt, shape, rc.CENTER)
    assert want.any() and not want.all()
    np.testing.assert_array_equal(got, want.astype(np.uint8))


def _swath_and_glt():
    rows, cols, bands = 211, 97, 5
    return oc.swath_of(rows, cols, bands), rc.glt_of(H, W, rows, cols, seed=3)


@pytest.mark.parametrize("name", ["footprint", "holed", "off-grid"])
def test_spatial_subset(torch_gpu, name):
    rings = CASES[name]
    swath, glt = _swath_and_glt()
    out = s2_emit.spatial_subset(glt, GT, rings, swath_shape=swath.shape)
    win = rc.bbox_window(rings, GT, (H, W))
    mask = rc.rasterize_ref(rings, GT, (H, W), rc.TOUCHED, win)
    clipped, rec = rc.glt_clip_ref(glt, mask, win)                       # emit_tools.py:557-573
    assert out.window == win and out.geotransform == (GT[0] + win[1] * GT[1], GT[1], 0.0, GT[3] + win[0] * GT[5], 0.0, GT[5])
    assert out.ranges.is_cuda and out.n_valid.is_cuda
    assert out.ranges.cpu().tolist() == rec[:4].tolist() and int(out.n_valid) == int(rec[4])
    np.testing.assert_array_equal(out.glt.cpu().numpy(), rc.glt_reindex_ref(clipped, rec))           # :594-595
    sub = out.slice(swath)
    np.testing.assert_array_equal(sub, swath[rec[0]:rec[1] + 1, rec[2]:rec[3] + 1])
    # the subset orthorectified == the whole swath orthorectified under the clipped table, on the window: the existing kernels
    full = np.zeros_like(glt)
    full[win[0]:win[0] + win[2], win[1]:win[1] + win[3]] = clipped
    a = s2_emit.ortho_scene(np.ascontiguousarray(sub), out.glt)
    b = s2_emit.ortho_scene(swath, full, window=out.window)
    np.testing.assert_array_equal(a.scene.cpu().numpy().view(np.uint32), b.scene.cpu().numpy().view(np.uint32))
    assert (a.scene != -9999.0).any() and int(a.dropped) == 0          # b counts the entries the re-index turned into no-data
    dev = s2_emit.spatial_subset(torch_gpu.from_numpy(glt).cuda(), GT, {"type": "MultiPolygon", "coordinates": [[r.tolist() for r in rings]]})
    assert torch_gpu.equal(dev.glt, out.glt) and torch_gpu.equal(dev.ranges, out.ranges)


def test_spatial_subset_empty_range(torch_gpu):
    swath, glt = _swath_and_glt()
    glt = np.where(glt > 0, 0, glt)                                        # no valid entry anywhere
    out = s2_emit.spatial_subset(glt, GT, FOOTPRINT)
    assert out.ranges.cpu().tolist() == [rc.I32_MAX, -1, rc.I32_MAX, -1] and int(out.n_valid) == 0 and not out.glt.any()
    with pytest.raises(ValueError, match="zero-size array to reduction operation minimum"):
        out.slice(swath)
    with pytest.raises(ValueError, match="do not overlap"):
        s2_emit.spatial_subset(glt, GT, [FOOTPRINT[0] + 1e7])


@pytest.mark.parametrize("crop", [True, False])
def test_clip_cube(torch_gpu, crop):
    torch = torch_gpu
    rng = np.random.default_rng(11)
    cube = torch.from_numpy(rng.random((3, H, W), dtype=np.float32)).cuda()
    before = cube.clone()
    for rings, touched, fill in ((FOOTPRINT, False, float("nan")), (HOLED, True, -9999.0)):
        got, gt = s2_emit.clip_cube(cube, rings, GT, fill=fill, crop=crop, all_touched=touched)
        win = rc.bbox_window(rings, GT, (H, W)) if crop else (0, 0, H, W)
        r0, c0, h, w = win
        mask = s2_emit.rasterize_roi(rings, GT, (H, W), all_touched=touched, invert=True, window=win)
        want = s2_emit.mask_cube(cube[:, r0:r0 + h, c0:c0 + w].clone(), mask, fill=fill)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        ref = rc.rasterize_ref(rings, GT, (H, W), rc.TOUCHED if touched else rc.CENTER, win)
        g = got.cpu().numpy()
        assert (np.isnan(g[:, ~ref]).all() if np.isnan(fill) else (g[:, ~ref] == fill).all())
        np.testing.assert_array_equal(g[:, ref], before.cpu().numpy()[:, r0:r0 + h, c0:c0 + w][:, ref])
        assert gt == (GT[0] + c0 * GT[1], GT[1], 0.0, GT[3] + r0 * GT[5], 0.0, GT[5])
    assert torch.equal(cube, before)
