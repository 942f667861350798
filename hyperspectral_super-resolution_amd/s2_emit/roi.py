"""Polygon regions of interest on the device.

The reference takes a polygon where every stage here took a rectangle: ``count_cloud_pixels`` and ``scl_metrics``
(``s2_data/cloud_utils.py``:33-53, :82-101) and ``_save_roi_from_asset`` (``s2_data/s2_utils.py``:361-383) call
``rasterio.mask.mask(ds, [roi], crop=True)``, and ``spatial_subset`` (``EMIT_data/emit_tools.py``:529-619) clips the GLT with
``rio.clip(..., all_touched=True)`` and cuts the swath to the rows and columns the clipped table still names.  Here (definition:
include/hsr_roi.h; kernels: csrc/hsr_roi.hip):

    rasterize_roi            a polygon set -> the (h, w) uint8 plane of a grid or of a window of it, centre or touched rule.
    scl_metrics_roi, count_cloud_pixels_roi   the reference's dict / tuple from ONE launch that reads the SCL under the polygon only.
    spatial_subset           the GLT clipped to the polygon and re-indexed to the swath slice it needs, ranges on the device.
    clip_cube                ``_save_roi_from_asset``'s crop + mask: the window slice and ``mask_cube`` under the inverted plane.

The rules are the header's, not GDAL's: in general position they are what ``all_touched=False`` / ``True`` mean; on ties (an edge
through a centre or along a lattice line) the header decides, and rasterio's window rounding is not claimed - the window is the
cells the vertex bounding box touches.  The even-odd rule runs over all rings together: a hole is a ring, overlapping parts cancel.
``overlap_emit_fraction`` (polygon against polygon) is host geometry and has no counterpart here; ``merge_emit``'s polygon needs
nothing new: pass its result to ``clip_cube``.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple

import numpy as np

from . import _native as nat
from ._engine import _ptr, _stream
from .clouds import CLOUD_CLASSES, SCL_NAMES, _OTHER, _plane, _plane_dev, mask_cube
from .ortho import _glt_i32, _i32, _shape_dtype, _INT_DTYPES
from .pairs import _dtype_name
from .reproject import tm_forward, utm_params
from .ridge import _is_torch

MAX_EDGES = nat.HSR_ROI_MAX_EDGES
_COORD_MAX = 1e300
_I32_MAX = (1 << 31) - 1
_RoiPlan = namedtuple("_RoiPlan", "verts offsets gt shape")


def _ring(r, what):
    if _is_torch(r):
        r = r.detach().cpu().numpy()
    a = np.asarray(r, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] < 2 or a.shape[0] < 1:
        raise ValueError(f"{what}: a ring is an (n, 2) array of (x, y) vertices, got shape {a.shape}")
    a = a[:, :2]                                                         # GeoJSON positions may carry a height
    if a.shape[0] > 3 and (a[0] == a[-1]).all():                         # a closing vertex: rings are closed implicitly
        a = a[:-1]
    return a


def _is_ring(x):
    if _is_torch(x) or isinstance(x, np.ndarray):
        return len(x.shape) == 2
    try:
        return len(x) > 0 and not hasattr(x[0], "shape") and np.ndim(x[0][0]) == 0
    except (TypeError, IndexError, KeyError):
        return False


def polygon_rings(polygons):
    """``polygons`` -> the list of its rings as (n, 2) float64 arrays.  Taken: one ring; a list of rings; a list of parts, each a
    list (exterior, hole, ...) of rings; a GeoJSON-style ``{"type": "Polygon" | "MultiPolygon", "coordinates": ...}`` dict, what
    ``shapely.geometry.mapping`` hands the reference's ``rio_mask``; anything with ``__geo_interface__``.  Rings are arrays, tensors
    or nested sequences; a repeated closing vertex is dropped.  Exterior and hole are not told apart: the rule is even-odd."""
    if hasattr(polygons, "__geo_interface__"):
        polygons = polygons.__geo_interface__
    if isinstance(polygons, dict):
        kind, coords = polygons.get("type"), polygons.get("coordinates")
        if kind == "Polygon":
            parts = [coords]
        elif kind == "MultiPolygon":
            parts = coords
        else:
            raise ValueError(f"polygons: a GeoJSON dict of type 'Polygon' or 'MultiPolygon', got {kind!r}")
        try:
            return [_ring(r, "polygons") for part in parts for r in part]
        except TypeError:
            raise ValueError("polygons: malformed GeoJSON coordinates") from None
    if _is_ring(polygons):
        return [_ring(polygons, "polygons")]
    try:
        items = list(polygons)
    except TypeError:
        raise ValueError(f"polygons: a list of rings, a list of parts or a GeoJSON dict, got {type(polygons).__name__}") from None
    rings = []
    for k, item in enumerate(items):
        if _is_ring(item):
            rings.append(_ring(item, f"polygons[{k}]"))
        else:
            try:
                sub = list(item)
            except TypeError:
                raise ValueError(f"polygons[{k}]: a ring (n, 2) or a part (a list of rings)") from None
            rings.extend(_ring(r, f"polygons[{k}][{j}]") for j, r in enumerate(sub))
    if not rings:
        raise ValueError("polygons: no ring")
    return rings


def _grid(transform, shape):
    try:
        gt = tuple(float(v) for v in transform)
        H, W = (_i32(v, "shape") for v in shape)
    except TypeError:
        raise ValueError("transform is a GDAL geotransform (x0, dx, 0, y0, 0, dy) and shape (H, W)") from None
    if len(gt) != 6:
        raise ValueError(f"transform={transform!r}: a GDAL geotransform (x0, dx, 0, y0, 0, dy)")
    if not all(math.isfinite(v) for v in gt) or gt[1] == 0.0 or gt[5] == 0.0:
        raise ValueError(f"transform={gt}: every term finite, dx and dy not 0")
    if gt[2] != 0.0 or gt[4] != 0.0:
        raise ValueError(f"transform={gt}: rotation terms are not supported")
    if H < 1 or W < 1:
        raise ValueError(f"shape={shape!r}: (H, W), both at least 1")
    return gt, (H, W)


def _plan_roi(polygons, transform, shape, crs=None, utm=None) -> _RoiPlan:
    """Everything of a polygon set and its grid that needs no GPU: the rings as one vertex array with offsets, through
    ``tm_forward`` when ``crs="wgs84"``, checked by ``hsr_roi_check_host`` (a ring below 3 vertices, a non-finite vertex and more
    than ``MAX_EDGES`` edges are refused, ``HsrError``)."""
    rings = polygon_rings(polygons)
    gt, shape = _grid(transform, shape)
    verts = np.ascontiguousarray(np.concatenate(rings, axis=0), dtype=np.float64)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)
    if crs is not None:
        if str(crs).lower() not in ("wgs84", "epsg:4326", "4326"):
            raise ValueError(f"crs={crs!r}: None (the grid's own) or 'wgs84' with utm=")
        if utm is None:
            raise ValueError("crs='wgs84' needs utm= (an EPSG code 326xx / 327xx, or the six parameters of utm_params)")
        params = tuple(utm) if isinstance(utm, (tuple, list)) and len(utm) == 6 else utm_params(utm)
        e, n = tm_forward(verts[:, 0], verts[:, 1], params)            # the vertices and only the vertices: shapely.ops.transform
        verts = np.ascontiguousarray(np.stack([e, n], axis=1))
    elif utm is not None:
        raise ValueError("utm= is used with crs='wgs84' only")
    lib = nat.load()
    nat.check(lib.hsr_roi_check_host(verts.ctypes.data, offsets.ctypes.data, len(rings), len(verts)), "hsr_roi_check_host")
    return _RoiPlan(verts, offsets, gt, shape)


def _bbox_window(verts, gt, shape):
    """(row_off, col_off, h, w) of the cells the vertex bounding box touches, clamped to the grid - it holds every touched cell -
    or None when the box misses the grid.  u, v as in include/hsr_roi.h."""
    H, W = shape
    with np.errstate(over="ignore"):
        u = np.clip((verts[:, 0] - gt[0]) / gt[1], -_COORD_MAX, _COORD_MAX)
        v = np.clip((verts[:, 1] - gt[3]) / gt[5], -_COORD_MAX, _COORD_MAX)
    c0, c1 = max(math.floor(u.min()), 0), min(math.floor(u.max()), W - 1)
    r0, r1 = max(math.floor(v.min()), 0), min(math.floor(v.max()), H - 1)
    if c0 > c1 or r0 > r1:
        return None
    return (int(r0), int(c0), int(r1 - r0 + 1), int(c1 - c0 + 1))


def _window(window, shape, what="window"):
    H, W = shape
    if window is None:
        return (0, 0, H, W)
    try:
        win = tuple(_i32(v, what) for v in window)
    except TypeError:
        raise ValueError(f"{what}={window!r}: (row_off, col_off, height, width) on the grid") from None
    if len(win) != 4:
        raise ValueError(f"{what}={window!r}: (row_off, col_off, height, width) on the grid")
    r0, c0, h, w = win
    if r0 < 0 or c0 < 0 or h < 1 or w < 1 or r0 + h > H or c0 + w > W:
        raise ValueError(f"{what}={win}: leaves the {H} x {W} grid")
    return win


def _upload(plan, torch, dev):
    return torch.from_numpy(plan.verts).to(dev), torch.from_numpy(plan.offsets).to(dev), (C.c_double * 6)(*plan.gt)


def rasterize_roi(polygons, transform, shape, *, all_touched=False, invert=False, window=None, out=None, crs=None, utm=None):
    """The polygon set on the grid ``transform`` (a GDAL geotransform without rotation; dy of either sign) x ``shape`` (H, W) ->
    an (h, w) uint8 device tensor: 1 where the cell is inside, 0 outside; ``invert`` swaps them, which gives the mask ``mask_cube``
    takes.  ``all_touched=False`` is the centre rule (``rasterio.mask``'s default), ``True`` the touched rule (``rio.clip`` in
    ``spatial_subset``); both as include/hsr_roi.h states them.  ``window`` (row_off, col_off, height, width): only that part, which
    IS the slice of the full plane.  ``out``: an (h, w) uint8 device tensor to write into (a row stride is kept).
    ``crs="wgs84"`` with ``utm=`` (an EPSG code or ``utm_params``' tuple): the vertices are (lon, lat) and go through
    ``tm_forward`` first, as the reference's ``reproject_geom`` sends them through ``shapely.ops.transform``.
    One launch on the current stream, every byte written once, no host synchronisation after the polygon's upload."""
    plan = _plan_roi(polygons, transform, shape, crs, utm)
    return _rasterize(plan, _window(window, plan.shape), all_touched, invert, out)


def _rasterize(plan, win, all_touched, invert, out=None, dev=None):
    """``rasterize_roi`` behind the planning: every check of ``out`` before the GPU is asked for, then the upload and the launch on
    ``out``'s device (or ``dev``, or the current one)."""
    r0, c0, h, w = win
    if out is not None:
        if not _is_torch(out) or tuple(out.shape) != (h, w) or _dtype_name(out) != "uint8" or out.stride(1) != 1 or out.stride(0) < w:
            raise ValueError(f"out: a ({h}, {w}) uint8 device tensor with contiguous rows")
        if not out.is_cuda:
            raise ValueError(f"out: a device tensor (it is written by the kernel), got one on {out.device}")
        if dev is not None and out.device != dev:
            raise ValueError(f"out: on {out.device}, the other operands on {dev}")
    torch = nat.require_gpu()
    lib = nat.load()
    if out is not None:
        dev = out.device
    elif dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    V, O, gt = _upload(plan, torch, dev)
    if out is None:
        out = torch.empty((h, w), dtype=torch.uint8, device=dev)
    nat.check(lib.hsr_roi_rasterize(_ptr(V), _ptr(O), len(plan.offsets) - 1, len(plan.verts), gt, plan.shape[0], plan.shape[1],
                                    nat.HSR_ROI_TOUCHED if all_touched else nat.HSR_ROI_CENTER, r0, c0, h, w, 0 if invert else 1,
                                    1 if invert else 0, _ptr(out), out.stride(0), _stream(torch, out)), "hsr_roi_rasterize")
    return out


def _roi_counts(scl, polygons, transform, all_touched, crs, utm):
    """-> (counts (16,) int64 of the inside cells, inside, window cells): one launch, one copy of 17 int32."""
    shape = _plane(scl, "scl")
    plan = _plan_roi(polygons, transform, shape, crs, utm)
    win = _bbox_window(plan.verts, plan.gt, shape)
    if win is None:
        raise ValueError("Input shapes do not overlap raster.")          # rasterio.mask's own words
    r0, c0, h, w = win
    if h * w > _I32_MAX:
        raise ValueError(f"a window of {h} x {w} cells: at most 2^31 - 1")
    torch = nat.require_gpu()
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    S, rs = _plane_dev(scl, torch, dev)
    V, O, gt = _upload(plan, torch, dev)
    res = torch.empty((nat.HSR_SCL_BINS + 1,), dtype=torch.int32, device=dev)
    nat.check(lib.hsr_roi_class_counts(_ptr(V), _ptr(O), len(plan.offsets) - 1, len(plan.verts), gt, shape[0], shape[1],
                                       nat.HSR_ROI_TOUCHED if all_touched else nat.HSR_ROI_CENTER, r0, c0, h, w, _ptr(S), rs, _ptr(res),
                                       C.c_void_p(res.data_ptr() + 4 * nat.HSR_SCL_BINS), _stream(torch)), "hsr_roi_class_counts")
    host = res.cpu().numpy().astype(np.int64)
    return host[:nat.HSR_SCL_BINS], int(host[nat.HSR_SCL_BINS]), h * w


def scl_metrics_roi(scl, polygons, transform, include_shadows: bool = False, *, all_touched=False, crs=None, utm=None):
    """The reference's ``scl_metrics(scl_tif, roi, include_shadows)`` (cloud_utils.py:82-101) on an SCL plane (H, W) uint8 - an
    array or a device tensor - with the plane's geotransform and the polygon: its dict, from ONE launch and one copy of 17 int32.
    ``rio_mask(..., crop=True, filled=True)`` hands the reference the polygon's window with 0 outside the polygon, so total_px is
    the window's cells (here: the cells the vertex bounding box touches; rasterio's window rounding is not claimed), nodata_px the
    window's cells less the non-zero cells inside, and the class counts those of the inside cells, the outside added to "No data".
    Values above 11 share the key "other", as in ``scl_metrics``.  A polygon that misses the plane raises ValueError, as rasterio
    does."""
    c, inside, cells = _roi_counts(scl, polygons, transform, all_touched, crs, utm)
    c = c.copy()
    c[0] += cells - inside
    cloud_set = [8, 9, 10] + ([3] if include_shadows else [])
    valid_px, cloud_px = int(cells - c[0]), int(c[cloud_set].sum())
    names = {k: SCL_NAMES.get(k, "other") for k in range(_OTHER + 1)}
    return {
        "total_px": int(cells),
        "valid_px": valid_px,
        "nodata_px": int(c[0]),
        "cloud_px": cloud_px,
        "cloud_frac_valid": (cloud_px / valid_px) if valid_px else np.nan,
        "class_counts": {names[k]: int(c[k]) for k in range(_OTHER + 1) if c[k]},
    }


def count_cloud_pixels_roi(scl, polygons, transform, *, all_touched=False, crs=None, utm=None):
    """The reference's ``count_cloud_pixels(scl_href, roi)`` (cloud_utils.py:33-53): ``(clouds, total)`` with total the cells inside
    the polygon that are not 0 and clouds those of ``CLOUD_CLASSES`` among them.  One launch, one copy of 17 int32."""
    c, inside, _ = _roi_counts(scl, polygons, transform, all_touched, crs, utm)
    return int(c[sorted(CLOUD_CLASSES)].sum()), int(inside - c[0])


class SubsetOutput(namedtuple("SubsetOutput", "glt window geotransform ranges n_valid")):
    """``spatial_subset``'s result.  glt (h, w, 2) int32 on the device, one-based on the swath slice; window (row_off, col_off, h,
    w) on the GLT grid; geotransform the window's; ranges a device int32 (4,) (down_lo, down_hi, cross_lo, cross_hi), zero-based
    like the reference's subset_down / subset_cross; n_valid a device int32 scalar."""
    __slots__ = ()

    def slice(self, swath):
        """``swath[down_lo:down_hi + 1, cross_lo:cross_hi + 1]`` (a view): the ONE host copy of the ranges.  An empty range raises
        the reference's ValueError (``np.min`` of an empty array, emit_tools.py:567)."""
        d0, d1, c0, c1 = (int(v) for v in self.ranges.cpu().tolist())
        if d0 > d1 or c0 > c1:
            raise ValueError("zero-size array to reduction operation minimum which has no identity")
        return swath[d0:d1 + 1, c0:c1 + 1]


def spatial_subset(glt, transform, polygons, *, swath_shape=None, crs=None, utm=None) -> SubsetOutput:
    """The reference's ``spatial_subset(ds, gdf)`` (emit_tools.py:529-619) on a lookup table ``glt`` (H, W, 2) of one-based (column,
    row) entries (``glt_from_xy``) with the GLT grid's geotransform: the step between ``emit_xarray`` and ``ortho_xr`` that
    ``ortho_scene(window=)`` does not replace, because it also shrinks the swath.

    The window is the cells the polygon's vertex bounding box touches, known on the host without a synchronisation.  One launch
    clips it under the touched rule (``rio.clip(..., all_touched=True)``): untouched entries become 0, and the minima and maxima
    of the valid ``glt_x`` / ``glt_y`` (:563-573) go to a device record; a second launch reads the record and writes
    ``max(glt - lo, 0)`` (:594-595).  ``SubsetOutput.slice(swath)`` is the swath the table then indexes, so that
    ``ortho_scene(out.slice(swath), out.glt)`` is the scene of the polygon.  ``swath_shape`` (rows, cols) is optional and only
    validated: no entry is read on the host, and an entry beyond the swath stays what it is for ``ortho_scene``, a dropped one.
    A polygon that misses the grid raises ValueError."""
    gshape, gdt = _shape_dtype(glt, "glt")
    if len(gshape) != 3 or gshape[2] != 2 or min(gshape) < 1 or gdt not in _INT_DTYPES:
        raise ValueError(f"glt: expected a non-empty integer (H, W, 2) table (glt_from_xy), got {gdt} {gshape}")
    if swath_shape is not None and (len(tuple(swath_shape)) < 2 or min(int(v) for v in tuple(swath_shape)[:2]) < 1):
        raise ValueError(f"swath_shape={swath_shape!r}: (rows, cols)")
    plan = _plan_roi(polygons, transform, gshape[:2], crs, utm)
    win = _bbox_window(plan.verts, plan.gt, plan.shape)
    if win is None:
        raise ValueError("the polygons do not overlap the GLT grid")
    r0, c0, h, w = win
    gt = plan.gt
    win_gt = (gt[0] + c0 * gt[1], gt[1], 0.0, gt[3] + r0 * gt[5], 0.0, gt[5])
    torch = nat.require_gpu()
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    G = _glt_i32(glt, 0, torch, dev)
    V, O, cgt = _upload(plan, torch, dev)
    out = torch.empty((h, w, 2), dtype=torch.int32, device=dev)
    rec = torch.empty((nat.HSR_ROI_RECORD,), dtype=torch.int32, device=dev)
    st = _stream(torch, out)
    nat.check(lib.hsr_roi_glt_clip(_ptr(V), _ptr(O), len(plan.offsets) - 1, len(plan.verts), cgt, gshape[0], gshape[1], _ptr(G), r0, c0, h,
                                   w, _ptr(out), _ptr(rec), st), "hsr_roi_glt_clip")
    nat.check(lib.hsr_roi_glt_reindex(_ptr(out), h, w, _ptr(rec), st), "hsr_roi_glt_reindex")
    return SubsetOutput(out, win, win_gt, rec[:4], rec[4])


def clip_cube(cube, polygons, transform, *, fill=float("nan"), crop=True, all_touched=False, crs=None, utm=None):
    """``_save_roi_from_asset``'s ``rio_mask(src, [roi], crop=True)`` (s2_utils.py:361-383) on a device cube (T, H, W) float32 with
    its geotransform -> ``(cube, geotransform)``: with ``crop`` the slice of the window the polygon's vertex bounding box touches
    (a copy; the input is left as it is) and the window's geotransform, otherwise a copy of the whole cube; ``fill`` outside the
    polygon.  Composition only: ``rasterize_roi(invert=True, window=)``'s launch and ``mask_cube``."""
    if not _is_torch(cube) or _dtype_name(cube) != "float32" or cube.dim() != 3 or min(cube.shape) < 1 or not cube.is_cuda:
        raise ValueError("cube: a non-empty (T, H, W) float32 device tensor")
    shape = (int(cube.shape[1]), int(cube.shape[2]))
    plan = _plan_roi(polygons, transform, shape, crs, utm)
    win = _bbox_window(plan.verts, plan.gt, shape) if crop else (0, 0) + shape
    if win is None:
        raise ValueError("Input shapes do not overlap raster.")
    r0, c0, h, w = win
    gt = plan.gt
    mask = _rasterize(plan, win, all_touched, True, dev=cube.device)                # the plan made above: one parse, one check, one upload
    part = cube[:, r0:r0 + h, c0:c0 + w].clone()
    return mask_cube(part, mask, fill=fill), (gt[0] + c0 * gt[1], gt[1], 0.0, gt[3] + r0 * gt[5], 0.0, gt[5])
