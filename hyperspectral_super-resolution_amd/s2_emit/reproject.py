"""An EMIT scene on its geographic grid -> the Sentinel-2 UTM grid on the device: the stage between ``ortho_scene`` and
``coregister_scene`` / the tile-pair drivers, which all expect an EMIT pixel to be the ``factor`` x ``factor`` block of S2 pixels,
both on the S2 60 m / 10 m UTM lattice.

The reference does this with ``gdalwarp -r cubic`` (EMIT_data/emit_proj.py:876-940) on an extent it derives itself
(``_bounds_to_out_crs``, ``_intersect``, ``_compute_te``, :309-382), for the data, loc and obs rasters alike (:1035,1135,1227).
GDAL and pyproj are a program and a library call; they are NOT reproduced.  What is here is the same flow on GPU tensors with the
algorithm defined in include/hsr_reproject.h, in two HIP stages (csrc/hsr_reproject.hip):

    coords  ``reproject_coords``  for every cell of the UTM output grid the fractional source index, by the inverse transverse
                                  Mercator projection (Krueger series to n^6)
    warp    ``remap_scene``       out[b] = Keys cubic (a = -0.5, GDAL's "cubic") of scene[b] at that index - under ANY field

``reproject_scene`` chains them; ``coords=`` reuses a field for the next raster of the same geometry.  ``utm_target_grid`` restates
the reference's extent rule on the host; ``tm_forward`` / ``tm_inverse`` are the projection in NumPy float64, host only.  Neither
the geometry nor the resampling claims GDAL's bits, the kernel is not widened for minification, and there is no antimeridian wrap.
A geotransform is GDAL's six numbers (x0, dx, 0, y0, 0, -dy) of a north-up raster; rotation terms must be zero.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

from . import _engine as eng
from . import _native as nat

ReprojectOutput = namedtuple("ReprojectOutput", "scene geotransform grid counts coords")

WGS84_A, WGS84_INV_F = 6378137.0, 298.257223563
_RULES = {"strict": nat.HSR_REPROJECT_STRICT, "renorm": nat.HSR_REPROJECT_RENORM}
_FOOTPRINT_SLACK = 1.25      # the staged box is sized for this much more than the grids' cell ratio; a wilder field still warps correctly
_EPS = 1e-9                  # emit_proj.py:370


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def utm_params(epsg):
    """(lon0_deg, k0, false_easting, false_northing, a, inv_f) of a WGS84 / UTM zone: EPSG 32601 - 32660 (north) and 32701 - 32760
    (south).  Anything else raises ValueError."""
    if isinstance(epsg, str) and epsg.upper().startswith("EPSG:"):
        epsg = epsg[5:]
    try:
        code = int(epsg)
    except (TypeError, ValueError):
        raise ValueError(f"epsg must be a WGS84 / UTM code 32601-32660 or 32701-32760, got {epsg!r}") from None
    if code != epsg and str(code) != str(epsg).strip():
        raise ValueError(f"epsg must be a WGS84 / UTM code 32601-32660 or 32701-32760, got {epsg!r}")
    if 32601 <= code <= 32660:
        zone, fn = code - 32600, 0.0
    elif 32701 <= code <= 32760:
        zone, fn = code - 32700, 10000000.0
    else:
        raise ValueError(f"epsg must be a WGS84 / UTM code 32601-32660 or 32701-32760, got {epsg!r}")
    return (6.0 * zone - 183.0, 0.9996, 500000.0, fn, WGS84_A, WGS84_INV_F)


def _series(a, inv_f):
    """(n, A, e, alpha[6], beta[6]) of the Krueger series to n^6 (Karney 2011; the coefficients of include/hsr_reproject.h)."""
    f = 1.0 / inv_f
    n = f / (2.0 - f)
    n2, n3, n4, n5, n6 = n * n, n ** 3, n ** 4, n ** 5, n ** 6
    A = a / (1.0 + n) * (1.0 + n2 / 4.0 + n4 / 64.0 + n6 / 256.0)
    alpha = (n / 2 - 2 / 3 * n2 + 5 / 16 * n3 + 41 / 180 * n4 - 127 / 288 * n5 + 7891 / 37800 * n6,
             13 / 48 * n2 - 3 / 5 * n3 + 557 / 1440 * n4 + 281 / 630 * n5 - 1983433 / 1935360 * n6,
             61 / 240 * n3 - 103 / 140 * n4 + 15061 / 26880 * n5 + 167603 / 181440 * n6,
             49561 / 161280 * n4 - 179 / 168 * n5 + 6601661 / 7257600 * n6,
             34729 / 80640 * n5 - 3418889 / 1995840 * n6,
             212378941 / 319334400 * n6)
    beta = (n / 2 - 2 / 3 * n2 + 37 / 96 * n3 - 1 / 360 * n4 - 81 / 512 * n5 + 96199 / 604800 * n6,
            1 / 48 * n2 + 1 / 15 * n3 - 437 / 1440 * n4 + 46 / 105 * n5 - 1118711 / 3870720 * n6,
            17 / 480 * n3 - 37 / 840 * n4 - 209 / 4480 * n5 + 5569 / 90720 * n6,
            4397 / 161280 * n4 - 11 / 504 * n5 - 830251 / 7257600 * n6,
            4583 / 161280 * n5 - 108847 / 3991680 * n6,
            20648693 / 638668800 * n6)
    return n, A, math.sqrt(f * (2.0 - f)), alpha, beta


def _taup(tau, e):
    sigma = np.sinh(e * np.arctanh(e * tau / np.sqrt(1.0 + tau * tau)))
    return tau * np.sqrt(1.0 + sigma * sigma) - sigma * np.sqrt(1.0 + tau * tau)


def tm_forward(lon_deg, lat_deg, params):
    """(E, N) of geographic points under ``params`` = (lon0_deg, k0, FE, FN, a, inv_f): the forward Krueger series to n^6 in NumPy
    float64.  Host only; it is what ``utm_target_grid`` needs for the extent.  No antimeridian wrap: lon - lon0 is taken as given."""
    lon0, k0, fe, fn, a, inv_f = (float(v) for v in params)
    _, A, e, alpha, _ = _series(a, inv_f)
    lam = np.radians(np.asarray(lon_deg, dtype=np.float64) - lon0)
    tau = np.tan(np.radians(np.asarray(lat_deg, dtype=np.float64)))
    taup = _taup(tau, e)
    xip = np.arctan2(taup, np.cos(lam))
    etap = np.arcsinh(np.sin(lam) / np.sqrt(taup * taup + np.cos(lam) ** 2))
    xi, eta = xip, etap
    for j, aj in enumerate(alpha, start=1):
        xi = xi + aj * np.sin(2 * j * xip) * np.cosh(2 * j * etap)
        eta = eta + aj * np.cos(2 * j * xip) * np.sinh(2 * j * etap)
    return fe + k0 * A * eta, fn + k0 * A * xi


def tm_inverse(easting, northing, params):
    """(lon_deg, lat_deg) of projected points: steps 2 - 4 of ``hsr_reproject_coords`` (include/hsr_reproject.h) in NumPy float64.
    Host only."""
    lon0, k0, fe, fn, a, inv_f = (float(v) for v in params)
    _, A, e, _, beta = _series(a, inv_f)
    e2m = 1.0 - e * e
    xi = (np.asarray(northing, dtype=np.float64) - fn) / (k0 * A)
    eta = (np.asarray(easting, dtype=np.float64) - fe) / (k0 * A)
    xip, etap = xi, eta
    for j, bj in enumerate(beta, start=1):
        xip = xip - bj * np.sin(2 * j * xi) * np.cosh(2 * j * eta)
        etap = etap - bj * np.cos(2 * j * xi) * np.sinh(2 * j * eta)
    taup = np.sin(xip) / np.sqrt(np.sinh(etap) ** 2 + np.cos(xip) ** 2)
    lam = np.arctan2(np.sinh(etap), np.cos(xip))
    tau = taup
    for _ in range(3):
        ti = _taup(tau, e)
        tau = tau + (taup - ti) / np.sqrt(1.0 + ti * ti) * (1.0 + e2m * tau * tau) / (e2m * np.sqrt(1.0 + tau * tau))
    return lon0 + np.degrees(lam), np.degrees(np.arctan(tau))


def _north_up(gt, what):
    g = tuple(float(v) for v in gt)
    if len(g) != 6:
        raise ValueError(f"{what} must be GDAL's six numbers (x0, dx, 0, y0, 0, -dy), got {gt!r}")
    if g[2] != 0.0 or g[4] != 0.0:
        raise ValueError(f"{what} has rotation terms {g[2]!r}, {g[4]!r}: only north-up rasters are taken")
    if not (g[1] > 0.0 and g[5] < 0.0 and all(math.isfinite(v) for v in g)):
        raise ValueError(f"{what} must be finite with dx > 0 and dy < 0 (north-up), got {gt!r}")
    return g


def _bounds(gt, shape):
    rows, cols = int(shape[-2]), int(shape[-1])
    if rows < 1 or cols < 1:
        raise ValueError(f"a raster needs at least one cell, got {(rows, cols)}")
    return gt[0], gt[3] + gt[5] * rows, gt[0] + gt[1] * cols, gt[3]            # left, bottom, right, top


def utm_target_grid(src_geotransform, src_shape, epsg, s2_geotransform, s2_shape, res=60.0):
    """The output extent on the Sentinel-2 lattice, as emit_proj.py derives it (``_bounds_to_out_crs`` :309-323, ``_intersect``
    :325-331, ``_compute_te`` :354-382): the source's four corners forward-transformed into the UTM zone ``epsg``, their bounding
    box intersected with the S2 extent, and the result snapped INWARD to the lattice of step ``res`` anchored at the S2 origin
    (with the reference's eps = 1e-9 cells, so an extent already on the lattice stays).  ``*_shape`` are (rows, cols) or
    (bands, rows, cols).  Raises ValueError when the extents do not overlap (touching is no overlap) or the snapped extent is
    empty.  -> (left, bottom, right, top, rows, cols)."""
    sg, tg = _north_up(src_geotransform, "src_geotransform"), _north_up(s2_geotransform, "s2_geotransform")
    step = float(res)
    if not (step > 0.0 and math.isfinite(step)):
        raise ValueError(f"res must be > 0, got {res!r}")
    l, b, r, t = _bounds(sg, src_shape)
    X, Y = tm_forward([l, l, r, r], [b, t, b, t], utm_params(epsg))
    src_te = (float(np.min(X)), float(np.min(Y)), float(np.max(X)), float(np.max(Y)))
    s2_te = _bounds(tg, s2_shape)
    il, ib, ir, it = max(src_te[0], s2_te[0]), max(src_te[1], s2_te[1]), min(src_te[2], s2_te[2]), min(src_te[3], s2_te[3])
    if ir <= il or it <= ib:
        raise ValueError("no overlap between the source's bounds and the S2 extent in the output CRS")
    x0, y0 = tg[0], tg[3]
    c0, c1 = math.ceil((il - x0) / step - _EPS), math.floor((ir - x0) / step + _EPS)
    r0, r1 = math.ceil((y0 - it) / step - _EPS), math.floor((y0 - ib) / step + _EPS)
    left, right, top, bottom = x0 + c0 * step, x0 + c1 * step, y0 - r0 * step, y0 - r1 * step
    if right <= left or top <= bottom:
        raise ValueError(f"the snapped extent is empty: {(left, bottom, right, top)}")
    return (left, bottom, right, top, r1 - r0, c1 - c0)


def _grid_cells(grid):
    left, bottom, right, top, rows, cols = grid
    rows, cols = int(rows), int(cols)
    if rows < 1 or cols < 1 or not (right > left and top > bottom):
        raise ValueError(f"grid must be (left, bottom, right, top, rows, cols) with a positive extent, got {grid!r}")
    return (float(left), float(top), (float(right) - float(left)) / cols, (float(top) - float(bottom)) / rows, rows, cols)


def reproject_coords(grid, epsg, src_geotransform, *, device=None, out=None):
    """The device (rows, cols, 2) float64 field (sy, sx): for every cell centre of ``grid`` = (left, bottom, right, top, rows, cols)
    in the UTM zone ``epsg`` the fractional row / column index in the geographic raster of ``src_geotransform``.  One launch on the
    current stream, no host synchronisation."""
    sg = _north_up(src_geotransform, "src_geotransform")
    return eng.reproject_coords(_grid_cells(grid), utm_params(epsg), (sg[0], sg[1], sg[3], sg[5]), device=device, out=out)


def remap_scene(scene, coords, *, nodata=None, fill=-9999.0, rule="renorm", out=None, max_footprint=1.5):
    """out[b, y, x] = Keys cubic of ``scene[b]`` at (sy, sx) = ``coords[y, x]``: ``scene`` (bands, rows, cols) float32 and ``coords``
    (h, w, 2) float64 on the device, ANY field.  A coordinate outside the scene, NaN or infinite gives ``fill``.  A sample is valid
    when it is finite and not ``nodata``; ``rule="strict"`` fills a pixel with an invalid tap (``warp_scene``'s rule), ``"renorm"``
    renormalises the valid taps when the nearest source pixel is valid - what a quality-masked scene needs.  ``max_footprint``:
    the field's bound in source pixels per output pixel, which sizes the staged footprint; a steeper field still warps correctly.
    -> (out (bands, h, w) float32, counts): counts is a device (2,) int64, [0] pixels outside the scene, [1] (band, pixel) samples
    inside it that the sample rule filled.  One launch on the current stream, no host synchronisation."""
    if rule not in _RULES:
        raise ValueError(f"rule must be 'strict' or 'renorm', got {rule!r}")
    if not float(max_footprint) >= 0.0:
        raise ValueError(f"max_footprint must be >= 0, got {max_footprint!r}")
    if not (_is_torch(scene) and _is_torch(coords)):
        raise ValueError("scene and coords must be GPU tensors")
    o, counts, _ = eng.reproject_warp(scene, coords, fill, _RULES[rule], max_footprint, nodata, out)
    return o, counts


def reproject_scene(scene, src_geotransform, *, epsg, s2_geotransform, s2_shape, res=60.0, nodata=-9999.0, fill=-9999.0,
                    rule="renorm", coords=None, out=None):
    """``utm_target_grid`` -> ``reproject_coords`` -> ``remap_scene``: an ``ortho_scene`` result (bands, rows, cols) float32 on the
    device with its geographic ``src_geotransform`` onto the lattice of the S2 raster (``s2_geotransform``, ``s2_shape``) in the
    UTM zone ``epsg`` at ``res`` metres - the reference's ``gdalwarp -r cubic -tr res res -te <snapped>`` (emit_proj.py:876-940).
    -> ReprojectOutput(scene (bands, h, w) float32, geotransform of it, grid (left, bottom, right, top, rows, cols), counts,
    coords).  ``scene`` goes into ``coregister_scene``, ``find_valid_paired_tiles`` or ``fuse_scene`` unchanged.  ``coords=`` (the
    ``coords`` of an earlier result on the same two grids) skips the first launch: the loc / obs case.  Two launches on the current
    stream and no host synchronisation."""
    if rule not in _RULES:
        raise ValueError(f"rule must be 'strict' or 'renorm', got {rule!r}")
    if not (_is_torch(scene) and scene.dim() == 3):
        raise ValueError("scene must be a (bands, rows, cols) GPU tensor")
    sg = _north_up(src_geotransform, "src_geotransform")
    grid = utm_target_grid(sg, scene.shape, epsg, s2_geotransform, s2_shape, res)
    left, _, _, top, rows, cols = grid
    if coords is None:
        coords = reproject_coords(grid, epsg, sg, device=scene.device)
    elif tuple(coords.shape) != (rows, cols, 2):
        raise ValueError(f"coords must be {(rows, cols, 2)} for this grid, got {tuple(coords.shape)}")
    # source pixels per output pixel, from below: a degree of latitude is at least pi a (1 - e^2) / 180 metres long and a degree of
    # longitude at least pi a cos(lat) / 180, at the source's latitude furthest from the equator
    _, south, _, north = _bounds(sg, scene.shape)
    e2 = (2.0 - 1.0 / WGS84_INV_F) / WGS84_INV_F
    cos_lat = max(math.cos(math.radians(min(max(abs(south), abs(north)), 90.0))), 1e-6)
    metres = math.pi * WGS84_A / 180.0
    footprint = _FOOTPRINT_SLACK * float(res) / min(sg[1] * metres * cos_lat, -sg[5] * metres * (1.0 - e2))
    o, counts = remap_scene(scene, coords, nodata=nodata, fill=fill, rule=rule, out=out, max_footprint=footprint)
    return ReprojectOutput(o, (left, float(res), 0.0, top, 0.0, -float(res)), grid, counts, coords)
