"""Adjacent EMIT scenes of one orbit onto one grid, on the device.

An EMIT scene is about 75 km of an orbit and a Sentinel-2 granule 110 km on a side: a granule is normally covered by two or three
consecutive scenes.  The reference merges them with ``merge_emit`` / ``is_adjacent`` (``EMIT_data/emit_tools.py``:622-704): every
granule is orthorectified and the results go to ``rioxarray.merge.merge_arrays(..., nodata=-9999)`` - rasterio's "first" rule on a
common grid.  Here (definition: include/hsr_merge.h; kernels: csrc/hsr_merge.hip):

    merge_grid     the common grid of N north-up geotransforms and every source's INTEGER offset on it (nearest-cell placement,
                   nothing is resampled; the sub-pixel remainders are returned); host only, float64.
    merge_scenes   the "first" rule over N orthorectified scenes, PER ELEMENT: a band that one scene's mask blanked is filled from
                   the next scene in the overlap.
    ortho_merge    N swaths with their lookup tables straight onto the merged grid in ONE launch; bit-equal to ``ortho_scene`` per
                   source followed by ``merge_scenes``, without the N intermediate scenes.
    merge_emit, is_adjacent   the reference's names.

rasterio's own window rounding is not claimed (include/hsr_merge.h says why); on aligned grids every rounding gives these offsets.
The geotransform that ``ortho_merge`` returns goes to ``reproject_scene`` unchanged.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from . import _native as nat
from ._engine import _ptr, _stream
from .ortho import (MAX_BANDS, _LAYOUTS, _dev, _from_numpy, _glt_i32, _i32, _plan_ortho, _qmask_u8, _shape_dtype)
from .ridge import _is_torch

MergeGrid = namedtuple("MergeGrid", "geotransform shape offsets residuals")
MergeOutput = namedtuple("MergeOutput", "scene source")
OrthoMergeOutput = namedtuple("OrthoMergeOutput", "scene dropped source geotransform")
MAX_SOURCES = nat.HSR_MERGE_MAX_SOURCES
NO_SOURCE = nat.HSR_MERGE_NO_SOURCE
_I32_MAX = (1 << 31) - 1
_MergePlan = namedtuple("_MergePlan", "n bands layout sizes offsets shape out_shape nodata nan source")
_OrthoMergePlan = namedtuple("_OrthoMergePlan", "n bands layout plans offsets shape out_shape nodata masked glt_nodata source geotransform")


def merge_grid(geotransforms, shapes, bounds=None) -> MergeGrid:
    """N GDAL geotransforms ``(x0, dx, 0, y0, 0, dy)`` and shapes ``(h, w)`` -> ``MergeGrid(geotransform, shape, offsets,
    residuals)`` under THE GRID of include/hsr_merge.h (``hsr_merge_grid``; host only, float64, no GPU needed).

    The grid has source 0's pixel size.  Without ``bounds`` it is the union of the sources; with ``bounds=(left, bottom, right,
    top)`` its origin is (left, top) and its width ``max(1, floor((right - left) / dx + 0.5))``, the height alike.  ``offsets[k]``
    = (off_y, off_x) places source k at the nearest cell, ``off_x = floor((x0_k - X0) / dx + 0.5)``; ``residuals[k]`` = (res_y,
    res_x) is what that rounding drops, in pixels.  Rotation terms, non-finite terms and a pixel size that differs from source
    0's by more than 0.01 pixel over the source's extent are refused (``HsrError``)."""
    try:
        gts = [[float(v) for v in g] for g in geotransforms]
        shp = [[_i32(v, "shapes") for v in s] for s in shapes]
    except TypeError:
        raise ValueError("merge_grid: geotransforms is a sequence of 6-tuples and shapes one of (h, w)") from None
    n = len(gts)
    if n != len(shp) or any(len(g) != 6 for g in gts) or any(len(s) != 2 for s in shp):
        raise ValueError(f"merge_grid: {n} geotransforms of 6 terms and {len(shp)} shapes (h, w): one pair per source")
    if not 1 <= n <= MAX_SOURCES:
        raise ValueError(f"merge_grid: {n} sources, 1 to {MAX_SOURCES}")
    b = None
    if bounds is not None:
        b = [float(v) for v in bounds]
        if len(b) != 4:
            raise ValueError(f"bounds={bounds!r}: (left, bottom, right, top)")
    lib = nat.load()
    g_in = (C.c_double * (6 * n))(*[v for g in gts for v in g])
    s_in = (C.c_int32 * (2 * n))(*[v for s in shp for v in s])
    gt, shape, off, res = (C.c_double * 6)(), (C.c_int32 * 2)(), (C.c_int32 * (2 * n))(), (C.c_double * (2 * n))()
    nat.check(lib.hsr_merge_grid(g_in, s_in, n, None if b is None else (C.c_double * 4)(*b), gt, shape, off, res), "hsr_merge_grid")
    return MergeGrid(tuple(gt), (int(shape[0]), int(shape[1])), tuple((int(off[2 * k]), int(off[2 * k + 1])) for k in range(n)),
                     tuple((float(res[2 * k]), float(res[2 * k + 1])) for k in range(n)))


def _placement(n, sizes, offsets, grid, shape, what):
    """-> (offsets, (H, W), geotransform or None) from either a MergeGrid or explicit offsets / shape."""
    if grid is not None:
        if offsets is not None or shape is not None:
            raise ValueError(f"{what}: give grid= (a MergeGrid) or offsets= / shape=, not both")
        if not isinstance(grid, MergeGrid) or len(grid.offsets) != n:
            raise ValueError(f"{what}: grid must be the MergeGrid of these {n} sources")
        offsets, shape, gt = grid.offsets, grid.shape, tuple(grid.geotransform)
    else:
        gt = None
        if offsets is None:
            offsets = [(0, 0)] * n
    try:
        offs = tuple((_i32(o[0], "offsets"), _i32(o[1], "offsets")) for o in offsets)
    except (TypeError, IndexError):
        raise ValueError(f"{what}: offsets is one (off_y, off_x) per source") from None
    if len(offs) != n or any(len(o) != 2 for o in offsets):
        raise ValueError(f"{what}: {len(offs)} offsets for {n} sources; each is (off_y, off_x)")
    if shape is None:
        shape = (max(o[0] + s[0] for o, s in zip(offs, sizes)), max(o[1] + s[1] for o, s in zip(offs, sizes)))
        if min(shape) < 1:
            raise ValueError(f"{what}: every source lies above or left of the origin; give shape=")
    try:
        H, W = (_i32(v, "shape") for v in shape)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: shape={shape!r}: (H, W)") from None
    if H < 1 or W < 1:
        raise ValueError(f"{what}: shape={shape!r}: (H, W), both at least 1")
    if H * W > _I32_MAX:
        raise ValueError(f"{what}: an output of {H} x {W} pixels: at most 2^31 - 1")
    return offs, (H, W), gt


def _number(v, what):
    try:
        return float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what}={v!r}: must be a number") from None


def _check_out(out, out_shape):
    if out is None:
        return
    oshape, odt = _shape_dtype(out, "out")
    if not _is_torch(out) or oshape != out_shape or odt != "float32":
        raise ValueError(f"out: expected a float32 device tensor of shape {out_shape}, got {type(out).__name__} {odt} {oshape}")
    if not out.is_contiguous():
        raise ValueError("out: must be contiguous")


def _sources(seq, what):
    try:
        seq = list(seq)
    except TypeError:
        raise ValueError(f"{what}: expected a sequence of arrays or tensors") from None
    if not 1 <= len(seq) <= MAX_SOURCES:
        raise ValueError(f"{what}: {len(seq)} sources, 1 to {MAX_SOURCES}")
    return seq


def _plan_merge(scenes, offsets=None, grid=None, layout="bsq", nodata=-9999.0, nan_is_nodata=False, shape=None, source=False,
                out=None) -> _MergePlan:
    """Every check of ``merge_scenes`` that needs no GPU (shapes and dtypes only; no value is read)."""
    scenes = _sources(scenes, "scenes")
    if layout not in _LAYOUTS:
        raise ValueError(f"layout={layout!r}: 'bip' (h, w, bands) or 'bsq' (bands, h, w)")
    sizes, bands = [], None
    for k, s in enumerate(scenes):
        sshape, sdt = _shape_dtype(s, f"scenes[{k}]")
        if len(sshape) != 3 or min(sshape) < 1:
            raise ValueError(f"scenes[{k}]: expected a non-empty 3-D scene in layout {layout!r}, got shape {sshape}")
        if sdt == "bool" or sdt.startswith("complex"):
            raise ValueError(f"scenes[{k}] is {sdt}: must be a real numeric dtype (cast to float32)")
        h, w, b = sshape if layout == "bip" else (sshape[1], sshape[2], sshape[0])
        if bands is None:
            bands = b
        if b != bands:
            raise ValueError(f"scenes[{k}] has {b} bands, scenes[0] has {bands}: the sources must agree")
        if h * w > _I32_MAX:
            raise ValueError(f"scenes[{k}] has {h} x {w} pixels: at most 2^31 - 1")
        sizes.append((h, w))
    if bands > MAX_BANDS:
        raise ValueError(f"scenes have {bands} bands: at most {MAX_BANDS}")
    offs, (H, W), _ = _placement(len(scenes), sizes, offsets, grid, shape, "merge_scenes")
    out_shape = (H, W, bands) if layout == "bip" else (bands, H, W)
    _check_out(out, out_shape)
    return _MergePlan(len(scenes), bands, layout, tuple(sizes), offs, (H, W), out_shape, _number(nodata, "nodata"), bool(nan_is_nodata),
                      bool(source))


def merge_scenes(scenes, offsets=None, *, grid=None, layout="bsq", nodata=-9999.0, nan_is_nodata=False, shape=None, source=False,
                 out=None) -> MergeOutput:
    """N orthorectified scenes - float32, or cast to it; device tensors or arrays (copied once); ``layout="bsq"`` (bands, h, w) or
    ``"bip"`` (h, w, bands) - onto one grid under rasterio's "first" rule -> ``MergeOutput(scene, source)``.

    Placement: ``grid=`` the ``MergeGrid`` of these sources (``merge_grid``), or ``offsets=`` one (off_y, off_x) per source (negative
    ones allowed; default all (0, 0)) with ``shape=`` (H, W) of the output (default: the extent the sources reach from the origin).
    A source wholly outside the output contributes nothing.

    The rule is PER ELEMENT (include/hsr_merge.h): an output element starts as ``nodata``; the first source, in the order given,
    that covers the cell and whose value there is not empty supplies its bits - NaN payloads, -0.0, denormals as they are.  A value
    is empty when it ``== nodata`` in float32; with ``nan_is_nodata`` a NaN is empty too (off by default, as in the reference,
    which tests equality with -9999 only).  So a band that one scene's band mask blanked, or a cell that its quality mask blanked,
    is filled from the next scene in the overlap.
    source   True: also the uint8 plane (H, W) of the first source that supplies ANY band of the cell, 255 where none does.
    out      optional preallocated float32 device tensor of the output's shape.

    One streaming launch on the current stream (two with ``source``), every output byte written once, no host synchronisation."""
    plan = _plan_merge(scenes, offsets, grid, layout, nodata, nan_is_nodata, shape, source, out)
    torch = nat.require_gpu()
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    held = [s.to(dev, torch.float32).contiguous() if _is_torch(s) else _from_numpy(s, torch, np.float32).to(dev) for s in scenes]
    table = (nat.MergeScene * plan.n)(*[nat.MergeScene(t.data_ptr(), h, w, oy, ox, plan.bands, 0)
                                        for t, (h, w), (oy, ox) in zip(held, plan.sizes, plan.offsets)])
    scene = out if out is not None else torch.empty(plan.out_shape, dtype=torch.float32, device=dev)
    plane = torch.empty(plan.shape, dtype=torch.uint8, device=dev) if plan.source else None
    nat.check(lib.hsr_merge_scenes(table, plan.n, _LAYOUTS[plan.layout], plan.shape[0], plan.shape[1], plan.nodata, int(plan.nan),
                                   _ptr(scene), _ptr(plane), _stream(torch, scene)), "hsr_merge_scenes")
    return MergeOutput(scene, plane)


def _per_source(seq, n, what):
    if seq is None:
        return [None] * n
    seq = list(seq)
    if len(seq) != n:
        raise ValueError(f"{what}: {len(seq)} entries for {n} sources (None where a source has none)")
    return seq


def _plan_ortho_merge(swaths, glts, offsets=None, grid=None, qmasks=None, band_masks=None, layout="bsq", nodata=-9999.0,
                      masked_value=-9999.0, glt_nodata=0, shape=None, source=False, out=None) -> _OrthoMergePlan:
    """Every check of ``ortho_merge`` that needs no GPU: ``_plan_ortho`` per source, then the placement."""
    swaths = _sources(swaths, "swaths")
    n = len(swaths)
    glts, qmasks, band_masks = _per_source(glts, n, "glts"), _per_source(qmasks, n, "qmasks"), _per_source(band_masks, n, "band_masks")
    plans = [_plan_ortho(swaths[k], glts[k], qmasks[k], band_masks[k], None, layout, nodata, masked_value, glt_nodata, None) for k in range(n)]
    bands = plans[0].bands
    for k, p in enumerate(plans):
        if p.bands != bands:
            raise ValueError(f"swaths[{k}] has {p.bands} bands, swaths[0] has {bands}: the sources must agree")
    sizes = [(p.glt_h, p.glt_w) for p in plans]
    offs, (H, W), gt = _placement(n, sizes, offsets, grid, shape, "ortho_merge")
    out_shape = (H, W, bands) if layout == "bip" else (bands, H, W)
    _check_out(out, out_shape)
    return _OrthoMergePlan(n, bands, layout, tuple(plans), offs, (H, W), out_shape, plans[0].fill, plans[0].masked, plans[0].nodata,
                           bool(source), gt)


def ortho_merge(swaths, glts, *, offsets=None, grid=None, qmasks=None, band_masks=None, layout="bsq", nodata=-9999.0,
                masked_value=-9999.0, glt_nodata=0, shape=None, source=False, out=None) -> OrthoMergeOutput:
    """N swaths (rows_k, cols_k, bands) with their lookup tables ``glts[k]`` (H_k, W_k, 2) - and optionally ``qmasks[k]`` /
    ``band_masks[k]``, each None or as ``ortho_scene`` takes them - orthorectified straight onto the merged grid in ONE launch
    -> ``OrthoMergeOutput(scene, dropped, source, geotransform)``.

    Source k's GLT grid sits at ``offsets[k]`` = (off_y, off_x) on the output (or ``grid=`` the ``MergeGrid`` of the GLT grids'
    geotransforms, which also fixes the output's shape).  For every source the value of a cell is exactly ``ortho_scene``'s with
    ``fill_value = nodata`` - the no-data entry, the entry outside the swath (counted in ``dropped[k]``), ``masked_value`` under the
    masks, the swath's bits - and ``merge_scenes``' first rule, per element, runs over those values: the scene is bit-equal to
    ``ortho_scene`` per source followed by ``merge_scenes``, without writing the N intermediate scenes.
    dropped       device int64 (N,): per source, the entries inside the output that point outside the swath.
    source        True: the uint8 plane (H, W) of the first source that supplies any band of the cell, 255 where none does.
    geotransform  the grid's, when ``grid=`` was given (else None): ``reproject_scene`` takes it as it is.

    No host synchronisation; the sources travel in the kernel's arguments, so the call can be captured in a graph."""
    plan = _plan_ortho_merge(swaths, glts, offsets, grid, qmasks, band_masks, layout, nodata, masked_value, glt_nodata, shape, source, out)
    torch = nat.require_gpu()
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    qmasks, band_masks = _per_source(qmasks, plan.n, "qmasks"), _per_source(band_masks, plan.n, "band_masks")
    held, rows = [], []
    for k, p in enumerate(plan.plans):
        sw = swaths[k]
        S = sw.to(dev, torch.float32).contiguous() if _is_torch(sw) else _from_numpy(sw, torch, np.float32).to(dev)
        G = _glt_i32(list(glts)[k], p.nodata, torch, dev)
        Q = None if qmasks[k] is None else _qmask_u8(qmasks[k], torch, dev)
        B = None if band_masks[k] is None else _dev(band_masks[k], torch, dev).contiguous()
        held.append((S, G, Q, B))
        oy, ox = plan.offsets[k]
        rows.append(nat.MergeSwath(S.data_ptr(), G.data_ptr(), None if Q is None else Q.data_ptr(), None if B is None else B.data_ptr(),
                                   p.rows, p.cols, p.glt_h, p.glt_w, oy, ox, p.bmask_bytes, plan.bands))
    table = (nat.MergeSwath * plan.n)(*rows)
    scene = out if out is not None else torch.empty(plan.out_shape, dtype=torch.float32, device=dev)
    dropped = torch.empty((plan.n,), dtype=torch.int64, device=dev)
    plane = torch.empty(plan.shape, dtype=torch.uint8, device=dev) if plan.source else None
    nat.check(lib.hsr_ortho_merge(table, plan.n, plan.glt_nodata, _LAYOUTS[plan.layout], plan.shape[0], plan.shape[1], plan.nodata,
                                  plan.masked, _ptr(scene), _ptr(dropped), _ptr(plane), _stream(torch, scene)), "hsr_ortho_merge")
    return OrthoMergeOutput(scene, dropped, plane, plan.geotransform)


def is_adjacent(scene, same_orbit):
    """The reference's ``is_adjacent`` (emit_tools.py:622-628): True when the scene numbers of the granule names in ``same_orbit`` -
    the last ``_``-separated field in front of the file extension, ``..._001.nc`` - rise by exactly one from each name to the
    next.  ``scene`` is not looked at, as in the reference."""
    numbers = []
    for name in same_orbit:
        stem = name.split(".")[-2]
        numbers.append(int(stem.rsplit("_", 1)[-1]))
    return all(later - earlier == 1 for earlier, later in zip(numbers, numbers[1:]))


def merge_emit(scenes, geotransforms, bounds=None, **kw):
    """The reference's ``merge_emit`` on device scenes: ``merge_grid`` over the scenes' geotransforms (``bounds`` as there: (left,
    bottom, right, top), the reference passes its polygon's), then ``merge_scenes`` with that grid -> ``(MergeOutput, MergeGrid)``.
    ``kw`` goes to ``merge_scenes`` (``layout``, ``nodata`` = -9999 as in the reference, ``nan_is_nodata``, ``source``, ``out``)."""
    layout = kw.get("layout", "bsq")
    if layout not in _LAYOUTS:
        raise ValueError(f"layout={layout!r}: 'bip' (h, w, bands) or 'bsq' (bands, h, w)")
    scenes = _sources(scenes, "scenes")
    shapes = []
    for k, s in enumerate(scenes):
        sshape, _ = _shape_dtype(s, f"scenes[{k}]")
        if len(sshape) != 3:
            raise ValueError(f"scenes[{k}]: expected a 3-D scene in layout {layout!r}, got shape {sshape}")
        shapes.append(sshape[:2] if layout == "bip" else sshape[1:])
    grid = merge_grid(geotransforms, shapes, bounds)
    return merge_scenes(scenes, grid=grid, **kw), grid
