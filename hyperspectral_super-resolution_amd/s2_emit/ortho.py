"""EMIT swath -> orthorectified scene on the device: the geometry-lookup-table gather with masks.

An EMIT L2A granule is a swath (downtrack, crosstrack, 285) with a geometry lookup table (``glt_x``, ``glt_y``: for every map
cell the ONE-based swath column and row, 0 = no data), a per-pixel quality mask and a bit-packed per-band mask.  The reference
turns it into a scene with NumPy: ``EMIT_data/emit_tools.py`` ``apply_glt`` (:153-181) under ``ortho_xr`` (:184-268), after
``emit_xarray`` (:115-119) has written -9999 into the swath where ``quality_mask`` (:271-298) is 1 or a bit of ``band_mask``
(:301-321) is set; ``EMIT_data/emit_proj.py`` ``nc_to_envi`` builds the same table (:683-687), drops the entries that leave the
swath (:691-717) and gathers 32 bands at a time (:947-987).

Here that is ``hsr_ortho_glt`` (csrc/hsr_ortho.hip, contract in include/hsr.h): ONE launch that fills, indexes, masks and - for
``layout="bsq"`` - transposes, writing every output byte once.  ``apply_glt`` has the reference's name and signature;
``ortho_scene`` adds the masks, a window of the GLT grid and the band-sequential layout that ``s2_emit.scenes`` takes.

What the result is NOT: it lies on the GLT's own grid (EMIT's geographic grid).  The reference then runs ``gdalwarp -r cubic``
onto the Sentinel-2 UTM grid (emit_proj.py:876-940): that stage is ``reproject_scene`` (s2_emit/reproject.py), which takes this
scene and its geotransform; a caller who builds a lookup table for the S2 60 m grid itself lands there directly with the same call.  Reading the netCDF is left to the caller too.
"""
from __future__ import annotations

import operator
from collections import namedtuple

import numpy as np

from . import _native as nat
from ._engine import _ptr, _stream
from .pairs import _dtype_name
from .ridge import _is_torch

OrthoOutput = namedtuple("OrthoOutput", "scene dropped window")
MAX_BANDS = 512                        # hsr_ortho_glt's band limit (the LDS tile of its bsq transposition)
_LAYOUTS = {"bip": 0, "bsq": 1}
_I32_MIN, _I32_MAX = -(1 << 31), (1 << 31) - 1
_INT_DTYPES = ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64")
_OrthoPlan = namedtuple("_OrthoPlan", "rows cols bands squeeze glt_h glt_w window layout bmask_bytes out_shape fill masked nodata")


def _shape_dtype(x, what: str):
    if not hasattr(x, "shape") or not hasattr(x, "dtype"):
        raise ValueError(f"{what}: expected an array or tensor, got {type(x).__name__}")
    return tuple(int(n) for n in x.shape), _dtype_name(x)


def _i32(v, what: str) -> int:
    if isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{what}={v!r}: must be an integer")
    try:
        i = operator.index(v)
    except TypeError:
        raise ValueError(f"{what}={v!r}: must be an integer") from None
    if not _I32_MIN <= i <= _I32_MAX:
        raise ValueError(f"{what}={i}: outside int32")
    return i


def _plan_ortho(swath, glt, qmask=None, band_mask=None, window=None, layout="bsq", fill_value=-9999.0, masked_value=-9999.0,
                glt_nodata=0, out=None) -> _OrthoPlan:
    """Every check of ``ortho_scene`` that needs no GPU (shapes and dtypes only; no value is read)."""
    sshape, sdt = _shape_dtype(swath, "swath")
    if len(sshape) not in (2, 3) or min(sshape) < 1:
        raise ValueError(f"swath: expected a non-empty (rows, cols, bands) or (rows, cols) array, got shape {sshape}")
    if sdt == "bool" or not (sdt.startswith("float") or sdt in _INT_DTYPES or sdt == "bfloat16"):
        raise ValueError(f"swath is {sdt}: must be a real numeric dtype (cast to float32)")
    rows, cols = sshape[:2]
    bands = sshape[2] if len(sshape) == 3 else 1
    if bands > MAX_BANDS:
        raise ValueError(f"swath has {bands} bands: at most {MAX_BANDS}")
    if rows * cols > _I32_MAX:
        raise ValueError(f"swath of {rows} x {cols} pixels: at most 2^31 - 1")
    gshape, gdt = _shape_dtype(glt, "glt")
    if len(gshape) != 3 or gshape[2] != 2 or min(gshape) < 1:
        raise ValueError(f"glt: expected a non-empty (H, W, 2) table (glt_from_xy), got shape {gshape}")
    if gdt not in _INT_DTYPES:
        raise ValueError(f"glt is {gdt}: must be an integer dtype (glt_from_xy builds it from the netCDF's float arrays)")
    glt_h, glt_w = gshape[:2]
    if window is None:
        win = (0, 0, glt_h, glt_w)
    else:
        try:
            win = tuple(_i32(v, "window") for v in window)
        except TypeError:
            raise ValueError(f"window={window!r}: (row_off, col_off, height, width) on the GLT grid") from None
        if len(win) != 4:
            raise ValueError(f"window={window!r}: (row_off, col_off, height, width) on the GLT grid")
        r0, c0, h, w = win
        if r0 < 0 or c0 < 0 or h < 1 or w < 1 or r0 + h > glt_h or c0 + w > glt_w:
            raise ValueError(f"window={win}: leaves the {glt_h} x {glt_w} GLT grid")
    if win[2] * win[3] > _I32_MAX:
        raise ValueError(f"window of {win[2]} x {win[3]} pixels: at most 2^31 - 1")
    if layout not in _LAYOUTS:
        raise ValueError(f"layout={layout!r}: 'bip' (h, w, bands) or 'bsq' (bands, h, w)")
    if qmask is not None:
        qshape, qdt = _shape_dtype(qmask, "qmask")
        if qshape != (rows, cols):
            raise ValueError(f"qmask has shape {qshape}: the swath is {rows} x {cols}")
        if qdt.startswith("complex"):
            raise ValueError(f"qmask is {qdt}: a numeric array that is compared with 1 (quality_mask's result)")
    bmask_bytes = 0
    if band_mask is not None:
        bshape, bdt = _shape_dtype(band_mask, "band_mask")
        need = (bands + 7) // 8
        if bdt != "uint8" or len(bshape) != 3 or bshape[:2] != (rows, cols):
            raise ValueError(f"band_mask: expected the PACKED uint8 mask ({rows}, {cols}, >= {need}), got {bdt} {bshape}")
        if bshape[2] < need:
            raise ValueError(f"band_mask has {bshape[2]} bytes a pixel: {bands} bands need {need}")
        bmask_bytes = bshape[2]
    try:
        fill, masked = float(fill_value), float(masked_value)
    except (TypeError, ValueError):
        raise ValueError(f"fill_value={fill_value!r}, masked_value={masked_value!r}: must be numbers") from None
    nodata = _i32(glt_nodata, "glt_nodata")
    out_shape = (win[2], win[3], bands) if layout == "bip" else (bands, win[2], win[3])
    if out is not None:
        oshape, odt = _shape_dtype(out, "out")
        if not _is_torch(out) or oshape != out_shape or odt != "float32":
            raise ValueError(f"out: expected a float32 device tensor of shape {out_shape}, got {type(out).__name__} {odt} {oshape}")
        if not out.is_contiguous():
            raise ValueError("out: must be contiguous")
    return _OrthoPlan(rows, cols, bands, len(sshape) == 2, glt_h, glt_w, win, layout, bmask_bytes, out_shape, fill, masked, nodata)


def _from_numpy(a, torch, dtype=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a if a.flags.writeable else a.copy())


def _dev(x, torch, dev):
    return (x if _is_torch(x) else _from_numpy(x, torch)).to(dev)


def _glt_i32(glt, nodata: int, torch, dev):
    """The table as contiguous device int32.  A value outside int32 is out of bounds by definition: it becomes -1 (-2 when -1 is
    the no-data value), which no swath holds."""
    oob = -2 if nodata == -1 else -1
    if not _is_torch(glt):
        g = np.asarray(glt)
        if g.dtype.itemsize > 2 and g.dtype != np.int32:
            big = (g > _I32_MAX) | (g < _I32_MIN) if g.dtype.kind == "i" else g > _I32_MAX
            g = np.where(big, oob, g)
        return _from_numpy(g, torch, np.int32).to(dev)
    if _dtype_name(glt) in ("int8", "int16", "int32", "uint8"):
        return glt.to(dev, torch.int32).contiguous()
    g = glt.to(dev)
    if _dtype_name(glt).startswith("uint"):                   # torch has few operators for wide unsigned types: through int64
        g = g.to(torch.int64)                                 # uint64 beyond 2^63 wraps negative: still outside int32
    big = (g > _I32_MAX) | (g < _I32_MIN)
    return torch.where(big, torch.full_like(g, oob), g).to(torch.int32).contiguous()


def _qmask_u8(qmask, torch, dev):
    """uint8 as it is (the kernel tests == 1); any other dtype as the uint8 of ``qmask == 1``."""
    q = _dev(qmask, torch, dev)
    return (q if q.dtype == torch.uint8 else (q == 1).to(torch.uint8)).contiguous()


def ortho_scene(swath, glt, *, qmask=None, band_mask=None, window=None, layout="bsq", fill_value=-9999.0, masked_value=-9999.0,
                glt_nodata=0, out=None) -> OrthoOutput:
    """A swath (rows, cols, bands) - float32, or cast to it; a device tensor or an array (copied once) - and its lookup table
    ``glt`` (H, W, 2) of ONE-based (column, row) entries (``glt_from_xy``) -> ``OrthoOutput(scene, dropped, window)``.

    scene    float32 on the device: ``layout="bsq"`` (bands, h, w), what ``find_valid_paired_tiles`` / ``fuse_scene`` take, or
             ``"bip"`` (h, w, bands), what the reference's ``apply_glt`` returns; the same bits.  A cell whose column or row is
             ``glt_nodata`` holds ``fill_value`` in every band; so does a cell that points outside the swath (``nc_to_envi``'s
             rule, emit_proj.py:691-717 - ``apply_glt`` alone would raise or wrap), which is also counted in ``dropped``; every
             other cell holds the bits of its swath pixel, except ``masked_value`` where ``qmask`` (rows, cols; compared with 1
             exactly as emit_tools.py:117) is 1, or where the band's bit of ``band_mask`` (rows, cols, >= ceil(bands / 8)) uint8,
             packed, ``np.unpackbits`` order (emit_tools.py:315-319) is set.  ``masked_value`` is the reference's -9999 literal, a
             parameter apart from ``fill_value``.
    dropped  a device int64 scalar: the cells that point outside the swath.
    window   (row_off, col_off, height, width) on the GLT grid, None = all of it: only that part is ever produced.
    out      optional preallocated float32 device tensor of the scene's shape.

    One launch on the current stream, every output byte written once, no host synchronisation.  The scene lies on the GLT's own
    grid, NOT on the Sentinel-2 UTM grid: ``reproject_scene`` is the reference's cubic warp onto it (emit_proj.py:876-940)."""
    plan = _plan_ortho(swath, glt, qmask, band_mask, window, layout, fill_value, masked_value, glt_nodata, out)
    torch = nat.require_gpu()
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    if _is_torch(swath):
        S = swath.to(dev, torch.float32).contiguous()
    else:
        S = _from_numpy(swath, torch, np.float32).to(dev)                  # NumPy's own cast, as its assignment
    G = _glt_i32(glt, plan.nodata, torch, dev)
    Q = None if qmask is None else _qmask_u8(qmask, torch, dev)
    B = None if band_mask is None else _dev(band_mask, torch, dev).contiguous()
    scene = out if out is not None else torch.empty(plan.out_shape, dtype=torch.float32, device=dev)
    dropped = torch.empty((), dtype=torch.int64, device=dev)
    r0, c0, h, w = plan.window
    nat.check(lib.hsr_ortho_glt(_ptr(S), plan.rows, plan.cols, plan.bands, _ptr(G), plan.glt_h, plan.glt_w, plan.nodata, r0, c0, h, w,
                                _ptr(Q), _ptr(B), plan.bmask_bytes, plan.fill, plan.masked, _LAYOUTS[plan.layout], _ptr(scene),
                                _ptr(dropped), _stream(torch, scene)), "hsr_ortho_glt")
    return OrthoOutput(scene, dropped, plan.window)


def apply_glt(ds_array, glt_array, fill_value=-9999, GLT_NODATA_VALUE=0):
    """The reference's ``apply_glt`` (emit_tools.py:153-181) on the GPU: ds_array (rows, cols, bands) or (rows, cols) - one band -
    and glt_array (H, W, 2) of any integer dtype -> (H, W, bands) float32 with the bits of the reference's result.  NumPy in
    gives NumPy out, a tensor in gives a device tensor.  A non-float32 input is cast to float32 first, which is what NumPy's
    assignment into the float32 output does.  One departure: an entry that points outside the swath gives ``fill_value``
    (``ortho_scene``'s dropped rule) where the reference raises an IndexError or wraps a negative index.  The result lies on
    the GLT's grid, not on the Sentinel-2 UTM grid (``reproject_scene`` takes it there)."""
    res = ortho_scene(ds_array, glt_array, layout="bip", fill_value=fill_value, glt_nodata=GLT_NODATA_VALUE)
    return res.scene if _is_torch(ds_array) else res.scene.cpu().numpy()


def glt_from_xy(glt_x, glt_y, nodata=0):
    """The (H, W, 2) int32 lookup table from the netCDF's two arrays (location/glt_x, location/glt_y: floats with NaN, or
    integers): NaN -> ``nodata``, stacked column first, as emit_tools.py:199-201 and emit_proj.py:683-687 build it.  Arrays give
    an array, tensors a tensor on their device."""
    nodata = _i32(nodata, "nodata")
    if tuple(glt_x.shape) != tuple(glt_y.shape) or len(glt_x.shape) != 2:
        raise ValueError(f"glt_x {tuple(glt_x.shape)} and glt_y {tuple(glt_y.shape)}: two (H, W) arrays of one shape")
    if _is_torch(glt_x) != _is_torch(glt_y):
        raise ValueError("glt_x and glt_y: both arrays or both tensors")
    if _is_torch(glt_x):
        import torch
        g = torch.stack([glt_x, glt_y], dim=-1)
        if g.is_floating_point():
            g = torch.nan_to_num(g, nan=float(nodata), posinf=torch.finfo(g.dtype).max, neginf=torch.finfo(g.dtype).min)
        return g.to(torch.int32)
    with np.errstate(invalid="ignore"):
        return np.nan_to_num(np.stack([np.asarray(glt_x), np.asarray(glt_y)], axis=-1), nan=nodata).astype(np.int32)


def quality_mask(mask_cube, quality_bands):
    """The reference's ``quality_mask`` rule (emit_tools.py:292-297) on the mask cube (rows, cols, flags) of an L2A mask file
    instead of its path: bands 5 or 6 (data, not flags) raise ``AttributeError``; otherwise the sum over the selected flags,
    clipped to 1.  Arrays give an array, tensors a tensor."""
    if any(x in quality_bands for x in [5, 6]):
        raise AttributeError("Selected flags include a data band (5 or 6) not just flag bands")
    if _is_torch(mask_cube):
        return mask_cube[:, :, list(quality_bands)].sum(dim=-1).clamp(max=1)
    q = np.sum(np.asarray(mask_cube)[:, :, quality_bands], axis=-1)
    q[q > 1] = 1
    return q
