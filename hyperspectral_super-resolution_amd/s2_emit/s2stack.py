"""The Sentinel-2 band planes of a granule to the cropped, model-ready 10 m stack on the device.

The reference makes the S2 scene of its pairs with two functions of ``s2_data/s2_utils.py``: ``download_s2_spectral_stack``
(:505-614) downloads the band rasters and warps them onto the grid of ``blue`` - ``Resampling.nearest`` for the four 10 m bands,
``Resampling.bilinear`` for the 20 m bands, 9 bands when ``nir08`` is missing or has the resolution of ``nir`` (:560-590) - and
``crop_s2_stack_to_te`` (:617-783) cuts the stack to a target extent snapped to the source grid.  Both open rasters with rasterio,
which is absent here and NOT reproduced: ours take the band planes themselves, (H, W) uint16 arrays or device tensors, as
``clouds.py`` takes the SCL plane.  The download and the decoding stay on the host.

    S2_STACK_BANDS      the reference's ``band_order`` (:567-586), value for value: (description, asset key, method);
    s2_crop_window      the window arithmetic of ``crop_s2_stack_to_te`` (:649-696) for a north-up transform, in plain Python;
    assemble_s2_stack   resampling, stacking, crop, the BOA offset and the conversion to reflectance in ONE launch
                        (``hsr_s2_stack``, include/hsr_s2stack.h), and the SCL plane under the same window at 10 m.
Not claimed: GDAL's bits.  The resampling is defined in include/hsr_s2stack.h - pixel-centre aligned, edge clamp, integer weights,
a nodata rule - and tested by equality against that definition.  The S2 bands share one UTM grid: nothing is reprojected.
"""
from __future__ import annotations

import math
import warnings
from collections import namedtuple
from collections.abc import Mapping

import numpy as np

from . import _native as nat
from ._engine import _ptr, _stream
from .pairs import _dtype_name
from .ridge import _is_torch
from .scenes import Window, _int

# s2_utils.py:567-586, value for value: the description written to the GeoTIFF, the asset key, the resampling
S2_STACK_BANDS = (
    ("B02_blue", "blue", "nearest"),
    ("B03_green", "green", "nearest"),
    ("B04_red", "red", "nearest"),
    ("B08_nir", "nir", "nearest"),
    ("B05_rededge1", "rededge1", "bilinear"),
    ("B06_rededge2", "rededge2", "bilinear"),
    ("B07_rededge3", "rededge3", "bilinear"),
    ("B8A_nir08", "nir08", "bilinear"),
    ("B11_swir16", "swir16", "bilinear"),
    ("B12_swir22", "swir22", "bilinear"),
)
_REQUIRED = ("blue", "green", "red", "nir", "rededge1", "rededge2", "rededge3", "swir16", "swir22")      # s2_utils.py:515
_METHODS = {"nearest": nat.HSR_S2_NEAREST, "bilinear": nat.HSR_S2_BILINEAR}
_RULES = {"strict": nat.HSR_S2_STRICT, "renorm": nat.HSR_S2_RENORM}
_DTYPES = {"uint16": nat.HSR_S2_U16, "float32": nat.HSR_S2_F32}

S2StackOutput = namedtuple("S2StackOutput", "stack names window scl invalid")


def s2_crop_window(te, geotransform, shape, *, snap: bool = True, cover: bool = True):
    """The window of ``crop_s2_stack_to_te`` (s2_utils.py:649-696) on a north-up raster, in plain Python: ``te`` is
    (left, bottom, right, top), ``geotransform`` GDAL's six numbers (x0, dx, 0, y0, 0, -dy), ``shape`` (..., rows, cols).

    1. ``snap``: every edge goes to the nearest grid line, half up - ``snap_x`` / ``snap_y`` with ``floor(v + 0.5)`` (:655-666);
       ``ValueError("Invalid TE after snapping to grid ...")`` when nothing is left (:668-669).
    2. ``from_bounds`` (:675): the fractional window of the extent.
    3. ``cover``: floor of the start and ceil of the end with the reference's 1e-9 (:677-683); else ``round`` of offset and size
       (:685-690).
    4. The intersection with the raster (:692-693); ``ValueError("Overlap window is empty ...")`` when nothing is left (:695-696).

    -> ``(Window(col_off, row_off, width, height), geotransform of the crop, info)`` with info the reference's ``te``,
    ``snapped_te`` and ``window`` entries."""
    from .reproject import _north_up
    left, bottom, right, top = (float(v) for v in te)
    g = _north_up(geotransform, "geotransform")
    rows, cols = int(shape[-2]), int(shape[-1])
    if rows < 1 or cols < 1:
        raise ValueError(f"a raster needs at least one cell, got {(rows, cols)}")
    x0, dx, y0, dy = g[0], abs(g[1]), g[3], abs(g[5])
    snapped = None
    if snap:
        def snap_x(x):
            return x0 + math.floor(((x - x0) / dx) + 0.5) * dx

        def snap_y(y):
            return y0 - math.floor(((y0 - y) / dy) + 0.5) * dy

        left_s, right_s, top_s, bottom_s = snap_x(left), snap_x(right), snap_y(top), snap_y(bottom)
        if right_s <= left_s or top_s <= bottom_s:
            raise ValueError(f"Invalid TE after snapping to grid: {(left_s, bottom_s, right_s, top_s)}")
        snapped = {"left": left_s, "bottom": bottom_s, "right": right_s, "top": top_s}
        left, bottom, right, top = left_s, bottom_s, right_s, top_s
    # from_bounds for a north-up transform: the inverse transform of the corners
    col_off, row_off = (left - x0) / dx, (y0 - top) / dy
    width, height = (right - x0) / dx - col_off, (y0 - bottom) / dy - row_off
    if cover:
        eps = 1e-9
        c0, r0 = int(math.floor(col_off + eps)), int(math.floor(row_off + eps))
        c1, r1 = int(math.ceil(col_off + width - eps)), int(math.ceil(row_off + height - eps))
    else:
        c0, r0 = int(round(col_off)), int(round(row_off))
        c1, r1 = c0 + int(round(width)), r0 + int(round(height))
    c0c, r0c, c1c, r1c = max(c0, 0), max(r0, 0), min(c1, cols), min(r1, rows)
    if c1c - c0c <= 0 or r1c - r0c <= 0:
        raise ValueError("Overlap window is empty after clipping. Check TE / CRS / alignment inputs.")
    win = Window(c0c, r0c, c1c - c0c, r1c - r0c)
    gt = (x0 + c0c * g[1], g[1], 0.0, y0 + r0c * g[5], 0.0, g[5])
    info = {"te": {"left": left, "bottom": bottom, "right": right, "top": top}, "snapped_te": snapped,
            "window": {"col_off": win.col_off, "row_off": win.row_off, "width": win.width, "height": win.height}}
    return win, gt, info


def _plane16(x, what: str):
    if not hasattr(x, "shape") or not hasattr(x, "dtype"):
        raise ValueError(f"{what}: expected an (H, W) uint16 array or tensor, got {type(x).__name__}")
    shape, dt = tuple(int(n) for n in x.shape), _dtype_name(x)
    if len(shape) != 2 or min(shape) < 1 or dt != "uint16":
        raise ValueError(f"{what}: expected a non-empty (H, W) uint16 plane, got {dt} {shape}")
    return shape


def _up_of(hw, grid, what: str) -> int:
    (H, W), (H10, W10) = hw, grid
    if (H, W) == (H10, W10):
        return 1
    if (H, W) == ((H10 + 1) // 2, (W10 + 1) // 2):
        return 2
    raise ValueError(f"{what}: a {H} x {W} plane is neither the {H10} x {W10} grid of blue (10 m) nor its half "
                     f"{(H10 + 1) // 2} x {(W10 + 1) // 2} (20 m)")


def _stack_plan(bands, window, out_dtype, rule, nodata, add_offset, quantification, nodata_out):
    """Everything that needs no GPU -> (band rows [(description, key, up, method, offset)], grid, Window, codes)."""
    if not isinstance(bands, Mapping):
        raise ValueError(f"bands: a mapping of asset keys to (H, W) uint16 planes, got {type(bands).__name__}")
    missing = [k for k in _REQUIRED if k not in bands]
    if missing:
        raise ValueError(f"Missing required assets: {missing}. Available: {list(bands.keys())}")      # s2_utils.py:516-518
    grid = _plane16(bands["blue"], "bands['blue']")
    ups = {k: _up_of(_plane16(bands[k], f"bands[{k!r}]"), grid, f"bands[{k!r}]") for k in _REQUIRED}
    include_nir08 = False
    if bands.get("nir08") is not None:
        ups["nir08"] = _up_of(_plane16(bands["nir08"], "bands['nir08']"), grid, "bands['nir08']")
        include_nir08 = ups["nir08"] != ups["nir"]                                                   # s2_utils.py:561-565
    if not include_nir08:
        warnings.warn("'nir08' not included (missing or same resolution as 'nir'). Output will have 9 bands.", stacklevel=3)
    if out_dtype not in _DTYPES:
        raise ValueError(f"out_dtype={out_dtype!r}: 'uint16' or 'float32'")
    if rule not in _RULES:
        raise ValueError(f"rule={rule!r}: 'strict' or 'renorm'")
    if nodata is not None:
        nodata = _int(nodata, "nodata", 0)
        if nodata > 65535:
            raise ValueError(f"nodata={nodata}: no uint16 value")
    if nodata_out not in (0, 65535) or isinstance(nodata_out, bool):
        raise ValueError(f"nodata_out={nodata_out!r}: 0 or 65535")
    try:
        quant = float(quantification)
    except (TypeError, ValueError):
        raise ValueError(f"quantification={quantification!r}: must be a number") from None
    if not (math.isfinite(quant) and quant > 0.0):
        raise ValueError(f"quantification={quant}: must be finite and > 0")
    rows = []
    for desc, key, method in S2_STACK_BANDS:
        if key == "nir08" and not include_nir08:
            continue
        off = add_offset.get(key, 0) if isinstance(add_offset, Mapping) else add_offset
        if isinstance(off, (bool, np.bool_)) or not isinstance(off, (int, np.integer)) or abs(int(off)) > 65535:
            raise ValueError(f"add_offset={off!r}: an integer of at most 65535 in size, or a mapping of asset keys to such")
        rows.append((desc, key, ups[key], _METHODS[method], int(off)))
    H10, W10 = grid
    if window is None:
        win = Window(0, 0, W10, H10)
    else:
        try:
            win = Window(*(_int(v, "window", lo) for v, lo in zip(window, (0, 0, 1, 1))))
        except TypeError:
            raise ValueError(f"window={window!r}: a Window(col_off, row_off, width, height)") from None
        if win.col_off + win.width > W10 or win.row_off + win.height > H10:
            raise ValueError(f"window={tuple(win)}: leaves the {H10} x {W10} grid")
    return rows, grid, win, _DTYPES[out_dtype], _RULES[rule], nodata, quant


def _dev16(x, torch, dev):
    """The plane on the device, rows contiguous (a row stride is kept)."""
    if not _is_torch(x):
        a = np.ascontiguousarray(x)
        x = torch.from_numpy(a if a.flags.writeable else a.copy())
    t = x.to(dev)
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def assemble_s2_stack(bands, *, window=None, out_dtype: str = "uint16", rule: str = "strict", nodata=0, add_offset=0,
                      quantification: float = 10000.0, fill: float = float("nan"), nodata_out: int = 0, scl=None, out=None,
                      count_invalid: bool = False) -> S2StackOutput:
    """``download_s2_spectral_stack`` + ``crop_s2_stack_to_te`` (s2_utils.py:505-783) without the I/O: ``bands`` maps the asset keys
    ``blue green red nir rededge1 rededge2 rededge3 swir16 swir22`` and optionally ``nir08`` to (H, W) uint16 arrays or device
    tensors as the granule delivers them.  ``blue`` is the 10 m grid; every other plane has that shape (10 m) or its half, rounded
    up (20 m) - ``up`` is inferred and anything else is a ValueError.  The stack has the order of ``S2_STACK_BANDS``; it has 9
    bands, with a warning, when ``nir08`` is missing or has the resolution of ``nir``.

    window          None (the granule) or ``Window(col_off, row_off, width, height)`` in 10 m pixels (``s2_crop_window``'s); the
                    result IS that window of the full-granule result, whatever the parity of its origin;
    out_dtype       "uint16": the rounded DN plus ``add_offset``, clamped into the values that are not ``nodata_out`` (0 or 65535);
                    "float32": ``(DN + add_offset) / quantification`` from one float64 expression, ``fill`` where invalid;
    rule, nodata    a tap is invalid when it equals ``nodata`` (None: every tap is valid); "strict": any invalid tap blanks the
                    output; "renorm": only the source pixel that contains the output pixel must be valid, the others drop out;
    add_offset      an int or a mapping of asset keys to ints: BOA_ADD_OFFSET of processing baseline 04.00 and later (-1000);
    scl             an (H, W) uint8 SCL plane at 10 m or 20 m: returned under the same window at 10 m (``hsr_s2_expand_u8``), so
                    that ``fuse_scene_clear`` takes it whatever the parity of the window;
    out             an (nbands, height, width) device tensor of ``out_dtype`` with contiguous rows to write into;
    count_invalid   ``invalid``: (nbands,) int64 on the device, the invalid outputs per band.

    -> ``S2StackOutput(stack, names, window, scl, invalid)``; stack is (nbands, height, width) on the device, contiguous unless
    ``out`` says otherwise, names the band descriptions.  One launch for all bands (two with ``scl``), no host synchronisation:
    ``invalid`` stays a device tensor.  NumPy planes are copied to the device once."""
    rows, (H10, W10), win, dt, rl, nodata, quant = _stack_plan(bands, window, out_dtype, rule, nodata, add_offset, quantification,
                                                                nodata_out)
    nb, h, w = len(rows), win.height, win.width
    scl_up = None
    if scl is not None:
        from .clouds import _plane, _up
        scl_up = _up((H10, W10), _plane(scl, "scl"), "scl")
    if out is not None and (not _is_torch(out) or tuple(out.shape) != (nb, h, w) or _dtype_name(out) != out_dtype or out.stride(2) != 1
                            or out.stride(1) < w or out.stride(0) < (h - 1) * out.stride(1) + w):
        raise ValueError(f"out: a ({nb}, {h}, {w}) {out_dtype} device tensor with contiguous rows")
    torch = nat.require_gpu()
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    if out is not None and not out.is_cuda:
        raise ValueError("out: a device tensor")
    st = _stream(torch, out)
    planes = [_dev16(bands[key], torch, dev) for _, key, _, _, _ in rows]
    table = (nat.S2Band * nb)()
    for e, p, (_, _, up, method, off) in zip(table, planes, rows):
        e.plane_dev, e.rs, e.H, e.W, e.up, e.method, e.add_offset = p.data_ptr(), p.stride(0), p.shape[0], p.shape[1], up, method, off
    if out is None:
        out = torch.empty((nb, h, w), dtype=getattr(torch, out_dtype), device=dev)
    invalid = torch.empty(nb, dtype=torch.int64, device=dev) if count_invalid else None
    nat.check(lib.hsr_s2_stack(table, nb, H10, W10, win.row_off, win.col_off, h, w, 0 if nodata is None else 1, nodata or 0, rl, dt,
                               _ptr(out), out.stride(0), out.stride(1), int(nodata_out), float(fill), quant, _ptr(invalid), st),
              "hsr_s2_stack")
    scl_out = None
    if scl is not None:
        from .clouds import _plane_dev
        S, rs = _plane_dev(scl, torch, dev)
        scl_out = torch.empty((h, w), dtype=torch.uint8, device=dev)
        nat.check(lib.hsr_s2_expand_u8(_ptr(S), S.shape[0], S.shape[1], rs, scl_up, H10, W10, win.row_off, win.col_off, h, w,
                                       _ptr(scl_out), w, st), "hsr_s2_expand_u8")
    return S2StackOutput(out, [r[0] for r in rows], win, scl_out, invalid)
