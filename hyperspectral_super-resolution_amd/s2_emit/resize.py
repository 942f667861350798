"""Area resampling at any ratio and origin on the device: the area-weighted mean of the source pixels under each destination cell.

The reference shrinks the S2 RGB onto the EMIT grid with ``resize_s2_rgb_to`` (s2_emit/viz.py:19-24, ``cv2.resize(...,
INTER_AREA)``) between ``pseudo_s2_rgb`` and ``apply_shared_percentile_stretch``, and its notebook brings one grid onto another of
the same CRS with ``downsample_s2_to_grid(resampling="average")``.  Both are one operation, defined exactly in include/hsr_resize.h:
cells from a float64 origin and scale, fractional coverage at the cells' edges, invalid samples skipped, float64 sums in a fixed
order.  cv2's bits and GDAL's are NOT claimed (cv2 works in float32 and drops slivers below 1e-3).

    resample_area            (h, w), (C, h, w) or (h, w, C) uint8 / uint16 / float32 device tensor -> ``AreaResampleOutput``;
    resample_to_grid         the same between two GDAL geotransforms of one CRS whose grids need not be aligned;
    grid_from_geotransforms  (origin, scale) of one grid in the pixels of another (``hsr_area_grid_from_geotransforms``);
    resize_s2_rgb_to         the reference's name: a device tensor stays on the device, a NumPy array takes the path it always took.
Enlarging is not this family's job: ``hsr_bilinear_upsample`` does it.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple

from . import _native as nat
from . import viz
from ._engine import _ptr, _stream
from .pairs import _dtype_name
from .ridge import _is_torch

AreaResampleOutput = namedtuple("AreaResampleOutput", "image invalid")
_CODES = {"float32": nat.HSR_AREA_F32, "uint8": nat.HSR_AREA_U8, "uint16": nat.HSR_AREA_U16}
_RULES = {"strict": nat.HSR_AREA_STRICT, "renorm": nat.HSR_AREA_RENORM}


def _hw(v, what):
    try:
        H, W = (int(n) for n in v)
    except (TypeError, ValueError):
        raise ValueError(f"{what}={v!r}: (rows, columns)") from None
    if H < 1 or W < 1:
        raise ValueError(f"{what}={v!r}: at least one row and one column")
    return H, W


def _pair(v, what):
    try:
        a, b = (float(n) for n in v)
    except (TypeError, ValueError):
        raise ValueError(f"{what}={v!r}: two numbers, (rows, columns)") from None
    if not (math.isfinite(a) and math.isfinite(b)):
        raise ValueError(f"{what}={v!r}: must be finite")
    return a, b


def _check_shrink(src_hw, dst_hw):
    if dst_hw[0] > src_hw[0] or dst_hw[1] > src_hw[1]:
        raise ValueError(f"target {tuple(dst_hw)} is larger than the source {tuple(src_hw)}: area resampling only shrinks; "
                         f"enlarging is hsr_bilinear_upsample's job")


def _axes(src, channel_axis):
    """-> (C, h, w, the tensor's dimension of the channel or None)."""
    if not _is_torch(src):
        raise ValueError(f"src: a uint8 / uint16 / float32 device tensor, got {type(src).__name__}")
    if _dtype_name(src) not in _CODES:
        raise ValueError(f"src: uint8, uint16 or float32, got {_dtype_name(src)}")
    if src.dim() == 2 and channel_axis is None:
        return 1, int(src.shape[0]), int(src.shape[1]), None
    if src.dim() != 3 or channel_axis not in (0, 2, -1, -3):
        raise ValueError(f"src: (h, w), or (C, h, w) with channel_axis=0, or (h, w, C) with channel_axis=-1; got shape "
                         f"{tuple(src.shape)} and channel_axis={channel_axis!r}")
    ca = channel_axis % 3
    rows, cols = (1, 2) if ca == 0 else (0, 1)
    Cn = int(src.shape[ca])
    if not 1 <= Cn <= nat.HSR_AREA_MAX_CHANNELS:
        raise ValueError(f"src: {Cn} channels, at most {nat.HSR_AREA_MAX_CHANNELS}")
    return Cn, int(src.shape[rows]), int(src.shape[cols]), ca


def _strides(t, ca):
    if ca is None:
        return 1, t.stride(0), t.stride(1)
    return (t.stride(0), t.stride(1), t.stride(2)) if ca == 0 else (t.stride(2), t.stride(0), t.stride(1))


def grid_from_geotransforms(src_gt, dst_gt):
    """``hsr_area_grid_from_geotransforms``: two GDAL geotransforms (x0, dx, 0, y0, 0, dy) of one CRS -> ``(origin, scale)`` of the
    destination grid in source pixels, each (rows, columns).  Rotation terms, pixel sizes of differing sign and a scale below 1
    are refused (``HsrError``).  Host only."""
    lib = nat.load()
    s, d, g = (C.c_double * 6)(*(float(v) for v in src_gt)), (C.c_double * 6)(*(float(v) for v in dst_gt)), (C.c_double * 4)()
    nat.check(lib.hsr_area_grid_from_geotransforms(s, d, g), "hsr_area_grid_from_geotransforms")
    return (g[0], g[1]), (g[2], g[3])


def resample_area(src, out_hw, *, origin=(0.0, 0.0), scale=None, channel_axis=None, nodata=None, rule="renorm", min_valid_frac=0.0,
                  out_dtype=None, post_scale=1.0, fill=float("nan"), nodata_out=None, out=None) -> AreaResampleOutput:
    """The area resampling of include/hsr_resize.h in one launch (``hsr_area_resample``), with no host synchronisation.

    src             (h, w), (C, h, w) with ``channel_axis=0`` or (h, w, C) with ``channel_axis=-1``: a uint8 / uint16 / float32
                    device tensor with any strides (padded rows, a channel slice of a wider image), C <= 16;
    out_hw          (H, W) of the result;
    origin, scale   (rows, columns) in source pixels, float64: destination cell j covers [x0 + j sx, x0 + (j + 1) sx], clipped to
                    the source.  ``scale`` defaults to (h / H, w / W): INTER_AREA's frame.  Each scale lies in [1, 64];
    nodata          a sample equal to it is invalid, as is every non-finite float32 sample; invalid samples are skipped;
    rule            "strict": an output is invalid when any of its taps is; "renorm": when no valid area is left, or less than
                    ``min_valid_frac`` of the cell's area inside the source.  A cell outside the source is invalid;
    out_dtype       the input's (default) or "float32"; a float32 output is multiplied by ``post_scale`` in float32 and ``fill``
                    where invalid; an integer output is rounded half to even and ``nodata_out`` (default 0) where invalid;
    out             a device tensor of the result's shape and dtype to write into (any strides without overlap).

    -> ``AreaResampleOutput(image, invalid)``: image in the layout of ``src``, invalid (C,) int64 on the device."""
    Cn, h, w, ca = _axes(src, channel_axis)
    H, W = _hw(out_hw, "out_hw")
    y0, x0 = _pair(origin, "origin")
    sy, sx = (h / H, w / W) if scale is None else _pair(scale, "scale")
    if rule not in _RULES:
        raise ValueError(f"rule={rule!r}: 'strict' or 'renorm'")
    in_name = _dtype_name(src)
    out_name = in_name if out_dtype is None else str(out_dtype).replace("torch.", "")
    if out_name not in (in_name, "float32"):
        raise ValueError(f"out_dtype={out_dtype!r}: the input's ({in_name}) or 'float32'")
    shape = (H, W) if ca is None else (Cn, H, W) if ca == 0 else (H, W, Cn)
    if out is not None and (not _is_torch(out) or tuple(out.shape) != shape or _dtype_name(out) != out_name):
        raise ValueError(f"out: a {shape} {out_name} device tensor")
    torch = nat.require_gpu()
    lib = nat.load()
    if not src.is_cuda or (out is not None and not out.is_cuda):
        raise ValueError("src and out: device tensors")
    st = _stream(torch, src)
    if out is None:
        out = torch.empty(shape, dtype=getattr(torch, out_name), device=src.device)
    invalid = torch.empty(Cn, dtype=torch.int64, device=src.device)
    scs, srs, sps = _strides(src, ca)
    dcs, drs, dps = _strides(out, ca)
    nat.check(lib.hsr_area_resample(_ptr(src), _CODES[in_name], Cn, h, w, scs, srs, sps, y0, x0, sy, sx, 0 if nodata is None else 1,
                                    float(nodata or 0.0), _RULES[rule], float(min_valid_frac), _ptr(out), _CODES[out_name], H, W, dcs, drs,
                                    dps, float(post_scale), float(fill), int(nodata_out or 0), _ptr(invalid), st), "hsr_area_resample")
    return AreaResampleOutput(out, invalid)


def resample_to_grid(src, src_gt, dst_gt, dst_hw, **kw) -> AreaResampleOutput:
    """The notebook's ``downsample_s2_to_grid(..., resampling="average")`` for grids of one CRS that need not be aligned: the
    destination grid ``dst_gt`` with ``dst_hw`` cells, in the pixels of ``src_gt`` (``grid_from_geotransforms``), then
    ``resample_area`` with every keyword of it but origin and scale."""
    if "origin" in kw or "scale" in kw:
        raise ValueError("resample_to_grid: origin and scale come from the geotransforms")
    origin, scale = grid_from_geotransforms(src_gt, dst_gt)
    return resample_area(src, dst_hw, origin=origin, scale=scale, **kw)


def resize_s2_rgb_to(s2_rgb, target_hw):
    """Area resampling to target (H, W) (reference s2_emit/viz.py:19-24).  A NumPy array takes the path it always took
    (``viz.resize_s2_rgb_to``: cv2's INTER_AREA when cv2 is installed, a block mean for exact integer ratios, else the ImportError).
    A (H, W) or (H, W, C) uint8 / uint16 / float32 device tensor returns a new device tensor of the same dtype in one launch
    without a host synchronisation: rule "renorm", no nodata, INTER_AREA's frame under the definition of include/hsr_resize.h - not
    cv2's bits.  A target larger than the source on either axis is a ValueError: that is ``hsr_bilinear_upsample``'s job."""
    if not _is_torch(s2_rgb):
        return viz.resize_s2_rgb_to(s2_rgb, target_hw)
    if s2_rgb.dim() not in (2, 3):
        raise ValueError(f"s2_rgb: (H, W) or (H, W, C), got shape {tuple(s2_rgb.shape)}")
    H, W = _hw(target_hw, "target_hw")
    _check_shrink(tuple(s2_rgb.shape[:2]), (H, W))
    return resample_area(s2_rgb, (H, W), channel_axis=None if s2_rgb.dim() == 2 else -1).image
