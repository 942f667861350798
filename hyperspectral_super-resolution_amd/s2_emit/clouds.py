"""The Sentinel-2 scene classification layer (SCL) on the device: class statistics, the buffered cloud mask, that mask on the
EMIT grid, and a scene fusion that knows what a cloud is.

The reference reads the SCL only to choose a granule: ``s2_data/cloud_utils.py`` has ``SCL_NAMES``, ``CLOUD_CLASSES``,
``count_cloud_pixels`` (:33-53) and ``scl_metrics`` (:82-101, with its ``include_shadows`` switch).  Both functions open a raster
by URL and cut a region of interest out of it with rasterio, which is absent here and NOT reproduced: ours take the SCL plane
itself, an (H, W) uint8 array or device tensor, as ``ortho.py`` and ``reproject.py`` take arrays where the reference takes paths.
The counts are the reference's, integer for integer.

What the reference does not have (csrc/hsr_scl.hip, include/hsr_scl.h):
    cloud_mask         the class mask with the safety buffer every SCL user applies, because SCL cloud edges leak;
    coarse_clear_mask  that mask on the 60 m EMIT grid, as a training mask and a per-window cloud count;
    mask_cube          a 10 m cube blanked under a mask, in place;
    fuse_scene_clear   ``fuse_scene`` that trains on clear cells only, rejects cloudy windows and blanks the cube under the
                       buffered mask.
Not claimed: Sen2Cor's classes are taken as given - there is no cloud detection of our own - and the SCL is not reprojected: it
shares the S2 grid, at 10 m or at 20 m (``up`` = 1 or 2 S2 pixels per SCL pixel).  NumPy arrays are copied to the device once.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional

import numpy as np

from . import _native as nat
from ._engine import _ptr, _stream
from .pairs import _dtype_name
from .ridge import _is_torch
from .scenes import _fuse_scene, _int, _cloud_frac

# cloud_utils.py:13-16 and :31, value for value
SCL_NAMES = {
    0: "No data", 1: "Saturated/Defective", 2: "Dark features/shadows", 3: "Cloud shadows",
    4: "Vegetation", 5: "Bare soils", 6: "Water", 7: "Unclassified", 8: "Cloud med", 9: "Cloud high", 10: "Thin cirrus", 11: "Snow/Ice"
}
CLOUD_CLASSES = {8, 9, 10, 11}

ClearSceneOutput = namedtuple("ClearSceneOutput", "cube tiles n_train status bands mask clear")
_SHAPES = {"disc": nat.HSR_SCL_DISC, "square": nat.HSR_SCL_SQUARE}
_OTHER = 12                                                             # the histogram's bin of every value above 11


def _plane(x, what: str):
    """(H, W) of a uint8 plane."""
    if not hasattr(x, "shape") or not hasattr(x, "dtype"):
        raise ValueError(f"{what}: expected an (H, W) uint8 array or tensor, got {type(x).__name__}")
    shape, dt = tuple(int(n) for n in x.shape), _dtype_name(x)
    if len(shape) != 2 or min(shape) < 1 or dt not in ("uint8", "bool"):
        raise ValueError(f"{what}: expected a non-empty (H, W) uint8 plane, got {dt} {shape}")
    return shape


def _plane_dev(x, torch, dev):
    """The plane on the device, uint8, rows contiguous (a row stride is kept); -> (tensor, row stride)."""
    if not _is_torch(x):
        a = np.ascontiguousarray(x)
        x = torch.from_numpy(a if a.flags.writeable else a.copy())      # torch takes no read-only array
    t = x.to(dev)
    t = t.view(torch.uint8) if t.dtype == torch.bool else t
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t, t.stride(0)


def _class_bits(classes, what: str) -> int:
    bits = 0
    try:
        for c in classes:
            c = _int(c, what, 0)
            if c < 32:                                                  # a value >= 32 is in neither set of hsr_scl_mask
                bits |= 1 << c
            elif c > 255:
                raise ValueError(f"{what}: class {c} is no uint8 value")
    except TypeError:
        raise ValueError(f"{what}={classes!r}: an iterable of class values") from None
    return bits


def _mask_params(classes, include_shadows, flat_classes, buffer, shape):
    grow = _class_bits(classes, "classes") | (1 << 3 if include_shadows else 0)
    flat = _class_bits(flat_classes, "flat_classes")
    r = _int(buffer, "buffer", 0)
    if r > nat.HSR_SCL_MAX_RADIUS:
        raise ValueError(f"buffer={r}: at most {nat.HSR_SCL_MAX_RADIUS} SCL pixels")
    if shape not in _SHAPES:
        raise ValueError(f"shape={shape!r}: 'disc' or 'square'")
    return grow, flat, r, _SHAPES[shape]


def _counts(scl, tile):
    """The (ny, nx, 16) int64 class histograms of the windows of ``tile`` (None: the whole plane), on the host: one launch and
    one small copy."""
    H, W = _plane(scl, "scl")
    if tile is None:
        th, tw = H, W
    else:
        th, tw = (_int(v, "tile") for v in (tile if isinstance(tile, (tuple, list)) else (tile, tile)))
        if th > H or tw > W:
            raise ValueError(f"tile={tile}: larger than the {H} x {W} plane")
    if th * tw > 2 ** 31 - 1:
        raise ValueError(f"a window of {th} x {tw} pixels: at most 2^31 - 1")
    torch = nat.require_gpu()
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    S, rs = _plane_dev(scl, torch, dev)
    counts = torch.empty((H // th, W // tw, nat.HSR_SCL_BINS), dtype=torch.int32, device=dev)
    nat.check(lib.hsr_scl_class_counts(_ptr(S), H, W, rs, th, tw, _ptr(counts), _stream(torch)), "hsr_scl_class_counts")
    return counts.cpu().numpy().astype(np.int64)


def scl_metrics(scl, include_shadows: bool = False, *, tile=None):
    """The reference's ``scl_metrics`` (cloud_utils.py:82-101) on the SCL plane itself: (H, W) uint8, a device tensor or a NumPy
    array.  The reference takes a raster path and a region of interest and reads the plane with rasterio; ours takes the array (no
    I/O).  Returns its dict - total_px, valid_px, nodata_px, cloud_px (classes 8, 9, 10 and, with ``include_shadows``, 3),
    cloud_frac_valid (NaN without a valid pixel) and class_counts keyed by ``SCL_NAMES`` with only the classes that occur - from
    ONE launch and one copy of 16 int32.  The values above 11, which ``np.unique`` would list one by one under ``str(value)``, share
    the key ``"other"``: Sen2Cor writes none.

    ``tile`` (an int or (th, tw)): the same per window of the regular grid (floor; ``hsr_scene_black_counts``' convention) -
    a dict of (ny, nx) arrays total_px, valid_px, nodata_px, cloud_px (int64), cloud_frac_valid (float64) and class_counts
    (ny, nx, 13) int64, bin 12 holding every value above 11."""
    c = _counts(scl, tile)
    cloud_set = [8, 9, 10] + ([3] if include_shadows else [])
    total = c.sum(axis=-1)
    valid = total - c[..., 0]
    cloud = c[..., cloud_set].sum(axis=-1)
    if tile is not None:
        with np.errstate(invalid="ignore", divide="ignore"):
            frac = np.where(valid > 0, cloud / valid, np.nan)
        return {"total_px": total, "valid_px": valid, "nodata_px": c[..., 0], "cloud_px": cloud, "cloud_frac_valid": frac,
                "class_counts": c[..., :_OTHER + 1]}
    c, total_px, valid_px, cloud_px = c[0, 0], int(total[0, 0]), int(valid[0, 0]), int(cloud[0, 0])
    names = {k: SCL_NAMES.get(k, "other") for k in range(_OTHER + 1)}
    return {
        "total_px": total_px,
        "valid_px": valid_px,
        "nodata_px": int(c[0]),
        "cloud_px": cloud_px,
        "cloud_frac_valid": (cloud_px / valid_px) if valid_px else np.nan,
        "class_counts": {names[k]: int(c[k]) for k in range(_OTHER + 1) if c[k]},
    }


def count_cloud_pixels(scl):
    """The reference's ``count_cloud_pixels`` (cloud_utils.py:33-53): ``(clouds, total)`` with total the pixels that are not 0 and
    clouds those of ``CLOUD_CLASSES`` (8, 9, 10 and 11 - snow counts here, as in the reference) among them.  The reference takes
    a URL and a geometry and reads the plane with rasterio; ours takes the (H, W) uint8 array or device tensor.  One launch, one
    copy of 16 int32."""
    c = _counts(scl, None)[0, 0]
    return int(c[sorted(CLOUD_CLASSES)].sum()), int(c.sum() - c[0])


def cloud_mask(scl, *, classes=(8, 9, 10), include_shadows: bool = False, flat_classes=(0, 1), buffer: int = 0, shape: str = "disc",
               out=None):
    """(H, W) uint8 0 / 1 on the device: 1 where the SCL pixel is to be left out.  ``classes`` are bad and buffered - dilated by a
    ``shape`` ("disc": dy^2 + dx^2 <= buffer^2, "square": max(|dy|, |dx|) <= buffer) of ``buffer`` SCL pixels (0 .. 32), because SCL
    cloud edges leak; ``include_shadows`` adds class 3 to them, as ``scl_metrics`` does; ``flat_classes`` (nodata, defective) are
    bad and not buffered.  Nothing outside the plane counts (no wrap, no clamp).  ``out``: a (H, W) uint8 device tensor to write
    into (a row stride is kept).  One launch (``hsr_scl_mask``), no host synchronisation."""
    H, W = _plane(scl, "scl")
    grow, flat, r, shp = _mask_params(classes, include_shadows, flat_classes, buffer, shape)
    if out is not None and (not _is_torch(out) or tuple(out.shape) != (H, W) or _dtype_name(out) != "uint8" or out.stride(1) != 1
                            or out.stride(0) < W):
        raise ValueError(f"out: a ({H}, {W}) uint8 device tensor with contiguous rows")
    torch = nat.require_gpu()
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    S, rs = _plane_dev(scl, torch, dev)
    return _mask_into(lib, torch, _stream(torch), S, rs, grow, flat, r, shp, out)


def _mask_into(lib, torch, st, S, rs, grow, flat, r, shp, out=None):
    H, W = S.shape
    if out is None:
        out = torch.empty((H, W), dtype=torch.uint8, device=S.device)
    nat.check(lib.hsr_scl_mask(_ptr(S), H, W, rs, grow, flat, r, shp, _ptr(out), out.stride(0), st), "hsr_scl_mask")
    return out


def _max_bad(max_bad_frac, k: int) -> int:
    try:
        frac = float(max_bad_frac)
    except (TypeError, ValueError):
        raise ValueError(f"max_bad_frac={max_bad_frac!r}: must be a number") from None
    if not 0.0 <= frac <= 1.0:
        raise ValueError(f"max_bad_frac={frac}: must lie in [0, 1]")
    return int(math.floor(frac * (k * k)))                               # float64 on the host


def _coarse_plan(shape, k, max_bad_frac, cell):
    H, W = shape
    k = _int(k, "k")
    if k > nat.HSR_SCL_MAX_K or k > H or k > W:
        raise ValueError(f"k={k}: at most {nat.HSR_SCL_MAX_K} and no larger than the {H} x {W} mask")
    max_bad = _max_bad(max_bad_frac, k)
    hc, wc = H // k, W // k
    if cell is not None:
        ch, cw = (_int(v, "cell") for v in (cell if isinstance(cell, (tuple, list)) else (cell, cell)))
        if ch > hc or cw > wc:
            raise ValueError(f"cell={cell}: larger than the {hc} x {wc} grid")
        cell = (ch, cw)
    return k, max_bad, hc, wc, cell


def _coarse_into(lib, torch, st, M, rs, k, max_bad, cell, win=None):
    H, W = M.shape
    hc, wc = H // k, W // k
    clear = torch.empty((hc, wc), dtype=torch.uint8, device=M.device)
    ch, cw = cell if cell is not None else (1, 1)
    if cell is not None and win is None:
        win = torch.empty((hc // ch, wc // cw), dtype=torch.int32, device=M.device)
    nat.check(lib.hsr_scl_coarse(_ptr(M), H, W, rs, k, max_bad, _ptr(clear), None, ch, cw, _ptr(win) if cell is not None else None, st),
              "hsr_scl_coarse")
    return clear, win if cell is not None else None


def coarse_clear_mask(mask, k: int, *, max_bad_frac: float = 0.0, cell=None):
    """A mask on the EMIT grid: ``mask`` (H, W) uint8 / bool (``cloud_mask``'s result), ``k`` mask pixels per EMIT pixel
    (factor / up, 1 .. 16) -> ``(clear, win_counts)``.  clear (H // k, W // k) uint8 on the device is 1 where the cell's k x k block
    holds at most ``max_bad = floor(max_bad_frac k^2)`` set mask pixels (the product in float64 on the host); the leftover strips
    are not read.  ``cell`` (an int or (ch, cw); None: no counts and ``win_counts`` is None): win_counts
    (hc // ch, wc // cw) int32 on the device, the not-clear cells of every window of ``cell`` EMIT cells - the ``cloud_counts``
    of ``select_tiles``, with ``cell`` the tile or the stride.  One launch (``hsr_scl_coarse``), no host synchronisation."""
    shape = _plane(mask, "mask")
    k, max_bad, hc, wc, cell = _coarse_plan(shape, k, max_bad_frac, cell)
    torch = nat.require_gpu()
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    M, rs = _plane_dev(mask, torch, dev)
    return _coarse_into(lib, torch, _stream(torch), M, rs, k, max_bad, cell)


def _up(cube_hw, mask_hw, what: str) -> int:
    """1 when the mask has the cube's grid, 2 when it has half of it (rounded up), else a ValueError."""
    (H, W), (Hm, Wm) = cube_hw, mask_hw
    if (Hm, Wm) == (H, W):
        return 1
    if (Hm, Wm) == ((H + 1) // 2, (W + 1) // 2):
        return 2
    raise ValueError(f"{what}: a {Hm} x {Wm} plane is neither the {H} x {W} grid (10 m) nor its half {(H + 1) // 2} x {(W + 1) // 2} "
                     "(20 m)")


def _apply_into(lib, torch, st, cube, M, mrs, up: int, fill: float, count=None):
    T, H, W = cube.shape
    nat.check(lib.hsr_scl_apply(_ptr(cube), T, H, W, cube.stride(0), cube.stride(1), _ptr(M), M.shape[0], M.shape[1], mrs, up,
                                float(fill), _ptr(count), st), "hsr_scl_apply")


def mask_cube(cube, mask, *, fill: float = float("nan")):
    """In place: ``cube`` (T, H, W) float32 on the device becomes ``fill`` where ``mask[y // up, x // up]`` is set, and no other
    byte is written.  ``up`` is inferred from the shapes: 1 when the mask is (H, W), 2 when it is (ceil(H / 2), ceil(W / 2)),
    anything else is a ValueError.  The cube may be a view with band and row strides of its own.  Returns the cube.  One launch
    (``hsr_scl_apply``) whose cost follows the cloud cover; no host synchronisation."""
    if not _is_torch(cube) or _dtype_name(cube) != "float32" or cube.dim() != 3 or min(cube.shape) < 1:
        raise ValueError("cube: a non-empty (T, H, W) float32 device tensor (it is changed in place)")
    T, H, W = (int(n) for n in cube.shape)
    up = _up((H, W), _plane(mask, "mask"), "mask")
    if cube.stride(2) != 1 or cube.stride(1) < W or cube.stride(0) < (H - 1) * cube.stride(1) + W:
        raise ValueError("cube: rows must be contiguous and rows and bands must not overlap")
    torch = nat.require_gpu()
    if not cube.is_cuda:
        raise ValueError("cube: a device tensor (it is changed in place)")
    lib = nat.load()
    M, mrs = _plane_dev(mask, torch, cube.device)
    _apply_into(lib, torch, _stream(torch, cube), cube, M, mrs, up, fill)
    return cube


class _Clouds:
    """The cloud-aware pieces of ``fuse_scene_clear`` for the loop it shares with ``fuse_scene`` (scenes._fuse_scene)."""

    def __init__(self, scl, max_cloud_frac, mask_output, max_bad_frac, mask_params):
        self.scl, self.mask_output, self.max_bad_frac, self.params = scl, bool(mask_output), max_bad_frac, mask_params
        self.limit = _cloud_frac(max_cloud_frac)
        self.mask = self.clear = None

    def check(self, plan):
        """Everything that needs no GPU."""
        _, hs, ws = plan.s2_shape
        self.up = _up((hs, ws), _plane(self.scl, "scl"), "scl")
        if plan.scale % self.up:
            raise ValueError(f"factor={plan.scale}: no multiple of the {self.up} S2 pixels of an SCL pixel")
        self.k, self.max_bad, hc, wc, _ = _coarse_plan(_plane(self.scl, "scl"), plan.scale // self.up, self.max_bad_frac, None)
        self.ce = plan.tile if plan.stride is None else plan.stride
        if self.ce > hc or self.ce > wc:
            raise ValueError(f"scl: the {hc} x {wc} EMIT cells under it hold no window of {self.ce}")

    def find(self, lib, torch, dev, st, plan):
        S, rs = _plane_dev(self.scl, torch, dev)
        self.mask = _mask_into(lib, torch, st, S, rs, *self.params)
        hc, wc = S.shape[0] // self.k, S.shape[1] // self.k
        grid = (hc // self.ce, wc // self.ce)

        def launch(segment):
            self.clear, _ = _coarse_into(lib, torch, st, self.mask, self.mask.stride(0), self.k, self.max_bad, (self.ce, self.ce),
                                         segment)

        if not plan.windows:                                            # no find: the grid of clear cells all the same
            self.clear, _ = _coarse_into(lib, torch, st, self.mask, self.mask.stride(0), self.k, self.max_bad, None)
        return grid, launch, self.limit

    def train_mask(self, lib, torch, st, origins, th: int, tw: int):
        org = torch.from_numpy(np.ascontiguousarray(origins, dtype=np.int32)).to(self.clear.device)
        out = torch.empty((len(origins), th, tw), dtype=torch.uint8, device=self.clear.device)
        hc, wc = self.clear.shape
        nat.check(lib.hsr_scl_gather_tiles(_ptr(self.clear), hc, wc, wc, _ptr(org), len(origins), th, tw, _ptr(out), st),
                  "hsr_scl_gather_tiles")
        return out

    def finish(self, lib, torch, st, cube):
        if self.mask_output:
            _apply_into(lib, torch, st, cube, self.mask, self.mask.stride(0), self.up, float("nan"))


def fuse_scene_clear(emit_scene, s2_scene, scl, *, max_cloud_frac: float = 0.5, mask_output: bool = True, max_bad_frac: float = 0.0,
                     classes=(8, 9, 10), include_shadows: bool = False, flat_classes=(0, 1), buffer: int = 0, shape: str = "disc",
                     tile: int = 100, factor: int = 6, max_black_frac: float = 0.0, max_tiles=None, batch: int = 64, bands=32,
                     degree: int = 3, alpha: float = 1.0, emit_nodata: Optional[float] = None, s2_nodata: Optional[float] = None,
                     eps: float = 1e-4, stride=None, blend=None) -> ClearSceneOutput:
    """``fuse_scene`` with the scene classification layer of the S2 granule: ``scl`` (H, W) uint8 on the S2 grid - (H_s2, W_s2) at
    10 m or (ceil(H_s2 / 2), ceil(W_s2 / 2)) at 20 m - an array or a device tensor.  Every keyword of ``fuse_scene`` and of
    ``cloud_mask`` is taken and means the same.

    1. ``cloud_mask(scl, classes=, include_shadows=, flat_classes=, buffer=, shape=)`` and ``coarse_clear_mask`` with
       ``k = factor / up`` and ``max_bad_frac`` (0: an EMIT cell is clear only when none of its SCL pixels is masked).
    2. The find: the count of not-clear cells of every window rides in the SAME device-to-host copy as the two black-count grids,
       so there is still ONE host synchronisation; a window is kept when it passes ``max_black_frac`` and has
       ``not-clear cells / tile^2 <= max_cloud_frac``, inside the same walk, so ``max_tiles`` keeps its meaning.  The tile dicts
       carry ``cloud_frac``.
    3. Per batch the byte gather of the windows of ``clear``, passed as ``train_mask=`` to ``fuse_tile_pairs``: the models see
       clear cells only.  The mosaic - or, with ``stride`` / ``blend="feather"``, the blend - as in ``fuse_scene``.
    4. Last, with ``mask_output``, the cube becomes NaN under the buffered mask (``hsr_scl_apply``): no prediction under a cloud.

    Returns ``ClearSceneOutput(cube, tiles, n_train, status, bands, mask, clear)``: the first five as ``fuse_scene`` returns them
    (``n_train`` counts the clear training cells), mask the (H, W) uint8 buffered mask and clear the (H // k, W // k) uint8 grid
    of clear EMIT cells, both on the device.  An all-clear SCL with ``mask_output=False`` gives ``fuse_scene``'s cube bit for bit.
    The loop is ``fuse_scene``'s own (scenes._fuse_scene)."""
    clouds = _Clouds(scl, max_cloud_frac, mask_output, max_bad_frac,
                     _mask_params(classes, include_shadows, flat_classes, buffer, shape))
    _max_bad(max_bad_frac, 1)
    out = _fuse_scene(emit_scene, s2_scene, clouds, tile, factor, max_black_frac, max_tiles, batch, bands, degree, alpha, emit_nodata,
                      s2_nodata, eps, stride, blend)
    return ClearSceneOutput(*out, clouds.mask, clouds.clear)
