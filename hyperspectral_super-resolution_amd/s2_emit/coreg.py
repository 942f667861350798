"""Co-registration of a Sentinel-2 scene to an EMIT scene on the device: the stage between ``ortho_scene`` and the tile-pair drivers
(``find_valid_paired_tiles``, ``extract_tile_pairs``, ``fuse_tile_pairs``, ``fuse_scene``), which all assume registered scenes.

The reference does this in ``s2_emit/arosics_coreg.py`` (``coregister_s2_granule_to_emit_granule``): it picks a band pair - S2 B08
(842 nm), then B04 (665 nm), against the closest EMIT band (``closest_band_1based``) - lays a grid of tie points, lets AROSICS
match a window at each, keeps the reliable shifts and warps the S2 granule with cubic resampling.  That function takes file paths
and needs rasterio and AROSICS; it is NOT reproduced here.  What is here is the same flow on arrays or GPU tensors with the
algorithm defined in include/hsr_coreg.h, on the sensor model of the rest of the package (an EMIT pixel is the ``factor`` x
``factor`` block mean of S2 pixels), in four HIP stages (csrc/hsr_coreg.hip):

    surface  ``match_windows``     zero-mean normalised cross-correlation of every tie point's EMIT window against S2 box sums, for
                                   every shift of up to ``max_shift`` S2 pixels
    peaks    ``match_windows``     surface -> record [cy, cx, dy, dx, score, sharpness, n_valid, status] with a sub-pixel peak
    fit      ``fit_shift_model``   records -> a translation or affine shift field, one outlier rejection pass
    warp     ``warp_scene``        S2'[y, x] = S2[y + dy, x + dx] by Keys cubic (a = -0.5, GDAL's "cubic") interpolation

Sign of the shift (dy, dx): EMIT pixel (i, j) ~ mean of S2[f i + dy + 0 .. f - 1, f j + dx + 0 .. f - 1].  GPU tensors in give
GPU tensors out with no host synchronisation; NumPy arrays are copied to the device and the results come back as arrays.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

from . import _engine as eng
from . import _native as nat

TiePoints = namedtuple("TiePoints", "table surface origins s2_shape max_shift")
ShiftModel = namedtuple("ShiftModel", "params max_abs_shift max_abs_slope")
CoregOutput = namedtuple("CoregOutput", "s2 model tie_points")

STATUS = {0: "OK", 1: "OUTSIDE", 2: "NO_SCORE", 3: "BORDER", 4: "LOW_SCORE", 5: "OUTLIER"}
_KINDS = {"translation": 0, "affine": 1}
_SLOPE_BOUND = 0.05          # |d shift / d pixel| the warp's staged footprint is sized for; a steeper model still warps correctly


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _check_params(window, factor, max_shift):
    if not (isinstance(window, (int, np.integer)) and 4 <= window <= 64):
        raise ValueError(f"window must be an integer in [4, 64], got {window!r}")
    if not (isinstance(factor, (int, np.integer)) and 1 <= factor <= 8):
        raise ValueError(f"factor must be an integer in [1, 8], got {factor!r}")
    if not (isinstance(max_shift, (int, np.integer)) and 1 <= max_shift <= 24):
        raise ValueError(f"max_shift must be an integer in [1, 24], got {max_shift!r}")


def closest_band(wavelengths_nm, target_nm) -> int:
    """Index of the band whose centre wavelength is closest to ``target_nm``; the first of equally close ones (np.argmin).  The
    reference's ``closest_band_1based`` minus one."""
    w = np.asarray(wavelengths_nm, dtype=np.float64).reshape(-1)
    if w.size == 0:
        raise ValueError("wavelengths_nm is empty")
    return int(np.argmin(np.abs(w - float(target_nm))))


def tie_point_grid(h_e, w_e, h_s, w_s, *, window=32, step=None, factor=6, max_shift=12, max_points=500):
    """(P, 2) int32 EMIT origins (i0, j0) of ``window`` x ``window`` windows, from the shapes alone (host only).  Origins start
    ceil(max_shift / factor) EMIT pixels in and stop where the search region f (i0 + window - 1) + max_shift + f - 1 would leave the
    S2 plane or the window the EMIT plane, ``step`` (default ``window``) apart; more than ``max_points`` are thinned evenly in
    row-major order.  A scene too small for one window gives (0, 2)."""
    _check_params(window, factor, max_shift)
    step = window if step is None else step
    if not (isinstance(step, (int, np.integer)) and step >= 1):
        raise ValueError(f"step must be a positive integer, got {step!r}")
    if not (isinstance(max_points, (int, np.integer)) and max_points >= 1):
        raise ValueError(f"max_points must be a positive integer, got {max_points!r}")
    inset = -(-max_shift // factor)

    def axis(n_e, n_s):
        hi = min(int(n_e) - window, (int(n_s) - max_shift - factor * window) // factor)
        return np.arange(inset, hi + 1, step, dtype=np.int64) if hi >= inset else np.zeros(0, np.int64)

    ii, jj = axis(h_e, h_s), axis(w_e, w_s)
    pts = np.stack(np.meshgrid(ii, jj, indexing="ij"), axis=-1).reshape(-1, 2)
    if len(pts) > max_points:
        keep = np.unique(np.round(np.linspace(0, len(pts) - 1, int(max_points))).astype(np.int64))
        pts = pts[keep]
    return np.ascontiguousarray(pts, dtype=np.int32)


def _to_device(torch, a, what, dtypes):
    if _is_torch(a):
        if not a.is_cuda:
            raise ValueError(f"{what} must be a GPU tensor (or a NumPy array)")
        return a
    a = np.asarray(a)
    if a.dtype not in dtypes:
        a = a.astype(dtypes[0])
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()


def match_windows(emit_plane, s2_plane, *, grid=None, emit_mask=None, s2_nodata=None, min_valid_frac=0.75, min_score=0.6,
                  window=32, step=None, factor=6, max_shift=12, max_points=500):
    """Score surfaces and tie-point records of one band pair: ``emit_plane`` (H_e, W_e) float32 and ``s2_plane`` (H_s, W_s) float32
    or uint16 (views of a scene's band pass without a copy).  ``grid``: (P, 2) int32 origins, default ``tie_point_grid`` of the two
    shapes.  A window needs ceil(min_valid_frac * window^2) valid pairs for a score.  Returns TiePoints(table (P, 8) float64,
    surface (P, 2R+1, 2R+1) float64, origins (P, 2) int32, ...); see include/hsr_coreg.h for the record and the status codes."""
    _check_params(window, factor, max_shift)
    if not 0.0 < float(min_valid_frac) <= 1.0:
        raise ValueError(f"min_valid_frac must be in (0, 1], got {min_valid_frac!r}")
    torch = nat.require_gpu()
    as_torch = _is_torch(emit_plane)
    e = _to_device(torch, emit_plane, "emit_plane", (np.float32,))
    s = _to_device(torch, s2_plane, "s2_plane", (np.float32, np.uint16))
    if e.dim() != 2 or s.dim() != 2:
        raise ValueError(f"emit_plane and s2_plane must be 2-D, got {tuple(e.shape)} and {tuple(s.shape)}")
    if e.dtype != torch.float32:
        e = e.to(torch.float32)
    m = None
    if emit_mask is not None:
        m = _to_device(torch, emit_mask, "emit_mask", (np.uint8, np.bool_))
        m = m if m.dtype in (torch.uint8, torch.bool) else (m != 0)
    if grid is None:
        grid = tie_point_grid(e.shape[0], e.shape[1], s.shape[0], s.shape[1], window=window, step=step, factor=factor,
                              max_shift=max_shift, max_points=max_points)
    if _is_torch(grid):
        origins = grid.to(device=e.device, dtype=torch.int32).contiguous()
    else:
        g = np.ascontiguousarray(np.asarray(grid).reshape(-1, 2), dtype=np.int32)
        if g.size == 0:
            origins = torch.empty((0, 2), dtype=torch.int32, device=e.device)           # a scene too small for one window
        else:
            origins = torch.from_numpy(g).pin_memory().to(e.device, non_blocking=True)  # pinned: the upload does not block the host
    min_valid = max(1, int(math.ceil(float(min_valid_frac) * window * window)))
    surface = eng.coreg_surface(e, s, origins, window, factor, max_shift, min_valid, m, s2_nodata)
    table = eng.coreg_peaks(surface, origins, window, factor, max_shift, e.shape, s.shape, min_score)
    tp = TiePoints(table, surface, origins, (int(s.shape[0]), int(s.shape[1])), int(max_shift))
    return tp if as_torch else tp._replace(table=table.cpu().numpy(), surface=surface.cpu().numpy(), origins=origins.cpu().numpy())


def fit_shift_model(tie_points, *, model="affine", reject_px=1.0, min_points=1):
    """Tie-point records -> ShiftModel.  ``model``: "translation" (the mean shift) or "affine" (least squares on the window
    centres; translation when fewer than 3 usable or collinear points).  Records further than ``reject_px`` from the first fit
    become OUTLIER (status 5, in ``tie_points.table``, in place) and the model is fitted once more without them.  Fewer than
    ``min_points`` usable records give the zero model (kind_used -1: the warp is the identity).  ``params`` is the 10 doubles
    [dy0, dy_x, dy_y, dx0, dx_x, dx_y, xc, yc, n_used, kind_used] - on the device for device records, an array for array records
    (then fitted by the kernel's host twin)."""
    if model not in _KINDS:
        raise ValueError(f"model must be 'translation' or 'affine', got {model!r}")
    if not float(reject_px) > 0.0:
        raise ValueError(f"reject_px must be > 0, got {reject_px!r}")
    if not (isinstance(min_points, (int, np.integer)) and min_points >= 0):
        raise ValueError(f"min_points must be a non-negative integer, got {min_points!r}")
    bound = float(tie_points.max_shift) + 1.0
    if _is_torch(tie_points.table):
        params = eng.coreg_fit_model(tie_points.table, _KINDS[model], min_points, reject_px, tie_points.s2_shape)
    else:
        table, params = eng.coreg_fit_model_host(tie_points.table, _KINDS[model], min_points, reject_px, tie_points.s2_shape)
        tie_points.table[...] = table
    return ShiftModel(params, bound, _SLOPE_BOUND)


def warp_scene(s2_scene, model, *, nodata=None, fill=None, out=None):
    """The corrected scene S2'[b, y, x] = S2[b](y + dy, x + dx), (bands, H, W) float32 or uint16, by Keys cubic interpolation in
    float64 (include/hsr_coreg.h); pixels whose source lies outside the scene, or touches an invalid sample (non-finite, or equal
    to ``nodata``) with a non-zero weight, become ``fill`` (default NaN for float32, ``nodata`` or 0 for uint16).  An integer
    translation is a bit-exact shifted copy.  ``out`` must not alias the input."""
    torch = nat.require_gpu()
    as_torch = _is_torch(s2_scene)
    s = _to_device(torch, s2_scene, "s2_scene", (np.float32, np.uint16))
    if s.dim() != 3:
        raise ValueError(f"s2_scene must be (bands, H, W), got {tuple(s.shape)}")
    if s.stride(2) != 1:
        s = s.contiguous()
    if fill is None:
        fill = float("nan") if s.dtype == torch.float32 else (0.0 if nodata is None else float(nodata))
    params = model.params
    if not _is_torch(params):
        params = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float64)).to(s.device)
    o, _ = eng.coreg_warp(s, params, fill, model.max_abs_shift, model.max_abs_slope, nodata, out)
    return o if as_torch else o.cpu().numpy()


def coregister_scene(emit_scene, s2_scene, *, emit_band, s2_band, factor=6, window=32, step=None, max_shift=12, max_points=500,
                     emit_mask=None, s2_nodata=None, min_valid_frac=0.75, min_score=0.6, model="affine", reject_px=1.0,
                     min_points=1, fill=None, out=None):
    """match_windows -> fit_shift_model -> warp_scene on an EMIT scene (bands, H_e, W_e) and an S2 scene (nb, H_s, W_s):
    CoregOutput(s2, model, tie_points), where ``s2`` has the S2 scene's shape and dtype and goes into ``find_valid_paired_tiles``
    or ``fuse_scene`` unchanged.

    ``s2_band`` is an index into the S2 scene.  ``emit_band`` is an index into the EMIT scene or a precomputed (H_e, W_e) plane such
    as a ``pseudo_s2_srf_integral`` band.  The reference matches S2 B08 (842 nm) and, failing that, B04 (665 nm) against the closest
    EMIT band: ``emit_band=closest_band(emit_wavelengths_nm, 842.0)`` with ``s2_band`` the index of B08 in the S2 stack."""
    torch = nat.require_gpu()
    as_torch = _is_torch(s2_scene)
    s = _to_device(torch, s2_scene, "s2_scene", (np.float32, np.uint16))
    if s.dim() != 3:
        raise ValueError(f"s2_scene must be (bands, H, W), got {tuple(s.shape)}")
    if s.stride(2) != 1:
        s = s.contiguous()
    if isinstance(emit_band, (int, np.integer)):
        e = _to_device(torch, emit_scene, "emit_scene", (np.float32,))
        if e.dim() != 3:
            raise ValueError(f"emit_scene must be (bands, H, W), got {tuple(e.shape)}")
        e = e[int(emit_band)]
    else:
        e = _to_device(torch, emit_band, "emit_band", (np.float32,))
    tp = match_windows(e, s[int(s2_band)], emit_mask=emit_mask, s2_nodata=s2_nodata, min_valid_frac=min_valid_frac,
                       min_score=min_score, window=window, step=step, factor=factor, max_shift=max_shift, max_points=max_points)
    sm = fit_shift_model(tp, model=model, reject_px=reject_px, min_points=min_points)
    warped = warp_scene(s, sm, nodata=s2_nodata, fill=fill, out=out)
    if as_torch:
        return CoregOutput(warped, sm, tp)
    return CoregOutput(warped.cpu().numpy(), sm._replace(params=sm.params.cpu().numpy()),
                       tp._replace(table=tp.table.cpu().numpy(), surface=tp.surface.cpu().numpy(), origins=tp.origins.cpu().numpy()))
