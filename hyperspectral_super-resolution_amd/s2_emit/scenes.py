"""Scene pairs -> tile pairs -> the fused 10 m scene: what stands before and behind ``fuse_tile_pairs``.

The reference gets its tile pairs from a co-registered EMIT scene (285, H, W) and an S2 scene (10, ~H f, ~W f):
``tiles_helpers/utils.py:223-305`` (``find_valid_paired_tiles``) walks a regular grid of ``tile`` x ``tile`` EMIT windows and their
``tile f`` x ``tile f`` S2 windows, marks the black pixels of every window (``is_black_mask``, :201-220: all bands close to
nodata, or all close to the masked value -0.01, or all zero) and keeps the windows whose black fraction is at most
``max_black_frac`` on both sides; ``save_tile_pair`` (:308-440) cuts them out and quantises EMIT to uint16.  Nothing in the
reference puts the fused tiles back onto the scene grid.

Here the scenes stay on the device (csrc/hsr_scene.hip):
    scan     ``hsr_scene_black_counts``: the black pixels of every window of a scene in one launch, with ``np.isclose``'s
             arithmetic; a wave stops reading bands when none of its pixels can still be black, so a clean scene costs about one
             band plane and only black regions read every band;
    gather   ``hsr_scene_gather_tiles``: the kept windows -> the (P, bands, th, tw) stacks ``fuse_tile_pairs`` takes, EMIT
             optionally in the reference's on-disk uint16 format (the bits of ``hsr_tile_encode_u16``);
    mosaic   ``hsr_scene_mosaic``: (P, T, th, tw) tile cubes -> the (T, H, W) scene grid, every byte written once;
    blend    ``hsr_scene_mosaic_blend``: the same for windows that overlap (``stride``), cross-faded by a tent weight, so that
             neighbouring windows' models leave no step at the window borders; still every byte written once.
``find_valid_paired_tiles`` has the reference's name, defaults and result (a list of dicts with rasterio's ``Window`` fields) on
arrays or device tensors instead of paths (rasterio is absent), and is the only function here that synchronises with the host:
once, to read the two small count arrays the selection needs.  ``fuse_scene`` chains find -> extract -> ``fuse_tile_pairs`` ->
mosaic in batches of tile pairs.
"""
from __future__ import annotations

import operator
from collections import namedtuple
from typing import Optional

import numpy as np

from . import _native as nat
from ._engine import _ptr, _stream
from .pairs import _DTYPES, _bands_index, _dtype_name, _stack_dev, fuse_tile_pairs
from .ridge import _is_torch, check_fit_features

Window = namedtuple("Window", "col_off row_off width height")            # rasterio.windows.Window's field names
SceneOutput = namedtuple("SceneOutput", "cube tiles n_train status bands")
_MAX_TILES_A_CALL = 65535                                               # hsr_scene_gather_tiles' bound on the windows of one call


def _int(v, what: str, lo: int = 1) -> int:
    if isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{what}={v!r}: must be an integer")
    try:
        i = operator.index(v)
    except TypeError:
        raise ValueError(f"{what}={v!r}: must be an integer") from None
    if i < lo:
        raise ValueError(f"{what}={i}: must be >= {lo}")
    return i


def _scene(x, what: str):
    """((bands, H, W), dtype name) of a scene."""
    if not hasattr(x, "shape") or not hasattr(x, "dtype"):
        raise ValueError(f"{what}: expected a (bands, H, W) array or tensor, got {type(x).__name__}")
    shape, dt = tuple(int(n) for n in x.shape), _dtype_name(x)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"{what}: expected a non-empty (bands, H, W) scene, got shape {shape}")
    if dt not in _DTYPES:
        raise ValueError(f"{what} is {dt}: must be uint16 or float32")
    return shape, dt


def _grid(h_e, w_e, h_s, w_s, tile, scale):
    h_e, w_e, h_s, w_s = (_int(v, n) for v, n in ((h_e, "h_e"), (w_e, "w_e"), (h_s, "h_s"), (w_s, "w_s")))
    tile, scale = _int(tile, "emit_tile_size"), _int(scale, "scale")
    if tile > h_e or tile > w_e:
        raise ValueError(f"emit_tile_size={tile}: larger than the {h_e} x {w_e} EMIT scene")
    return h_e, w_e, h_s, w_s, tile, scale


def _stride(stride, tile: int):
    """``stride`` of the window walk in EMIT pixels: None (the reference's walk: the windows do not overlap), or a divisor of
    ``tile``."""
    if stride is None:
        return None
    stride = _int(stride, "stride")
    if stride > tile or tile % stride:
        raise ValueError(f"stride={stride}: must divide emit_tile_size={tile}")
    return stride


def scene_windows(h_e: int, w_e: int, h_s: int, w_s: int, tile: int = 100, scale: int = 6, stride=None):
    """The (emit_window, s2_window) pairs of the reference's loop (:256-277), in its order: EMIT rows and columns over
    ``range(0, h - tile + 1, tile)``; a pair whose S2 window would pass the S2 bounds is skipped.  With ``stride`` (EMIT pixels,
    a divisor of ``tile``) the rows and columns run over ``range(0, h - tile + 1, stride)``: windows that overlap, for
    ``mosaic_tiles(blend="feather")``.  Host only."""
    h_e, w_e, h_s, w_s, tile, scale = _grid(h_e, w_e, h_s, w_s, tile, scale)
    step = _stride(stride, tile) or tile
    ts = tile * scale
    out = []
    for row_e in range(0, h_e - tile + 1, step):
        for col_e in range(0, w_e - tile + 1, step):
            row_s, col_s = row_e * scale, col_e * scale
            if row_s + ts > h_s or col_s + ts > w_s:
                continue
            out.append((Window(col_e, row_e, tile, tile), Window(col_s, row_s, ts, ts)))
    return out


def _limits(max_black_frac, max_tiles):
    try:
        frac = float(max_black_frac)
    except (TypeError, ValueError):
        raise ValueError(f"max_black_frac={max_black_frac!r}: must be a number") from None
    if frac != frac:
        raise ValueError("max_black_frac is NaN")
    return frac, None if max_tiles is None else _int(max_tiles, "max_tiles")


def _cloud_frac(max_cloud_frac) -> float:
    try:
        frac = float(max_cloud_frac)
    except (TypeError, ValueError):
        raise ValueError(f"max_cloud_frac={max_cloud_frac!r}: must be a number") from None
    if frac != frac:
        raise ValueError("max_cloud_frac is NaN")
    return frac


def select_tiles(windows, emit_counts, s2_counts, tile: int = 100, scale: int = 6, max_black_frac: float = 0.0, max_tiles=None,
                 stride=None, cloud_counts=None, max_cloud_frac: float = 1.0):
    """The reference's selection (:285-302) from the black counts of the window grids: ``emit_counts`` (h_e // tile, w_e // tile)
    and ``s2_counts`` (h_s // (tile scale), w_s // (tile scale)) integers, ``windows`` as ``scene_windows`` returns them.  A window
    pair is kept when ``count / size <= max_black_frac`` (float64) on both sides; ``idx`` counts the kept pairs and the walk stops
    at ``max_tiles``.  Returns the reference's list of dicts: idx, emit_window, s2_window, emit_black_frac, s2_black_frac.
    With ``stride`` the two arrays are grids of cells of ``stride`` (EMIT) and ``stride scale`` (S2) pixels, (h // cell, w // cell),
    the windows lie on the cell grid and a window's count is the integer sum of its ``(tile / stride)^2`` cells: the same
    fractions as from a count of the window itself.
    ``cloud_counts`` (None: nothing changes) is a third grid on the EMIT cells, the not-clear EMIT pixels of every cell
    (``coarse_clear_mask``'s ``win_counts``): a window is kept when it also has ``cloud cells / tile^2 <= max_cloud_frac``, inside
    the same walk, so ``max_tiles`` keeps its meaning, and its dict gains ``cloud_frac``.  Host only."""
    tile, scale = _int(tile, "emit_tile_size"), _int(scale, "scale")
    cell = _stride(stride, tile) or tile
    frac, max_tiles = _limits(max_black_frac, max_tiles)
    cc = None
    if cloud_counts is not None:
        cc = np.asarray(cloud_counts)
        if cc.ndim != 2 or cc.dtype.kind not in "iu":
            raise ValueError(f"select_tiles: cloud_counts is a 2-d integer array, got {cc.dtype} {cc.shape}")
        cloud_limit = _cloud_frac(max_cloud_frac)
    ec, sc = np.asarray(emit_counts), np.asarray(s2_counts)
    if ec.ndim != 2 or sc.ndim != 2 or ec.dtype.kind not in "iu" or sc.dtype.kind not in "iu":
        raise ValueError(f"select_tiles: the counts are 2-d integer arrays, got {ec.dtype} {ec.shape} and {sc.dtype} {sc.shape}")
    ts, cs, k = tile * scale, cell * scale, tile // cell
    tiles = []
    for w_emit, w_s2 in windows:
        ie, je, i_s, j_s = w_emit.row_off // cell, w_emit.col_off // cell, w_s2.row_off // cs, w_s2.col_off // cs
        if (w_emit.row_off % cell or w_emit.col_off % cell or w_s2.row_off % cs or w_s2.col_off % cs or
                not (0 <= ie <= ec.shape[0] - k and 0 <= je <= ec.shape[1] - k and 0 <= i_s <= sc.shape[0] - k and
                     0 <= j_s <= sc.shape[1] - k)):
            raise ValueError(f"select_tiles: {w_emit} / {w_s2} is not a window of the {ec.shape} / {sc.shape} count grids")
        emit_black_frac = int(ec[ie:ie + k, je:je + k].sum(dtype=np.int64)) / (tile * tile)
        s2_black_frac = int(sc[i_s:i_s + k, j_s:j_s + k].sum(dtype=np.int64)) / (ts * ts)
        if cc is not None:
            if not (ie <= cc.shape[0] - k and je <= cc.shape[1] - k):
                raise ValueError(f"select_tiles: {w_emit} is not a window of the {cc.shape} cloud count grid")
            cloud_frac = int(cc[ie:ie + k, je:je + k].sum(dtype=np.int64)) / (tile * tile)
            if cloud_frac > cloud_limit:
                continue
        if emit_black_frac <= frac and s2_black_frac <= frac:
            tiles.append({"idx": len(tiles), "emit_window": w_emit, "s2_window": w_s2, "emit_black_frac": emit_black_frac,
                          "s2_black_frac": s2_black_frac})
            if cc is not None:
                tiles[-1]["cloud_frac"] = cloud_frac
            if max_tiles is not None and len(tiles) >= max_tiles:
                break
    return tiles


_FindPlan = namedtuple("_FindPlan", "emit_shape emit_dtype s2_shape s2_dtype tile scale frac max_tiles windows stride")


def _plan_find(emit_scene, s2_scene, tile, scale, max_black_frac, max_tiles, stride=None) -> _FindPlan:
    """Every check of ``find_valid_paired_tiles`` that needs no GPU, and the window list."""
    (be, he, we), edt = _scene(emit_scene, "emit_scene")
    (bs, hs, ws), sdt = _scene(s2_scene, "s2_scene")
    _, _, _, _, tile, scale = _grid(he, we, hs, ws, tile, scale)
    stride = _stride(stride, tile)
    frac, max_tiles = _limits(max_black_frac, max_tiles)
    return _FindPlan((be, he, we), edt, (bs, hs, ws), sdt, tile, scale, frac, max_tiles,
                     scene_windows(he, we, hs, ws, tile, scale, stride), stride)


def _nodata(v, what: str):
    if v is None:
        return 0, 0.0
    try:
        return 1, float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what}={v!r}: must be a number or None") from None


def _scan(lib, st, scene, dtype: str, shape, th: int, tw: int, nodata, masked_val, nodata_atol, zero_atol, counts):
    bands, h, w = shape
    use, nd = nodata
    nat.check(lib.hsr_scene_black_counts(_ptr(scene), _DTYPES[dtype], bands, h, w, th, tw, use, nd, float(masked_val),
                                         float(nodata_atol), float(zero_atol), _ptr(counts), st), "hsr_scene_black_counts")


def _find(lib, torch, dev, plan: _FindPlan, E, S, emit_nodata, s2_nodata, masked_val, nodata_atol, zero_atol, cloud=None):
    """``cloud``: None, or (grid shape, launch, max_cloud_frac) - a third count grid on the EMIT cells that ``launch(segment)``
    fills on the current stream; it rides in the same copy to the host as the two black-count grids."""
    if not plan.windows:
        return []
    (_, he, we), (_, hs, ws) = plan.emit_shape, plan.s2_shape
    ce = plan.tile if plan.stride is None else plan.stride               # the cell of the count grids: the window, or the stride
    cs = ce * plan.scale
    ne, ns = (he // ce, we // ce), (hs // cs, ws // cs)
    nc = cloud[0] if cloud is not None else (0, 0)
    n_black = ne[0] * ne[1] + ns[0] * ns[1]
    counts = torch.empty(n_black + nc[0] * nc[1], dtype=torch.int32, device=dev)   # every grid: one copy to the host
    st = _stream(torch)
    _scan(lib, st, E, plan.emit_dtype, plan.emit_shape, ce, ce, emit_nodata, masked_val, nodata_atol, zero_atol, counts)
    _scan(lib, st, S, plan.s2_dtype, plan.s2_shape, cs, cs, s2_nodata, masked_val, nodata_atol, zero_atol,
          counts[ne[0] * ne[1]:])
    if cloud is not None:
        cloud[1](counts[n_black:])
    host = counts.cpu().numpy()                        # THE host synchronisation: a few hundred int32
    clouds = dict(cloud_counts=host[n_black:].reshape(nc), max_cloud_frac=cloud[2]) if cloud is not None else {}
    return select_tiles(plan.windows, host[:ne[0] * ne[1]].reshape(ne), host[ne[0] * ne[1]:n_black].reshape(ns), plan.tile, plan.scale,
                        plan.frac, plan.max_tiles, plan.stride, **clouds)


def find_valid_paired_tiles(emit_scene, s2_scene, emit_tile_size: int = 100, scale: int = 6, max_black_frac: float = 0.0,
                            max_tiles=None, *, emit_nodata: Optional[float] = None, s2_nodata: Optional[float] = None,
                            masked_val: float = -0.01, nodata_atol: float = 1e-3, zero_atol: float = 1e-6, stride=None):
    """The reference's ``find_valid_paired_tiles`` (:223-305) on scenes in memory: emit_scene (bands, h, w) and s2_scene
    (nb, ~h scale, ~w scale), float32 or uint16, device tensors or NumPy arrays (copied to the device once).  ``emit_nodata`` /
    ``s2_nodata`` stand for the datasets' nodata attributes.  Two scan launches on the current stream, then ONE host
    synchronisation - the two count arrays, one int32 per window - and ``select_tiles`` on the host.  Returns the reference's list
    of dicts (``Window`` has rasterio's fields).  ``stride`` (EMIT pixels, a divisor of ``emit_tile_size``) walks windows that
    overlap (``scene_windows``): the same two launches count cells of ``stride`` pixels, one int32 per cell, and
    ``select_tiles`` sums a window's cells."""
    plan = _plan_find(emit_scene, s2_scene, emit_tile_size, scale, max_black_frac, max_tiles, stride)
    end, snd = _nodata(emit_nodata, "emit_nodata"), _nodata(s2_nodata, "s2_nodata")
    if not plan.windows:
        return []
    torch = nat.require_gpu()
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    return _find(lib, torch, dev, plan, _stack_dev(emit_scene, torch, dev), _stack_dev(s2_scene, torch, dev), end, snd, masked_val,
                 nodata_atol, zero_atol)


def _origins(tiles, key: str, shape):
    """(P, 2) int32 (row, col) origins and the common (height, width) of the ``key`` windows of ``tiles``, all inside the scene."""
    _, h, w = shape
    if not isinstance(tiles, (list, tuple)) or not tiles:
        raise ValueError("tiles: a non-empty list of tile dicts (find_valid_paired_tiles' result)")
    if len(tiles) > _MAX_TILES_A_CALL:
        raise ValueError(f"{len(tiles)} tiles: at most {_MAX_TILES_A_CALL} a call")
    wins = []
    for t in tiles:
        try:
            win = t[key]
            wins.append(tuple(operator.index(v) for v in (win.row_off, win.col_off, win.height, win.width)))
        except (KeyError, TypeError, AttributeError):
            raise ValueError(f"tiles: every tile is a dict with a {key!r} Window of integers") from None
    sizes = {(ht, wd) for _, _, ht, wd in wins}
    if len(sizes) != 1:
        raise ValueError(f"{key}: the windows of a call must share one size, got {sorted(sizes)}")
    th, tw = sizes.pop()
    if th < 1 or tw < 1:
        raise ValueError(f"{key}: empty window {th} x {tw}")
    for r, c, _, _ in wins:
        if r < 0 or c < 0 or r + th > h or c + tw > w:
            raise ValueError(f"{key}: window at row {r}, col {c} of {th} x {tw} is outside the {h} x {w} scene")
    return np.array([(r, c) for r, c, _, _ in wins], dtype=np.int32).reshape(-1, 2), th, tw


def _gather(lib, torch, st, scene, dtype: str, shape, origins: np.ndarray, th: int, tw: int, encode=None):
    """The windows at ``origins`` of a device scene -> (P, bands, th, tw); encode = (scale, has_src_nodata, src_nodata, nodata_u16)
    quantises a float32 scene to uint16.  ``origins``: (P, 2) int32, a host array (copied) or a device tensor.  uint16 stacks are
    returned as torch.uint16 views."""
    bands, h, w = shape
    P = len(origins)
    org = origins if _is_torch(origins) else torch.from_numpy(np.ascontiguousarray(origins, dtype=np.int32)).to(scene.device)
    out_u16 = encode is not None or dtype == "uint16"
    out = torch.empty((P, bands, th, tw), dtype=torch.int16 if out_u16 else torch.float32, device=scene.device)
    scale, has_nd, nd, nd16 = encode if encode is not None else (1.0, 0, 0.0, 65535)
    nat.check(lib.hsr_scene_gather_tiles(_ptr(scene), _DTYPES[dtype], bands, h, w, _ptr(org), P, th, tw, int(encode is not None),
                                         scale, has_nd, nd, nd16, _ptr(out), st), "hsr_scene_gather_tiles")
    return out.view(torch.uint16) if out_u16 else out


def _plan_extract(emit_scene, s2_scene, tiles, emit_uint16, emit_scale, emit_nodata, emit_nodata_u16):
    eshape, edt = _scene(emit_scene, "emit_scene")
    sshape, sdt = _scene(s2_scene, "s2_scene")
    eo, eth, etw = _origins(tiles, "emit_window", eshape)
    so, sth, stw = _origins(tiles, "s2_window", sshape)
    encode = None
    if emit_uint16 and edt == "float32":
        has_nd, nd = _nodata(emit_nodata, "emit_nodata")
        nd16 = _int(emit_nodata_u16, "emit_nodata_u16")
        if nd16 > 65535:
            raise ValueError(f"emit_nodata_u16={nd16}: must lie in [1, 65535]")
        encode = (float(emit_scale), has_nd, nd, nd16)
    return (eshape, edt, eo, eth, etw), (sshape, sdt, so, sth, stw), encode


def extract_tile_pairs(emit_scene, s2_scene, tiles, *, emit_uint16: bool = True, emit_scale: float = 10000.0,
                       emit_nodata: Optional[float] = None, emit_nodata_u16: int = 65535):
    """``save_tile_pair`` (:308-440) without the files: the windows of ``tiles`` (any list of dicts with ``emit_window`` and
    ``s2_window``; origins need not lie on a grid, duplicates are allowed) cut out of the two scenes -> ``(emits, s2s)``, device
    stacks (P, bands, th, tw) ready for ``fuse_tile_pairs``.  S2 keeps its dtype and bits.  A float32 EMIT scene is quantised to the
    reference's uint16 format with ``emit_uint16`` (:362-374: ``emit_scale``, the dataset's ``emit_nodata``, ``emit_nodata_u16``;
    the bits of ``hsr_tile_encode_u16``) and copied as it is without; a uint16 EMIT scene is in that format already and is copied
    as it is.  Two launches on the current stream, no host synchronisation."""
    e, s, encode = _plan_extract(emit_scene, s2_scene, tiles, emit_uint16, emit_scale, emit_nodata, emit_nodata_u16)
    torch = nat.require_gpu()
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = _stream(torch)
    E, S = _stack_dev(emit_scene, torch, dev), _stack_dev(s2_scene, torch, dev)
    return (_gather(lib, torch, st, E, e[1], e[0], e[2], e[3], e[4], encode),
            _gather(lib, torch, st, S, s[1], s[0], s[2], s[3], s[4]))


def _mosaic_windows(cube_shape, cube_dtype: str, tiles, scene_hw):
    """The checks the two mosaics share -> ((P, 2) int32 origins of the ``s2_window``s, H, W, th, tw)."""
    try:
        H, W = (_int(v, "scene_hw") for v in scene_hw)
    except TypeError:
        raise ValueError(f"scene_hw={scene_hw!r}: the (H, W) of the output") from None
    if len(cube_shape) != 4 or min(cube_shape) < 1 or cube_dtype != "float32":
        raise ValueError(f"cubes: expected a non-empty float32 (P, T, th, tw) stack, got {cube_dtype} {tuple(cube_shape)}")
    P, _, th, tw = cube_shape
    if not isinstance(tiles, (list, tuple)) or len(tiles) != P:
        raise ValueError(f"tiles: {P} cubes need a list of {P} tile dicts")
    org, wh, ww = _origins(tiles, "s2_window", (1, H, W))
    if (wh, ww) != (th, tw):
        raise ValueError(f"the s2_windows are {wh} x {ww} but the cubes are {th} x {tw}")
    return org, H, W, th, tw


def _plan_mosaic(cube_shape, cube_dtype: str, tiles, scene_hw):
    """The (ny, nx) slot grid of ``mosaic_tiles`` (cube index per window, -1 elsewhere) and (H, W, th, tw)."""
    org, H, W, th, tw = _mosaic_windows(cube_shape, cube_dtype, tiles, scene_hw)
    slot = np.full((H // th, W // tw), -1, dtype=np.int32)
    for k, (r, c) in enumerate(org):
        if r % th or c % tw:
            raise ValueError(f"s2_window at row {r}, col {c} is not on the {th} x {tw} grid")
        if slot[r // th, c // tw] != -1:
            raise ValueError(f"two tiles share the s2_window at row {r}, col {c}")
        slot[r // th, c // tw] = k
    return slot, H, W, th, tw


def _mosaic_into(lib, torch, st, cubes, out, slot, th: int, tw: int, fill: float, fill_rest: bool):
    """``slot``: (ny, nx) int32, a host array (copied) or a device tensor."""
    T, H, W = out.shape
    sl = slot if _is_torch(slot) else torch.from_numpy(np.ascontiguousarray(slot, dtype=np.int32)).to(out.device)
    nat.check(lib.hsr_scene_mosaic(_ptr(cubes), cubes.shape[0], T, th, tw, _ptr(out), H, W, _ptr(sl), slot.shape[0], slot.shape[1],
                                   fill, int(fill_rest), st), "hsr_scene_mosaic")


_BLEND_MAX = 16                        # hsr_scene_mosaic_blend: the windows over one pixel, at most
_BLEND_WEIGHTS = 1 << 24               # ... and what their weights may add up to: an exact float32 integer


def _check_blend(ky: int, kx: int, th: int, tw: int):
    """hsr_scene_mosaic_blend's two limits for ``ky`` x ``kx`` windows of ``th`` x ``tw`` over a pixel, as ValueErrors."""
    K = ky * kx
    if K > _BLEND_MAX:
        raise ValueError(f"blend: {ky} x {kx} = {K} windows of {th} x {tw} overlap in a pixel, at most {_BLEND_MAX}: use a larger "
                         "stride")
    wsum = K * ((th + 1) // 2) * ((tw + 1) // 2)
    if wsum > _BLEND_WEIGHTS:
        raise ValueError(f"blend: the weights of a pixel can add up to {K} x ceil({th} / 2) x ceil({tw} / 2) = {wsum} > 2^24, no "
                         "exact float32 integer: use smaller tiles or a larger stride")


def _plan_blend(cube_shape, cube_dtype: str, tiles, scene_hw):
    """``mosaic_tiles(blend="feather")`` on the host: the lattice pitch (sy, sx) - the largest that divides the tile and every
    origin - and the (ny, nx) start table (the cube whose window starts at lattice cell (j, i), -1 none; one row and column per
    cell at which a window inside the output can start) -> (start, sy, sx, H, W, th, tw).  Raises before any GPU work."""
    org, H, W, th, tw = _mosaic_windows(cube_shape, cube_dtype, tiles, scene_hw)
    sy = int(np.gcd.reduce(org[:, 0].astype(np.int64), initial=th))
    sx = int(np.gcd.reduce(org[:, 1].astype(np.int64), initial=tw))
    _check_blend(th // sy, tw // sx, th, tw)
    start = np.full(((H - th) // sy + 1, (W - tw) // sx + 1), -1, dtype=np.int32)
    for k, (r, c) in enumerate(org):
        if start[r // sy, c // sx] != -1:
            raise ValueError(f"two tiles share the s2_window at row {r}, col {c}")
        start[r // sy, c // sx] = k
    return start, sy, sx, H, W, th, tw


def _blend_into(lib, torch, st, cubes, out, start, sy: int, sx: int, th: int, tw: int, fill: float):
    """``start``: (ny, nx) int32, a host array (copied) or a device tensor."""
    T, H, W = out.shape
    sd = start if _is_torch(start) else torch.from_numpy(np.ascontiguousarray(start, dtype=np.int32)).to(out.device)
    nat.check(lib.hsr_scene_mosaic_blend(_ptr(cubes), cubes.shape[0], T, th, tw, sy, sx, _ptr(sd), start.shape[0], start.shape[1],
                                         _ptr(out), H, W, fill, st), "hsr_scene_mosaic_blend")


def _blend_mode(blend):
    if blend is not None and blend != "feather":
        raise ValueError(f"blend={blend!r}: None or 'feather'")
    return blend


def mosaic_tiles(cubes, tiles, scene_hw, *, fill: float = float("nan"), blend=None):
    """cubes (P, T, th, tw) float32 (``fuse_tile_pairs(...).cube``; a device tensor or an array) -> the (T, H, W) device image on
    the grid of the tiles' ``s2_window``s: window i holds the bits of ``cubes[i]``, every other window and the strips right of and
    below the grid hold ``fill``.  One launch that writes every byte of the output once; no host synchronisation.

    ``blend="feather"``: the windows may overlap and need lie on no grid of tiles.  A pixel is the mean of the cubes over it,
    each weighted by the tent ``min(r + 1, th - r) min(c + 1, tw - c)`` of its own position (r, c) in that cube, NaN samples
    left out (``hsr_scene_mosaic_blend``, include/hsr.h): the bits of the one cube where one covers it, ``fill`` where none
    does, and the same result whatever the order of the tiles.  At most 16 windows may overlap in a pixel; two tiles with the
    same origin are refused.  Still one launch, every byte written once."""
    if _blend_mode(blend) is None:
        slot, H, W, th, tw = _plan_mosaic(tuple(cubes.shape), _dtype_name(cubes), tiles, scene_hw)
    else:
        start, sy, sx, H, W, th, tw = _plan_blend(tuple(cubes.shape), _dtype_name(cubes), tiles, scene_hw)
    torch = nat.require_gpu()
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    C = (cubes if _is_torch(cubes) else torch.from_numpy(np.ascontiguousarray(cubes))).to(dev).contiguous()
    out = torch.empty((C.shape[1], H, W), dtype=torch.float32, device=dev)
    if blend is None:
        _mosaic_into(lib, torch, _stream(torch), C, out, slot, th, tw, float(fill), True)
    else:
        _blend_into(lib, torch, _stream(torch), C, out, start, sy, sx, th, tw, float(fill))
    return out


def _blend_stack_bytes(ntiles: int, T: int, th: int, tw: int) -> int:
    """The bytes of the (P, T, th, tw) float32 stack ``fuse_scene`` keeps until its one blend launch."""
    return 4 * ntiles * T * th * tw


def _check_blend_stack(torch, dev, ntiles: int, T: int, th: int, tw: int):
    need = _blend_stack_bytes(ntiles, T, th, tw)
    free, _ = torch.cuda.mem_get_info(dev)
    free += torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)       # what torch's allocator holds and can reuse
    if need > free:
        raise ValueError(f"fuse_scene: the stack of {ntiles} cubes of {T} x {th} x {tw} float32 needs {need} bytes, {free} are "
                         "free on the device: use fewer bands, a larger stride or max_tiles")


def _plan_fuse(emit_scene, s2_scene, tile, factor, max_black_frac, max_tiles, batch, bands, degree, stride=None, blend=None):
    """Every check of ``fuse_scene`` that needs no GPU -> (plan, batch, band indices, feather).  feather: the cubes are blended,
    which an explicit ``blend="feather"`` or windows that overlap (``stride < tile``) ask for."""
    plan = _plan_find(emit_scene, s2_scene, tile, factor, max_black_frac, max_tiles, stride)
    feather = _blend_mode(blend) is not None or (plan.stride is not None and plan.stride < plan.tile)
    if feather:
        k = plan.tile // (plan.stride or plan.tile)
        _check_blend(k, k, plan.tile * plan.scale, plan.tile * plan.scale)
    batch = _int(batch, "batch")
    if batch > _MAX_TILES_A_CALL:
        raise ValueError(f"batch={batch}: at most {_MAX_TILES_A_CALL} pairs a batch")
    if not 1 <= int(degree) <= 3:
        raise ValueError(f"degree={degree}: 1, 2 or 3")
    if not 1 <= plan.s2_shape[0] <= nat.HSR_MAX_BANDS:
        raise ValueError(f"s2_scene has {plan.s2_shape[0]} bands: 1 .. {nat.HSR_MAX_BANDS} supported")
    check_fit_features(plan.s2_shape[0], degree)
    return plan, batch, _bands_index(bands, plan.emit_shape[0]), feather


def fuse_scene(emit_scene, s2_scene, *, tile: int = 100, factor: int = 6, max_black_frac: float = 0.0, max_tiles=None,
               batch: int = 64, bands=32, degree: int = 3, alpha: float = 1.0, emit_nodata: Optional[float] = None,
               s2_nodata: Optional[float] = None, eps: float = 1e-4, stride=None, blend=None) -> SceneOutput:
    """Two co-registered scenes -> the fused 10 m scene: ``find_valid_paired_tiles`` (``emit_tile_size=tile``, ``scale=factor``),
    then per batch of ``batch`` kept pairs the gather of both sides (EMIT is not quantised), ``fuse_tile_pairs`` (``bands``,
    ``degree``, ``alpha``, ``factor``, the nodata values, ``eps``) and the mosaic of its cubes into one preallocated cube.

    Returns ``SceneOutput(cube, tiles, n_train, status, bands)``: cube (T, H_s2, W_s2) float32 on the device - inside the
    ``s2_window`` of tile i the bits of ``fuse_tile_pairs`` on that extracted pair, NaN in rejected windows and right of and below
    the window grid; every byte is written once (the first batch's mosaic fills, the others leave alone what they do not own);
    tiles, the list ``find_valid_paired_tiles`` returns; n_train (P,) int64 and status (P,) int32 of the pairs in tile order; bands
    (T,) the EMIT band indices.  No kept window gives an all-NaN cube and empty lists without a launch on an empty grid.  The one
    host synchronisation is ``find_valid_paired_tiles``'.

    ``stride`` (EMIT pixels, a divisor of ``tile``; None: ``tile``) walks windows that overlap, and with ``stride < tile`` - or
    with an explicit ``blend="feather"`` - the cubes are cross-faded instead of butted together, which takes the step out of the
    window borders: find with ``stride``, per batch gather -> ``fuse_tile_pairs`` -> a copy of its cubes into one preallocated
    (P, T, th, tw) stack, and ONE ``hsr_scene_mosaic_blend`` launch at the end, so ``cube`` holds the bits of
    ``mosaic_tiles(..., blend="feather")`` on the cubes of all kept pairs and NaN where no kept window reaches.  ``tile / stride``
    is at most 4 (16 windows over a pixel).  The stack costs ``P T th tw 4`` bytes on top of the cube (25 GB for a 1242 x 1280
    EMIT scene at half stride and 32 bands); it is checked against the free device memory after the find and a ValueError says
    what is needed.  Blending strip by strip to bound that memory is not implemented.  ``n_train`` and ``status`` are per kept
    window in tile order, and the one host synchronisation is still the find.

    ``report``, ``validate``, ``train_mask`` and ``pool`` of ``fuse_tile_pairs`` are not forwarded: callers who need them chain
    ``find_valid_paired_tiles``, ``extract_tile_pairs``, ``fuse_tile_pairs`` and ``mosaic_tiles`` themselves;
    ``s2_emit.clouds.fuse_scene_clear`` forwards a training mask of its own, from the scene classification layer."""
    return _fuse_scene(emit_scene, s2_scene, None, tile, factor, max_black_frac, max_tiles, batch, bands, degree, alpha, emit_nodata,
                       s2_nodata, eps, stride, blend)


def _fuse_scene(emit_scene, s2_scene, clouds, tile, factor, max_black_frac, max_tiles, batch, bands, degree, alpha, emit_nodata,
                s2_nodata, eps, stride, blend) -> SceneOutput:
    """The loop of ``fuse_scene``.  ``clouds``: None, or the cloud-aware pieces of ``fuse_scene_clear`` (s2_emit/clouds.py:
    ``_Clouds``), each where it belongs - ``check(plan)`` before the GPU is asked for, ``find(...)`` a third count grid for the
    find, ``train_mask(...)`` the clear cells of a batch's windows, ``finish(...)`` on the finished cube."""
    plan, batch, idx, feather = _plan_fuse(emit_scene, s2_scene, tile, factor, max_black_frac, max_tiles, batch, bands, degree,
                                           stride, blend)
    end, snd = _nodata(emit_nodata, "emit_nodata"), _nodata(s2_nodata, "s2_nodata")
    if clouds is not None:
        clouds.check(plan)
    torch = nat.require_gpu()
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    E, S = _stack_dev(emit_scene, torch, dev), _stack_dev(s2_scene, torch, dev)
    st = _stream(torch)
    tiles = _find(lib, torch, dev, plan, E, S, end, snd, -0.01, 1e-3, 1e-6,
                  clouds.find(lib, torch, dev, st, plan) if clouds is not None else None)
    (_, hs, ws), T, nan = plan.s2_shape, len(idx), float("nan")
    if not tiles:
        return SceneOutput(torch.full((T, hs, ws), nan, dtype=torch.float32, device=dev), [],
                           torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev), idx)
    eo, eth, etw = _origins(tiles, "emit_window", plan.emit_shape)
    so, sth, stw = _origins(tiles, "s2_window", plan.s2_shape)
    if feather:                                                          # every cube is kept until the one blend launch
        start, sy, sx, *_ = _plan_blend((len(tiles), T, sth, stw), "float32", tiles, (hs, ws))
        _check_blend_stack(torch, dev, len(tiles), T, sth, stw)
        stack = torch.empty((len(tiles), T, sth, stw), dtype=torch.float32, device=dev)
    else:
        owner = np.full((hs // sth, ws // stw), -1, dtype=np.int64)      # the tile of every S2 window, -1: rejected
        owner[so[:, 0] // sth, so[:, 1] // stw] = np.arange(len(tiles))
    cube = torch.empty((T, hs, ws), dtype=torch.float32, device=dev)
    n_train, status = [], []
    for b0 in range(0, len(tiles), batch):
        b1 = min(b0 + batch, len(tiles))
        emits = _gather(lib, torch, st, E, plan.emit_dtype, plan.emit_shape, eo[b0:b1], eth, etw)
        s2s = _gather(lib, torch, st, S, plan.s2_dtype, plan.s2_shape, so[b0:b1], sth, stw)
        masks = dict(train_mask=clouds.train_mask(lib, torch, st, eo[b0:b1], eth, etw)) if clouds is not None else {}
        out = fuse_tile_pairs(emits, s2s, bands=idx, degree=degree, alpha=alpha, factor=plan.scale, emit_nodata=emit_nodata,
                              s2_nodata=s2_nodata, eps=eps, **masks)
        if feather:
            stack[b0:b1].copy_(out.cube)
        else:
            slot = np.full(owner.shape, -2, dtype=np.int32)              # -2: another batch's window
            if b0 == 0:
                slot[owner < 0] = -1                                     # the first launch fills what no batch owns
            own = (owner >= b0) & (owner < b1)
            slot[own] = owner[own] - b0
            _mosaic_into(lib, torch, st, out.cube, cube, slot, sth, stw, nan, b0 == 0)
        n_train.append(out.n_train)
        status.append(out.status)
    if feather:
        _blend_into(lib, torch, st, stack, cube, start, sy, sx, sth, stw, nan)
    if clouds is not None:
        clouds.finish(lib, torch, st, cube)
    return SceneOutput(cube, tiles, torch.cat(n_train), torch.cat(status), idx)
