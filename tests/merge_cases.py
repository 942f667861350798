"""The scene-merging family (include/hsr_merge.h, csrc/hsr_merge.hip) for the tests: the NumPy statement of the header's definition,
the case tables and a mirror of the instance choice.  Not a test module itself; everything here is NumPy.

Shared by tests/test_merge_host.py (the planner, hsr_merge_grid, the host twin and what the tables claim - no GPU),
tests/test_gpu_merge_instances.py (every row through the C ABI with the launch record), tests/test_gpu_merge.py (the Python entry
points and the chain ortho_scene + merge_scenes) and tests/test_gpu_merge_capture.py.

No fixture can be frozen from the reference: merge_emit (EMIT_data/emit_tools.py:631-704) needs rioxarray, rasterio and xarray, which
are not installed, so there is no run of the reference's own code behind these numbers.  merge_ref RESTATES rasterio's copy_first -
per element, `dest empty and source not empty` - as the header gives it: a loop over the sources with np.where on the empty test,
on uint32 bit patterns, so that NaN payloads compare.  The value of a cell of one source is the ortho rule, restated as in
tests/ortho_cases.py (ortho_ref).  merge_grid_ref is the header's grid in float64.  rasterio's window rounding is not claimed.

Mirrors of the kernels' constants: ortho_merge keeps hsr_ortho_glt's workgroup of PX = 64 consecutive output pixels; a workgroup of
merge_scenes owns RUN = 1024 elements of one output row, a thread the 4 that share a 16-byte line of the output.  Mirror of the
instance choice:
    hsr_ortho_merge    layout 0: ortho_merge_bip_kernel<kMask, kVec>, kMask = some source has a quality or band mask, kVec = bands %
                       4 == 0 and the output and EVERY swath start on 16 bytes; layout 1: ortho_merge_bsq_kernel<kMask>.
    hsr_merge_scenes   merge_scenes_kernel, then merge_source_kernel when a source plane is asked for.
Pointer alignments are byte offsets from a 256-byte boundary, which is where the tests' buffers start.
"""
import functools

import numpy as np

import ortho_cases as oc

PX, RUN, LINE, MAX_SOURCES, MAX_BANDS, NO_SOURCE = oc.PX, 1024, 4, 8, 512, 255
INSTANCE_COUNT = 8
BIP, BSQ = oc.BIP, oc.BSQ
NODATA = -9999.0


def _b(flag):
    return "true" if flag else "false"


def ortho_merge_instance(layout, bands, mask, swath_offs=(0,), out_off=0):
    if layout == BIP:
        vec = bands % 4 == 0 and out_off % 16 == 0 and all(o % 16 == 0 for o in swath_offs)
        return f"ortho_merge_bip_kernel<{_b(mask)}, {_b(vec)}>"
    return f"ortho_merge_bsq_kernel<{_b(mask)}>"


def merge_scenes_instances(source):
    return ["merge_scenes_kernel"] + (["merge_source_kernel"] if source else [])


def all_instances():
    return [ortho_merge_instance(BIP, b, m) for m in (False, True) for b in (3, 4)] + [ortho_merge_instance(BSQ, 3, m) for m in (False, True)] \
        + merge_scenes_instances(True)


# =============================================================================================================================
# the statement
# =============================================================================================================================
def is_empty(v, nodata, nan_is_nodata=False):
    """v float32 array: v == nodata in float32 comparison; with nan_is_nodata a NaN too."""
    with np.errstate(invalid="ignore"):
        e = v == np.float32(nodata)
    return e | np.isnan(v) if nan_is_nodata else e


def merge_ref(scenes, offsets, shape, nodata=NODATA, nan_is_nodata=False):
    """scenes: float32 (h_k, w_k, bands) each; offsets (off_y, off_x) each; shape (H, W) -> (bits uint32 (H, W, bands), source uint8
    (H, W)).  The first rule, per element."""
    H, W = shape
    bands = scenes[0].shape[2]
    out = np.full((H, W, bands), oc.f32_bits(nodata), np.uint32)
    filled = np.zeros((H, W, bands), bool)
    source = np.full((H, W), NO_SOURCE, np.uint8)
    for k, (s, (oy, ox)) in enumerate(zip(scenes, offsets)):
        h, w = s.shape[:2]
        y0, y1, x0, x1 = max(oy, 0), min(oy + h, H), max(ox, 0), min(ox + w, W)
        if y0 >= y1 or x0 >= x1:
            continue
        sub = np.ascontiguousarray(s[y0 - oy:y1 - oy, x0 - ox:x1 - ox], np.float32)
        take = ~filled[y0:y1, x0:x1] & ~is_empty(sub, nodata, nan_is_nodata)
        out[y0:y1, x0:x1] = np.where(take, sub.view(np.uint32), out[y0:y1, x0:x1])
        filled[y0:y1, x0:x1] |= take
        first = take.any(axis=-1) & (source[y0:y1, x0:x1] == NO_SOURCE)
        source[y0:y1, x0:x1] = np.where(first, np.uint8(k), source[y0:y1, x0:x1])
    return out, source


def dropped_inside(glt, rows, cols, offset, shape, nodata=0):
    """The entries of a GLT placed at `offset` that lie inside the output and point outside the swath (the ortho rule, step 2)."""
    g = glt.astype(np.int64)
    valid = (g[..., 0] != nodata) & (g[..., 1] != nodata)
    sx, sy = g[..., 0] - 1, g[..., 1] - 1
    inside = (sx >= 0) & (sx < cols) & (sy >= 0) & (sy < rows)
    oy, ox = offset
    yy, xx = np.mgrid[0:g.shape[0], 0:g.shape[1]]
    seen = (yy + oy >= 0) & (yy + oy < shape[0]) & (xx + ox >= 0) & (xx + ox < shape[1])
    return int((valid & ~inside & seen).sum())


def merge_grid_ref(geotransforms, shapes, bounds=None):
    """-> (geotransform, (H, W), offsets, residuals) in float64, operation by operation as the header writes them."""
    g = np.asarray(geotransforms, np.float64)
    dx, dy = g[0, 1], g[0, 5]
    if bounds is None:
        X0 = g[:, 0].min()
        Y0 = g[:, 3].max() if dy < 0 else g[:, 3].min()
    else:
        left, bottom, right, top = (np.float64(v) for v in bounds)
        X0, Y0 = left, (top if dy < 0 else bottom)
    fx, fy = (g[:, 0] - X0) / dx, (g[:, 3] - Y0) / dy
    ox, oy = np.floor(fx + 0.5), np.floor(fy + 0.5)
    if bounds is None:
        W = max(int(o) + s[1] for o, s in zip(ox, shapes))
        H = max(int(o) + s[0] for o, s in zip(oy, shapes))
    else:
        W = max(1, int(np.floor((right - left) / dx + 0.5)))
        H = max(1, int(np.floor((top - bottom) / abs(dy) + 0.5)))
    return ((float(X0), float(dx), 0.0, float(Y0), 0.0, float(dy)), (H, W), tuple((int(a), int(b)) for a, b in zip(oy, ox)),
            tuple((float(a - c), float(b - d)) for a, b, c, d in zip(fy, fx, oy, ox)))


# =============================================================================================================================
# the case table
# =============================================================================================================================
def S(gh, gw, oy, ox, grid="mixed", q=False, bm=0, plant=False, off=0):
    """One source: a GLT grid of gh x gw at (oy, ox); grid: one of ortho_cases.glt_of's kinds; q / bm: a quality / band mask; plant:
    -9999 written into bands of the swath; off: the swath's (and, for merge_scenes, the scene's) base past a 256-byte boundary."""
    return dict(gh=gh, gw=gw, oy=oy, ox=ox, grid=grid, q=q, bm=bm, plant=plant, off=off)


# name -> dict(bands, layout, H, W, sources, nodata, masked, out_off, nan (merge_scenes only: nan_is_nodata), count (dropped given))
ROWS = {}


def _row(name, bands, layout, H, W, sources, *, nodata=NODATA, masked=NODATA, out_off=0, nan=False, count=True):
    assert name not in ROWS and 1 <= len(sources) <= MAX_SOURCES, name
    ROWS[name] = dict(bands=bands, layout=layout, H=H, W=W, sources=sources, nodata=nodata, masked=masked, out_off=out_off, nan=nan,
                      count=count)


def _ln(layout):
    return "bip" if layout == BIP else "bsq"


# output widths against the 64-pixel workgroup, heights 1 and 3: two sources that overlap in the middle third
for _layout in (BIP, BSQ):
    for _wi, _w in enumerate((1, 63, 64, 65, 129)):
        _h = 3 if _wi % 2 else 1
        _a, _o = max(1, 2 * _w // 3), _w // 3
        _row(f"w{_w}-{_ln(_layout)}", 5, _layout, _h, _w, [S(_h, _a, 0, 0, q=_wi % 2 == 0), S(_h, _w - _o, 0, _o, bm=_wi % 2)])
# band counts against the float4 runs, the tail and the bsq tile limit; bases on and off 16 bytes
_OFFS = ((0, 0, 0), (4, 8, 12), (16, 0, 32), (0, 16, 4), (8, 8, 8), (0, 0, 16), (12, 4, 0))            # swath 0, swath 1, output
for _layout in (BIP, BSQ):
    for _bi, _bands in enumerate((1, 3, 4, 5, 8, 285, 512)):
        _s0, _s1, _oo = _OFFS[_bi] if _layout == BIP else _OFFS[(_bi + 3) % 7]
        _h = 1 if _bands == 512 else 3
        _row(f"b{_bands}-{_ln(_layout)}", _bands, _layout, _h, PX + 1, [S(_h, 45, 0, 0, q=_bi % 2 == 1, bm=int(_bi % 3 == 0), off=_s0),
                                                                       S(_h, 40, 0, 25, bm=int(_bi % 3 == 1), off=_s1)], out_off=_oo)
    # every base on 16 bytes: the aligned float4 path (bip), with and without masks
    _row(f"vec-b8-{_ln(_layout)}", 8, _layout, 3, PX + 1, [S(3, 45, 0, 0, off=16), S(3, 40, 0, 25, off=32)], out_off=48)
    _row(f"vec-mask-b4-{_ln(_layout)}", 4, _layout, 3, PX + 1, [S(3, 45, 0, 0, q=True, off=16), S(3, 40, 0, 25, bm=1)], out_off=16)
    _row(f"novec-b4-{_ln(_layout)}", 4, _layout, 3, PX + 1, [S(3, 45, 0, 0), S(3, 40, 0, 25, off=4)])
    _row(f"nomask-b3-{_ln(_layout)}", 3, _layout, 3, PX + 1, [S(3, 45, 0, 0), S(3, 40, 0, 25)])
    # N = 1 (the identity with hsr_ortho_glt), 3 and 8
    _row(f"n1-identity-{_ln(_layout)}", 5, _layout, 3, PX + 6, [S(3, PX + 6, 0, 0, q=True, bm=1)])
    _row(f"n1-b285-{_ln(_layout)}", 285, _layout, 2, PX + 1, [S(2, PX + 1, 0, 0, bm=1)])
    _row(f"n3-dropped-{_ln(_layout)}", 5, _layout, 5, PX + 6, [S(3, 50, 0, 0, grid="dropped"), S(3, 50, 1, 10, grid="mixed", q=True),
                                                             S(4, 50, 2, 25, grid="dropped", bm=1)])        # a row and five columns of it outside
    _row(f"n8-{_ln(_layout)}", 3, _layout, 10, 2 * PX + 1, [S(3, 40, _k, 13 * _k, q=_k % 3 == 0, bm=int(_k % 3 == 1)) for _k in range(8)])
    # placement: negative offsets on both axes, a source wholly outside, identical rectangles, one row / one column of overlap
    _row(f"negative-{_ln(_layout)}", 5, _layout, 3, PX + 1, [S(4, 40, -1, -5), S(5, 70, -2, 10, q=True)])
    _row(f"outside-{_ln(_layout)}", 5, _layout, 3, PX + 1, [S(3, 30, 0, 0), S(3, 30, 0, 200, grid="dropped"), S(3, 30, -3, 10, grid="dropped"),
                                                          S(3, 40, 0, 25)])
    _row(f"identical-{_ln(_layout)}", 5, _layout, 3, PX + 1, [S(3, PX + 1, 0, 0, bm=1), S(3, PX + 1, 0, 0)])
    _row(f"one-row-{_ln(_layout)}", 5, _layout, 3, PX + 1, [S(2, PX + 1, 0, 0, grid="valid", bm=1), S(2, PX + 1, 1, 0, grid="valid")])
    _row(f"one-col-{_ln(_layout)}", 5, _layout, 3, 69, [S(3, 40, 0, 0, grid="valid", q=True), S(3, 30, 0, 39, grid="valid")])
    # a run boundary of merge_scenes (1024 elements) inside a source's edge: bip 129 x 8 = 1032 elements a row, bsq 1100
    _row(f"run-{_ln(_layout)}", 8 if _layout == BIP else 3, _layout, 2, 129 if _layout == BIP else 1100,
         [S(2, 127 if _layout == BIP else 1030, 0, 0), S(2, 60 if _layout == BIP else 90, 0, 69 if _layout == BIP else 1010, bm=1)])
    # empty elements in the overlap: single bands (band mask), whole pixels (quality mask), -9999 planted in a swath
    _row(f"empty-bmask-{_ln(_layout)}", 13, _layout, 3, PX + 1, [S(3, 50, 0, 0, grid="valid", bm=1), S(3, 50, 0, 15, grid="valid")])
    _row(f"empty-qmask-{_ln(_layout)}", 13, _layout, 3, PX + 1, [S(3, 50, 0, 0, grid="valid", q=True), S(3, 50, 0, 15, grid="valid")])
    _row(f"empty-planted-{_ln(_layout)}", 13, _layout, 3, PX + 1, [S(3, 50, 0, 0, grid="valid", plant=True), S(3, 50, 0, 15, grid="valid")])
    # every source empty at a cell: nodata and source 255
    _row(f"all-empty-{_ln(_layout)}", 5, _layout, 3, PX + 1, [S(3, 50, 0, 0, grid="nodata"), S(3, 50, 0, 15, grid="nodata")])
    # constants that are NOT empty: `masked` apart from nodata ends a pixel's walk; a NaN nodata makes a fill cell win
    _row(f"masked-wins-{_ln(_layout)}", 5, _layout, 3, PX + 1, [S(3, 50, 0, 0, q=True, bm=1), S(3, 50, 0, 15, q=True)], masked=-7777.5)
    _row(f"nan-nodata-{_ln(_layout)}", 5, _layout, 3, PX + 1, [S(3, 50, 0, 0, q=True), S(3, 50, 0, 15)], nodata=float("nan"))
    _row(f"zero-nodata-{_ln(_layout)}", 5, _layout, 3, PX + 1, [S(3, 50, 0, 0), S(3, 50, 0, 15)], nodata=0.0, masked=0.0)
    _row(f"no-counter-{_ln(_layout)}", 5, _layout, 3, PX + 1, [S(3, 50, 0, 0, bm=1), S(3, 50, 0, 15)], count=False)
    # merge_scenes only: NaN falls through
    _row(f"nan-falls-{_ln(_layout)}", 5, _layout, 3, PX + 1, [S(3, 50, 0, 0, grid="valid"), S(3, 50, 0, 15, grid="valid")], nan=True)

ORTHO_ROWS = [n for n, r in ROWS.items() if not r["nan"]]               # hsr_ortho_merge has no nan_is_nodata


def swath_dims(k):
    return 4 + k, 5 + k                                                # rows, cols of source k: every source its own bits


def row_mask(r):
    return any(s["q"] or s["bm"] for s in r["sources"])


def ortho_instance_of(r):
    return ortho_merge_instance(r["layout"], r["bands"], row_mask(r), [s["off"] for s in r["sources"]], r["out_off"])


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(swaths, glts, qmasks, bmasks (None where absent), scenes (float32 bip, what hsr_ortho_glt gives per source), offsets,
    ref (uint32 bits in the row's layout), ref_bip, source, dropped (per source))."""
    r = ROWS[name]
    swaths, glts, qmasks, bmasks, scenes, dropped = [], [], [], [], [], []
    for k, s in enumerate(r["sources"]):
        rows, cols = swath_dims(k)
        sw = oc.swath_of(rows, cols, r["bands"])
        if s["plant"]:
            sw = sw.copy()
            sw[::2, :, ::3] = np.float32(r["nodata"])
            sw[1, 1, :] = np.float32(r["nodata"])
            sw.setflags(write=False)
        glt = oc.glt_of(s["grid"], s["gh"], s["gw"], rows, cols)
        q = oc.qmask_of(rows, cols) if s["q"] else None
        bm = oc.bmask_of(rows, cols, r["bands"], (r["bands"] + 7) // 8 + k % 2) if s["bm"] else None
        bits, _ = oc.ortho_ref(sw, glt, None, q, bm, r["nodata"], r["masked"], 0, BIP)
        swaths.append(sw), glts.append(glt), qmasks.append(q), bmasks.append(bm), scenes.append(bits.view(np.float32))
        dropped.append(dropped_inside(glt, rows, cols, (s["oy"], s["ox"]), (r["H"], r["W"])))
    offsets = [(s["oy"], s["ox"]) for s in r["sources"]]
    ref_bip, source = merge_ref(scenes, offsets, (r["H"], r["W"]), r["nodata"], r["nan"])
    ref = ref_bip if r["layout"] == BIP else np.ascontiguousarray(ref_bip.transpose(2, 0, 1))
    return dict(swaths=swaths, glts=glts, qmasks=qmasks, bmasks=bmasks, scenes=scenes, offsets=offsets, ref=ref, ref_bip=ref_bip,
                source=source, dropped=dropped)


def in_layout(scene_bip, layout):
    return np.ascontiguousarray(scene_bip if layout == BIP else scene_bip.transpose(2, 0, 1))
