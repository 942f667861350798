"""The area-resampling family (include/hsr_resize.h) for the tests: a NumPy statement of the header's definition, the case tables,
the strided layouts and the argument lists of hsr_area_resample / hsr_area_resample_host.  A plain module: no test in it.

No fixture can be frozen from the reference: resize_s2_rgb_to (s2_emit/viz.py:19-24) needs cv2, which is absent, and cv2's bits are
not claimed.  The reference of every test is `area_ref` below: vectorised over the outputs, a loop over the tap offsets in the
defined order, and np.where so that a skipped sample contributes nothing."""
import ctypes as C
import math

import numpy as np

TILE_H, TILE_W, MAX_SCALE, MAX_C, LDS_BYTES = 8, 32, 64, 16, 81920
F32, U8, U16 = 0, 1, 2
STRICT, RENORM = 0, 1
CODES = {"float32": F32, "uint8": U8, "uint16": U16}
RULES = {"strict": STRICT, "renorm": RENORM}
TAGS = {"float32": "F32", "uint8": "U8", "uint16": "U16"}
PAIRS = (("float32", "float32"), ("uint8", "uint8"), ("uint8", "float32"), ("uint16", "uint16"), ("uint16", "float32"))
SENT = 0xA5


# ---- the statement ------------------------------------------------------------------------------------------------------------------------
def spans(o, s, n_out, n_src):
    """Cells 0 .. n_out - 1 of an axis -> (lo, hi, a, b): the cell is [lo, hi], its taps a .. b - 1; a == b: outside."""
    e = np.float64(o) + np.arange(n_out + 1, dtype=np.float64) * np.float64(s)         # one multiply, one add, each rounded
    lo, hi = np.maximum(e[:-1], 0.0), np.minimum(e[1:], np.float64(n_src))
    inside = hi > lo
    a = np.where(inside, np.floor(lo), 0.0).astype(np.int64)
    b = np.where(inside, np.ceil(hi), 0.0).astype(np.int64)
    return lo, hi, a, b


def weight(lo, hi, i):
    return np.minimum(hi, (i + 1).astype(np.float64)) - np.maximum(lo, i.astype(np.float64))


def valid_of(src, nodata):
    ok = np.isfinite(src) if src.dtype == np.float32 else np.ones(src.shape, bool)
    if nodata is not None:
        ok = ok & ~(src.astype(np.float64) == np.float64(nodata))
    return ok


def area_ref(src, out_hw, origin=(0.0, 0.0), scale=None, nodata=None, rule="renorm", mvf=0.0, out_dtype=None, post=1.0, fill=np.nan,
             nodata_out=0):
    """src (C, h, w) uint8 / uint16 / float32 -> (out (C, H, W) of out_dtype, invalid (C,) int64) under include/hsr_resize.h."""
    src = np.asarray(src)
    Cn, h, w = src.shape
    H, W = out_hw
    sy, sx = (h / H, w / W) if scale is None else scale
    out_dtype = np.dtype(out_dtype or src.dtype)
    ylo, yhi, ya, yb = spans(origin[0], sy, H, h)
    xlo, xhi, xa, xb = spans(origin[1], sx, W, w)
    ok = valid_of(src, nodata)
    v64 = np.where(ok, src, 0).astype(np.float64)
    # the row pass, for every source row: (C, h, W)
    R, M, F = np.zeros((Cn, h, W)), np.zeros((Cn, h, W)), np.zeros(W)
    rbad = np.zeros((Cn, h, W), bool)
    for k in range(int((xb - xa).max(initial=0))):
        i = xa + k
        active = i < xb
        ic = np.minimum(i, w - 1)
        wx = np.where(active, weight(xlo, xhi, i), 0.0)
        use = ok[:, :, ic] & active
        R = np.where(use, R + wx * v64[:, :, ic], R)
        M = np.where(use, M + wx, M)
        F = np.where(active, F + wx, F)
        rbad |= ~ok[:, :, ic] & active
    # the column pass: (C, H, W)
    S, A, Full = np.zeros((Cn, H, W)), np.zeros((Cn, H, W)), np.zeros((H, W))
    bad = np.zeros((Cn, H, W), bool)
    for k in range(int((yb - ya).max(initial=0))):
        r = ya + k
        active = (r < yb)[:, None]
        rc = np.minimum(r, h - 1)
        wy = np.where(active, weight(ylo, yhi, r)[:, None], 0.0)
        S = np.where(active, S + wy * R[:, rc, :], S)
        A = np.where(active, A + wy * M[:, rc, :], A)
        Full = np.where(active, Full + wy * F[None, :], Full)
        bad |= rbad[:, rc, :] & active
    outside = (ya == yb)[:, None] | (xa == xb)[None, :]
    good = ~bad if rule == "strict" else ~((A == 0.0) | (A < np.float64(mvf) * Full))
    good = good & ~outside
    with np.errstate(invalid="ignore", divide="ignore"):
        q = S / A
    if out_dtype == np.float32:
        with np.errstate(invalid="ignore", over="ignore"):
            out = np.where(good, q.astype(np.float32) * np.float32(post), np.float32(fill)).astype(np.float32)
    else:
        top = np.iinfo(out_dtype).max
        out = np.where(good, np.clip(np.rint(np.where(good, q, 0.0)), 0, top), nodata_out).astype(out_dtype)
    return out, (~good).reshape(Cn, -1).sum(axis=1).astype(np.int64)


def tap_counts(r):
    """The most taps a cell of the row has, per axis: (rows, columns)."""
    (h, w), (H, W) = r["src"], r["dst"]
    sy, sx = scale_of(r)
    _, _, ya, yb = spans(r["origin"][0], sy, H, h)
    _, _, xa, xb = spans(r["origin"][1], sx, W, w)
    return int((yb - ya).max()), int((xb - xa).max())


# ---- the instance: a mirror of the host's choice (hsr_area_resample_instance) ----------------------------------------------------
def round16(n):
    return (n + 15) // 16 * 16


def staged_bytes(itemsize, Cn, ps, pixmajor, sy, sx):
    rows, cols = math.ceil(TILE_H * sy) + 3, math.ceil(TILE_W * sx) + 3
    elems = (cols - 1) * ps + Cn if pixmajor else cols
    return rows * (round16(elems * itemsize) + 16) + rows * TILE_W * 16 + round16(rows * TILE_W)


def instance_of(in_dtype, out_dtype, Cn, cs, ps, sy, sx):
    pair = f"{TAGS[in_dtype]}, {TAGS[out_dtype]}"
    item = np.dtype(in_dtype).itemsize
    if ps == 1 and staged_bytes(item, Cn, 1, False, sy, sx) <= LDS_BYTES:
        return f"area_staged_kernel<{pair}, PLANAR>"
    if ps != 1 and cs == 1 and Cn <= ps <= 64 and staged_bytes(item, Cn, ps, True, sy, sx) <= LDS_BYTES:
        return f"area_staged_kernel<{pair}, PIXMAJOR>"
    return f"area_gather_kernel<{pair}>"


def all_instances():
    return [f"area_staged_kernel<{TAGS[i]}, {TAGS[o]}, {lay}>" for lay in ("PLANAR", "PIXMAJOR") for i, o in PAIRS] + \
           [f"area_gather_kernel<{TAGS[i]}, {TAGS[o]}>" for i, o in PAIRS]


# ---- the rows ---------------------------------------------------------------------------------------------------------------------------
def row(src, dst, **kw):
    r = dict(src=src, dst=dst, dtype="uint8", out=None, C=1, layout="planar", origin=(0.0, 0.0), scale=None, nodata=None, rule="renorm",
             mvf=0.0, post=1.0, fill=np.nan, nodata_out=0, row_pad=0, pix=None, src_off=0, dst_off=0, out_row_pad=0, holes=None, count=True,
             seed=1, kind="staged", taps=None)
    assert set(kw) <= set(r), set(kw) - set(r)
    r.update(kw)
    r["out"] = r["out"] or r["dtype"]
    return r


def scale_of(r):
    return (r["src"][0] / r["dst"][0], r["src"][1] / r["dst"][1]) if r["scale"] is None else r["scale"]


EXTENT_ROWS = {
    "ext-1x1": row((3, 5), (1, 1), taps=(3, 5)),
    "ext-w31": row((16, 62), (8, TILE_W - 1), taps=(2, 2)),
    "ext-w32": row((16, 64), (8, TILE_W), taps=(2, 2)),
    "ext-w33": row((16, 66), (8, TILE_W + 1), taps=(2, 2)),
    "ext-h7": row((11, 48), (TILE_H - 1, TILE_W), scale=(1.5, 1.5), taps=(2, 2)),
    "ext-h8": row((12, 48), (TILE_H, TILE_W), scale=(1.5, 1.5), taps=(2, 2)),
    "ext-h9": row((14, 48), (TILE_H + 1, TILE_W), scale=(1.5, 1.5), taps=(2, 2)),
    "ext-two-tiles-plus-one": row((34, 130), (2 * TILE_H + 1, 2 * TILE_W + 1), taps=(2, 2)),
    "ext-wide": row((9, 600), (3, 100), dtype="uint16", taps=(3, 6)),
    "ext-tall": row((600, 10), (120, 4), dtype="float32", taps=(5, 3)),
}
SCALE_ROWS = {
    "scale-1": row((20, 40), (20, 40), taps=(1, 1)),
    "scale-1.5": row((30, 60), (20, 40), taps=(2, 2)),
    "scale-2": row((40, 80), (20, 40), dtype="uint16", taps=(2, 2)),
    "scale-2.5": row((50, 100), (20, 40), taps=(3, 3)),
    "scale-6": row((120, 240), (20, 40), dtype="uint16", out="float32", taps=(6, 6)),
    "scale-6.2-6.25": row((62, 100), (10, 16), taps=(7, 7)),
    "scale-64-one": row((64, 64), (1, 1), kind="gather", taps=(64, 64)),
    "scale-64-two": row((130, 130), (2, 2), scale=(64.0, 64.0), kind="gather", taps=(64, 64)),
    "scale-10.75-staged": row((119, 398), (11, 37), scale=(10.75, 10.75), taps=(12, 12)),
    "scale-11-gather": row((121, 407), (11, 37), scale=(11.0, 11.0), kind="gather", taps=(11, 11)),
    "origin-0.25": row((41, 81), (20, 40), scale=(2.0, 2.0), origin=(0.25, 0.25), taps=(3, 3)),
    "origin-left-clip": row((40, 80), (20, 40), scale=(2.0, 2.0), origin=(-0.5, -0.5), taps=(3, 3)),
    "origin-right-clip": row((40, 80), (20, 40), scale=(2.0, 2.0), origin=(1.5, 1.5), taps=(3, 3)),
    "origin-cells-outside": row((40, 80), (24, 45), scale=(2.0, 2.0), origin=(-5.0, -5.0), taps=(2, 2)),
    "origin-all-outside": row((10, 10), (9, 33), scale=(2.0, 2.0), origin=(30.0, -80.0), taps=(0, 0)),
}
LAYOUT_ROWS = dict(
    [(f"pair-{i}-{o}", row((27, 75), (9, 35), dtype=i, out=o, scale=(2.5, 2.0), origin=(0.5, 0.3), taps=(3, 3), post=0.5)) for i, o in PAIRS] +
    [(f"planar-C{c}", row((24, 70), (9, 33), dtype="uint16", C=c, taps=(4, 4))) for c in (1, 3, 10, 16)] +
    [(f"pixmajor-C{c}", row((24, 70), (9, 33), dtype="uint8", C=c, layout="pixmajor", pix=max(c, 2), taps=(4, 4))) for c in (1, 3, 4)] +
    [(f"pixmajor-pair-{i}-{o}", row((27, 75), (9, 35), dtype=i, out=o, C=3, layout="pixmajor", scale=(2.5, 2.0), origin=(0.5, 0.3),
                                   taps=(3, 3))) for i, o in PAIRS] +
    [(f"gather-pair-{i}-{o}", row((27, 75), (9, 35), dtype=i, out=o, C=2, layout="colmajor", scale=(2.5, 2.0), origin=(0.5, 0.3), kind="gather",
                                 taps=(3, 3))) for i, o in PAIRS] +
    [("padded-rows", row((24, 70), (9, 33), dtype="uint16", C=3, row_pad=5, out_row_pad=3, taps=(4, 4))),
     ("padded-rows-pixmajor", row((24, 70), (9, 33), C=3, layout="pixmajor", row_pad=7, out_row_pad=2, taps=(4, 4))),
     ("channel-slice", row((24, 70), (9, 33), C=3, layout="pixmajor", pix=4, taps=(4, 4))),
     ("channel-slice-f32", row((24, 70), (9, 33), dtype="float32", C=2, layout="pixmajor", pix=5, taps=(4, 4)))] +
    [(f"misaligned-{k}-{dt}", row((24, 150), (9, 33), dtype=dt, src_off=k, dst_off=k, row_pad=k, taps=(4, 6)))
     for k in (1, 2, 3) for dt in ("uint8", "uint16", "float32")])
VALIDITY_ROWS = dict(
    [(f"holes-{dt}-{rule}-{mvf}", row((50, 100), (20, 40), dtype=dt, C=2, nodata=7, rule=rule, mvf=mvf, holes="taps", fill=-1.0, nodata_out=9,
                                     taps=(3, 3)))
     for dt in ("float32", "uint8", "uint16") for rule, mvf in (("strict", 0.0), ("renorm", 0.0), ("renorm", 0.5), ("renorm", 1.0))] +
    [("holes-pixmajor", row((50, 100), (20, 40), dtype="float32", C=3, layout="pixmajor", nodata=7, holes="taps", taps=(3, 3))),
     ("holes-gather", row((50, 100), (20, 40), dtype="float32", C=2, layout="colmajor", nodata=7, holes="taps", kind="gather", taps=(3, 3))),
     ("holes-no-count", row((50, 100), (20, 40), dtype="float32", nodata=7, holes="taps", count=False, taps=(3, 3))),
     ("holes-random-strict", row((50, 100), (20, 40), dtype="float32", holes="random", rule="strict", taps=(3, 3))),
     ("holes-random-half", row((50, 100), (20, 40), dtype="uint16", out="float32", nodata=0, holes="random", mvf=0.5, taps=(3, 3)))])
ROUNDING_ROWS = {
    "round-half-even": row((40, 80), (20, 40), holes="halves", taps=(2, 2)),
    "saturate-u8": row((30, 60), (20, 40), holes="top", taps=(2, 2)),
    "saturate-u16": row((30, 60), (20, 40), dtype="uint16", holes="top", taps=(2, 2)),
    "post-scale-255": row((40, 80), (20, 40), out="float32", post=float(np.float32(1.0 / 255.0)), taps=(2, 2)),
}


def _sweep():
    rng = np.random.default_rng(20261021)
    rows = {}
    for k in range(24):
        i, o = PAIRS[k % 5]
        layout = ("planar", "pixmajor", "colmajor")[int(rng.integers(0, 3))]
        Cn = int(rng.integers(1, 5))
        H, W = int(rng.integers(1, 30)), int(rng.integers(1, 80))
        sy, sx = (float(rng.uniform(1.0, 12.0)), float(rng.uniform(1.0, 12.0))) if k % 3 else (float(rng.integers(1, 7)), float(rng.integers(1, 7)))
        h, w = max(1, int(H * sy + rng.integers(-2, 3))), max(1, int(W * sx + rng.integers(-2, 3)))
        rows[f"sweep-{k}"] = row((h, w), (H, W), dtype=i, out=o, C=Cn, layout=layout, pix=Cn + int(rng.integers(0, 2)) if layout == "pixmajor" else None,
                                 scale=(sy, sx), origin=(float(rng.uniform(-2, 2)), float(rng.uniform(-2, 2))), nodata=3,
                                 rule=("strict", "renorm")[k % 2], mvf=float(rng.choice([0.0, 0.25, 0.9])), holes="random", fill=-2.0, nodata_out=1,
                                 row_pad=int(rng.integers(0, 4)), src_off=int(rng.integers(0, 4)), seed=100 + k, kind=None)
    return rows


SWEEP_ROWS = _sweep()
ALL_ROWS = {**EXTENT_ROWS, **SCALE_ROWS, **LAYOUT_ROWS, **VALIDITY_ROWS, **ROUNDING_ROWS, **SWEEP_ROWS}


# ---- sources ----------------------------------------------------------------------------------------------------------------------------
HOLE_SPOTS = ((0, 0), (0, 1), (0, 2), (1, 0), (2, 0), (2, 2), (1, 1))     # (row, column) of a cell's taps: 0 first, 1 inner, 2 last


def hole_cells(r):
    """The cells that get a hole and the spot of each; the last entry is a cell whose taps are all invalid."""
    H, W = r["dst"]
    cells = [((3 * k + 1) % H, (7 * k + 2) % W, HOLE_SPOTS[k % len(HOLE_SPOTS)]) for k in range(14)]
    return cells, (H // 2, W // 2)


def source(name):
    """The (C, h, w) source image of a row."""
    r = ALL_ROWS[name]
    rng = np.random.default_rng(r["seed"] + sum(map(ord, name)))
    (h, w), Cn, dt = r["src"], r["C"], np.dtype(r["dtype"])
    if dt == np.float32:
        img = rng.uniform(-4.0, 4.0, size=(Cn, h, w)).astype(np.float32)
    else:
        img = rng.integers(8, np.iinfo(dt).max + 1, size=(Cn, h, w)).astype(dt)
    holes = r["holes"]
    if holes == "halves":                                   # 2 x 2 blocks (k, k, k + 1, k + 1): a mean of exactly k + 0.5
        H, W = r["dst"]
        k = (np.arange(H * W).reshape(H, W) % 254).astype(dt)
        img = np.repeat(np.repeat(k, 2, 0), 2, 1)[None].copy()
        img[:, 1::2, :] += 1
    elif holes == "top":
        img[:] = np.iinfo(dt).max
    elif holes == "random":
        bad = rng.random(img.shape) < 0.1
        if dt == np.float32:
            img[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf, 3.0], np.float32), size=int(bad.sum()))
        elif r["nodata"] is not None:
            img[bad] = r["nodata"]
    elif holes == "taps":
        sy, sx = scale_of(r)
        _, _, ya, yb = spans(r["origin"][0], sy, r["dst"][0], h)
        _, _, xa, xb = spans(r["origin"][1], sx, r["dst"][1], w)
        poison = [np.nan, np.inf, -np.inf, r["nodata"]] if dt == np.float32 else [r["nodata"]]
        cells, whole = hole_cells(r)
        pick = lambda a, b, s: (a, (a + b - 1) // 2, b - 1)[s]  # noqa: E731
        for n, (Y, X, (sr, scol)) in enumerate(cells):
            img[n % Cn, pick(ya[Y], yb[Y], sr), pick(xa[X], xb[X], scol)] = poison[n % len(poison)]
        Y, X = whole
        img[:, ya[Y]:yb[Y], xa[X]:xb[X]] = poison[0]
    return img


_REF = {}


def reference(name):
    """(out (C, H, W), invalid (C,)) of a row under the statement; computed once."""
    if name not in _REF:
        r = ALL_ROWS[name]
        out, inv = area_ref(source(name), r["dst"], r["origin"], r["scale"], r["nodata"], r["rule"], r["mvf"], r["out"], r["post"], r["fill"],
                            r["nodata_out"])
        out.setflags(write=False)
        inv.setflags(write=False)
        _REF[name] = (out, inv)
    return _REF[name]


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------
def strides(kind, Cn, rows, cols, row_pad=0, pix=None):
    """(channel, row, pixel) strides in elements."""
    if kind == "planar":
        rs = cols + row_pad
        return rows * rs + (7 if row_pad else 0), rs, 1
    if kind == "pixmajor":
        ps = pix or Cn
        return 1, cols * ps + row_pad, ps
    assert kind == "colmajor"                               # rows contiguous down a column: neither staged layout
    ps = rows + row_pad
    return cols * ps, 1, ps


def extent(Cn, rows, cols, st):
    return (Cn - 1) * st[0] + (rows - 1) * st[1] + (cols - 1) * st[2] + 1


def _index(Cn, rows, cols, st):
    c, y, x = np.meshgrid(np.arange(Cn), np.arange(rows), np.arange(cols), indexing="ij")
    return c * st[0] + y * st[1] + x * st[2]


def scatter(img, st, fill_byte=SENT):
    """(C, rows, cols) -> the flat buffer of the layout, sentinel bytes in the gaps."""
    Cn, rows, cols = img.shape
    flat = np.full(extent(Cn, rows, cols, st) * img.dtype.itemsize, fill_byte, np.uint8).view(img.dtype)
    flat[_index(Cn, rows, cols, st)] = img
    return flat


def gather(flat, Cn, rows, cols, st):
    """-> ((C, rows, cols) image, the gap elements as bytes)."""
    idx = _index(Cn, rows, cols, st)
    gap = np.ones(flat.size, bool)
    gap[idx.reshape(-1)] = False
    return flat[idx], flat[gap].view(np.uint8)


def layout(name):
    """-> (source flat, its byte offset past a 16-byte boundary, source strides, output elements, output byte offset, output strides)."""
    r = ALL_ROWS[name]
    (h, w), (H, W), Cn = r["src"], r["dst"], r["C"]
    sst = strides(r["layout"], Cn, h, w, r["row_pad"], r["pix"])
    dst = strides(r["layout"], Cn, H, W, r["out_row_pad"], r["pix"])
    item, oitem = np.dtype(r["dtype"]).itemsize, np.dtype(r["out"]).itemsize
    return scatter(source(name), sst), r["src_off"] * item, sst, extent(Cn, H, W, dst), r["dst_off"] * oitem, dst


def call_args(name, src_ptr, dst_ptr, invalid_ptr):
    """The arguments of hsr_area_resample_host, and of hsr_area_resample up to the stream."""
    r = ALL_ROWS[name]
    _, _, sst, _, _, dst = layout(name)
    (h, w), (H, W) = r["src"], r["dst"]
    sy, sx = scale_of(r)
    return [src_ptr, CODES[r["dtype"]], r["C"], h, w, sst[0], sst[1], sst[2], r["origin"][0], r["origin"][1], sy, sx,
            0 if r["nodata"] is None else 1, float(r["nodata"] or 0), RULES[r["rule"]], r["mvf"], dst_ptr, CODES[r["out"]], H, W, dst[0], dst[1],
            dst[2], C.c_float(r["post"]), C.c_float(r["fill"]), r["nodata_out"], invalid_ptr if r["count"] else None]


def same(got, want, what):
    """Equality of two arrays of one dtype; float32: NaN in the same places, every other element the same bits."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), f"{what}: NaN positions differ ({int(gn.sum())} vs {int(wn.sum())})"
        bad = (got.view(np.uint32) != want.view(np.uint32)) & ~gn
    else:
        bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first {got[bad][:4]} vs {want[bad][:4]}"


def check_output(name, out_flat, invalid):
    """out_flat: the output buffer as its dtype; invalid: (C,) int64 or None."""
    r = ALL_ROWS[name]
    _, _, _, _, _, dst = layout(name)
    want, winv = reference(name)
    got, gaps = gather(out_flat, r["C"], r["dst"][0], r["dst"][1], dst)
    same(got, want, name)
    assert (gaps == SENT).all(), f"{name}: a write between the output's elements"
    if invalid is not None:
        np.testing.assert_array_equal(invalid, winv, err_msg=name)


def instance_name(name):
    r = ALL_ROWS[name]
    _, _, sst, _, _, _ = layout(name)
    sy, sx = scale_of(r)
    return instance_of(r["dtype"], r["out"], r["C"], sst[0], sst[2], sy, sx)
