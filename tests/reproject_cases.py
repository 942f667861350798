"""Case tables, references and bars of the reprojection family (include/hsr_reproject.h); NumPy only, not a test module.

Geometry.  The reference is tests/golden/g18_tm_points.npz (tests/golden/gen_g18.py: mpmath at 50 digits).  The bar of a source
index is COORD_ULPS * ulp(180 degrees) / |g1| source pixels, 1.35e-8 px at EMIT's 0.000542 degree cell: the result passes through a
few dozen roundings at the magnitude of a longitude in degrees, everything else is relative 1e-16.  It holds for the host twin
and for the kernel.

Remap.  warp_ref is the header's statements in NumPy float64, one rounding per product and sum, in the header's order: the kernel
must give its bits, its counts and its status word on every row.  The rows' sizes go by the loop bounds of the 64 x 8 tile.

Sweep.  draw(seed, index) gives a seeded row in the table's form; valid(row) mirrors the header's argument rules; admitted(row,
case) is the table's admission condition (some output sample is computed, not filled)."""
import functools
import os
import zlib

import numpy as np

TILE_W, TILE_H, LDS_LIMIT = 64, 8, 32 * 1024
STRICT, RENORM = 0, 1
RULE_NAMES = ("STRICT", "RENORM")
COORD_ULPS = 256
WGS84 = (0.9996, 500000.0, 6378137.0, 298.257223563)          # k0, FE, a, inv_f
EMIT_CELL = 0.000542
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_tm_points.npz")
SEEDS, ROWS_PER_SEED, MAX_SKIPPED = (1, 2), 24, 0.10


def all_instances():
    return ["reproject_coords_kernel"] + ["reproject_warp_kernel<%s, %s>" % (i, r) for i in ("LDS", "DIRECT") for r in RULE_NAMES]


# =============================================================================================================================
# geometry
# =============================================================================================================================
def coord_bar(g1):
    """Source pixels: COORD_ULPS ulps of 180 degrees over the cell size."""
    return COORD_ULPS * float(np.spacing(180.0)) / abs(float(g1))


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    for v in g.values():
        v.setflags(write=False)
    return g


def fixture_groups():
    """The fixture by projection: [(lon0, FN, indices)], so that each group is one call of a coordinate entry."""
    g = fixture()
    keys = sorted({(float(a), float(b)) for a, b in zip(g["lon0"], g["FN"])})
    return [(lon0, fn, np.flatnonzero((g["lon0"] == lon0) & (g["FN"] == fn))) for lon0, fn in keys]


def point_call(E, N, lon0, fn, cell=EMIT_CELL):
    """The arguments of hsr_reproject_coords for ONE fixture point as a 1 x 1 grid of 2 m cells centred on it (E, N are rounded to
    millimetres, so e0 + 0.5 * 2 and n0 - 0.5 * 2 are exact), on a source grid of `cell` degrees whose origin is a whole degree
    near the point; and (g0, g3)."""
    g0, g3 = float(np.floor(lon0 - 8.0)), (84.0 if fn == 0.0 else 0.0)
    return [E - 1.0, N + 1.0, 2.0, 2.0, 1, 1, lon0, WGS84[0], WGS84[1], fn, WGS84[2], WGS84[3], g0, cell, g3, -cell], (g0, g3)


# =============================================================================================================================
# the remap
# =============================================================================================================================
def keys(t):
    return [((-0.5 * t + 1.0) * t - 0.5) * t, ((1.5 * t - 2.5) * t) * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t,
            ((0.5 * t - 0.5) * t) * t]


def src_valid(a, nodata):
    ok = np.isfinite(a)
    if nodata is not None:
        ok &= a.astype(np.float64) != float(nodata)
    return ok


def _geometry(coords, hs, ws):
    sy, sx = coords[..., 0], coords[..., 1]
    with np.errstate(invalid="ignore"):
        inside = (sy >= 0.0) & (sy <= hs - 1.0) & (sx >= 0.0) & (sx <= ws - 1.0)
    sy, sx = np.where(inside, sy, 0.0), np.where(inside, sx, 0.0)
    fy, fx = np.floor(sy), np.floor(sx)
    t_y, t_x = sy - fy, sx - fx
    ty = [np.clip(fy.astype(np.int64) - 1 + k, 0, hs - 1) for k in range(4)]
    tx = [np.clip(fx.astype(np.int64) - 1 + k, 0, ws - 1) for k in range(4)]
    return inside, t_y, t_x, ty, tx


def warp_ref(src, coords, nodata, fill, rule):
    """-> (out (bands, h, w) float32, counts (2,) int64, info): the header's statements in float64.  info: inside (h, w), and per
    band `bad` (a consulted tap is invalid), `filled` (inside and filled by the sample rule), `zero_weight_invalid` (an invalid
    tap under a weight of exactly 0)."""
    bands, hs, ws = src.shape
    inside, t_y, t_x, ty, tx = _geometry(coords, hs, ws)
    wy, wx = keys(t_y), keys(t_x)
    ny = np.where(t_y >= 0.5, ty[2], ty[1])
    nx = np.where(t_x >= 0.5, tx[2], tx[1])
    valid = src_valid(src, nodata)
    out = np.empty((bands,) + inside.shape, np.float32)
    bad_all, filled_all, zero_all = (np.zeros((bands,) + inside.shape, bool) for _ in range(3))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for b in range(bands):
            plane = src[b].astype(np.float64)
            bad = np.zeros(inside.shape, bool)
            acc = wsum = None
            for k in range(4):
                row = roww = None
                for c in range(4):
                    consulted = (wy[k] != 0.0) & (wx[c] != 0.0)
                    ok = valid[b][ty[k], tx[c]]
                    use = consulted & ok
                    bad |= consulted & ~ok
                    zero_all[b] |= ~consulted & ~ok
                    term = np.where(use, wx[c] * plane[ty[k], tx[c]], 0.0)
                    wterm = np.where(use, wx[c], 0.0)
                    row = term if row is None else row + term
                    roww = wterm if roww is None else roww + wterm
                row = np.where(wy[k] != 0.0, wy[k] * row, 0.0)
                roww = np.where(wy[k] != 0.0, wy[k] * roww, 0.0)
                acc = row if acc is None else acc + row
                wsum = roww if wsum is None else wsum + roww
            if rule == RENORM:
                near_ok = valid[b][ny, nx]
                val = np.where(bad, acc / np.where(bad & near_ok, wsum, 1.0), acc)
                filled = bad & ~near_ok
            else:
                val, filled = acc, bad
            res = val.astype(np.float32)
            res[~inside | filled] = np.float32(fill)
            out[b] = res
            bad_all[b], filled_all[b] = bad & inside, filled & inside
            zero_all[b] &= inside
    counts = np.array([int((~inside).sum()), int(filled_all.sum())], np.int64)
    return out, counts, dict(inside=inside, bad=bad_all, filled=filled_all, zero_weight_invalid=zero_all)


def boxes(max_footprint):
    """(box_w, box_h, direct): the staged box of a tile under the caller's bound and whether the host picks the direct instance."""
    if not max_footprint <= 1024.0:
        return None, None, True
    bw, bh = int(np.ceil(TILE_W * max_footprint)) + 5, int(np.ceil(TILE_H * max_footprint)) + 5
    return bw, bh, bw * bh * 4 > LDS_LIMIT


def warp_instance(max_footprint, rule):
    return "reproject_warp_kernel<%s, %s>" % ("DIRECT" if boxes(max_footprint)[2] else "LDS", RULE_NAMES[rule])


def tile_footprints(coords, hs, ws):
    """[(fw, fh)] of every 64 x 8 output tile: the extent of the clamped taps of its inside pixels, (0, 0) when it has none."""
    inside, _, _, ty, tx = _geometry(coords, hs, ws)
    h, w = inside.shape
    res = []
    for y0 in range(0, h, TILE_H):
        for x0 in range(0, w, TILE_W):
            m = inside[y0:y0 + TILE_H, x0:x0 + TILE_W]
            if not m.any():
                res.append((0, 0))
                continue
            sl = (slice(y0, y0 + TILE_H), slice(x0, x0 + TILE_W))
            res.append((int(tx[3][sl][m].max() - tx[0][sl][m].min()) + 1, int(ty[3][sl][m].max() - ty[0][sl][m].min()) + 1))
    return res


def warp_status(coords, hs, ws, max_footprint):
    """(status word, tiles whose footprint fits the staged capacity, tiles with an inside pixel that do not)."""
    bw, bh, _ = boxes(max_footprint)
    fps = tile_footprints(coords, hs, ws)
    if bw is None:
        return 0, 0, sum(1 for fw, fh in fps if fw)
    status = int(any(fw > bw or fh > bh for fw, fh in fps))
    fits = sum(1 for fw, fh in fps if fw and fw * fh <= bw * bh)
    return status, fits, sum(1 for fw, fh in fps if fw) - fits


# ---- fields ---------------------------------------------------------------------------------------------------------------------
SPECIALS = (float("nan"), float("inf"), float("-inf"), 1e300, -1e300, 2.0 ** 31, -2.0 ** 31, 2.0 ** 31 + 0.5, 2.0 ** 63, -0.0)


def make_field(spec, h, w, hs, ws, seed):
    """(h, w, 2) float64 (sy, sx) of a row's field spec."""
    kind = spec[0]
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    rng = np.random.default_rng([seed, zlib.crc32(kind.encode())])
    if kind == "identity":
        sy, sx = yy, xx
    elif kind == "shift":
        sy, sx = yy + spec[1], xx + spec[2]
    elif kind == "affine":                                           # rotation and scale about both centres: the TM-like case
        th, s = np.radians(spec[1]), spec[2]
        u, v = xx - 0.5 * (w - 1), yy - 0.5 * (h - 1)
        sx = 0.5 * (ws - 1) + s * (np.cos(th) * u - np.sin(th) * v)
        sy = 0.5 * (hs - 1) + s * (np.sin(th) * u + np.cos(th) * v)
    elif kind == "scale":                                            # cell centres: output cell y covers source [s y, s (y + 1))
        sy, sx = (yy + 0.5) * spec[1] - 0.5, (xx + 0.5) * spec[1] - 0.5
    elif kind == "random":
        sy, sx = rng.uniform(-1.5, hs + 0.5, (h, w)), rng.uniform(-1.5, ws + 0.5, (h, w))
    elif kind == "special":                                          # the identity with every special value planted on both axes
        sy, sx = yy.copy(), xx.copy()
        cells = rng.permutation(h * w)[:2 * len(SPECIALS)]
        for i, cell in enumerate(cells):
            (sy if i % 2 else sx).reshape(-1)[cell] = SPECIALS[i // 2]
    elif kind == "edges":                                            # exactly on the first and last sample, and 1e-12 outside them
        vy = np.array([0.0, -1e-12, hs - 1.0, hs - 1.0 + 1e-12, 0.5 * (hs - 1)])
        vx = np.array([0.0, -1e-12, ws - 1.0, ws - 1.0 + 1e-12, 0.5 * (ws - 1)])
        sy, sx = vy[(yy.astype(int) + xx.astype(int) // 5) % 5], vx[xx.astype(int) % 5]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(np.stack([sy, sx], axis=-1), dtype=np.float64)


# ---- rows -----------------------------------------------------------------------------------------------------------------------
# name: bands, output (h, w), source (hs, ws), field spec, bad (none | one | nan | nodata | mixed | dense | all), nodata (the
# argument, None: has_nodata = 0), fill, rule, mf (max_footprint), src_pad / out_pad (base offset in bytes, row padding in
# elements, gap after every band in elements), seed (default: from the name)
def warp_row(bands, h, w, hs, ws, field, bad="none", nodata=None, fill=-9999.0, rule=RENORM, mf=1.5, src_pad=(0, 0, 0),
             out_pad=(0, 0, 0), seed=None):
    return dict(bands=bands, h=h, w=w, hs=hs, ws=ws, field=tuple(field), bad=bad, nodata=nodata, fill=fill, rule=rule, mf=mf,
                src_pad=tuple(src_pad), out_pad=tuple(out_pad), seed=seed)


_R = warp_row
T1, T2 = (TILE_H, TILE_W), (2 * TILE_H + 3, 2 * TILE_W + 2)
WARP_ROWS = {
    # sizes by the loop bounds of the tile; the source's shape is never the output's
    "size-1x1": _R(1, 1, 1, 3, 4, ("shift", 1.25, 1.5)),
    "size-1x65": _R(2, 1, TILE_W + 1, 4, 70, ("shift", 1.5, 2.25), bad="nan", rule=STRICT),
    "size-9x1": _R(2, TILE_H + 1, 1, 21, 3, ("shift", 2.25, 0.5), bad="nodata", nodata=-9999.0),
    "size-7x63": _R(5, TILE_H - 1, TILE_W - 1, 19, 70, ("shift", 1.75, 3.5), bad="nan", src_pad=(4, 3, 5), out_pad=(12, 7, 9)),
    "size-8x64": _R(2, TILE_H, TILE_W, 21, 66, ("shift", 2.5, 0.75), bad="nodata", nodata=-9999.0, rule=STRICT),
    "size-9x65": _R(2, TILE_H + 1, TILE_W + 1, 23, 71, ("shift", 3.125, 2.625), bad="nan", src_pad=(8, 2, 0), out_pad=(4, 5, 11)),
    "size-19x130": _R(5, T2[0], T2[1], 41, 139, ("shift", 2.375, 4.875), bad="mixed", nodata=-9999.0, src_pad=(0, 1, 3)),
    "bands-285": _R(285, 20, 12, 17, 19, ("affine", 3.0, 0.8), bad="nan", out_pad=(4, 1, 2)),
    # fields
    "identity": _R(2, 33, 70, 40, 75, ("identity",), bad="nan", fill=float("nan")),
    "int-shift": _R(2, 33, 70, 40, 80, ("shift", 3.0, 5.0), bad="dense", nodata=-9999.0),
    "int-shift-strict": _R(2, 33, 70, 40, 80, ("shift", 3.0, 5.0), bad="dense", nodata=-9999.0, rule=STRICT),
    "half-shift": _R(2, 33, 70, 40, 80, ("shift", 2.5, 4.5), bad="nan"),
    "affine": _R(2, 40, 131, 52, 140, ("affine", 3.0, 0.8), bad="mixed", nodata=-9999.0, src_pad=(4, 3, 0), out_pad=(0, 2, 7)),
    "affine-strict": _R(2, 40, 131, 52, 140, ("affine", 3.0, 0.8), bad="mixed", nodata=-9999.0, rule=STRICT),
    "magnify-7": _R(2, 40, 131, 9, 22, ("scale", 1.0 / 7.0), bad="one"),
    "minify-5": _R(2, 20, 70, 104, 356, ("scale", 5.0), bad="nan"),                     # the footprint exceeds the staged box
    "minify-5-direct": _R(2, 20, 70, 104, 356, ("scale", 5.0), bad="nan", mf=5.0, rule=STRICT),
    "random": _R(2, 35, 70, 60, 90, ("random",), bad="nan"),
    "random-direct": _R(1, 35, 70, 30, 45, ("random",), bad="nodata", nodata=-9999.0, mf=float("inf")),
    "special": _R(2, 20, 70, 24, 75, ("special",), bad="nan"),
    "special-direct": _R(1, 20, 70, 24, 75, ("special",), mf=4.0, rule=STRICT),
    "edges": _R(2, 10, 70, 21, 33, ("edges",), bad="none"),
    "edges-invalid": _R(1, 10, 70, 21, 33, ("edges",), bad="dense", nodata=-9999.0),
    "half-outside": _R(2, 20, 70, 30, 60, ("shift", 0.25, -31.5), bad="nan"),
    "wholly-outside": _R(2, 20, 70, 30, 60, ("shift", 100.0, 0.0)),
    # samples
    "one-invalid-strict": _R(1, 20, 30, 24, 36, ("shift", 1.5, 2.5), bad="one", rule=STRICT),
    "one-invalid-renorm": _R(1, 20, 30, 24, 36, ("shift", 1.5, 2.5), bad="one"),
    "nodata-is-a-value": _R(1, 20, 30, 24, 36, ("shift", 1.25, 2.75), bad="nodata", nodata=None),   # -9999 samples without has_nodata
    "nan-and-nodata": _R(2, 20, 30, 24, 36, ("shift", 1.25, 2.75), bad="mixed", nodata=-9999.0),
    "nearest-invalid": _R(2, 20, 30, 24, 36, ("shift", 1.625, 2.375), bad="dense", nodata=-9999.0),
    "all-invalid": _R(2, 20, 30, 24, 36, ("shift", 1.5, 2.5), bad="all", nodata=-9999.0),
    "all-invalid-strict": _R(1, 20, 30, 24, 36, ("shift", 1.5, 2.5), bad="all", rule=STRICT, fill=float("nan")),
    "fill-nan": _R(2, 20, 70, 24, 60, ("shift", 0.5, 1.5), bad="dense", nodata=-9999.0, fill=float("nan")),
    # the largest bound that stages and the smallest that does not
    "bound-3.6-lds": _R(1, 20, 70, 80, 260, ("scale", 3.6), bad="nan", mf=3.6),
    "bound-3.7-direct": _R(1, 20, 70, 80, 260, ("scale", 3.6), bad="nan", mf=3.7),
    "direct-renorm": _R(2, 33, 70, 40, 80, ("shift", 2.5, 4.5), bad="dense", nodata=-9999.0, mf=8.0, src_pad=(8, 2, 1), out_pad=(4, 5, 3)),
}
# what a row's name claims, for tests/test_reproject_host.py
FALLBACK_ROWS = ("minify-5", "random")                    # LDS instance, some tile's footprint exceeds the staged capacity
FITTING_ROWS = ("affine", "size-19x130", "magnify-7", "bound-3.6-lds")


def _seed(name):
    return zlib.crc32(name.encode()) % 1000


def make_source(r, seed):
    """The (bands, hs, ws) float32 source of a row and its invalid samples."""
    bands, hs, ws = r["bands"], r["hs"], r["ws"]
    rng = np.random.default_rng([seed, 7])
    yy, xx = np.meshgrid(np.arange(hs), np.arange(ws), indexing="ij")
    base = 0.3 * np.sin(0.37 * yy + 0.11 * xx) + 0.002 * yy * xx / max(hs * ws, 1)
    src = np.stack([(np.roll(base, 3 * b, axis=1) + (b % 7) * 0.1 + rng.uniform(-0.2, 0.2, (hs, ws))) for b in range(bands)])
    src = src.astype(np.float32)
    bad = r["bad"]
    if bad == "one":
        src[0, hs // 2, ws // 2] = np.nan
    elif bad in ("nan", "nodata", "mixed", "dense"):
        p = 0.3 if bad == "dense" else 0.02
        hit = rng.random(src.shape) < p
        kind = rng.integers(0, 3, src.shape)
        src[hit & ((bad == "nan") | ((bad in ("mixed", "dense")) & (kind == 0)))] = np.nan
        src[hit & ((bad == "nodata") | ((bad in ("mixed", "dense")) & (kind == 1)))] = -9999.0
        if bad in ("mixed", "dense"):
            src[hit & (kind == 2)] = np.inf
        src[0, min(2, hs - 1), min(3, ws - 1)] = -np.inf if bad != "nodata" else -9999.0
    elif bad == "all":
        src[:] = np.where(rng.random(src.shape) < 0.5, np.float32(np.nan), np.float32(-9999.0))
    return src


def warp_case_of(r, seed=None):
    seed = (r["seed"] if r["seed"] is not None else 0) if seed is None else seed
    src = make_source(r, seed)
    coords = make_field(r["field"], r["h"], r["w"], r["hs"], r["ws"], seed)
    ref, counts, info = warp_ref(src, coords, r["nodata"], r["fill"], r["rule"])
    status, fits, falls = warp_status(coords, r["hs"], r["ws"], r["mf"])
    out = dict(src=src, coords=coords, ref=ref, counts=counts, status=status, fits=fits, falls=falls, **info)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def warp_case(name):
    return warp_case_of(WARP_ROWS[name], _seed(name))


def pack(scene, pad, sentinel):
    """The backing array of `scene` under pad = (base offset, row padding, gap): (bands, h (w + extra) + gap) elements."""
    _, extra, gap = pad
    bands, h, w = scene.shape
    back = np.full((bands, h * (w + extra) + gap), sentinel, dtype=scene.dtype)
    back[:, :h * (w + extra)].reshape(bands, h, w + extra)[:, :, :w] = scene
    return back


def unpack(back, h, w, pad):
    """(the (bands, h, w) payload, a mask of the elements outside it)."""
    _, extra, _ = pad
    rows = back[:, :h * (w + extra)].reshape(back.shape[0], h, w + extra)
    outside = np.ones(back.shape, bool)
    outside[:, :h * (w + extra)].reshape(back.shape[0], h, w + extra)[:, :, :w] = False
    return rows[:, :, :w], outside


# =============================================================================================================================
# the seeded sweep
# =============================================================================================================================
SWEEP_FIELDS = (("identity",), ("shift",), ("affine",), ("scale",), ("random",), ("special",), ("edges",))


def _size(rng, lo, hi, c):
    if rng.random() < 0.5:
        near = sorted({k * c + d for k in range(1, hi // c + 2) for d in (-1, 0, 1) if lo <= k * c + d <= hi})
        if near:
            return int(rng.choice(near))
    return int(rng.integers(lo, hi + 1))


def draw(seed, index):
    """Row `index` of seed `seed`, from np.random.default_rng([seed, index, salt]): any row can be rebuilt without the others.  The
    rule and the instance walk through their four combinations with the index; everything else is drawn."""
    rng = np.random.default_rng([seed, index, zlib.crc32(b"reproject-warp")])
    stratum = (index + seed) % 4
    rule, direct = stratum % 2, stratum // 2
    h, w = _size(rng, 1, 40, TILE_H), _size(rng, 1, 140, TILE_W)
    kind = SWEEP_FIELDS[int(rng.integers(0, len(SWEEP_FIELDS)))][0]
    if kind == "identity":
        field, hs, ws = ("identity",), h + int(rng.integers(0, 4)), w + int(rng.integers(0, 6))
    elif kind == "shift":
        dy, dx = (float(rng.integers(-3, 9)) / 8.0 + float(rng.integers(0, 3)) for _ in range(2))
        field, hs, ws = ("shift", dy, dx), h + int(rng.integers(1, 6)), w + int(rng.integers(1, 6))
    elif kind == "affine":
        s = float(rng.uniform(0.5, 1.6))
        field = ("affine", float(rng.uniform(-8.0, 8.0)), s)
        hs, ws = max(int(h * s * rng.uniform(0.8, 1.3)) + 2, 1), max(int(w * s * rng.uniform(0.8, 1.3)) + 2, 1)
    elif kind == "scale":
        s = float(rng.choice((1.0 / 7.0, 0.5, 1.0 / 1.2, 1.2, 2.5, 5.0)))
        field, hs, ws = ("scale", s), max(int(np.ceil(h * s)), 1) + int(rng.integers(0, 3)), max(int(np.ceil(w * s)), 1) + int(rng.integers(0, 3))
    else:
        field, hs, ws = (kind,), int(rng.integers(1, 50)), int(rng.integers(1, 90))
        if kind == "special":
            hs, ws = h + int(rng.integers(0, 4)), w + int(rng.integers(0, 4))
    mf = float(rng.choice((3.7, 6.0, float("inf")))) if direct else float(rng.choice((0.0, 1.0, 1.5, 3.6)))
    bad = str(rng.choice(("none", "one", "nan", "nodata", "mixed", "dense", "all"), p=(0.1, 0.1, 0.2, 0.15, 0.2, 0.2, 0.05)))
    nodata = None if bad in ("none", "one", "nan") or rng.integers(0, 6) == 0 else -9999.0
    bands = 33 if rng.integers(0, 10) == 0 else int(rng.integers(1, 6))
    pads = [(4 * int(rng.integers(0, 8)), int(rng.integers(0, 9)), int(rng.integers(0, 12))) for _ in range(2)]
    return warp_row(bands, h, w, hs, ws, field, bad=bad, nodata=nodata, fill=float(rng.choice((-9999.0, float("nan"), 0.0))),
                    rule=rule, mf=mf, src_pad=pads[0], out_pad=pads[1], seed=int(rng.integers(0, 1000)))


def valid(r):
    """include/hsr_reproject.h above hsr_reproject_warp: what is refused, negated; and the float alignment of both bases."""
    return (min(r["bands"], r["h"], r["w"], r["hs"], r["ws"]) >= 1 and r["rule"] in (0, 1) and r["mf"] >= 0.0
            and all(p[0] % 4 == 0 and p[1] >= 0 and p[2] >= 0 for p in (r["src_pad"], r["out_pad"])))


def admitted(r, case):
    """The table's admission condition: some output sample is computed, not filled."""
    return bool((case["inside"][None] & ~case["filled"]).any())
