"""The NumPy statement of include/hsr_roi.h and the case tables of the polygon family.  Not a test module.

The statement is brute force - every cell against every edge, written straight from the header's rules in float64, operation for
operation (NumPy rounds every operation once, like the library built without contraction):

    pixel_edges(rings, gt)             the edges a -> b of all rings in pixel coordinates, clamped to +-1e300
    rasterize_ref(rings, gt, shape, rule, window)   -> (h, w) bool: the centre rule, or the touched rule
    glt_clip_ref(glt, mask, window)    -> (clipped (h, w, 2) int32, record (8,) int32): emit_tools.py:557-573 under our mask
    glt_reindex_ref(clipped, record)   -> emit_tools.py:594-595

ROWS is the table the host twins (tests/test_roi_host.py) and the kernels (tests/test_gpu_roi_instances.py) run, each row under
both rules: grids of at most a few hundred cells a side with widths and heights 1, one less than, equal to and one more than the
store run (16), the tile (64 rows, 256 columns), grids that cross a tile boundary each way, both signs of dy, row strides and
buffer offsets of their own, windows of every origin parity; polygons from a triangle to a 1500-vertex comb whose every row holds
more than a thousand crossings; the ties the header decides; vertices at +-1e300.

Two references that share no code with the statement: matplotlib's Path.contains_points for the centre rule and an exact
fractions.Fraction test of "the boundary meets the closed cell or the centre is inside" for the touched rule, each on seeded
polygons in general position (general_polygon, dyadic_polygon)."""
import functools
import math
from fractions import Fraction

import numpy as np

CENTER, TOUCHED = 0, 1
RULES = {"center": CENTER, "touched": TOUCHED}
TILE_H, TILE_W, RUN, MAX_EDGES, RECORD = 64, 256, 16, 8192, 8
COORD_MAX = 1e300
I32_MAX = 2 ** 31 - 1
INSTANCES = ["roi_raster_kernel<CENTER>", "roi_raster_kernel<TOUCHED>", "roi_counts_kernel<CENTER>", "roi_counts_kernel<TOUCHED>",
             "roi_record_init_kernel", "roi_glt_clip_kernel", "roi_glt_reindex_kernel"]
INSTANCE_COUNT = len(INSTANCES)
GT_UTM = (600000.0, 10.0, 0.0, 4100000.0, 0.0, -10.0)          # 10 u and 600000 + 10 u are exact for small dyadic u
GT_UP = (600000.0, 10.0, 0.0, 4000000.0, 0.0, 10.0)            # dy > 0: row 0 is the southernmost
GT_EXACT = (1024.0, 0.5, 0.0, 2048.0, 0.0, -0.25)              # powers of two: every dyadic pixel coordinate survives the round trip


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def flatten(rings):
    """-> (verts (n, 2) float64, ring_offsets (nrings + 1) int32)."""
    rings = [np.asarray(r, np.float64).reshape(-1, 2) for r in rings]
    return np.ascontiguousarray(np.concatenate(rings, axis=0)), np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)


def pixel_edges(rings, gt):
    """-> ua, va, ub, vb: one entry per edge, ring by ring, vertex i to i + 1 and the last to the first."""
    a, b = [], []
    for r in rings:
        r = np.asarray(r, np.float64).reshape(-1, 2)
        a.append(r)
        b.append(np.roll(r, -1, axis=0))
    a, b = np.concatenate(a), np.concatenate(b)
    with np.errstate(over="ignore"):
        px = lambda p: (np.clip((p[:, 0] - gt[0]) / gt[1], -COORD_MAX, COORD_MAX), np.clip((p[:, 1] - gt[3]) / gt[5], -COORD_MAX, COORD_MAX))  # noqa: E731
        (ua, va), (ub, vb) = px(a), px(b)
    return ua, va, ub, vb


def rasterize_ref(rings, gt, shape, rule, window=None):
    """The header's rules on every cell of the window against every edge -> (h, w) bool."""
    H, W = shape
    r0, c0, h, w = (0, 0, H, W) if window is None else window
    rows, cols = np.arange(r0, r0 + h, dtype=np.float64), np.arange(c0, c0 + w, dtype=np.float64)
    pv, pu = rows + 0.5, cols + 0.5
    inside, touched = np.zeros((h, w), bool), np.zeros((h, w), bool)
    with np.errstate(all="ignore"):
        for ua, va, ub, vb in zip(*pixel_edges(rings, gt)):
            first = (va <= pv) != (vb <= pv)
            xc = ua + (pv - va) * (ub - ua) / (vb - va)
            inside ^= first[:, None] & (pu[None, :] < xc[:, None])
            if rule != TOUCHED:
                continue
            vmin, vmax = min(va, vb), max(va, vb)
            reach = (math.floor(vmin) <= rows) & (rows <= math.floor(vmax))
            if va == vb:
                u1, u2 = np.full(h, ua), np.full(h, ub)
            else:
                lo, hi = np.maximum(vmin, rows), np.minimum(vmax, rows + 1.0)
                at = lambda t: np.where(t == va, ua, np.where(t == vb, ub, ua + (t - va) * (ub - ua) / (vb - va)))  # noqa: E731
                u1, u2 = at(lo), at(hi)
            flo, fhi = np.floor(np.minimum(u1, u2)), np.floor(np.maximum(u1, u2))
            touched |= reach[:, None] & (flo[:, None] <= cols[None, :]) & (cols[None, :] <= fhi[:, None])
    return inside | touched


def bbox_window(rings, gt, shape):
    """The cells the vertex bounding box touches, clamped to the grid, or None."""
    H, W = shape
    ua, va, _, _ = pixel_edges(rings, gt)
    c0, c1 = max(math.floor(ua.min()), 0), min(math.floor(ua.max()), W - 1)
    r0, r1 = max(math.floor(va.min()), 0), min(math.floor(va.max()), H - 1)
    return None if c0 > c1 or r0 > r1 else (r0, c0, r1 - r0 + 1, c1 - c0 + 1)


def glt_clip_ref(glt, mask, window):
    """emit_tools.py:557-573 on the window of `glt` (H, W, 2) under `mask` (h, w) bool -> (clipped, record)."""
    r0, c0, h, w = window
    clipped = np.where(mask[:, :, None], glt[r0:r0 + h, c0:c0 + w], 0).astype(np.int32)
    gx, gy = clipped[..., 0], clipped[..., 1]
    rec = np.zeros(RECORD, np.int32)
    rec[0], rec[1] = (int(gy[gy > 0].min()) - 1, int(gy[gy > 0].max()) - 1) if (gy > 0).any() else (I32_MAX, -1)
    rec[2], rec[3] = (int(gx[gx > 0].min()) - 1, int(gx[gx > 0].max()) - 1) if (gx > 0).any() else (I32_MAX, -1)
    rec[4] = int(((gx > 0) & (gy > 0)).sum())
    return clipped, rec


def glt_reindex_ref(clipped, rec):
    out = clipped.astype(np.int64)
    out[..., 0] = np.maximum(out[..., 0] - int(rec[2]), 0)
    out[..., 1] = np.maximum(out[..., 1] - int(rec[0]), 0)
    return out.astype(np.int32)


def class_counts_ref(plane, mask, window):
    """-> (counts (16,) int64 of the inside cells with hsr_scl_class_counts' bins, inside)."""
    r0, c0, h, w = window
    v = plane[r0:r0 + h, c0:c0 + w][mask].astype(np.int64)
    return np.bincount(np.minimum(v, 12), minlength=16).astype(np.int64), int(mask.sum())


def glt_of(H, W, rows, cols, seed):
    """A lookup table (H, W, 2) int32 of one-based (column, row) entries with no-data, negative and INT32_MIN entries."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    g = np.stack([1 + (xx * cols) // W, 1 + (yy * rows) // H], axis=-1).astype(np.int32)
    g[rng.random((H, W)) < 0.15] = 0
    g[..., 0][rng.random((H, W)) < 0.03] = 0
    g[..., 1][rng.random((H, W)) < 0.03] = -3
    g[rng.random((H, W)) < 0.01] = np.iinfo(np.int32).min
    return g


# ---- the table -------------------------------------------------------------------------------------------------------------------
def to_world(ring_px, gt):
    r = np.asarray(ring_px, np.float64).reshape(-1, 2)
    return np.stack([gt[0] + r[:, 0] * gt[1], gt[3] + r[:, 1] * gt[5]], axis=1)


def _frac(H, W, pts):
    """Vertices given as fractions of the grid, snapped to 1/64 pixel plus 1/128: off every centre and lattice line."""
    return [(math.floor(fx * W * 64) / 64 + 1 / 128, math.floor(fy * H * 64) / 64 + 1 / 128) for fx, fy in pts]


def triangle(H, W):
    return [_frac(H, W, [(0.12, 0.08), (0.93, 0.47), (0.31, 0.96)])]


def concave(H, W):
    return [_frac(H, W, [(0.05, 0.05), (0.95, 0.1), (0.9, 0.9), (0.6, 0.92), (0.62, 0.3), (0.3, 0.28), (0.33, 0.95), (0.08, 0.9)])]


def holed(H, W):
    return [_frac(H, W, [(0.05, 0.07), (0.94, 0.04), (0.96, 0.93), (0.03, 0.95)]), _frac(H, W, [(0.3, 0.3), (0.32, 0.7), (0.7, 0.68), (0.66, 0.27)])]


def two_parts(H, W):
    return [_frac(H, W, [(0.02, 0.1), (0.45, 0.05), (0.4, 0.8)]), _frac(H, W, [(0.55, 0.2), (0.98, 0.3), (0.9, 0.97), (0.6, 0.9)])]


def bow_tie(H, W):
    return [_frac(H, W, [(0.1, 0.1), (0.9, 0.9), (0.9, 0.1), (0.1, 0.9)])]


def overlapping(H, W):
    """Two parts that overlap: the overlap is OUTSIDE (even-odd over all rings; not a union)."""
    return [_frac(H, W, [(0.1, 0.1), (0.7, 0.1), (0.7, 0.7), (0.1, 0.7)]), _frac(H, W, [(0.4, 0.4), (0.95, 0.4), (0.95, 0.95), (0.4, 0.95)])]


def ripple(H, W, n=1500):
    """A 1500-vertex circle whose radius ripples 40 times: up to some eighty crossings in a row, short edges (the comb is the row with
    more than a thousand)."""
    t = 2 * np.pi * np.arange(n) / n
    r = 0.47 * (0.72 + 0.28 * np.cos(40 * t))
    return [np.stack([W * (0.5 + r * np.cos(t)) + 1 / 128, H * (0.5 + r * np.sin(t)) + 1 / 128], axis=1)]


def comb(H, W, n=1500):
    """A 1500-vertex zigzag from the top to the bottom of the grid and back: every row in between holds about n crossings."""
    i = np.arange(n)
    return [np.stack([(i + 0.37) * W / n, np.where(i % 2 == 0, 0.06 * H + 1 / 128, 0.94 * H + 1 / 128)], axis=1)]


def covering(H, W):
    return [[(-3.3, -2.2), (W + 4.1, -1.7), (W + 2.9, H + 3.3), (-2.6, H + 1.2)]]


def shifted(rings, du, dv):
    return [[(u + du, v + dv) for u, v in r] for r in rings]


def _row(H, W, rings_px, gt=GT_UTM, window=None, pad=0, off=0, world=None):
    return dict(H=H, W=W, gt=gt, rings=[to_world(r, gt) for r in rings_px] if world is None else world, window=window, pad=pad, off=off)


def _rows():
    rows = {}
    # grid sizes round the store run, the tile height and width, with strides and offsets of their own
    for W in (1, 15, 16, 17, 255, 256, 257):
        rows[f"w{W}"] = _row(37, W, triangle(37, W), pad=(W * 7) % 5, off=W % 3)
    for H in (1, 63, 64, 65):
        rows[f"h{H}"] = _row(H, 45, concave(H, 45), pad=3, off=1)
    rows["w16-aligned"] = _row(20, 16, holed(20, 16))                       # the 16-byte stores: stride and base multiples of 16
    rows["w256-aligned"] = _row(64, 256, holed(64, 256))
    rows["w300-stride320"] = _row(70, 300, concave(70, 300), pad=20)            # stride 320: 16-byte stores with a tail run
    # neither the base nor the stride on 16 bytes, as every real plane (10980 = 16 x 686 + 4): the interior of a row still goes in
    # 16-byte runs anchored on the address, with a head and a tail of single bytes that change from row to row
    rows["w274-dense-off3"] = _row(70, 274, holed(70, 274), off=3)             # stride 274 = 16 x 17 + 2, like 10980
    rows["w300-stride301"] = _row(66, 300, concave(66, 300), pad=1, off=1)     # an odd stride: every head length 0 .. 15 occurs
    rows["w20-stride21"] = _row(40, 20, triangle(40, 20), pad=1, off=2)        # rows shorter than head + one run
    rows["cross-tiles"] = _row(130, 520, holed(130, 520), pad=8)             # three tiles each way
    rows["cross-tiles-up"] = _row(130, 520, two_parts(130, 520), gt=GT_UP)
    for name, fn in (("triangle", triangle), ("concave", concave), ("holed", holed), ("two-parts", two_parts), ("bow-tie", bow_tie),
                     ("overlapping", overlapping)):
        rows[name] = _row(90, 140, fn(90, 140), pad=4)
        rows[name + "-up"] = _row(90, 140, fn(90, 140), gt=GT_UP, off=2)
    rows["ripple-1500"] = _row(70, 300, ripple(70, 300))
    rows["comb-1500"] = _row(40, 300, comb(40, 300), pad=5)
    rows["comb-1500-window"] = _row(40, 300, comb(40, 300), window=(7, 131, 20, 150))
    rows["outside"] = _row(30, 40, shifted(triangle(30, 40), 100, -200))
    rows["covering"] = _row(66, 258, covering(66, 258), pad=6, off=1)
    for name, du, dv in (("off-left", -0.6, 0.0), ("off-right", 0.6, 0.0), ("off-top", 0.0, -0.6), ("off-bottom", 0.0, 0.6)):
        rows[name] = _row(50, 80, shifted(holed(50, 80), du * 80, dv * 50), pad=1)
    # windows of every origin parity, inside one grid; the last leaves the first tile both ways
    for k, win in enumerate(((0, 0, 33, 41), (0, 1, 20, 299), (1, 0, 69, 17), (1, 1, 69, 299), (3, 250, 66, 50), (64, 256, 6, 44), (63, 255, 7, 45))):
        rows[f"window-{k}"] = _row(70, 300, holed(70, 300) + two_parts(70, 300), window=win, pad=k % 3, off=k % 2)
    big = COORD_MAX
    rows["huge-1e300"] = _row(40, 60, None, world=[np.array([[-big, -big], [big, 4099800.0], [600250.0, big]])])
    rows["huge-1e300-band"] = _row(40, 60, None, world=[np.array([[-big, 4099895.0], [big, 4099893.0], [big, 4099701.0], [-big, 4099707.0]])])
    rows["huge-tiny-pixels"] = _row(20, 30, None, gt=(0.0, 1e-9, 0.0, 0.0, 0.0, -1e-9), world=[np.array([[-big, big], [big, big], [1.2e-8, -1.7e-8]])])
    rows["zero-area"] = _row(30, 40, [[(3.2, 4.1), (30.7, 22.6), (3.2, 4.1), (30.7, 22.6)]])               # out and back
    rows["zero-area-point"] = _row(30, 40, [[(7.3, 9.6)] * 3])
    rows["collinear"] = _row(30, 40, [[(2.25, 3.25), (12.25, 13.25), (22.25, 23.25)]], gt=GT_EXACT)
    rows["closing-vertex"] = _row(30, 40, [triangle(30, 40)[0] + triangle(30, 40)[0][:1]])
    # the ties the header decides, on a grid whose round trip is exact
    e = dict(gt=GT_EXACT)
    rows["tie-vertex-on-centre"] = _row(20, 24, [[(3.5, 4.5), (20.5, 9.5), (8.5, 17.5)]], **e)
    rows["tie-horizontal-through-centres"] = _row(20, 24, [[(1.5, 4.5), (19.5, 4.5), (19.5, 12.5), (1.5, 12.5)]], **e)
    rows["tie-vertical-through-centres"] = _row(20, 24, [[(5.5, 1.25), (5.5, 17.75), (18.5, 17.75), (18.5, 1.25)]], **e)
    rows["tie-diagonal-through-centres"] = _row(20, 24, [[(1.5, 1.5), (16.5, 16.5), (1.5, 16.5)]], **e)
    rows["tie-lattice-rectangle"] = _row(20, 24, [[(2.0, 3.0), (19.0, 3.0), (19.0, 15.0), (2.0, 15.0)]], **e)
    rows["tie-lattice-diagonal"] = _row(20, 24, [[(1.0, 1.0), (17.0, 17.0), (1.0, 17.0)]], **e)
    rows["tie-lattice-antidiagonal"] = _row(20, 24, [[(17.0, 1.0), (1.0, 17.0), (17.0, 17.0)]], **e)
    rows["tie-lattice-window"] = _row(20, 24, [[(2.0, 3.0), (19.0, 3.0), (19.0, 15.0), (2.0, 15.0)]], window=(2, 1, 15, 20), **e)
    rows["tie-grid-edges"] = _row(20, 24, [[(0.0, 0.0), (24.0, 0.0), (24.0, 20.0), (0.0, 20.0)]], **e)
    return rows


ROWS = _rows()
EXTREME_ROWS = ("huge-1e300", "huge-1e300-band", "huge-tiny-pixels", "outside", "zero-area", "zero-area-point")


def window_of(r):
    return (0, 0, r["H"], r["W"]) if r["window"] is None else r["window"]


@functools.lru_cache(maxsize=None)
def case(name, rule):
    """-> the statement's (h, w) bool plane of the row, read-only."""
    r = ROWS[name]
    m = rasterize_ref(r["rings"], r["gt"], (r["H"], r["W"]), rule, r["window"])
    m.setflags(write=False)
    return m


def sweep_rows(seed=20260, count=24):
    """A seeded sweep: random grids, windows, strides and polygons of 3 to 40 vertices in one to three rings, some far outside."""
    rng = np.random.default_rng(seed)
    out = {}
    for k in range(count):
        H, W = int(rng.integers(1, 140)), int(rng.integers(1, 530))
        gt = (GT_UTM, GT_UP, (-118.5, 0.000542232520256367, 0.0, 35.25, 0.0, -0.000542232520256367))[k % 3]
        rings = []
        for _ in range(int(rng.integers(1, 4))):
            n = int(rng.integers(3, 41))
            rings.append(np.stack([rng.uniform(-0.3 * W - 2, 1.3 * W + 2, n), rng.uniform(-0.3 * H - 2, 1.3 * H + 2, n)], axis=1))
        win = None
        if k % 2:
            r0, c0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            win = (r0, c0, int(rng.integers(1, H - r0 + 1)), int(rng.integers(1, W - c0 + 1)))
        out[f"sweep-{k}"] = _row(H, W, rings, gt=gt, window=win, pad=int(rng.integers(0, 9)), off=int(rng.integers(0, 4)))
    return out


SWEEP = sweep_rows()


# ---- the centre rule's independent reference: matplotlib ---------------------------------------------------------------------------
def general_polygon(rng, H, W, margin=1e-6):
    """A seeded ring of 3 - 12 vertices in pixel coordinates with no edge within `margin` pixel of a cell centre -> (ring, redraws)."""
    cy, cx = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    p = np.stack([cx.ravel(), cy.ravel()], axis=1)
    redraws = 0
    while True:
        n = int(rng.integers(3, 13))
        ring = np.stack([rng.uniform(-0.2 * W, 1.2 * W, n), rng.uniform(-0.2 * H, 1.2 * H, n)], axis=1)
        a, b = ring, np.roll(ring, -1, axis=0)
        d = b - a
        t = np.clip(((p[:, None, :] - a[None]) * d[None]).sum(-1) / (d * d).sum(-1)[None], 0.0, 1.0)
        dist = np.linalg.norm(p[:, None, :] - (a[None] + t[..., None] * d[None]), axis=-1)
        if dist.min() >= margin:
            return ring, redraws
        redraws += 1


def contains_points_ref(rings_px, H, W):
    """Even-odd over all rings with matplotlib's point-in-path test of every centre, ring by ring -> (H, W) bool."""
    from matplotlib.path import Path
    cy, cx = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    p = np.stack([cx.ravel(), cy.ravel()], axis=1)
    inside = np.zeros(H * W, bool)
    for ring in rings_px:
        inside ^= Path(np.asarray(ring, np.float64), closed=False).contains_points(p)
    return inside.reshape(H, W)


# ---- the touched rule's independent reference: exact rationals -----------------------------------------------------------------------
def _u_on_line(a, b, v):
    """Exact u where the edge a -> b meets the line at height v (the edge is not horizontal)."""
    return a[0] + (v - a[1]) * (b[0] - a[0]) / (b[1] - a[1])


def dyadic_polygon(rng, H, W, margin=Fraction(1, 10 ** 9)):
    """A seeded ring of 3 - 7 vertices with coordinates k / 16, k odd (never on a lattice line, never on a centre line), redrawn when
    an exact crossing of a lattice row line lies within `margin` of a lattice column line, or an exact crossing of a centre row line
    within `margin` of a centre -> (ring of Fraction pairs, redraws)."""
    redraws = 0
    while True:
        n = int(rng.integers(3, 8))
        ring = [(Fraction(2 * int(rng.integers(-8 * W // 4, 8 * W + 8 * W // 4)) + 1, 16), Fraction(2 * int(rng.integers(-8 * H // 4, 8 * H + 8 * H // 4)) + 1, 16))
                for _ in range(n)]
        ok = True
        for i in range(n):
            a, b = ring[i], ring[(i + 1) % n]
            if a[1] == b[1]:
                continue
            lo, hi = min(a[1], b[1]), max(a[1], b[1])
            for line2 in range(2 * math.ceil(lo), 2 * math.floor(hi) + 1):          # v = line2 / 2: lattice lines and centre lines
                v = Fraction(line2, 2)
                if not lo <= v <= hi:
                    continue
                u = _u_on_line(a, b, v)
                near = u - Fraction(1, 2) if line2 % 2 else u                        # a centre line: distance to c + 1/2
                if abs(near - round(near)) < margin:
                    ok = False
        if ok:
            return ring, redraws
        redraws += 1


def _meets_closed_cell(a, b, r, c):
    """Liang - Barsky in exact arithmetic: does the segment a -> b meet [c, c + 1] x [r, r + 1]?"""
    t0, t1 = Fraction(0), Fraction(1)
    for p, q in ((-(b[0] - a[0]), a[0] - c), (b[0] - a[0], c + 1 - a[0]), (-(b[1] - a[1]), a[1] - r), (b[1] - a[1], r + 1 - a[1])):
        if p == 0:
            if q < 0:
                return False
        else:
            t = q / p
            if p < 0:
                t0 = max(t0, t)
            else:
                t1 = min(t1, t)
    return t0 <= t1


def touched_exact_ref(rings, H, W):
    """"The boundary meets the closed cell or the centre is inside (even-odd)", exactly -> (H, W) bool."""
    out = np.zeros((H, W), bool)
    edges = [(ring[i], ring[(i + 1) % len(ring)]) for ring in rings for i in range(len(ring))]
    for r in range(H):
        pv = Fraction(2 * r + 1, 2)
        xs = [_u_on_line(a, b, pv) for a, b in edges if (a[1] <= pv) != (b[1] <= pv)]
        for c in range(W):
            inside = sum(1 for x in xs if Fraction(2 * c + 1, 2) < x) % 2 == 1
            out[r, c] = inside or any(_meets_closed_cell(a, b, r, c) for a, b in edges)
    return out
