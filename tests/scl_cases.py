"""The case tables of the scene-classification kernels (csrc/hsr_scl.hip, include/hsr_scl.h) and the NumPy references they are
compared with.  No GPU, no library; not a test module.

Every output of the family is an integer or a copied bit pattern, so every comparison is an equality.

References
    counts_ref    np.unique(scl, return_counts=True) per window, as scl_metrics does for the whole plane (cloud_utils.py:87-89),
                  folded into the header's bins; metrics_ref / cloud_pixels_ref restate cloud_utils.py:87-101 and :49-53 on an
                  array (the reference's functions open rasters through rasterio, which is absent: there is no golden fixture);
    dilate_ref    the mask from its definition: the OR of one zero-padded shifted copy of the grow flags per offset of the
                  structuring element - no rows, no distances, no table of half widths;
    coarse_ref    block counts by reshape;  gather_ref  host slicing;  apply_ref  NumPy masking.
Sizes follow the kernels' loop bounds (a 64 x 32 mask tile, a wave of 64 lanes, 16-byte segments), not the workload: nothing is
larger than about 300 x 400."""
import functools
from math import comb

import numpy as np

BINS, MAX_RADIUS, DISC, SQUARE, MAX_K = 16, 32, 0, 1, 16
TILE_W, TILE_H = 64, 32                                   # the mask kernel's output tile
SENT = 0xA5                                               # gpu_harness.FILL
SHAPES = {"disc": DISC, "square": SQUARE}
VALUES = np.array(list(range(13)) + [31, 32, 255], dtype=np.uint8)      # every class, the first "other", both sides of bit 31
RADII = (0, 1, 2, 5, 16, 32)
WIDTHS = (1, 63, 64, 65, 127, 128, 129, 165)              # 165 = two tiles and a remainder
HEIGHTS = (1, TILE_H - 1, TILE_H + 1)
DENSITIES = (0.001, 0.05, 0.5)


def all_instances():
    return ["scl_counts_kernel", "scl_mask_kernel<LOOKUP>", "scl_mask_kernel<DISC>", "scl_mask_kernel<SQUARE>", "scl_coarse_kernel",
            "scl_gather_kernel", "scl_apply_kernel<UP1>", "scl_apply_kernel<UP2>"]


def bits(classes):
    out = 0
    for c in classes:
        out |= 1 << c
    return out


def strided(a, rs, fill=SENT):
    """The (H, W) plane `a` laid out with a row stride of rs elements: (H - 1) rs + W elements, the gaps holding `fill`."""
    H, W = a.shape
    buf = np.full((H - 1) * rs + W, fill, dtype=a.dtype)
    for y in range(H):
        buf[y * rs: y * rs + W] = a[y]
    return buf


def unstrided(buf, H, W, rs):
    """-> (the (H, W) plane, the gap elements)."""
    rows = np.stack([buf[y * rs: y * rs + W] for y in range(H)])
    gaps = np.concatenate([buf[y * rs + W: (y + 1) * rs] for y in range(H - 1)]) if H > 1 else buf[:0]
    return rows, gaps


# ---- references ---------------------------------------------------------------------------------------------------------------------
def counts_ref(scl, th, tw):
    H, W = scl.shape
    out = np.zeros((H // th, W // tw, BINS), dtype=np.int32)
    for i in range(H // th):
        for j in range(W // tw):
            vals, counts = np.unique(scl[i * th:(i + 1) * th, j * tw:(j + 1) * tw], return_counts=True)     # cloud_utils.py:87
            for v, c in zip(vals, counts):
                out[i, j, int(v) if v < 12 else 12] += c
    return out


def metrics_ref(scl, names, include_shadows=False):
    """cloud_utils.py:87-101 on the array."""
    vals, counts = np.unique(scl, return_counts=True)
    total = int(counts.sum())
    by_class = {int(v): int(c) for v, c in zip(vals, counts)}
    valid_mask = scl != 0
    cloud_set = {8, 9, 10} | ({3} if include_shadows else set())
    cloud_px = int(np.isin(scl, list(cloud_set))[valid_mask].sum())
    valid_px = int(valid_mask.sum())
    return {"total_px": total, "valid_px": valid_px, "nodata_px": by_class.get(0, 0), "cloud_px": cloud_px,
            "cloud_frac_valid": (cloud_px / valid_px) if valid_px else np.nan,
            "class_counts": {names.get(k, str(k)): v for k, v in by_class.items()}}


def cloud_pixels_ref(scl, cloud_classes):
    """cloud_utils.py:49-53 on the array."""
    valid = scl != 0
    return int(np.isin(scl[valid], list(cloud_classes)).sum()), int(valid.sum())


def class_flags(scl, set_bits):
    lut = np.array([(set_bits >> v) & 1 if v < 32 else 0 for v in range(256)], dtype=np.uint8)
    return lut[scl]


def dilate_ref(scl, grow_bits, flat_bits, r, shape):
    H, W = scl.shape
    g = class_flags(scl, grow_bits)
    pad = np.zeros((H + 2 * r, W + 2 * r), dtype=np.uint8)
    pad[r:r + H, r:r + W] = g
    out = class_flags(scl, flat_bits).copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            inside = dy * dy + dx * dx <= r * r if shape == DISC else max(abs(dy), abs(dx)) <= r
            if inside:
                out |= pad[r + dy:r + dy + H, r + dx:r + dx + W]
    return out


def coarse_ref(mask, k, max_bad, cell=None):
    """-> clear, cell_bad, win_counts (None without a cell)."""
    H, W = mask.shape
    hc, wc = H // k, W // k
    n = (mask[:hc * k, :wc * k] != 0).reshape(hc, k, wc, k).sum(axis=(1, 3))
    clear = (n <= max_bad).astype(np.uint8)
    win = None
    if cell is not None:
        ch, cw = cell
        win = (1 - clear[:hc // ch * ch, :wc // cw * cw].astype(np.int32)).reshape(hc // ch, ch, wc // cw, cw).sum(axis=(1, 3)).astype(np.int32)
    return clear, np.minimum(n, 255).astype(np.uint8), win


def gather_ref(plane, origins, th, tw):
    H, W = plane.shape
    out = np.full((len(origins), th, tw), SENT, dtype=np.uint8)
    for i, (r, c) in enumerate(origins):
        if r >= 0 and c >= 0 and r + th <= H and c + tw <= W:
            out[i] = plane[r:r + th, c:c + tw]
    return out


def apply_ref(cube, mask, up, fill):
    T, H, W = cube.shape
    m = np.repeat(np.repeat(mask != 0, up, axis=0), up, axis=1)[:H, :W]
    out = cube.copy()
    out[:, m] = np.float32(fill)
    return out, int(m.sum())


# ---- the mask rows ------------------------------------------------------------------------------------------------------------------
GROW, FLAT = bits([8, 9, 10]), bits([0, 1])
POSITIONS = ("tl", "tr", "bl", "br", "top", "bottom", "left", "right", "centre")


def _mask_row(H, W, r, shape, content, rs=None, mrs=None, grow=GROW, flat=FLAT, seed=0, off=0):
    return dict(H=H, W=W, r=r, shape=shape, content=content, rs=W + 5 if rs is None else rs, mrs=W + 3 if mrs is None else mrs, grow=grow,
                flat=flat, seed=seed, off=off)


def _mask_rows():
    rows = {}
    for sname, shape in SHAPES.items():
        for r in RADII[1:]:                                # a single flag: the output is exactly the clipped disc / square
            for pos in POSITIONS:
                rows[f"single-{pos}-{sname}-r{r}"] = _mask_row(45, 131, r, shape, ("single", pos))
        for r in RADII:
            for d in DENSITIES:
                rows[f"random-{d}-{sname}-r{r}"] = _mask_row(70, 150, r, shape, ("random", d), seed=r + 1)
            rows[f"none-{sname}-r{r}"] = _mask_row(40, 70, r, shape, ("random", 0.0))
            rows[f"all-{sname}-r{r}"] = _mask_row(40, 70, r, shape, ("random", 1.0))
        for W in WIDTHS:
            for H in HEIGHTS:
                rows[f"size-{H}x{W}-{sname}"] = _mask_row(H, W, 5 if shape == DISC else 2, shape, ("random", 0.05), seed=H + W)
        for H, W, r in ((3, 5, 16), (1, 1, 32), (10, 20, 32), (2, 70, 5)):     # planes smaller than r
            rows[f"small-{H}x{W}-{sname}-r{r}"] = _mask_row(H, W, r, shape, ("random", 0.2), seed=H)
        rows[f"values-{sname}-r2"] = _mask_row(50, 100, 2, shape, ("values",), grow=bits([8, 9, 10, 31]), flat=bits([0, 1, 12]))
    rows["big-disc-r5"] = _mask_row(300, 400, 5, DISC, ("random", 0.01), seed=3)
    # the lookup instance: 16-byte rows (bases and strides multiples of 16) with a byte tail, and rows that are not
    rows["lookup-vec"] = _mask_row(9, 165, 0, DISC, ("values",), rs=176, mrs=192, grow=bits([8, 9, 10, 31]), flat=bits([0, 1, 12]))
    rows["lookup-vec-exact"] = _mask_row(5, 4096 + 128, 0, SQUARE, ("values",), rs=4096 + 128, mrs=4096 + 128, grow=bits([3, 31]), flat=bits([0]))
    rows["lookup-unaligned-base"] = _mask_row(9, 165, 0, DISC, ("values",), rs=176, mrs=192, off=3)
    rows["lookup-odd-stride"] = _mask_row(9, 165, 0, DISC, ("values",), rs=171, mrs=167)
    return rows


MASK_ROWS = _mask_rows()


@functools.lru_cache(maxsize=None)
def mask_plane(name):
    r = MASK_ROWS[name]
    H, W, rng = r["H"], r["W"], np.random.default_rng(r["seed"])
    kind = r["content"][0]
    if kind == "single":
        scl = np.full((H, W), 4, dtype=np.uint8)
        y, x = {"tl": (0, 0), "tr": (0, W - 1), "bl": (H - 1, 0), "br": (H - 1, W - 1), "top": (0, W // 2), "bottom": (H - 1, W // 2),
                "left": (H // 2, 0), "right": (H // 2, W - 1), "centre": (H // 2, W // 2)}[r["content"][1]]
        scl[y, x] = 9
    elif kind == "random":
        scl = np.where(rng.random((H, W)) < r["content"][1], rng.choice([8, 9, 10], size=(H, W)), rng.choice([4, 5, 6, 7, 0], size=(H, W),
                       p=[0.4, 0.3, 0.2, 0.09, 0.01])).astype(np.uint8)
    else:
        scl = rng.choice(VALUES, size=(H, W)).astype(np.uint8)
    scl.setflags(write=False)
    return scl


@functools.lru_cache(maxsize=None)
def mask_ref(name):
    r = MASK_ROWS[name]
    out = dilate_ref(mask_plane(name), r["grow"], r["flat"], r["r"], r["shape"])
    out.setflags(write=False)
    return out


def mask_instance(r, shape):
    return "scl_mask_kernel<%s>" % ("LOOKUP" if r == 0 else ("DISC", "SQUARE")[shape])


# ---- counts, coarse, gather, apply ---------------------------------------------------------------------------------------------------
# H, W, rs, tile_h, tile_w, off (bytes past a 256-byte boundary: the 16-byte segments of a row start anywhere)
COUNT_ROWS = {
    "one-pixel": (1, 1, 1, 1, 1, 0),
    "whole-plane": (37, 165, 170, 37, 165, 0),
    "whole-plane-off3": (37, 165, 165, 37, 165, 3),
    "tile-8": (70, 150, 160, 8, 8, 0),
    "tile-33x64-off5": (70, 150, 151, 33, 64, 5),
    "tile-1": (5, 40, 48, 1, 1, 0),
    "tile-3x17": (20, 70, 70, 3, 17, 1),
    "rows-only": (300, 15, 16, 300, 15, 0),
    "wide": (3, 400, 400, 3, 400, 7),
}


@functools.lru_cache(maxsize=None)
def count_plane(name):
    H, W = COUNT_ROWS[name][:2]
    scl = np.random.default_rng(len(name)).choice(VALUES, size=(H, W)).astype(np.uint8)
    scl.setflags(write=False)
    return scl


def _coarse_rows():
    rows, cells = {}, (None, (2, 3), (1, 1), (3, 2))
    n = 0
    for k in (1, 2, 3, 6, 16):
        for max_bad in (0, 1, k * k - 1, k * k):
            cell = cells[n % 4]
            rows[f"k{k}-bad{max_bad}"] = dict(H=100, W=135, rs=140, k=k, max_bad=max_bad, cell=cell, cell_bad=n % 2 == 0, density=0.3 if k < 6 else 0.9)
            n += 1
    rows["k16-all-set"] = dict(H=64, W=48, rs=48, k=16, max_bad=255, cell=(2, 2), cell_bad=True, density=1.0)   # 256 in a block: stored as 255
    rows["k6-exact-windows"] = dict(H=120, W=180, rs=180, k=6, max_bad=0, cell=(10, 10), cell_bad=False, density=0.02)
    rows["k6-leftover-windows"] = dict(H=130, W=400, rs=401, k=6, max_bad=0, cell=(10, 20), cell_bad=True, density=0.02)
    rows["k3-wide-windows"] = dict(H=30, W=399, rs=399, k=3, max_bad=2, cell=(3, 100), cell_bad=False, density=0.4)  # a wave inside one window
    return rows


COARSE_ROWS = _coarse_rows()


@functools.lru_cache(maxsize=None)
def coarse_plane(name):
    r = COARSE_ROWS[name]
    rng = np.random.default_rng(len(name) + r["k"])
    m = (rng.random((r["H"], r["W"])) < r["density"]).astype(np.uint8) * rng.choice([1, 1, 7, 255], size=(r["H"], r["W"])).astype(np.uint8)
    m.setflags(write=False)
    return m


# H, W, rs, th, tw, origins: inside, duplicated, touching the far edge, leaving the plane on every side
GATHER_ROWS = {
    "tiles-8x12": (60, 90, 96, 8, 12, [(0, 0), (5, 7), (5, 7), (52, 78), (52, 0), (0, 78), (53, 78), (52, 79), (-1, 0), (0, -1), (60, 90),
                                        (2 ** 31 - 8, 0), (0, 2 ** 31 - 12), (-2 ** 31, -2 ** 31), (20, 30)]),
    "one-pixel": (5, 7, 7, 1, 1, [(4, 6), (0, 0), (5, 6), (4, 7)]),
    "whole-plane": (33, 65, 70, 33, 65, [(0, 0), (1, 0), (0, 0)]),
    "tile-20": (43, 62, 62, 20, 20, [(0, 0), (0, 20), (20, 40), (23, 42), (24, 42)]),
    "long-tile": (70, 300, 300, 69, 299, [(1, 1), (2, 1)]),
}


@functools.lru_cache(maxsize=None)
def gather_plane(name):
    H, W = GATHER_ROWS[name][:2]
    p = np.random.default_rng(len(name)).integers(0, 256, size=(H, W)).astype(np.uint8)
    p.setflags(write=False)
    return p


# T, H, W, rs, bs, up, fill, density
APPLY_ROWS = {
    "up1-nan": (5, 37, 75, 78, 37 * 78 + 7, 1, np.nan, 0.3),
    "up2-nan": (5, 37, 75, 78, 37 * 78 + 7, 2, np.nan, 0.3),
    "up1-fill": (1, 37, 75, 75, 37 * 75, 1, -9999.0, 0.3),
    "up2-fill": (1, 37, 75, 75, 37 * 75, 2, -9999.0, 0.3),
    "up1-clear": (5, 33, 300, 300, 33 * 300, 1, np.nan, 0.0),
    "up2-all": (5, 33, 300, 301, 33 * 301, 2, -9999.0, 1.0),
    "up2-wide": (2, 3, 401, 401, 3 * 401, 2, np.nan, 0.5),
    "up1-one": (1, 1, 1, 1, 1, 1, np.nan, 1.0),
    "up1-vec": (3, 33, 300, 304, 33 * 304, 1, np.nan, 0.7),          # strides in multiples of four: 16-byte stores under runs of the mask
    "up2-vec": (2, 34, 302, 304, 34 * 304 + 4, 2, -9999.0, 0.6),
}


@functools.lru_cache(maxsize=None)
def apply_case(name):
    T, H, W, rs, bs, up, fill, density = APPLY_ROWS[name]
    rng = np.random.default_rng(len(name) + up)
    cube = rng.standard_normal((T, H, W)).astype(np.float32)
    Hm, Wm = -(-H // up), -(-W // up)
    mask = (rng.random((Hm, Wm)) < density).astype(np.uint8) * rng.choice([1, 2, 255], size=(Hm, Wm)).astype(np.uint8)
    ref, count = apply_ref(cube, mask, up, fill)
    for a in (cube, mask, ref):
        a.setflags(write=False)
    return dict(cube=cube, mask=mask, mrs=Wm + 2, ref=ref, count=count)


# ---- the driver scenes: tests/test_gpu_scene_tiles.py's pair with an SCL ---------------------------------------------------------------
T20, F, NB, DEGREE, BANDS_OUT = 20, 6, 3, 2, 4
N_FEATURES = comb(NB + DEGREE, DEGREE)                     # the monomials of degree <= 2 in 3 variables, the constant among them


@functools.lru_cache(maxsize=None)
def scene_pair():
    """EMIT (12, 43, 62) float32 and S2 (3, 258, 372) float32 as tests/test_gpu_scene_tiles.py builds them: 2 x 3 windows of 20 x 20
    at factor 6 with remainders on both sides; window (0, 1) is black on the EMIT side, window (1, 2) on the S2 side."""
    rng = np.random.default_rng(20)
    h, w = 43, 62
    yy, xx = np.mgrid[0:h * F, 0:w * F].astype(np.float32)
    s2 = np.stack([0.25 + 0.2 * np.sin(yy / (9 + 3 * c) + c) * np.cos(xx / (11 + 2 * c)) for c in range(3)]).astype(np.float32)
    s2 += rng.normal(0, 0.01, s2.shape).astype(np.float32)
    coarse = s2.reshape(3, h, F, w, F).mean(axis=(2, 4))
    emit = np.stack([0.1 + 0.05 * b / 12 + (0.6 + 0.02 * b) * coarse[b % 3] + 0.2 * coarse[(b + 1) % 3] ** 2 for b in range(12)])
    emit = np.clip(emit + rng.normal(0, 0.003, emit.shape), 0.01, 0.95).astype(np.float32)
    emit[:, 0:20, 20:40] = -0.01
    s2[:, 120:240, 240:360] = 0.0
    emit[:, 5, 5] = np.nan
    for a in (emit, s2):
        a.setflags(write=False)
    return emit, s2


@functools.lru_cache(maxsize=None)
def scene_scl(up):
    """The SCL of the pair at 10 m (up 1: 258 x 372) or 20 m (up 2: 129 x 186), in S2 10 m pixels: a high cloud over about a
    fifth of window (0, 0), cirrus over most of window (1, 0) - more than half: the window is rejected -, a cloud shadow in window
    (1, 1), a strip of nodata along the right edge of window (0, 2) and a cloud that straddles windows (0, 2) and (1, 2)."""
    scl = np.full((258, 372), 4, dtype=np.uint8)
    scl[:, 186:] = 5
    scl[10:64, 20:70] = 9
    scl[130:230, 6:110] = 10
    scl[150:170, 150:200] = 3
    scl[0:120, 352:360] = 0
    scl[100:140, 250:300] = 8
    scl = scl[::up, ::up].copy()
    scl.setflags(write=False)
    return scl


def window_cloud_counts(clear, cell):
    """The not-clear cells of every cell x cell window of the (hc, wc) grid `clear`, floor."""
    hc, wc = clear.shape
    c = 1 - clear[:hc // cell * cell, :wc // cell * cell].astype(np.int64)
    return c.reshape(hc // cell, cell, wc // cell, cell).sum(axis=(1, 3))


# buffer, shape, up, stride, max_cloud_frac
DRIVER_ROWS = {
    "butted-10m": (2, "disc", 1, None, 0.5),
    "butted-20m": (1, "square", 2, None, 0.5),
    "half-stride-10m": (2, "disc", 1, 10, 0.5),
    "half-stride-20m": (0, "disc", 2, 10, 0.6),
}


@functools.lru_cache(maxsize=None)
def driver_case(name):
    """The NumPy side of a driver row: the buffered mask, the clear grid, the windows fuse_scene_clear must keep (those of the
    black rule that also pass the cloud fraction) and their clear training cells."""
    buffer, shape, up, stride, frac = DRIVER_ROWS[name]
    emit, s2 = scene_pair()
    scl = scene_scl(up)
    mask = dilate_ref(scl, GROW, FLAT, buffer, SHAPES[shape])
    k = F // up
    clear, _, _ = coarse_ref(mask, k, 0)
    step = stride or T20
    kept, train = [], []
    for r in range(0, 43 - T20 + 1, step):
        for c in range(0, 62 - T20 + 1, step):
            if r * F + T20 * F > 258 or c * F + T20 * F > 372:
                continue
            e, s = emit[:, r:r + T20, c:c + T20], s2[:, r * F:(r + T20) * F, c * F:(c + T20) * F]
            black_e = (np.abs(e + 0.01) <= 1e-3 + 1e-5 * 0.01).all(axis=0) | (np.abs(e) < 1e-6).all(axis=0)
            black_s = (np.abs(s + 0.01) <= 1e-3 + 1e-5 * 0.01).all(axis=0) | (np.abs(s) < 1e-6).all(axis=0)
            if black_e.any() or black_s.any():
                continue
            cl = clear[r:r + T20, c:c + T20]
            cloud_frac = int((cl == 0).sum()) / (T20 * T20)
            if cloud_frac <= frac:
                kept.append((r, c, cloud_frac))
                train.append(int((cl != 0).sum() - (np.isnan(e).any(axis=0) & (cl != 0)).sum()))
    return dict(scl=scl, mask=mask, clear=clear, k=k, up=up, kept=kept, train=train)
