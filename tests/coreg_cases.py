"""Case tables, references and bars of the co-registration family (include/hsr_coreg.h); NumPy / SciPy only, not a test module.

Scenes.  Gaussian-filtered noise (sigma 2 and 6 S2 pixels, each normalised, summed, scaled to [0, 1]) is the S2 scene T; the EMIT
scene is the block mean of T displaced by a known shift field with an order-3 spline, E(i, j) = mean T(f i + a + dy, f j + b + dx):
the sign convention of the header, so the truth at a tie point is the field at its window centre.

References and bars.
  surface  np.longdouble, two-pass.  Bar per entry 8 n eps64 sqrt(sum e^2 sum m^2) / sqrt(S_ee S_mm): the cancellation bound of
           any fixed-order float64 evaluation from sums.  The table's own conditions (tests/test_coreg_host.py): every finite
           entry's bar <= 1e-8, and the peak's margin over every other entry >= 1e-4, so a kernel inside the bars has the
           reference's peak.
  peaks    the header's statements in float64, one for one: bit equality.
  model    np.linalg.lstsq on the same rows in the scaled coordinates of the header; bar 64 n eps64 cond(G) max|d| on the scaled
           coefficients (G the 3 x 3 Gram of the rows used; cond = 1 for a translation).
  warp     the header's statements in float64, one for one: bit equality.
"""
import functools

import numpy as np
from scipy import ndimage

LD = np.longdouble
EPS = 2.0 ** -52
REC, MODEL = 8, 10
OK, OUTSIDE, NO_SCORE, BORDER, LOW_SCORE, OUTLIER = range(6)
BAR_CAP, MARGIN = 1e-8, 1e-4
PAD = 32                                    # S2 pixels of scene beyond every edge, for the displaced sampling
TILE_W, TILE_H, LDS_LIMIT = 64, 16, 32 * 1024


def all_instances():
    return ["coreg_surface_kernel<float>", "coreg_surface_kernel<uint16_t>", "coreg_peaks_kernel", "coreg_fit_model_kernel",
            "coreg_warp_kernel<float, LDS>", "coreg_warp_kernel<float, DIRECT>",
            "coreg_warp_kernel<uint16_t, LDS>", "coreg_warp_kernel<uint16_t, DIRECT>"]


# =============================================================================================================================
# scenes
# =============================================================================================================================
def shift_field(model, y, x):
    """(dy, dx) of the 10-double model at (y, x), the header's expression in float64."""
    m = np.asarray(model, np.float64)
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    dy = (m[0] + m[1] * (x - m[6])) + m[2] * (y - m[7])
    dx = (m[3] + m[4] * (x - m[6])) + m[5] * (y - m[7])
    return dy, dx


def make_model(hs, ws, dy0=0.0, dx0=0.0, dy_x=0.0, dy_y=0.0, dx_x=0.0, dx_y=0.0, kind=1, n=0):
    return np.array([dy0, dy_x, dy_y, dx0, dx_x, dx_y, 0.5 * (ws - 1), 0.5 * (hs - 1), n, kind], np.float64)


@functools.lru_cache(maxsize=None)
def texture(hs, ws, seed):
    """(hs + 2 PAD, ws + 2 PAD) float64 in [0, 1]."""
    rng = np.random.default_rng(seed)
    shape = (hs + 2 * PAD, ws + 2 * PAD)
    a = ndimage.gaussian_filter(rng.standard_normal(shape), 2.0, mode="wrap")
    b = ndimage.gaussian_filter(rng.standard_normal(shape), 6.0, mode="wrap")
    t = a / a.std() + b / b.std()
    t = (t - t.min()) / (t.max() - t.min())
    t.setflags(write=False)
    return t


def scene_pair(he, we, f, model, seed, dtype="f32", hs=None, ws=None):
    """(emit (he, we) float32, s2 (hs, ws) float32 or uint16; hs, ws default to he f, we f).  S2 is the texture, cut to (hs, ws);
    EMIT the block mean of the texture displaced by `model` (order-3 spline) over its own he f x we f S2 pixels, whatever the cut."""
    he_s, we_s = he * f, we * f
    hs, ws = he_s if hs is None else hs, we_s if ws is None else ws
    t = texture(max(hs, he_s), max(ws, we_s), seed)
    yy, xx = np.meshgrid(np.arange(he_s, dtype=np.float64), np.arange(we_s, dtype=np.float64), indexing="ij")
    dy, dx = shift_field(model, yy, xx)
    disp = ndimage.map_coordinates(t, [yy + dy + PAD, xx + dx + PAD], order=3, mode="nearest")
    emit = disp.reshape(he, f, we, f).mean(axis=(1, 3)).astype(np.float32)
    s2 = t[PAD:PAD + hs, PAD:PAD + ws]
    s2 = np.round(s2 * 10000.0).astype(np.uint16) if dtype == "u16" else s2.astype(np.float32)
    return emit, np.ascontiguousarray(s2)


def strided(a, extra, sentinel):
    """A copy of the 2-D `a` inside rows `extra` elements longer (filled with `sentinel`): (view, row stride, backing array)."""
    back = np.full((a.shape[0], a.shape[1] + extra), sentinel, dtype=a.dtype)
    back[:, :a.shape[1]] = a
    return back[:, :a.shape[1]], a.shape[1] + extra, back


# =============================================================================================================================
# stage 1: surfaces
# =============================================================================================================================
def region_inside(i0, j0, w, f, R, he, we, hs, ws):
    return (i0 >= 0 and j0 >= 0 and i0 + w <= he and j0 + w <= we and f * i0 - R >= 0 and f * j0 - R >= 0
            and f * (i0 + w - 1) + R + f - 1 <= hs - 1 and f * (j0 + w - 1) + R + f - 1 <= ws - 1)


def s2_valid(a, nodata):
    ok = np.isfinite(a.astype(np.float64))
    if nodata is not None:
        ok &= a.astype(np.float64) != float(nodata)
    return ok


def surface_ref(emit, mask, s2, nodata, origins, w, f, R, min_valid):
    """(surface, bar), both (P, 2R+1, 2R+1) float64; long double, two-pass."""
    he, we = emit.shape
    hs, ws = s2.shape
    D = 2 * R + 1
    surf = np.full((len(origins), D, D), np.nan)
    bar = np.full((len(origins), D, D), np.nan)
    for p, (i0, j0) in enumerate(np.asarray(origins, np.int64)):
        if not region_inside(i0, j0, w, f, R, he, we, hs, ws):
            continue
        e = emit[i0:i0 + w, j0:j0 + w]
        ev = np.isfinite(e)
        if mask is not None:
            ev &= mask[i0:i0 + w, j0:j0 + w] != 0
        n_reg = f * w + 2 * R
        reg = s2[f * i0 - R:f * i0 - R + n_reg, f * j0 - R:f * j0 - R + n_reg]
        rv = s2_valid(reg, nodata)
        regl = np.where(rv, reg, 0).astype(LD)
        nb = n_reg - f + 1
        box, bad = np.zeros((nb, nb), LD), np.zeros((nb, nb), np.int64)
        for a in range(f):
            for b in range(f):
                box += regl[a:a + nb, b:b + nb]
                bad += ~rv[a:a + nb, b:b + nb]
        el = np.where(ev, e, 0).astype(LD)
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                m = box[dy + R::f, dx + R::f][:w, :w]
                pair = ev & (bad[dy + R::f, dx + R::f][:w, :w] == 0)
                n = int(pair.sum())
                if n < min_valid:
                    continue
                e_, m_ = el[pair], m[pair]
                if e_.max() == e_.min() or m_.max() == m_.min():
                    continue
                de, dm = e_ - e_.sum() / n, m_ - m_.sum() / n
                see, smm, sem = (de * de).sum(), (dm * dm).sum(), (de * dm).sum()
                surf[p, dy + R, dx + R] = float(sem / np.sqrt(see * smm))
                bar[p, dy + R, dx + R] = float(8 * n * EPS * np.sqrt((e_ * e_).sum() * (m_ * m_).sum()) / np.sqrt(see * smm))
    return surf, bar


def peak_margin(surface):
    """The peak's margin over every other finite entry (inf with fewer than two finite entries)."""
    v = np.sort(surface[np.isfinite(surface)])
    return float(v[-1] - v[-2]) if v.size >= 2 else np.inf


# name: he, we (EMIT), f, w, R, origins, dtype, extra (row-stride padding, elements), mask, min_valid, truth (dy0, dx0), seed
#   mask: none | part (a black S2 rectangle = nodata / NaN, and a masked EMIT corner) | all (every EMIT pixel masked)
#   min_valid: an int, or "met" / "missed": exactly the count of valid pairs of the worst candidate, and one more
#   hs, ws: the S2 plane, default f he, f we.  pads: (EMIT, S2, mask) row-stride paddings of their own, default `extra` for all
#   three.  offs: (EMIT, S2, mask) base offsets in bytes past a 256-byte boundary, default (4, 12 or 2 for uint16, 1).
#   inside: what the region test must say of every origin, for the rows whose origins straddle it
#   black, corner, hole, emit_nan, s2_inf: where mask == "part" puts what it plants - the black S2 rectangle (r0, r1, c0, c1), whose
#   last five rows are NaN for float32; the masked EMIT corner (rows, columns); one more masked EMIT pixel; one NaN EMIT pixel; one
#   +inf S2 sample (float32)
def _srow(he, we, f, w, R, origins, dtype="f32", extra=0, mask="none", min_valid=None, truth=(0.0, 0.0), seed=1, const=False,
          hs=None, ws=None, pads=None, offs=None, inside=None, black=(60, 75, 58, 80), corner=(4, 5), hole=(10, 10),
          emit_nan=(12, 11), s2_inf=(76, 60)):
    return dict(he=he, we=we, f=f, w=w, R=R, origins=origins, dtype=dtype, extra=extra, mask=mask,
                min_valid=min_valid if min_valid is not None else max(1, (3 * w * w + 3) // 4), truth=truth, seed=seed, const=const,
                hs=he * f if hs is None else hs, ws=we * f if ws is None else ws, pads=pads if pads is not None else (extra,) * 3,
                offs=offs if offs is not None else (4, 2 if dtype == "u16" else 12, 1), inside=inside, black=black, corner=corner,
                hole=hole, emit_nan=emit_nan, s2_inf=s2_inf)


surface_row = _srow                                # the pure constructor, under the name the sweeps use


def _grid65():
    return [(2 + 2 * (k // 13), 2 + 2 * (k % 13)) for k in range(65)]


SURFACE_ROWS = {
    # loop bounds: w in {4, 8, 9, 32, 64}, R in {1, 3, 6, 7, 12, 24} (R < f, = f, > f), f in {1, 2, 6}, P in {1, 2, 65}
    "w8-R3-f6": _srow(16, 16, 6, 8, 3, [(3, 4)], truth=(1.3, -0.6)),
    "w4-R1-f6": _srow(16, 16, 6, 4, 1, [(2, 3), (9, 8)], truth=(0.2, -0.3), seed=2),
    "w9-R6-f6": _srow(16, 16, 6, 9, 6, [(2, 3), (5, 4)], truth=(-2.4, 3.1), seed=3, extra=5),
    "w8-R7-f6": _srow(16, 16, 6, 8, 7, [(4, 4)], truth=(4.2, -3.3), seed=4),
    "w32-R12-f6": _srow(40, 40, 6, 32, 12, [(3, 4)], truth=(-5.5, 7.25), seed=5, extra=3),
    "w32-R24-f6": _srow(48, 48, 6, 32, 24, [(6, 8)], truth=(10.5, -14.2), seed=6),
    "w8-R3-f1": _srow(40, 40, 1, 8, 3, [(5, 6), (20, 21)], truth=(1.0, -2.0), seed=7),
    "w64-R24-f1": _srow(120, 120, 1, 64, 24, [(25, 27)], truth=(-6.0, 9.0), seed=8),
    "w64-R3-f2": _srow(72, 72, 2, 64, 3, [(3, 4)], truth=(1.6, 0.4), seed=9, dtype="u16", extra=2),
    "w9-R7-f2": _srow(40, 40, 2, 9, 7, [(6, 5), (20, 18)], truth=(-3.2, 2.7), seed=10),
    "P65-w8-R3-f6": _srow(40, 40, 6, 8, 3, _grid65(), truth=(0.7, -1.2), seed=11),
    "P65-u16": _srow(40, 40, 6, 8, 3, _grid65(), truth=(-1.1, 0.4), seed=12, dtype="u16", extra=6),
    "u16-w32-R12": _srow(40, 40, 6, 32, 12, [(3, 4), (4, 3)], truth=(3.0, -4.0), seed=13, dtype="u16"),
    # masks and validity
    "mask-part": _srow(24, 24, 6, 8, 6, [(2, 2), (8, 8), (13, 12)], mask="part", truth=(1.3, -0.7), seed=14, min_valid=20),
    "mask-part-u16": _srow(24, 24, 6, 8, 6, [(2, 2), (8, 8), (13, 12)], mask="part", truth=(1.3, -0.7), seed=15, min_valid=20,
                           dtype="u16"),
    "mask-all": _srow(16, 16, 6, 8, 3, [(3, 4)], mask="all", seed=16),
    "constant": _srow(16, 16, 6, 8, 3, [(3, 4), (1, 1)], seed=17, const=True),
    "min-valid-met": _srow(24, 24, 6, 8, 6, [(8, 8)], mask="part", truth=(1.3, -0.7), seed=14, min_valid="met"),
    "min-valid-missed": _srow(24, 24, 6, 8, 6, [(8, 8)], mask="part", truth=(1.3, -0.7), seed=14, min_valid="missed"),
    # the four edges, touched (R = f: f i0 - R = 0 at i0 = 1; f (i0 + w) + R = hs at i0 = 15) and crossed
    "edges": _srow(24, 24, 6, 8, 6, [(1, 5), (0, 5), (15, 5), (16, 5), (5, 1), (5, 0), (5, 15), (5, 16), (1, 1), (15, 15), (-1, 5),
                                     (5, -3), (17, 5), (5, 40)], truth=(1.0, 1.0), seed=18),
    # rectangular planes, f in {3, 4, 5, 7, 8}; R above and equal to f here, below it in strides-mask-u16
    "rect-f3-R4": _srow(20, 34, 3, 8, 4, [(3, 5), (9, 20)], truth=(1.3, -2.4), seed=31),
    "rect-f4-R5": _srow(30, 18, 4, 9, 5, [(4, 2), (17, 7)], truth=(-2.3, 3.2), seed=32, dtype="u16"),
    "rect-f5-R5": _srow(18, 26, 5, 8, 5, [(2, 11), (8, 3)], truth=(3.3, -1.7), seed=33),
    "rect-f7-R9": _srow(14, 22, 7, 9, 9, [(2, 9), (3, 4)], truth=(-6.2, 4.4), seed=34, dtype="u16"),
    "rect-f8-R8": _srow(22, 13, 8, 8, 8, [(9, 1), (3, 4)], truth=(5.3, -6.7), seed=35),
    "rect-f8-R24": _srow(16, 26, 8, 8, 24, [(4, 9)], truth=(-13.3, 17.25), seed=36, dtype="u16"),
    # strides of their own: the EMIT plane, the S2 plane and the mask padded by three different amounts, at three different offsets
    "strides-mask": _srow(24, 30, 6, 8, 6, [(2, 2), (8, 8), (13, 12), (4, 20)], mask="part", truth=(1.3, -0.7), seed=37, min_valid=20,
                          pads=(5, 11, 3), offs=(8, 20, 3)),
    "strides-mask-u16": _srow(20, 28, 4, 8, 3, [(2, 2), (9, 12), (11, 3)], mask="part", truth=(0.7, -1.2), seed=38, min_valid=20,
                              dtype="u16", pads=(7, 2, 13), offs=(12, 6, 2)),
    # an S2 plane that is not f x EMIT.  short-wide: rows i0 <= 12 by EMIT but <= 8 by S2, columns j0 <= 8 by EMIT but <= 10 by S2, so
    # (9, 4) passes the EMIT bound and fails the S2 bound on rows, (4, 9) the reverse on columns; tall-narrow is its transpose
    "s2-short-wide": _srow(20, 16, 6, 8, 6, [(1, 1), (8, 8), (5, 3), (9, 4), (12, 4), (13, 4), (4, 9), (4, 10), (4, 11)], hs=104, ws=118,
                           truth=(1.2, -0.8), seed=39, inside=[True, True, True, False, False, False, False, False, False]),
    "s2-tall-narrow": _srow(16, 20, 6, 8, 6, [(1, 1), (8, 8), (3, 5), (4, 9), (4, 12), (4, 13), (9, 4), (10, 4), (11, 4)], hs=118, ws=104,
                            truth=(-0.8, 1.2), seed=40, dtype="u16", inside=[True, True, True, False, False, False, False, False, False]),
    # the eight inequalities on a plane with he, we, hs / f, ws / f all different (24, 30, 27, 22), each touched and crossed by an
    # origin of its own.  Rows: f i0 - R >= 0 at 1 | 0, i0 >= 0 at 0 | -1, i0 + w <= he at 16 | 17, the S2 bound at 18 | 19.
    # Columns: 1 | 0, 0 | -1, the S2 bound at 13 | 14, j0 + w <= we at 22 | 23.  Then the two inside corners.
    "edges-rect": _srow(24, 30, 6, 8, 6, [(1, 5), (0, 5), (-1, 5), (16, 5), (17, 5), (18, 5), (19, 5), (5, 1), (5, 0), (5, -1), (5, 13),
                                          (5, 14), (5, 22), (5, 23), (1, 1), (16, 13)], hs=162, ws=132, truth=(1.0, 1.0), seed=41,
                        inside=[True, False, False, True, False, False, False, True, False, False, True, False, False, False, True, True]),
}
EDGES_INSIDE = [True, False, True, False, True, False, True, False, True, True, False, False, False, False]
SURFACE_ROWS["edges"]["inside"] = EDGES_INSIDE
NODATA_F32, NODATA_U16 = -9999.0, 0


@functools.lru_cache(maxsize=None)
def surface_case(name):
    return surface_case_of(SURFACE_ROWS[name])


def surface_case_of(r):
    """The inputs, backing arrays and reference of the surface row `r`."""
    he, we, f, w, R = r["he"], r["we"], r["f"], r["w"], r["R"]
    hs, ws = r["hs"], r["ws"]
    emit, s2 = scene_pair(he, we, f, make_model(hs, ws, *r["truth"]), r["seed"], r["dtype"], hs, ws)
    mask, nodata = None, None
    origins = np.array(r["origins"], np.int32).reshape(-1, 2)
    if r["const"]:                                   # point 0: a constant EMIT window; point 1: a constant S2 region
        i0, j0 = origins[0]
        emit[i0:i0 + w, j0:j0 + w] = 0.25
        i1, j1 = origins[1]
        s2[f * i1 - R:f * (i1 + w) + R, f * j1 - R:f * (j1 + w) + R] = s2[0, 0]
    if r["mask"] == "part":
        nodata = NODATA_U16 if r["dtype"] == "u16" else NODATA_F32
        s2[np.equal(s2, nodata)] = 1                  # no accidental nodata
        r0, r1, c0, c1 = r["black"]
        s2[r0:r1, c0:c1] = nodata                     # the black rectangle
        if r["dtype"] == "f32":
            s2[max(r0, r1 - 5):r1, c0:c1] = np.nan
            s2[r["s2_inf"]] = np.inf
        mask = np.ones((he, we), np.uint8)
        mask[:r["corner"][0], :r["corner"][1]] = 0    # the masked corner
        mask[r["hole"]] = 0
        mask[mask != 0] = 1 + (np.arange(int(mask.sum())) % 3).astype(np.uint8)
        emit[r["emit_nan"]] = np.nan
    if r["mask"] == "all":
        mask = np.zeros((he, we), np.uint8)
    min_valid = r["min_valid"]
    if isinstance(min_valid, str):
        probe, _ = surface_ref_counts(emit, mask, s2, nodata, origins, w, f, R)
        min_valid = int(probe.min()) + (1 if min_valid == "missed" else 0)
    ref, bar = surface_ref(emit, mask, s2, nodata, origins, w, f, R, min_valid)
    ev, ers, eback = strided(emit, r["pads"][0], np.float32(np.nan))
    sv, srs, sback = strided(s2, r["pads"][1], s2.dtype.type(7))
    mback, mrs = None, 0
    if mask is not None:
        _, mrs, mback = strided(mask, r["pads"][2], np.uint8(1))
    out = dict(emit=emit, s2=s2, mask=mask, nodata=nodata, origins=origins, min_valid=min_valid, ref=ref, bar=bar,
               emit_back=eback, emit_rs=ers, s2_back=sback, s2_rs=srs, mask_back=mback, mask_rs=mrs, hs=hs, ws=ws)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def surface_instance(r):
    return "coreg_surface_kernel<%s>" % ("uint16_t" if r["dtype"] == "u16" else "float")


def surface_ref_counts(emit, mask, s2, nodata, origins, w, f, R):
    """Valid pairs of every candidate, (P, D, D) int; -1 outside."""
    he, we = emit.shape
    hs, ws = s2.shape
    D = 2 * R + 1
    cnt = np.full((len(origins), D, D), -1, np.int64)
    for p, (i0, j0) in enumerate(np.asarray(origins, np.int64)):
        if not region_inside(i0, j0, w, f, R, he, we, hs, ws):
            continue
        ev = np.isfinite(emit[i0:i0 + w, j0:j0 + w])
        if mask is not None:
            ev &= mask[i0:i0 + w, j0:j0 + w] != 0
        n_reg = f * w + 2 * R
        rv = s2_valid(s2[f * i0 - R:f * i0 - R + n_reg, f * j0 - R:f * j0 - R + n_reg], nodata)
        nb = n_reg - f + 1
        bad = np.zeros((nb, nb), np.int64)
        for a in range(f):
            for b in range(f):
                bad += ~rv[a:a + nb, b:b + nb]
        for dy in range(D):
            for dx in range(D):
                cnt[p, dy, dx] = int((ev & (bad[dy::f, dx::f][:w, :w] == 0)).sum())
    return cnt, None


# =============================================================================================================================
# stage 2: peaks
# =============================================================================================================================
def _offset(l, c, r):
    den = (l - 2.0 * c) + r
    o = 0.5 * (l - r) / den if den < 0.0 else 0.0
    return min(max(o, -0.5), 0.5)


def peaks_ref(surface, origins, w, f, R, he, we, hs, ws, min_score):
    """The (P, 8) records of the header, float64 statement for statement."""
    D = 2 * R + 1
    table = np.zeros((len(origins), REC), np.float64)
    for p, (i0, j0) in enumerate(np.asarray(origins, np.int64)):
        S = np.asarray(surface[p], np.float64)
        fin = np.isfinite(S)
        rec = table[p]
        rec[0] = float(f) * (float(i0) + 0.5 * float(w)) - 0.5
        rec[1] = float(f) * (float(j0) + 0.5 * float(w)) - 0.5
        rec[4] = rec[5] = np.nan
        rec[6] = float(fin.sum())
        if not region_inside(i0, j0, w, f, R, he, we, hs, ws):
            rec[7] = OUTSIDE
            continue
        if not fin.any():
            rec[7] = NO_SCORE
            continue
        k = int(np.argmax(np.where(fin, S, -np.inf)))                # the first of equal maxima in row-major order
        py, px = divmod(k, D)
        c = S[py, px]
        rec[4] = c
        out = fin.copy()
        out[max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = False
        if out.any():
            rec[5] = c - S[out].max()
        border = py in (0, D - 1) or px in (0, D - 1)
        if not border:
            up, dn, lf, rt = S[py - 1, px], S[py + 1, px], S[py, px - 1], S[py, px + 1]
            border = not (np.isfinite(up) and np.isfinite(dn) and np.isfinite(lf) and np.isfinite(rt))
        if border:
            rec[7] = BORDER
        elif c < min_score:
            rec[7] = LOW_SCORE
        else:
            rec[2] = float(py - R) + _offset(up, c, dn)
            rec[3] = float(px - R) + _offset(lf, c, rt)
    return table


def _bump(R, py, px, top=0.9, fall=0.05):
    """A cone with its apex at (py, px)."""
    D = 2 * R + 1
    yy, xx = np.meshgrid(np.arange(D), np.arange(D), indexing="ij")
    return top - fall * np.hypot(yy - py, xx - px)


def _peak_surfaces():
    R = 3
    s = {}
    s["plain"] = (_bump(R, 4, 2), OK)
    a = _bump(R, 2, 2)
    a[4, 5] = a[2, 2]                                                 # an exact tie: the first in row-major order wins
    s["tie"] = (a, OK)
    a = _bump(R, 3, 3)
    a[3, 4] = a[3, 3]                                                 # a tie with the right neighbour: den < 0, offset +0.5 exactly
    s["tie-neighbour"] = (a, OK)
    for tag, (py, px) in dict(top=(0, 3), bottom=(6, 3), left=(3, 0), right=(3, 6), corner=(6, 6)).items():
        s["border-" + tag] = (_bump(R, py, px), BORDER)
    a = _bump(R, 3, 3)
    a[2, 3] = np.nan
    s["nan-neighbour"] = (a, BORDER)
    a = _bump(R, 3, 3)
    a[2, 2] = np.nan                                                  # a diagonal neighbour does not count
    s["nan-diagonal"] = (a, OK)
    a = np.full((7, 7), 0.1)
    a[3, 3] = 0.8
    a[3, 2], a[3, 4] = 0.8, 0.5                                       # (3, 2) comes first; its row 0.1, 0.8, 0.8: offset +0.5
    s["row-tie"] = (a, OK)
    # den = (l - 2 c) + r <= 0 at the first of the maxima, whatever the rounding (l, r <= c and rounding is monotone), so den > 0
    # cannot be fed; den == 0 needs l - 2 c to round to -c and r == c: c = 1, l = 1 - 2^-53 (l - 2 = -1 - 2^-53 ties to -1)
    a = np.full((7, 7), 0.5)
    a[3, 3], a[3, 4], a[3, 2] = 1.0, 1.0, 1.0 - 2.0 ** -53
    s["den-zero"] = (a, OK)
    a = np.full((7, 7), np.nan)
    a[2:5, 2:5] = 0.2
    a[3, 3] = 0.7                                                     # nothing outside the 3 x 3: sharpness NaN
    s["sharpness-none"] = (a, OK)
    a = _bump(R, 3, 3)
    a[3, 2] = a[3, 3] - 1e-9                                          # a steep right side: the offset at the -0.5 clip
    a[3, 4] = a[3, 3] - 0.3
    s["clip-minus"] = (a, OK)
    a = _bump(R, 3, 3)
    a[4, 3] = a[3, 3] - 1e-9
    a[2, 3] = a[3, 3] - 0.3
    s["clip-plus"] = (a, OK)
    s["all-nan"] = (np.full((7, 7), np.nan), NO_SCORE)
    a = np.full((7, 7), np.nan)
    a[0, 0] = 0.3
    s["one-finite-corner"] = (a, BORDER)
    s["score-at-min"] = (_bump(R, 3, 3, top=0.6), OK)                 # score == min_score: not below it
    s["score-below-min"] = (_bump(R, 3, 3, top=np.nextafter(0.6, 0.0)), LOW_SCORE)
    s["outside"] = (_bump(R, 3, 3), OUTSIDE)
    a = _bump(R, 3, 3)
    a[5, 5] = np.inf                                                  # not finite: ignored like NaN
    s["inf-entry"] = (a, OK)
    return s


PEAK_R, PEAK_W, PEAK_F, PEAK_MIN_SCORE = 3, 8, 6, 0.6
PEAK_SHAPES = dict(he=24, we=24, hs=144, ws=144)
PEAK_SURFACES = _peak_surfaces()


# the rectangular set: rows i0 in 1 .. 14 (the S2 bound; EMIT allows 16), columns j0 in 1 .. 22 (the EMIT bound; S2 allows 23)
PEAK_SHAPES_RECT = dict(he=24, we=30, hs=138, ws=190)
PEAK_OUTSIDE_RECT = {"outside-top": (0, 5), "outside-bottom": (15, 5), "outside-left": (5, 0), "outside-right": (5, 23)}


def peak_case(rect=False):
    """All crafted surfaces as one call: (names, surface (P, 7, 7), origins, expected status).  rect: on PEAK_SHAPES_RECT, every
    origin with i0 != j0, and one OUTSIDE record per axis and side, each outside on that axis only."""
    names = list(PEAK_SURFACES)
    if rect:
        names = [n for n in names if n != "outside"] + list(PEAK_OUTSIDE_RECT)
    surf = np.stack([PEAK_SURFACES["outside" if n in PEAK_OUTSIDE_RECT else n][0] for n in names]).astype(np.float64)
    if rect:
        origins = np.array([PEAK_OUTSIDE_RECT[n] if n in PEAK_OUTSIDE_RECT else (3 + k % 5, 9 + k % 7) for k, n in enumerate(names)], np.int32)
    else:
        origins = np.array([(0, 0) if n == "outside" else (3 + k % 5, 2 + k % 7) for k, n in enumerate(names)], np.int32)
    want = np.array([OUTSIDE if n in PEAK_OUTSIDE_RECT else PEAK_SURFACES[n][1] for n in names])
    return names, surf, origins, want


# =============================================================================================================================
# stage 3: the model
# =============================================================================================================================
def _design(table, hs, ws):
    xc, yc = 0.5 * (ws - 1), 0.5 * (hs - 1)
    hx, hy = max(xc, 1.0), max(yc, 1.0)
    use = table[:, 7] == OK
    u, v = (table[use, 1] - xc) / hx, (table[use, 0] - yc) / hy
    return use, np.stack([np.ones(use.sum()), u, v], axis=1), (xc, yc, hx, hy)


def _fit_ref(table, kind, min_points, hs, ws):
    """(model, scaled coefficients (2, 3), bar) of one pass."""
    use, X, (xc, yc, hx, hy) = _design(table, hs, ws)
    n = int(use.sum())
    m = np.zeros(MODEL)
    if n < max(min_points, 1):
        m[9] = -1
        return m, np.zeros((2, 3)), 0.0
    d = table[use][:, 2:4]
    m[6], m[7], m[8] = xc, yc, n
    scale = max(float(np.abs(d).max()), 1e-300)
    coef, cond, used = np.array([[d[:, 0].astype(LD).mean(), 0, 0], [d[:, 1].astype(LD).mean(), 0, 0]], np.float64), 1.0, 0
    if kind == 1 and n >= 3:
        ev = np.linalg.eigvalsh(X.T @ X)
        if ev[0] >= 1e-10 * ev[-1]:
            coef = np.linalg.lstsq(X, d, rcond=None)[0].T
            cond, used = float(ev[-1] / ev[0]), 1
    m[0], m[1], m[2] = coef[0, 0], coef[0, 1] / hx, coef[0, 2] / hy
    m[3], m[4], m[5] = coef[1, 0], coef[1, 1] / hx, coef[1, 2] / hy
    m[9] = used
    return m, coef, 64 * n * EPS * cond * scale


def model_ref(table, kind, min_points, reject_px, hs, ws):
    """(records after the rejection pass, model, scaled coefficients, bar)."""
    t = np.array(table, np.float64)
    m, coef, bar = _fit_ref(t, kind, min_points, hs, ws)
    if m[9] < 0:
        return t, m, coef, bar
    any_out = False
    for r in t:
        if r[7] != OK:
            continue
        dy, dx = shift_field(m, r[0], r[1])
        if np.hypot(r[2] - dy, r[3] - dx) > reject_px:
            r[7], r[2], r[3], any_out = OUTLIER, 0.0, 0.0, True
    if any_out:
        m, coef, bar = _fit_ref(t, kind, min_points, hs, ws)
    return t, m, coef, bar


def scaled_coefficients(model, hs, ws):
    hx, hy = max(0.5 * (ws - 1), 1.0), max(0.5 * (hs - 1), 1.0)
    m = np.asarray(model, np.float64)
    return np.array([[m[0], m[1] * hx, m[2] * hy], [m[3], m[4] * hx, m[5] * hy]])


MODEL_HS, MODEL_WS = 288, 288


def _records(points, truth, status=None):
    """Records at window centres `points` (cy, cx) with the shifts of the model `truth`."""
    t = np.zeros((len(points), REC))
    for k, (cy, cx) in enumerate(points):
        dy, dx = shift_field(truth, cy, cx)
        t[k] = [cy, cx, dy, dx, 0.9, 0.1, 49.0, OK if status is None else status[k]]
    return t


def _scaled(points, hs, ws):
    """Points laid out on the 288 x 288 scene, stretched to (hs, ws); unchanged at 288 x 288."""
    ky, kx = hs / 288.0, ws / 288.0
    return [(cy * ky, cx * kx) for cy, cx in points]


def _grid_points(n=5, lo=47.5, step=48.0, hs=MODEL_HS, ws=MODEL_WS):
    return _scaled([(lo + step * i, lo + step * j) for i in range(n) for j in range(n)], hs, ws)


def _with_outlier(delta_sign, reject_px=1.0, hs=MODEL_HS, ws=MODEL_WS):
    """The regular grid with exact affine shifts and one record pushed so that its residual after the first fit is reject_px
    times (1 + 1e-3 delta_sign): just outside (+1) or just inside (-1)."""
    truth = make_model(hs, ws, 1.25, -2.5, 0.004, -0.003, 0.002, 0.005)
    base = _records(_grid_points(hs=hs, ws=ws), truth)
    probe = base.copy()
    probe[7, 2] += 1.0
    _, m, _, _ = model_ref(probe, 1, 1, 1e9, hs, ws)
    dy, dx = shift_field(m, probe[7, 0], probe[7, 1])
    rho = float(np.hypot(probe[7, 2] - dy, probe[7, 3] - dx))           # the residual of a unit push (linear in the push)
    base[7, 2] += reject_px * (1.0 + 1e-3 * delta_sign) / rho
    return base


def _model_rows(hs=MODEL_HS, ws=MODEL_WS):
    """The rows on a (hs, ws) scene: the same truths, the tables rebuilt from them at that shape."""
    truth = make_model(hs, ws, 1.25, -2.5, 0.004, -0.003, 0.002, 0.005)
    shift = make_model(hs, ws, -0.75, 3.5)
    grid = _grid_points(hs=hs, ws=ws)
    rows = {}
    rows["affine-grid"] = dict(table=_records(grid, truth), kind=1, kind_used=1, n_used=25)
    rows["translation-grid"] = dict(table=_records(grid, shift), kind=0, kind_used=0, n_used=25)
    rows["translation-of-affine"] = dict(table=_records(grid, truth), kind=0, kind_used=0, reject_px=5.0, n_used=25)
    rows["outlier-outside"] = dict(table=_with_outlier(+1, hs=hs, ws=ws), kind=1, kind_used=1, n_used=24, outliers=[7])
    rows["outlier-inside"] = dict(table=_with_outlier(-1, hs=hs, ws=ws), kind=1, kind_used=1, n_used=25)
    far = _records(grid, truth)
    far[3, 2:4] += (1.8, -2.4)
    far[20, 2:4] -= (2.0, 2.0)
    rows["two-outliers"] = dict(table=far, kind=1, kind_used=1, n_used=23, outliers=[3, 20])
    rows["two-outliers-translation"] = dict(table=_with_far(shift, grid), kind=0, kind_used=0, n_used=23, outliers=[3, 20])
    line = _scaled([(47.5 + 30.0 * k, 20.5 + 15.0 * k) for k in range(8)], hs, ws)
    rows["collinear"] = dict(table=_records(line, shift), kind=1, kind_used=0, n_used=8)
    column = _scaled([(47.5 + 30.0 * k, 100.5) for k in range(6)], hs, ws)
    rows["collinear-column"] = dict(table=_records(column, shift), kind=1, kind_used=0, n_used=6)
    for n_ok in (0, 1, 2, 3):
        st = [OK if k < n_ok else (LOW_SCORE, BORDER, OUTSIDE, NO_SCORE)[k % 4] for k in range(9)]
        pts = _scaled([(40.5, 30.5), (200.5, 60.5), (90.5, 250.5)], hs, ws) + _grid_points(3, hs=hs, ws=ws)[3:]
        t = _records(pts, truth, st)
        t[n_ok:, 2:4] = 0.0
        rows[f"ok-{n_ok}"] = dict(table=t, kind=1, kind_used=-1 if n_ok == 0 else (1 if n_ok == 3 else 0), n_used=n_ok)
    rows["no-records"] = dict(table=np.zeros((0, REC)), kind=1, kind_used=-1, n_used=0)
    rows["min-points-unmet"] = dict(table=_records(grid, truth), kind=1, min_points=26, kind_used=-1, n_used=0)
    rows["min-points-met"] = dict(table=_records(grid, truth), kind=1, min_points=25, kind_used=1, n_used=25)
    # the rejection leaves fewer than min_points: the second pass gives the zero model
    rows["min-points-after-rejection"] = dict(table=far.copy(), kind=1, min_points=24, kind_used=-1, n_used=0, outliers=[3, 20])
    return _finish_model_rows(rows, hs, ws)


def _finish_model_rows(rows, hs, ws):
    for r in rows.values():
        r.setdefault("min_points", 1)
        r.setdefault("reject_px", 1.0)
        r.setdefault("outliers", [])
        r.setdefault("hs", hs)
        r.setdefault("ws", ws)
        r["table"].setflags(write=False)
    return rows


def _clamp_rows():
    """Scenes one, two or three pixels across: xc = (ws - 1) / 2 <= 1 or yc <= 1, so the fit scales that axis by max(.., 1) = 1.
    The records are a 5 x 5 grid about the scene centre; the fit takes records as they come, inside the scene or not."""
    rows = {}
    for hs, ws in ((200, 1), (200, 3), (2, 344), (2, 1)):
        truth = make_model(hs, ws, 1.25, -2.5, 0.004, -0.003, 0.002, 0.005)
        sy, sx = max(hs, 6) / 6.0, max(ws, 6) / 6.0
        pts = [(truth[7] + sy * (i - 2), truth[6] + sx * (j - 2)) for i in range(5) for j in range(5)]
        rows[f"clamp-{hs}x{ws}"] = dict(table=_records(pts, truth), kind=1, kind_used=1, n_used=25, hs=hs, ws=ws)
        far = _records(pts, truth)
        far[3, 2:4] += (1.8, -2.4)
        rows[f"clamp-{hs}x{ws}-outlier"] = dict(table=far, kind=1, kind_used=1, n_used=24, outliers=[3], hs=hs, ws=ws)
    return _finish_model_rows(rows, None, None)


def _with_far(shift, grid):
    t = _records(grid, shift)
    t[3, 2:4] += (1.8, -2.4)
    t[20, 2:4] -= (2.0, 2.0)
    return t


MODEL_ROWS = _model_rows()
MODEL_RECT = (200, 344)                            # xc != yc and hx != hy
MODEL_ROWS_ALL = dict(MODEL_ROWS, **{"rect-" + k: v for k, v in _model_rows(*MODEL_RECT).items()}, **_clamp_rows())


# =============================================================================================================================
# stage 4: the warp
# =============================================================================================================================
def keys(t):
    return [((-0.5 * t + 1.0) * t - 0.5) * t, ((1.5 * t - 2.5) * t) * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t,
            ((0.5 * t - 0.5) * t) * t]


def warp_ref(scene, model, nodata, fill):
    """(out in the scene's dtype, raw float64 values with NaN where the output is fill): the header's statements in float64."""
    bands, h, w = scene.shape
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    dy, dx = shift_field(model, yy, xx)
    sy, sx = yy + dy, xx + dx
    with np.errstate(invalid="ignore"):
        inside = (sy >= 0.0) & (sy <= h - 1.0) & (sx >= 0.0) & (sx <= w - 1.0)
    sy, sx = np.where(inside, sy, 0.0), np.where(inside, sx, 0.0)
    fy, fx = np.floor(sy), np.floor(sx)
    wy, wx = keys(sy - fy), keys(sx - fx)
    ty = [np.clip(fy.astype(np.int64) - 1 + k, 0, h - 1) for k in range(4)]
    tx = [np.clip(fx.astype(np.int64) - 1 + k, 0, w - 1) for k in range(4)]
    valid = s2_valid(scene, nodata)
    raw = np.empty((bands, h, w), np.float64)
    for b in range(bands):
        ok, acc = inside.copy(), None
        plane = scene[b].astype(np.float64)
        for k in range(4):
            row = None
            for c in range(4):
                live = (wy[k] != 0.0) & (wx[c] != 0.0)
                with np.errstate(invalid="ignore", over="ignore"):
                    term = np.where(live, wx[c] * plane[ty[k], tx[c]], 0.0)
                ok &= ~live | valid[b][ty[k], tx[c]]
                row = term if row is None else row + term
            with np.errstate(invalid="ignore", over="ignore"):
                row = np.where(wy[k] != 0.0, wy[k] * row, 0.0)
                acc = row if acc is None else acc + row
        raw[b] = np.where(ok, acc, np.nan)
    if scene.dtype == np.uint16:
        out = np.clip(np.rint(np.where(np.isnan(raw), 0.0, raw)), 0.0, 65535.0).astype(np.uint16)
        fill_v = np.uint16(min(max(np.rint(0.0 if np.isnan(fill) else fill), 0.0), 65535.0))
    else:
        with np.errstate(over="ignore"):
            out = raw.astype(np.float32)
        fill_v = np.float32(fill)
    out[np.isnan(raw)] = fill_v
    return out, raw


def warp_instance(dtype, slope_bound):
    esz = 2 if dtype == "u16" else 4
    spread = slope_bound * (TILE_W + TILE_H)
    direct = spread > 4096.0 or (TILE_W + int(np.ceil(spread)) + 5) * (TILE_H + int(np.ceil(spread)) + 5) * esz > LDS_LIMIT
    return "coreg_warp_kernel<%s, %s>" % ("uint16_t" if dtype == "u16" else "float", "DIRECT" if direct else "LDS")


# name: dtype, bands, h, w, model terms, bad (none | nan | nodata), bound (max_abs_shift, max_abs_slope), off (base misalignment,
# bytes), extra (row-stride padding), fill, status (what the device-side check of the bound must say)
#   out_off, out_extra: the same two of the output, default the input's.  in_gap, out_gap: elements between the bands, so that the
#   band stride is h rs + gap.  centre: (xc, yc) of the model, default the centre of the scene that is warped.  seed: what picks the
#   texture and the bad samples, default the length of the row's name
def _wrow(dtype, bands, h, w, model, bad="none", bound=(13.0, 0.05), off=0, extra=0, fill=None, status=0, kind="texture",
          out_off=None, out_extra=None, in_gap=0, out_gap=0, centre=None, seed=None):
    return dict(dtype=dtype, bands=bands, h=h, w=w, model=model, bad=bad, bound=bound, off=off, extra=extra, fill=fill, status=status,
                kind=kind, out_off=off if out_off is None else out_off, out_extra=extra if out_extra is None else out_extra,
                in_gap=in_gap, out_gap=out_gap, centre=centre, seed=seed)


_STEEP = dict(dy0=0.8, dx0=-1.1, dy_x=0.3, dy_y=-0.2, dx_x=0.25, dx_y=0.3)
_OFF_CENTRE = (299.5, 209.5)                       # the centre of a 420 x 600 scene, of which the rows warp a 50 x 131 corner
WARP_TILE_W, WARP_TILE_H = (63, 64, 65, 128), (15, 16, 17, 32)
WARP_THIN = ((1, 1), (1, 70), (40, 1), (2, 3), (3, 2))


WARP_ROWS = {
    "identity": _wrow("f32", 2, 40, 70, dict()),
    "identity-zero-model": _wrow("f32", 1, 33, 65, dict(kind=-1), bad="nan"),
    "int-plus": _wrow("f32", 2, 40, 70, dict(dy0=3.0, dx0=5.0), bad="nan"),
    "int-minus": _wrow("f32", 2, 37, 129, dict(dy0=-2.0, dx0=-7.0), bad="nodata", off=4, extra=3),
    "int-u16": _wrow("u16", 3, 40, 67, dict(dy0=-4.0, dx0=6.0), bad="nodata", off=2, extra=1),
    "frac": _wrow("f32", 2, 40, 70, dict(dy0=1.25, dx0=-0.75), bad="nan"),
    "frac-nodata": _wrow("f32", 1, 35, 67, dict(dy0=-0.5, dx0=2.125), bad="nodata", off=12, extra=2, fill=-1.0),
    "frac-u16": _wrow("u16", 2, 40, 70, dict(dy0=0.375, dx0=-1.5), bad="nodata", fill=7.0),
    "half-u16-rounding": _wrow("u16", 1, 20, 66, dict(dx0=0.5), kind="ramp"),
    "affine": _wrow("f32", 2, 50, 131, dict(dy0=0.8, dx0=-1.1, dy_x=0.01, dy_y=-0.02, dx_x=0.015, dx_y=0.012), bad="nan", extra=5),
    "affine-u16": _wrow("u16", 2, 50, 131, dict(dy0=-0.3, dx0=0.6, dy_x=-0.02, dy_y=0.01, dx_x=0.02, dx_y=-0.015), bad="nodata"),
    "past-top-left": _wrow("f32", 1, 40, 70, dict(dy0=-9.5, dx0=-12.25)),
    "past-bottom-right": _wrow("f32", 1, 40, 70, dict(dy0=10.5, dx0=11.75)),
    "past-edges-u16": _wrow("u16", 1, 40, 70, dict(dy0=6.0, dx0=-5.5), fill=65535.0),
    "wholly-outside": _wrow("f32", 1, 20, 30, dict(dy0=100.0), bound=(100.0, 0.05)),
    "direct": _wrow("f32", 2, 50, 131, dict(dy0=0.8, dx0=-1.1, dy_x=0.3, dy_y=-0.2, dx_x=0.25, dx_y=0.3), bad="nan", bound=(80.0, 2.0)),
    "direct-u16": _wrow("u16", 1, 40, 70, dict(dy0=1.5, dx0=2.5, dx_x=0.5), bad="nodata", bound=(40.0, 2.0)),
    "bound-exceeded": _wrow("f32", 1, 50, 131, dict(dy0=0.8, dx0=-1.1, dy_x=0.3, dy_y=-0.2, dx_x=0.25, dx_y=0.3), bad="nan", status=1),
    "shift-bound-exceeded": _wrow("u16", 1, 30, 40, dict(dy0=14.0), status=1),
    "nan-model": _wrow("f32", 1, 20, 30, dict(dy0=float("nan")), status=1),
    # the output with a row stride, a band stride and a base offset of its own; gaps between the bands on one side or on both
    "strides-lds": _wrow("f32", 2, 40, 70, dict(dy0=1.25, dx0=-0.75), bad="nan", off=4, extra=3, out_off=12, out_extra=7, in_gap=5,
                         out_gap=9),
    "strides-direct": _wrow("f32", 2, 37, 67, _STEEP, bad="nan", bound=(80.0, 2.0), off=8, extra=2, out_off=4, out_extra=5, out_gap=11),
    "strides-u16-lds": _wrow("u16", 3, 40, 67, dict(dy0=0.375, dx0=-1.5), bad="nodata", off=2, extra=1, out_off=6, out_extra=4, in_gap=7),
    "strides-u16-direct": _wrow("u16", 2, 37, 70, dict(dy0=1.5, dx0=2.5, dx_x=0.5), bad="nodata", bound=(40.0, 2.0), off=6, extra=5,
                                out_off=2, out_extra=2, in_gap=3, out_gap=1),
    # a model centred on a larger scene: m[6], m[7] are not ((w - 1) / 2, (h - 1) / 2)
    "off-centre": _wrow("f32", 2, 50, 131, dict(dy0=0.8, dx0=-1.1, dy_x=0.01, dy_y=-0.02, dx_x=0.015, dx_y=0.012), bad="nan",
                        centre=_OFF_CENTRE),
    "off-centre-direct": _wrow("u16", 2, 50, 131, dict(dy0=0.5, dx0=1.0, dy_x=0.05, dy_y=-0.04, dx_x=0.06, dx_y=0.03), bad="nodata",
                               bound=(80.0, 2.0), centre=_OFF_CENTRE),
    # extents at a multiple of the 64 x 16 tile, one less and one more
    "tile-15x63": _wrow("f32", 2, 15, 63, dict(dy0=0.6, dx0=-1.3), bad="nan"),
    "tile-16x64": _wrow("f32", 2, 16, 64, dict(dy0=-0.6, dx0=1.3), bad="nan"),
    "tile-17x65": _wrow("u16", 2, 17, 65, dict(dy0=0.6, dx0=-1.3), bad="nodata"),
    "tile-32x128": _wrow("f32", 2, 32, 128, dict(dy0=-1.6, dx0=0.3), bad="nodata"),
    "tile-16x65-direct": _wrow("f32", 2, 16, 65, dict(dy0=0.6, dx0=-1.3, dx_y=0.2), bound=(40.0, 2.0)),
}
# planes thinner than the four taps: every tap clamps.  A fractional shift along the axes longer than one pixel, small enough that
# some pixels stay inside, and an integer one; a 1 x 1 plane has the zero shift alone to stay inside
for _h, _w in WARP_THIN:
    _dt = "u16" if (_h, _w) in ((40, 1), (3, 2)) else "f32"
    WARP_ROWS[f"thin-{_h}x{_w}-frac"] = _wrow(_dt, 2, _h, _w, dict(dy0=0.25 if _h > 1 else 0.0, dx0=-0.375 if _w > 1 else 0.0))
    WARP_ROWS[f"thin-{_h}x{_w}-int"] = _wrow(_dt, 2, _h, _w, dict(dy0=1.0 if _h > 1 else 0.0, dx0=-1.0 if _w > 1 else 0.0))
WARP_ROWS["thin-1x1-outside"] = _wrow("f32", 1, 1, 1, dict(dx0=0.25))
WARP_ROWS["thin-2x3-direct"] = _wrow("u16", 2, 2, 3, dict(dy0=0.25, dx0=-0.375), bound=(13.0, 2.0))


warp_row = _wrow                                   # the pure constructor, under the name the sweeps use


@functools.lru_cache(maxsize=None)
def warp_case(name):
    return warp_case_of(WARP_ROWS[name], len(name))


def warp_case_of(r, seed=None):
    """The scene, model and reference of the warp row `r`; `seed` (default: the row's) picks the texture and the bad samples."""
    seed = r["seed"] if seed is None else seed
    bands, h, w = r["bands"], r["h"], r["w"]
    if r["kind"] == "ramp":
        # rows of ramps (results k + 1.5: round half to even both ways) and of 0 / 65535 steps (overshoot past both ends)
        scene = np.zeros((bands, h, w), np.float64)
        scene[:, 0::2] = np.arange(w)[None, None, :]
        scene[:, 1::2] = np.where((np.arange(w) // 3) % 2 == 0, 0.0, 65535.0)[None, None, :]
    else:
        t = texture(max(h, 64), max(w, 64), 30 + seed)
        scene = np.stack([np.roll(t, 11 * b, axis=1)[PAD:PAD + h, PAD:PAD + w] for b in range(bands)])
        scene = scene * 10000.0 if r["dtype"] == "u16" else scene * 2.0 - 0.5
    scene = np.round(scene).astype(np.uint16) if r["dtype"] == "u16" else scene.astype(np.float32)
    nodata = None
    rng = np.random.default_rng(seed)
    if r["bad"] == "nan":
        scene[rng.random(scene.shape) < 0.01] = np.nan
        scene[0, min(5, h - 1), min(7, w - 1)] = np.inf
    if r["bad"] == "nodata":
        nodata = 0 if r["dtype"] == "u16" else -9999.0
        scene[np.equal(scene, nodata)] = 1
        scene[rng.random(scene.shape) < 0.01] = nodata
        scene[:, 10:14, 20:26] = nodata
    terms = dict(r["model"])
    kind = terms.pop("kind", 1)
    model = make_model(h, w, kind=kind, **terms)
    if r["centre"] is not None:
        model[6], model[7] = r["centre"]
    if kind == -1:
        model[:] = 0.0
        model[9] = -1.0
    fill = r["fill"] if r["fill"] is not None else (float("nan") if r["dtype"] == "f32" else float(nodata or 0))
    ref, raw = warp_ref(scene, model, nodata, fill)
    out = dict(scene=scene, model=model, nodata=nodata, fill=fill, ref=ref, raw=raw)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def pack_scene(scene, extra, sentinel, gap=0):
    """(bands, h (w + extra) + gap) backing array holding `scene` in rows of w + extra elements, the row padding and the gap after
    every band filled with `sentinel`; band b of the scene is unpack_scene(back, h, w, extra)[b]."""
    bands, h, w = scene.shape
    back = np.full((bands, h * (w + extra) + gap), sentinel, dtype=scene.dtype)
    back[:, :h * (w + extra)].reshape(bands, h, w + extra)[:, :, :w] = scene
    return back


def unpack_scene(back, h, w, extra):
    """(the (bands, h, w) payload of a pack_scene array, a mask of its elements outside the payload)."""
    rows = back[:, :h * (w + extra)].reshape(back.shape[0], h, w + extra)
    outside = np.ones(back.shape, bool)
    outside[:, :h * (w + extra)].reshape(back.shape[0], h, w + extra)[:, :, :w] = False
    return rows[:, :, :w], outside


# =============================================================================================================================
# end to end
# =============================================================================================================================
E2E = dict(he=48, we=48, f=6, w=8, step=8, R=6, min_valid_frac=0.75, min_score=0.6, reject_px=1.0)
E2E_MODELS = {
    "translation": dict(dy0=2.3, dx0=-3.6),
    "affine": dict(dy0=1.4, dx0=-2.2, dy_x=0.006, dy_y=-0.004, dx_x=0.005, dx_y=0.007),
}
DECOY = 12                                         # the tie point whose EMIT window is replaced by one (-4, +3) S2 pixels off


# a rectangular pair: he != we, and an S2 scene five rows longer than f he
E2E_RECT = dict(E2E, he=48, we=60, hs=48 * 6 + 5, ws=60 * 6, seed=22)


def e2e_origins(p=E2E):
    he, we, f, w, R, step = p["he"], p["we"], p["f"], p["w"], p["R"], p["step"]
    hs, ws = p.get("hs", he * f), p.get("ws", we * f)
    inset = -(-R // f)
    ai = np.arange(inset, min(he - w, (hs - R - f * w) // f) + 1, step)
    aj = np.arange(inset, min(we - w, (ws - R - f * w) // f) + 1, step)
    return np.stack(np.meshgrid(ai, aj, indexing="ij"), axis=-1).reshape(-1, 2).astype(np.int32)


@functools.lru_cache(maxsize=None)
def e2e_case(name, dtype="f32", rect=False):
    """The scene pair with a planted decoy, the reference chain (surface -> peaks -> model) and the truth."""
    p = dict(E2E_RECT if rect else E2E)
    he, we, f, R = p["he"], p["we"], p["f"], p["R"]
    hs, ws, seed = p.get("hs", he * f), p.get("ws", we * f), p.get("seed", 21)
    truth = make_model(hs, ws, **E2E_MODELS[name])
    emit, s2 = scene_pair(he, we, f, truth, seed, dtype, hs, ws)
    origins = e2e_origins(p)
    i0, j0 = origins[DECOY]
    off = make_model(hs, ws, truth[0] - 4.0, truth[3] + 3.0, *truth[[1, 2, 4, 5]])
    decoy, _ = scene_pair(he, we, f, off, seed, dtype, hs, ws)
    emit[i0:i0 + p["w"], j0:j0 + p["w"]] = decoy[i0:i0 + p["w"], j0:j0 + p["w"]]
    min_valid = int(np.ceil(p["min_valid_frac"] * p["w"] ** 2))
    surf, bar = surface_ref(emit, None, s2, None, origins, p["w"], f, R, min_valid)
    table0 = peaks_ref(surf, origins, p["w"], f, R, he, we, hs, ws, p["min_score"])
    table, model, coef, mbar = model_ref(table0, 1 if name == "affine" else 0, 1, p["reject_px"], hs, ws)
    out = dict(emit=emit, s2=s2, origins=origins, truth=truth, surface=surf, bar=bar, table0=table0, table=table, model=model,
               coef=coef, model_bar=mbar, min_valid=min_valid, hs=hs, ws=ws, params=p)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def masked_case(dtype="f32"):
    """The rectangular translation pair with an EMIT mask and S2 nodata: one window wholly masked, one half masked, a masked
    stripe through others, a nodata rectangle in the S2 scene (NaN and inf beside it for float32), and the reference chain under
    them.  (emit, mask uint8, s2, nodata, origins, surface, bar, table0, min_valid, params)."""
    c = e2e_case("translation", dtype, True)
    p = c["params"]
    emit, s2, origins = c["emit"].copy(), c["s2"].copy(), c["origins"]
    nodata = NODATA_U16 if dtype == "u16" else NODATA_F32
    s2[np.equal(s2, nodata)] = 1
    s2[150:200, 100:130] = nodata
    if dtype == "f32":
        s2[150:200, 130:136] = np.nan
        s2[210, 260] = np.inf
    mask = np.ones(emit.shape, np.uint8)
    i0, j0 = origins[9]
    mask[i0:i0 + p["w"], j0:j0 + p["w"]] = 0                 # a whole window
    i0, j0 = origins[3]
    mask[i0:i0 + p["w"], j0:j0 + 4] = 0                      # half a window: fewer pairs than min_valid
    mask[40:42, :] = 0                                       # a stripe through the last row of windows: still enough pairs
    mask[mask != 0] = 1 + (np.arange(int(mask.sum())) % 250).astype(np.uint8)
    surf, bar = surface_ref(emit, mask, s2, nodata, origins, p["w"], p["f"], p["R"], c["min_valid"])
    table0 = peaks_ref(surf, origins, p["w"], p["f"], p["R"], p["he"], p["we"], c["hs"], c["ws"], p["min_score"])
    out = dict(emit=emit, mask=mask, s2=s2, nodata=nodata, origins=origins, surface=surf, bar=bar, table0=table0,
               min_valid=c["min_valid"], params=p, hs=c["hs"], ws=c["ws"])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def shift_bar(surface, bar, table0, R):
    """Per OK record the propagated bound 2 bar (|l - r| + |den|) / den^2 of both shift components, and min |den|."""
    out = np.zeros((len(table0), 2))
    den_min = np.full(len(table0), np.inf)
    for p, rec in enumerate(table0):
        if rec[7] != OK:
            continue
        S, B = surface[p], bar[p]
        py, px = int(np.nanargmax(S)) // S.shape[1], int(np.nanargmax(S)) % S.shape[1]
        for a, (l, r, bl, br) in enumerate(((S[py - 1, px], S[py + 1, px], B[py - 1, px], B[py + 1, px]),
                                            (S[py, px - 1], S[py, px + 1], B[py, px - 1], B[py, px + 1]))):
            den = (l - 2.0 * S[py, px]) + r
            b = max(bl, br, B[py, px])
            out[p, a] = 2.0 * b * (abs(l - r) + abs(den)) / den ** 2 if den != 0 else np.inf
            den_min[p] = min(den_min[p], abs(den))
    return out, den_min
