"""Seeded random rows for the scene, ortho, colour and co-registration kernels; NumPy only, not a test module.

draw(sweep, seed, index) gives one row of the sweep's family, in the form the family's *_cases.py table holds, from
np.random.default_rng([seed, index, salt of the sweep]): any row can be rebuilt without drawing the others.  A row is judged by
the reference and the bar of its family's table (case(sweep, row) builds the inputs and the reference with the family's own
code); a row that fails the table's admission condition is skipped and counted (SWEEPS[sweep].admitted(row, case)).

Every generator draws only calls that the headers document as valid (SWEEPS[sweep].valid(row) is the Python mirror of those
argument rules, checked by tests/test_sweep_cases_host.py): no refused argument, no offset near 2^31, nothing meant to fault.  Each size is
drawn half the time from the neighbourhood (-1, 0, +1) of a multiple of a kernel constant that the cases module mirrors and
uniformly otherwise (_size); offsets, paddings, dtypes, masks, special values and optional arguments are drawn independently of
the sizes.  The ranges are the smallest at which the kernels' loops, tails and staging paths all still occur.

Shared by tests/test_sweep_cases_host.py (the rows on the reference alone), tests/test_gpu_family_sweeps.py (24 rows of seeds 1
and 2 per sweep on the GPU) and tools/dbg/stress_families.py (long runs)."""
import zlib

import numpy as np

import affine_cases as ac
import coreg_cases as cc
import ortho_cases as oc
import scene_cases as sc

SEEDS, ROWS_PER_SEED, MAX_SKIPPED = (1, 2), 24, 0.10


def _rng(sweep, seed, index, extra=0):
    return np.random.default_rng([seed, index, zlib.crc32(sweep.encode()), extra])


def _size(rng, lo, hi, consts):
    """An int in [lo, hi]: half the time k c - 1, k c or k c + 1 for a constant c of `consts`, uniformly otherwise."""
    if rng.random() < 0.5:
        near = sorted({k * c + d for c in consts for k in range(1, hi // c + 2) for d in (-1, 0, 1) if lo <= k * c + d <= hi})
        if near:
            return int(rng.choice(near))
    return int(rng.integers(lo, hi + 1))


def _pick(rng, values):
    return values[int(rng.integers(0, len(values)))]


def rows_equal(a, b):
    """Row equality that looks into arrays (bit patterns, so NaN equals NaN) and nested containers."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(rows_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(rows_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, (float, np.floating)):
        return type(a) is type(b) and np.asarray(a).tobytes() == np.asarray(b).tobytes()
    return type(a) is type(b) and a == b


# =============================================================================================================================
# ortho: hsr_ortho_glt
# =============================================================================================================================
ORTHO_BANDS = tuple(range(1, 10)) + (63, 64, 65, 127, 128, 129)
ORTHO_OFFS = (0, 4, 8, 12, 16, 32, 48)
ORTHO_FILLS = (-9999.0, float("nan"))                        # the table's fills and masked values, and NaN for both
ORTHO_MASKED = (-7777.5, float("inf"), float("nan"))


def draw_ortho(seed, index):
    """The layout, the mask combination and whether the float4 path is open (bands % 4 == 0, both bases on 16 bytes: one draw in
    twelve if left to chance) walk through their 16 combinations with the index, from a start the seed picks: any 16 consecutive
    rows reach all six instances.  Everything else is drawn."""
    rng = _rng("ortho", seed, index)
    stratum = (index + 5 * seed) % 16
    layout, (q, bm), vec = stratum % 2, oc.MASKS[stratum // 2 % 4], stratum // 8
    rows, cols = _size(rng, 1, 40, (oc.PX_WAVE_BSQ, oc.PX_WAVE)), _size(rng, 1, 70, (oc.PX_WAVE, oc.PX))
    bands = 285 if rng.integers(0, 8) == 0 else _pick(rng, ORTHO_BANDS)
    offs = (_pick(rng, ORTHO_OFFS), _pick(rng, ORTHO_OFFS))
    if vec:
        bands, offs = _pick(rng, (4, 8, 64, 128)), (_pick(rng, (0, 16, 32, 48)), _pick(rng, (0, 16, 32, 48)))
    gh, gw = _size(rng, 1, 24, (oc.AHEAD, oc.PX_WAVE_BSQ)), _size(rng, 1, 200, (oc.PX,))
    shape = rng.integers(0, 6)
    if shape == 0:
        h, w = gh, gw                                                     # the full grid
    elif shape == 1:
        h, w = 1, 1
    else:
        h, w = _size(rng, 1, gh, (oc.AHEAD,)), _size(rng, 1, gw, (oc.PX, oc.PX_WAVE))
    r0, c0 = int(rng.integers(0, gh - h + 1)), int(rng.integers(0, gw - w + 1))
    return oc.make_row(bands, layout, w, h, rows=rows, cols=cols, grid=("drawn", seed, index), q=bool(q),
                       bm=int(bm), extra_bytes=int(rng.integers(0, 4)), window=(r0, c0, h, w), gh=gh, gw=gw,
                       swath_off=offs[0], out_off=offs[1], fill=_pick(rng, ORTHO_FILLS),
                       masked=_pick(rng, ORTHO_MASKED), nodata=_pick(rng, (0, 7, -1)), count=bool(rng.integers(0, 2)))


def valid_ortho(r):
    """include/hsr.h above hsr_ortho_glt: what is refused, negated; and the float alignment of both bases."""
    r0, c0, h, w = r["window"]
    return (min(r["rows"], r["cols"], r["bands"], r["gh"], r["gw"], h, w) >= 1 and r0 >= 0 and c0 >= 0 and r0 + h <= r["gh"]
            and c0 + w <= r["gw"] and (r["bbytes"] == 0 or r["bbytes"] >= (r["bands"] + 7) // 8) and r["layout"] in (0, 1)
            and r["bands"] <= oc.MAX_BANDS and r["rows"] * r["cols"] < 2 ** 31 and h * w < 2 ** 31
            and r["swath_off"] % 4 == 0 and r["out_off"] % 4 == 0 and h * w * r["bands"] * 4 < 2 ** 31
            and r["rows"] * r["cols"] * max(r["bands"] * 4, r["bbytes"]) < 2 ** 31)


# =============================================================================================================================
# co-registration: hsr_coreg_surface, hsr_coreg_peaks, hsr_coreg_fit_model, hsr_coreg_warp
# =============================================================================================================================
SURFACE_W = (4, 5, 7, 8, 9, 12, 16)


def _axis_origins(w, f, R, n_emit, n_s2):
    """The origins along one axis that pass the region test."""
    return [i for i in range(0, n_emit) if i + w <= n_emit and f * i - R >= 0 and f * (i + w - 1) + R + f - 1 <= n_s2 - 1]


def draw_surface(seed, index):
    rng = _rng("coreg-surface", seed, index)
    f, R = int(rng.integers(1, 9)), int(rng.integers(1, 11))
    w = 32 if rng.integers(0, 8) == 0 else _pick(rng, SURFACE_W)
    inset = -(-R // f)
    he, we = w + 2 * inset + int(rng.integers(0, 9)), w + 2 * inset + int(rng.integers(0, 13))
    hs, ws = he * f, we * f
    if f > 1:                                                             # the S2 plane cut or extended by up to f - 1, each axis on its own
        hs += int(rng.integers(-(f - 1), f)) * int(rng.integers(0, 2))
        ws += int(rng.integers(-(f - 1), f)) * int(rng.integers(0, 2))
    if not _axis_origins(w, f, R, he, hs):
        hs = he * f
    if not _axis_origins(w, f, R, we, ws):
        ws = we * f
    ai, aj = _axis_origins(w, f, R, he, hs), _axis_origins(w, f, R, we, ws)
    origins = [(_pick(rng, ai), _pick(rng, aj)) for _ in range(int(rng.integers(1, 4)))]
    if len(origins) > 1 and rng.integers(0, 2):                           # one origin one step past a bound of the region test
        i, j = origins[-1]
        origins[-1] = _pick(rng, ((ai[0] - 1, j), (ai[-1] + 1, j), (i, aj[0] - 1), (i, aj[-1] + 1)))
    inside = [bool(cc.region_inside(i, j, w, f, R, he, we, hs, ws)) for i, j in origins]
    lim = max(R - 1.0, 0.4)
    truth = tuple(float(np.clip(int(rng.integers(-(R - 1), R)) + rng.uniform(-0.4, 0.4), -lim, lim)) for _ in range(2))
    dtype = _pick(rng, ("f32", "u16"))
    pads = tuple(int(v) for v in rng.integers(0, 14, 3))
    offs = (4 * int(rng.integers(0, 6)), (2 if dtype == "u16" else 4) * int(rng.integers(0, 8)), int(rng.integers(0, 8)))
    mask = _pick(rng, ("none", "part"))
    bh, bw = int(rng.integers(1, 16)), int(rng.integers(1, 23))
    b0, b1 = int(rng.integers(0, max(hs - bh, 0) + 1)), int(rng.integers(0, max(ws - bw, 0) + 1))
    min_valid = _pick(rng, (None, "met", "missed")) if mask == "part" else _pick(rng, (None, None, w * w, w * w + 1))
    r = cc.surface_row(he, we, f, w, R, origins, dtype=dtype, mask=mask, min_valid=min_valid, truth=truth,
                       seed=int(rng.integers(100, 200)), hs=hs, ws=ws, pads=pads, offs=offs, inside=inside,
                       black=(b0, min(b0 + bh, hs), b1, min(b1 + bw, ws)), corner=(int(rng.integers(0, 5)), int(rng.integers(0, 6))),
                       hole=(int(rng.integers(0, he)), int(rng.integers(0, we))),
                       emit_nan=(int(rng.integers(0, he)), int(rng.integers(0, we))),
                       s2_inf=(int(rng.integers(0, hs)), int(rng.integers(0, ws))))
    if isinstance(min_valid, str):
        # "met" / "missed" are the count of valid pairs of the worst candidate of the inside origins, and one more: resolved here,
        # on the row's own scene, so that the row holds the argument itself - at least 1, which is what the entry point takes
        c = cc.surface_case_of(dict(r, origins=[o for o, ok in zip(origins, inside) if ok], min_valid=1))
        cnt, _ = cc.surface_ref_counts(c["emit"], c["mask"], c["s2"], c["nodata"], c["origins"], w, f, R)
        r["min_valid"] = max(1, int(cnt.min()) + (1 if min_valid == "missed" else 0))
    return r


def valid_surface(r):
    """include/hsr_coreg.h above hsr_coreg_surface: what is refused, negated; and the alignment of the three bases."""
    esz = 2 if r["dtype"] == "u16" else 4
    return (4 <= r["w"] <= 64 and 1 <= r["f"] <= 8 and 1 <= r["R"] <= 24 and len(r["origins"]) >= 0 and min(r["he"], r["we"], r["hs"], r["ws"]) >= 1
            and min(r["pads"]) >= 0 and r["offs"][0] % 4 == 0 and r["offs"][1] % esz == 0
            and isinstance(r["min_valid"], int) and r["min_valid"] >= 1 and r["dtype"] in ("f32", "u16")
            and r["hs"] * (r["ws"] + r["pads"][1]) * esz < 2 ** 31)


def admitted_surface(r, c):
    """The surface table's own condition (tests/test_coreg_host.py): every finite entry's bar <= BAR_CAP, the peak's margin over
    every other entry >= MARGIN."""
    fin = np.isfinite(c["ref"])
    return bool((c["bar"][fin] <= cc.BAR_CAP).all()) and all(cc.peak_margin(s) >= cc.MARGIN for s in c["ref"] if np.isfinite(s).any())


# ---- peaks -------------------------------------------------------------------------------------------------------------------------
PEAK_KINDS = ("interior", "ring", "tie", "tie-neighbour", "nan-neighbour", "nan-diagonal", "all-nan", "one-finite", "inf-entry", "noise")


def draw_peaks(seed, index):
    """A peaks job: the shapes and parameters; the surfaces themselves are built by peaks_case from `key`."""
    rng = _rng("coreg-peaks", seed, index)
    f, R, w = int(rng.integers(1, 9)), int(rng.integers(1, 17)), _pick(rng, SURFACE_W)
    inset = -(-R // f)
    he, we = w + 2 * inset + int(rng.integers(1, 9)), w + 2 * inset + int(rng.integers(1, 13))
    if he == we:
        we += 1
    return dict(w=w, f=f, R=R, he=he, we=we, hs=he * f + int(rng.integers(0, f)), ws=we * f + int(rng.integers(0, f)),
                min_score=0.6, P=int(rng.integers(1, 13)), key=(seed, index))


def peaks_case(r):
    """(surface (P, D, D), origins, kinds): cones (cc._bump) with the apex anywhere, the border ring included, exact ties, NaN
    beside the apex, all-NaN and single-entry surfaces, noise; the origins inside the planes but for about one in eight."""
    rng = _rng("coreg-peaks", *r["key"], extra=1)
    R, D, P = r["R"], 2 * r["R"] + 1, r["P"]
    ai = _axis_origins(r["w"], r["f"], R, r["he"], r["hs"])
    aj = _axis_origins(r["w"], r["f"], R, r["we"], r["ws"])
    surf, origins, kinds = np.empty((P, D, D)), np.empty((P, 2), np.int32), []
    for p in range(P):
        kind = _pick(rng, PEAK_KINDS)
        py, px = (int(v) for v in rng.integers(0, D, 2))
        if kind not in ("ring", "noise", "one-finite") and D > 2:
            py, px = (int(v) for v in rng.integers(1, D - 1, 2))
        if kind == "ring":
            py, px = _pick(rng, ((0, px), (D - 1, px), (py, 0), (py, D - 1)))
        a = cc._bump(R, py, px, top=float(_pick(rng, (0.9, 0.6, np.nextafter(0.6, 0.0), rng.uniform(0.3, 0.95)))), fall=float(rng.uniform(0.01, 0.1)))
        if kind == "tie":
            qy, qx = (int(v) for v in rng.integers(0, D, 2))
            a[qy, qx] = a[py, px]
        if kind == "tie-neighbour":
            a[py, px + 1] = a[py, px]
        if kind == "nan-neighbour":
            dy, dx = _pick(rng, ((-1, 0), (1, 0), (0, -1), (0, 1)))
            a[py + dy, px + dx] = np.nan
        if kind == "nan-diagonal":
            a[py - 1, px + 1] = np.nan
        if kind == "all-nan":
            a[:] = np.nan
        if kind == "one-finite":
            v = a[py, px]
            a[:] = np.nan
            a[py, px] = v
        if kind == "inf-entry":
            a[tuple(int(v) for v in rng.integers(0, D, 2))] = _pick(rng, (np.inf, -np.inf))
        if kind == "noise":
            a = rng.uniform(-1.0, 1.0, (D, D))
            a[rng.random((D, D)) < 0.2] = np.nan
        surf[p] = a
        origins[p] = (_pick(rng, ai), _pick(rng, aj))
        if rng.integers(0, 8) == 0:
            origins[p] = _pick(rng, ((ai[0] - 1, origins[p][1]), (ai[-1] + 1, origins[p][1]), (origins[p][0], aj[0] - 1), (origins[p][0], aj[-1] + 1)))
        kinds.append(kind)
    return dict(surface=surf, origins=origins, kinds=kinds,
                ref=cc.peaks_ref(surf, origins, r["w"], r["f"], R, r["he"], r["we"], r["hs"], r["ws"], r["min_score"]))


def valid_peaks(r):
    return 4 <= r["w"] <= 64 and 1 <= r["f"] <= 8 and 1 <= r["R"] <= 24 and r["P"] >= 0 and min(r["he"], r["we"], r["hs"], r["ws"]) >= 1


# ---- model -------------------------------------------------------------------------------------------------------------------------
def draw_model(seed, index):
    """A model row in the form of cc.MODEL_ROWS: 3 .. 40 records at random places of a random plane, exact shifts of a random model
    plus noise below 0.05 pixels, random statuses, zero or one record pushed 3 .. 6 pixels off, min_points about the OK count."""
    rng = _rng("coreg-model", seed, index)
    n = _size(rng, 3, 40, (32,))
    hs, ws = int(_pick(rng, (1, 2, 3, int(rng.integers(4, 400)), int(rng.integers(4, 400))))), int(rng.integers(2, 400))
    kind = int(rng.integers(0, 2))
    truth = cc.make_model(hs, ws, rng.uniform(-4, 4), rng.uniform(-4, 4), *(rng.uniform(-0.01, 0.01, 4) if kind else np.zeros(4)))
    pts = [(rng.uniform(0, max(hs - 1, 1)), rng.uniform(0, max(ws - 1, 1))) for _ in range(n)]
    status = [cc.OK if rng.random() < 0.75 else _pick(rng, (cc.OUTSIDE, cc.NO_SCORE, cc.BORDER, cc.LOW_SCORE)) for _ in range(n)]
    t = cc._records(pts, truth, status)
    ok = np.flatnonzero(t[:, 7] == cc.OK)
    t[ok, 2:4] += rng.uniform(-0.05, 0.05, (len(ok), 2))
    t[t[:, 7] != cc.OK, 2:4] = 0.0
    if len(ok) and rng.integers(0, 2):
        t[_pick(rng, ok), 2:4] += rng.uniform(3.0, 6.0, 2) * rng.choice([-1.0, 1.0], 2)
    n_ok = len(ok)
    min_points = max(0, _pick(rng, (0, 1, 1, n_ok - 1, n_ok, n_ok + 1)))
    t.setflags(write=False)
    return dict(table=t, kind=kind, min_points=int(min_points), reject_px=1.0, hs=hs, ws=ws)


def valid_model(r):
    return r["kind"] in (0, 1) and r["min_points"] >= 0 and r["reject_px"] > 0 and min(r["hs"], r["ws"]) >= 1 and r["table"].shape[1] == cc.REC


def model_case(r):
    t, m, coef, bar = cc.model_ref(r["table"], r["kind"], r["min_points"], r["reject_px"], r["hs"], r["ws"])
    return dict(table=t, model=m, coef=coef, bar=bar)


def admitted_model(r, c):
    """The fit's decisions are compared exactly, so a row is judged only where the reference's own decisions stand clear of their
    thresholds - as the table's rows do (its nearest is the outlier 1e-3 of reject_px beside it): every residual of the first pass
    at least 1e-6 away from reject_px, and the Gram's eigenvalue ratio a factor 100 away from 1e-10."""
    t0 = np.array(r["table"], np.float64)
    m0, _, _ = cc._fit_ref(t0, r["kind"], r["min_points"], r["hs"], r["ws"])
    if m0[9] >= 0:
        use = t0[:, 7] == cc.OK
        dy, dx = cc.shift_field(m0, t0[use, 0], t0[use, 1])
        if (np.abs(np.hypot(t0[use, 2] - dy, t0[use, 3] - dx) - r["reject_px"]) < 1e-6).any():
            return False
    for t in (t0, c["table"]):
        use, X, _ = cc._design(t, r["hs"], r["ws"])
        if r["kind"] == 1 and use.sum() >= 3:
            ev = np.linalg.eigvalsh(X.T @ X)
            if 1e-12 * ev[-1] <= ev[0] <= 1e-8 * ev[-1]:
                return False
    return True


# ---- warp --------------------------------------------------------------------------------------------------------------------------
WARP_SLOPES = (0.05, 0.3, 2.0)


def draw_warp(seed, index):
    rng = _rng("coreg-warp", seed, index)
    if rng.integers(0, 6) == 0:
        h, w = _pick(rng, cc.WARP_THIN)
    else:
        h, w = _size(rng, 1, 50, (cc.TILE_H,)), _size(rng, 1, 200, (cc.TILE_W,))
    dtype = _pick(rng, ("f32", "u16"))
    esz = 2 if dtype == "u16" else 4
    form = _pick(rng, ("int", "frac", "affine", "steep", "zero-model"))
    reach = (min(h - 1, 12), min(w - 1, 12))
    terms = dict(dy0=float(rng.integers(-reach[0], reach[0] + 1)), dx0=float(rng.integers(-reach[1], reach[1] + 1)))
    if form != "int":
        terms = dict(dy0=terms["dy0"] + float(rng.integers(-7, 8)) / 8, dx0=terms["dx0"] + float(rng.integers(-7, 8)) / 8)
    if form in ("affine", "steep"):
        k = 0.02 if form == "affine" else 1.0
        terms.update({n: float(k * cc._STEEP[n] * rng.uniform(-1, 1)) for n in ("dy_x", "dy_y", "dx_x", "dx_y")})
    if form == "zero-model":
        terms = dict(kind=-1)
    centre = (float(rng.integers(0, 600)) + 0.5, float(rng.integers(0, 420)) + 0.5) if form in ("affine", "int") and rng.integers(0, 3) == 0 else None
    # the caller's bound: what the model reaches over the plane (at a corner), and one of the slope classes at or above its slopes
    m = cc.make_model(h, w, **{k: v for k, v in terms.items() if k != "kind"})
    if centre is not None:
        m[6], m[7] = centre
    ys, xs = np.array([0.0, 0.0, h - 1.0, h - 1.0]), np.array([0.0, w - 1.0, 0.0, w - 1.0])
    dy, dx = cc.shift_field(m, ys, xs)
    shift = float(max(np.abs(dy).max(), np.abs(dx).max())) if form != "zero-model" else 0.0
    slope = float(np.abs(m[[1, 2, 4, 5]]).max()) if form != "zero-model" else 0.0
    bound = (shift * 1.01 + float(_pick(rng, (0.0, 0.5, 13.0))), float(_pick(rng, [s for s in WARP_SLOPES if s >= slope] + [slope])))
    bad = _pick(rng, ("none", "nan", "nodata")) if dtype == "f32" else _pick(rng, ("none", "nodata"))
    fill = _pick(rng, (None, -1.0, 7.0, 65535.0, float("nan")))
    return cc.warp_row(dtype, int(rng.integers(1, 4)), h, w, terms, bad=bad, bound=bound, off=esz * int(rng.integers(0, 8)),
                       extra=int(rng.integers(0, 8)), fill=fill, status=0, out_off=esz * int(rng.integers(0, 8)),
                       out_extra=int(rng.integers(0, 8)), in_gap=int(rng.integers(0, 12)), out_gap=int(rng.integers(0, 12)), centre=centre,
                       seed=1000 * seed + index)


def valid_warp(r):
    esz = 2 if r["dtype"] == "u16" else 4
    return (r["dtype"] in ("f32", "u16") and min(r["bands"], r["h"], r["w"]) >= 1 and min(r["extra"], r["out_extra"], r["in_gap"], r["out_gap"]) >= 0
            and r["bound"][0] >= 0 and r["bound"][1] >= 0 and r["off"] % esz == 0 and r["out_off"] % esz == 0 and r["h"] <= 50 and r["w"] <= 200)


# =============================================================================================================================
# scene: hsr_scene_black_counts, hsr_scene_gather_tiles, hsr_scene_mosaic, hsr_scene_mosaic_blend
# =============================================================================================================================
SCENE_BANDS = (1, 2, 8, 9, 10, 17, 33)
SCENE_T = (1, 2, 3, 32, 33)
F32, U16 = sc.F32, sc.U16


def _scene_shape(rng):
    """bands, H, W: up to 150 each way; a wave covers 64 pixels of a row."""
    return _pick(rng, SCENE_BANDS), _size(rng, 1, 150, (64,)), _size(rng, 1, 150, (64,))


def draw_scan(seed, index):
    """The dtype alternates with the index; each criterion is on or off on its own: nodata given or not (a NaN is passed where it is
    not in use), the zero test switched off by zero_atol = 0, the masked value moved away from every sample."""
    rng = _rng("scene-scan", seed, index)
    dtype = (F32, U16)[(index + seed) % 2]
    bands, H, W = _scene_shape(rng)
    th, tw = _size(rng, 1, min(24, H), (4,)), _size(rng, 1, min(70, W), (64, 16))
    if dtype == F32:
        nodata = _pick(rng, (None, -9999.0, -9999.0, 0.3, -0.01, 7.0, float("inf"), float("nan")))
        atol = _pick(rng, (1e-3, 1e-3, 1e-6, 0.0))
    else:
        nodata = _pick(rng, (None, 65535.0, 65535.0, 100.5))
        atol = _pick(rng, (1e-3, 1.0, 0.5, 0.02))
    return sc.scan_row(dtype, bands, H, W, th, tw, nodata=nodata, masked_val=_pick(rng, (-0.01, -0.01, 123.25)), nodata_atol=atol,
                       zero_atol=_pick(rng, (1e-6, 1e-6, 0.0, 1.5 if dtype == U16 else 1e-6)), passed=_pick(rng, (0.0, float("nan"))),
                       key=1000 * seed + index, density=_pick(rng, (0.1, 0.3, 0.6)))


def valid_scan(r):
    """csrc/hsr_scene.hip, hsr_scene_black_counts: what is refused, negated."""
    return (r["dtype"] in (F32, U16) and min(r["bands"], r["H"], r["W"]) >= 1 and 1 <= r["th"] <= r["H"] and 1 <= r["tw"] <= r["W"]
            and r["nodata_atol"] >= 0 and r["zero_atol"] >= 0 and r["bands"] * r["H"] * r["W"] * 4 < 2 ** 31)


def draw_gather(seed, index):
    """The six instances - float32, uint16 and the encoding form, each with and without the vector store - in turn with the index;
    1 .. 12 origins inside the scene: drawn, pushed against an edge, or a repeat of the one before."""
    rng = _rng("scene-gather", seed, index)
    stratum = (index + seed) % 6
    dtype, encode = ((F32, None), (U16, None), (F32, _pick(rng, (sc.ENC_ND, sc.ENC_PLAIN, sc.ENC_SMALL))))[stratum % 3]
    bands, H, W = _scene_shape(rng)
    th = _size(rng, 1, min(24, H), (4,))
    esz = 2 if (encode or dtype == U16) else 4
    if stratum // 3 and W >= 4:                                           # the vector store: tw % 4 == 0 and the output on four samples
        tw, off = 4 * int(rng.integers(1, min(70, W) // 4 + 1)), 4 * esz * int(rng.integers(0, 4))
    else:
        tw, off = _size(rng, 1, min(70, W), (4, 64)), esz * int(rng.integers(0, 8))
    origins = []
    for _ in range(int(rng.integers(1, 13))):
        r0, c0 = int(rng.integers(0, H - th + 1)), int(rng.integers(0, W - tw + 1))
        how = rng.integers(0, 4)
        if how == 0:
            r0, c0 = _pick(rng, (0, H - th)), _pick(rng, (0, W - tw))
        if how == 1 and origins:
            r0, c0 = origins[-1]
        origins.append((r0, c0))
    return sc.gather_row(dtype, encode, th, tw, off, shape=(bands, H, W), origins=origins)


def valid_gather(row):
    dtype, encode, (bands, H, W), org, th, tw, off = row
    esz = 2 if (encode or dtype == U16) else 4
    return (dtype in (F32, U16) and (encode is None or (dtype == F32 and 1 <= encode[3] <= 65535)) and 1 <= bands <= 65535 and 1 <= th <= H
            and 1 <= tw <= W and 1 <= len(org) <= 65535 and off % esz == 0
            and all(sc.origin_inside(r, c, th, tw, H, W) for r, c in org))


def draw_mosaic(seed, index):
    """The vector and the scalar instance alternate with the index; windows up to 24 x 70 on a grid of 1 .. 3 x 1 .. 3, strips of
    0 .. 5 rows and columns beside them, a stack of 0 .. 6 cubes, both fills, every slot drawn on its own (the case)."""
    rng = _rng("scene-mosaic", seed, index)
    vec = (index + seed) % 2
    th, ny, nx = _size(rng, 1, 24, (4,)), int(rng.integers(1, 4)), int(rng.integers(1, 4))
    if vec:
        tw = 4 * int(rng.integers(1, 18))
        W = nx * tw + 4 * int(rng.integers(0, 2))
        out_off, cubes_off = 16 * int(rng.integers(0, 3)), 16 * int(rng.integers(0, 3))
    else:
        tw = _size(rng, 1, 70, (4,))
        W = nx * tw + int(rng.integers(0, 6))
        out_off, cubes_off = 4 * int(rng.integers(0, 8)), 4 * int(rng.integers(0, 8))
    fills = _pick(rng, (sc.BOTH, sc.BOTH[:1], sc.BOTH[1:], ((np.float32(-1.5), True),)))
    return (_pick(rng, SCENE_T), ny * th + int(rng.integers(0, 6)), W, th, tw, int(rng.integers(0, 7)), out_off, cubes_off, fills,
            1000 * seed + index)


def valid_mosaic(row):
    T, H, W, th, tw, P, out_off, cubes_off, fills, _ = row
    return (P >= 0 and 1 <= T <= 65535 and min(H, W, th, tw) >= 1 and H // th >= 1 and W // tw >= 1 and out_off % 4 == 0 and cubes_off % 4 == 0
            and len(fills) >= 1)


BLEND_K = {1: ((1, 1),), 2: ((2, 1), (1, 2)), 4: ((2, 2), (1, 4), (4, 1), (3, 1), (1, 3)), 8: ((5, 1), (2, 4), (4, 2), (2, 3), (3, 2), (1, 5), (1, 7)),
           16: ((3, 3), (3, 4), (4, 4), (5, 2), (2, 5), (5, 3), (3, 5), (4, 3))}          # ky x kx by the KMAX they are unrolled to


def draw_blend(seed, index):
    """The ten instances - KMAX 1, 2, 4, 8, 16, each vector and scalar - in turn with the index; the lattices of sc.LATTICES and
    others with ky, kx up to 5 (K <= 16); pitches from 1 up, tiles up to 24 x 70; one to four lattice steps of room each way."""
    rng = _rng("scene-blend", seed, index)
    stratum = (index + seed) % 10
    ky, kx = _pick(rng, BLEND_K[(1, 2, 4, 8, 16)[stratum % 5]])
    vec = stratum // 5
    sy = int(rng.integers(1, 24 // ky + 1))
    sx = 4 * int(rng.integers(1, max(70 // (4 * kx), 1) + 1)) if vec else int(rng.integers(1, min(70 // kx, 9) + 1))
    th, tw = sy * ky, sx * kx
    H = th + int(rng.integers(1, 5)) * sy + int(rng.integers(0, sy))
    W = tw + int(rng.integers(1, 5)) * sx + (0 if vec else int(rng.integers(0, sx + 1)))
    if not vec and sc.blend_vec(W, tw, sx, 0, 0):
        W += 1
    offs = (16 * int(rng.integers(0, 3)), 16 * int(rng.integers(0, 3))) if vec else (4 * int(rng.integers(0, 8)), 4 * int(rng.integers(0, 8)))
    r = sc.blend_row(th, tw, sy, sx, H, W, T=_pick(rng, SCENE_T), out_off=offs[0], cubes_off=offs[1])
    return dict(r, fill=_pick(rng, (np.float32(np.nan), np.float32(7.25))), key=1000 * seed + index)


def valid_blend(r):
    """include/hsr.h above hsr_scene_mosaic_blend: what is refused, negated."""
    if min(r["sy"], r["sx"]) < 1:
        return False
    K = (r["th"] // r["sy"]) * (r["tw"] // r["sx"])
    return (min(r["T"], r["th"], r["tw"], r["sy"], r["sx"], r["H"], r["W"]) >= 1 and r["th"] % r["sy"] == 0 and r["tw"] % r["sx"] == 0 and K <= 16
            and K * -(-r["th"] // 2) * -(-r["tw"] // 2) <= 2 ** 24 and r["T"] <= 65535 and r["out_off"] % 4 == 0 and r["cubes_off"] % 4 == 0)


# =============================================================================================================================
# colour: hsr_affine_moments, hsr_affine_moments_f64, hsr_affine_reduce_solve, hsr_affine_apply
# =============================================================================================================================
SLOTS_64, SLOTS_CAP = 64 * ac.SLOT_PIXELS, ac.MAX_SLOTS * ac.SLOT_PIXELS        # the largest npix with 64 slots; with per-slot rows = 2048
COLOR_LOHI = (None, ac.LOHI_PLAIN, ac.LOHI_FLAT, ac.LOHI_Y)
COLOR_AT = (ac.AT_PLAIN, ac.AT_ZEROS, ac.AT_WIDE)


def _npix(rng, big=True):
    """Around 1 and around 1, 2 and 3 times PASS half the time - one draw in eight around the count where slots() passes 64, one in
    twelve around the count where it reaches its cap (moments only) - and uniform up to three slots otherwise."""
    if big and rng.integers(0, 8) == 0:
        return SLOTS_64 + int(rng.integers(-1, 2))
    if big and rng.integers(0, 12) == 0:
        return _pick(rng, (SLOTS_CAP - ac.SLOT_PIXELS, SLOTS_CAP)) + int(rng.integers(-1, 2))   # 511 -> 512 slots; 512 slots of 2048 -> 2052 rows
    if rng.random() < 0.5:
        return max(1, _pick(rng, (1, ac.PASS, 2 * ac.PASS, 3 * ac.PASS)) + int(rng.integers(-1, 2)))
    return int(rng.integers(1, 3 * ac.SLOT_PIXELS + 2))


def _place(rng, want):
    """A (layout, byte offset) whose load / store mode (ac.mode) is `want`; offsets past a 16-byte boundary in whole floats."""
    if want == 1:
        return (ac.PADDED, 16 * int(rng.integers(0, 3)))
    if want == 2:
        return (ac.PACKED, 16 * int(rng.integers(0, 3)))
    layout = _pick(rng, (ac.PLANAR, ac.PADDED, ac.PACKED))
    return (layout, 4 * int(rng.integers(0, 8))) if layout == ac.PLANAR else (layout, 16 * int(rng.integers(0, 2)) + _pick(rng, (4, 8, 12)))


def _random_lohi(rng):
    lo = rng.uniform(-0.1, 0.4, 3)
    return np.stack([lo, lo + rng.uniform(0.2, 0.9, 3)], axis=1)


def draw_moments(seed, index):
    """The nine (x, y) load modes and the float64 entry point walk through twelve strata with the index (nine for the image kernel,
    three for hsr_affine_moments_f64); everything else is drawn."""
    rng = _rng("color-moments", seed, index)
    stratum = (index + 5 * seed) % 12
    npix = _npix(rng)
    lohi_x = _pick(rng, COLOR_LOHI + (_random_lohi(rng),))
    lohi_y = _pick(rng, (None, None, ac.LOHI_Y, _random_lohi(rng)))
    r = ac.moment_row(npix, x=_place(rng, stratum % 3), y=_place(rng, stratum // 3 % 3), mask=_pick(rng, ("none", "all", "clear", "part", "part")),
                      bad=_pick(rng, ("none", "x", "y", "both")), lohi_x=lohi_x, lohi_y=lohi_y)
    if stratum >= 9:
        r = dict(r, x=(ac.PACKED, 0), y=(ac.PACKED, 0), mask="none", lohi_x=None, lohi_y=None, npix=min(npix, SLOTS_64 + 1))
    return dict(r, entry="f64" if stratum >= 9 else "image", rs=(int(rng.integers(3, 6)), int(rng.integers(3, 6))), key=1000 * seed + index)


def moments_case(r):
    if r["entry"] == "image":
        return ac.moment_case_of(r, r["key"])
    x, y = ac.image_pair(r["npix"], r["key"])
    rng = _rng("color-moments", r["key"], 0, extra=1)
    xs, ys = x.astype(np.float64) + 1e-9 * rng.standard_normal(x.shape), y.astype(np.float64) + 1e-9 * rng.standard_normal(y.shape)
    bad_x, bad_y = xs.astype(np.float32), ys.astype(np.float32)
    ac.poison(bad_x, bad_y, r["bad"], r["key"])
    xs[~np.isfinite(bad_x)], ys[~np.isfinite(bad_y)] = bad_x[~np.isfinite(bad_x)], bad_y[~np.isfinite(bad_y)]
    ok = ac.usable(xs, ys, None)
    ref, mag = ac.moments_ld(xs[ok], ys[ok])
    return dict(xs=xs, ys=ys, ok=ok, ref=ref, mag=mag, n=int(ok.sum()))


def moments_instances(r):
    return [ac.moments_instance(r) if r["entry"] == "image" else "affine_moments_f64_kernel", "affine_reduce_solve_kernel"]


def _valid_place(place):
    return place[0] in (ac.PACKED, ac.PADDED, ac.PLANAR) and place[1] >= 0 and place[1] % 4 == 0


def valid_moments(r):
    """include/hsr_color.h: npix >= 0 (the sweeps draw >= 1), the three layouts (no overlapping strides), float-aligned bases,
    row strides of the float64 entry point >= 3."""
    return (1 <= r["npix"] <= SLOTS_CAP + 1 and _valid_place(r["x"]) and _valid_place(r["y"]) and min(r["rs"]) >= 3
            and r["mask"] in ("none", "all", "clear", "part") and r["entry"] in ("image", "f64")
            and all(l is None or np.shape(l) == (3, 2) for l in (r["lohi_x"], r["lohi_y"])))


def draw_apply(seed, index):
    """The nine (load, store) modes walk through nine strata with the index; everything else is drawn."""
    rng = _rng("color-apply", seed, index)
    stratum = (index + 5 * seed) % 9
    npix = 66001 + int(rng.integers(-1, 2)) if rng.integers(0, 12) == 0 else _npix(rng, big=False)
    At = _pick(rng, COLOR_AT + (rng.uniform(-2.0, 2.0, 12), rng.uniform(-2.0, 2.0, 12) * (rng.random(12) < 0.7)))
    r = ac.apply_row(npix, x=_place(rng, stratum % 3), out=_place(rng, stratum // 3), mask=_pick(rng, ("none", "all", "clear", "part", "part")),
                     clip=int(rng.integers(0, 3)), lohi=_pick(rng, COLOR_LOHI[:3] + (_random_lohi(rng),)), At=np.ascontiguousarray(At, np.float64),
                     bad=bool(rng.integers(0, 2)))
    return dict(r, key=1000 * seed + index)


def valid_apply(r):
    return (1 <= r["npix"] < 2 ** 24 and _valid_place(r["x"]) and _valid_place(r["out"]) and r["clip"] in (0, 1, 2) and np.shape(r["At"]) == (12,)
            and (r["lohi"] is None or np.shape(r["lohi"]) == (3, 2)) and r["mask"] in ("none", "all", "clear", "part"))


SOLVE_KINDS = {"full": 4, "equal-channels": 3, "gray": 2, "constant": 1, "narrow": 4}


def draw_solve(seed, index):
    """A solve row in the form of ac.SOLVE_ROWS, with the slots its hand-built partials fill: 1 .. cap, around 64 and its
    multiples half the time when drawn from the whole range, one, or fewer than 64; min_count on both sides of n."""
    rng = _rng("color-solve", seed, index)
    kind = tuple(SOLVE_KINDS)[(index + seed) % len(SOLVE_KINDS)]          # the rank classes in turn
    n = _pick(rng, (0, 1, 2, 3, int(rng.integers(4, 40)))) if rng.integers(0, 4) == 0 else int(rng.integers(300 if kind == "narrow" else 40, 5001))
    min_count = max(0, _pick(rng, (0, 0, 1, n - 1, n, n + 1, ac.MIN_COUNT)))
    return dict(ac.solve_row(kind, n, min(n, SOLVE_KINDS[kind]), min_count), nslots=_pick(rng, (1, int(rng.integers(2, 64)), _size(rng, 1, ac.MAX_SLOTS, (64,)))), key=1000 * seed + index)


def solve_case(r):
    """The table's case, and partials (nslots, 22): the rows cut into nslots contiguous runs of random lengths (empty ones among
    them), each run's moments summed in long double and rounded once; mom_ref, mom_mag: their long-double sum and sum of |.|."""
    c = ac.solve_case_of(r, 300 + r["key"])
    rng = _rng("color-solve", r["key"], 0, extra=1)
    cuts = np.sort(rng.integers(0, r["n"] + 1, r["nslots"] - 1))
    edges = np.concatenate([[0], cuts, [r["n"]]]).astype(int)
    partials = np.stack([ac.moments_ld(c["xs"][a:b], c["ys"][a:b])[0].astype(np.float64) for a, b in zip(edges[:-1], edges[1:])])
    return dict(c, partials=partials, mom_ref=partials.astype(ac.LD).sum(axis=0), mom_mag=np.abs(partials).astype(ac.LD).sum(axis=0))


def valid_solve(r):
    return 1 <= r["nslots"] <= ac.MAX_SLOTS and r["min_count"] >= 0 and r["n"] >= 0


def admitted_solve(r, c):
    """The solve table's rank-class condition (tests/test_affine_host.py): every eigenvalue of the Gram is either at least 1e-9 of
    the largest or at most EPS of it, and those at least 1e-9 are the row's rank and the ones the cut keeps."""
    if c["identity"] or r["n"] == 0:
        return True
    ev = ac.spectrum(c["xs"])
    rel = ev / ev.max()
    return bool(((rel >= 1e-9) | (rel <= ac.EPS)).all()) and int((rel >= 1e-9).sum()) == r["rank"] == len(ac.kept(ev, r["n"]))


# =============================================================================================================================
# the sweeps
# =============================================================================================================================
class Sweep:
    """draw(seed, index) -> row; case(row) -> inputs and reference; valid(row): the mirror of the documented argument rules;
    instances(row) -> the kernel names the call(s) record; admitted(row, case): the table's admission condition; sizes(row) ->
    {name: value} of the size parameters; table: the rows of the family's table, for sizes()."""

    def __init__(self, family, draw, case, valid, instances, admitted=None, sizes=None, table=()):
        self.family, self.draw, self.case, self.valid, self.instances = family, draw, case, valid, instances
        self.admitted = admitted or (lambda r, c: True)
        self.sizes, self.table = sizes, table


def _surface_sizes(r):
    return dict(he=r["he"], we=r["we"], hs=r["hs"], ws=r["ws"])


# the scan has no table of rows: these are the shapes and windows its tests run (tests/test_gpu_scene_instances.py)
SCAN_TABLE = ([sc.scan_row(d, b, *sc.DECIDING_HW, th, tw) for d in (F32, U16) for b in sc.DECIDING_BANDS for th, tw in sc.scan_tilings(*sc.DECIDING_HW)]
              + [sc.scan_row(F32, 3, *sc.f32_edge_scene()[0].shape[1:], th, tw) for th, tw in ((1, 1), (5, 3), sc.f32_edge_scene()[0].shape[1:])]
              + [sc.scan_row(U16, 3, 2, 70, 1, 1), sc.scan_row(U16, 3, 2, 70, 2, 70), sc.scan_row(F32, 2, 11, 140, *sc.STRIP_TILE)]
              + [sc.scan_row(F32, 1, *sc.LARGE_HW, th, tw) for th, tw in sc.LARGE_TILINGS])
SWEEPS = {
    "ortho": Sweep("ortho", draw_ortho, oc.case_of, valid_ortho, lambda r: [oc.instance_of(r)],
                   sizes=lambda r: dict(rows=r["rows"], cols=r["cols"], bands=r["bands"], gh=r["gh"], gw=r["gw"], out_h=r["window"][2],
                                        out_w=r["window"][3]), table=list(oc.ROWS.values())),
    "scene-scan": Sweep("scene", draw_scan, sc.scan_case_of, valid_scan, lambda r: [sc.scan_instance(r["dtype"])],
                        sizes=lambda r: dict(H=r["H"], W=r["W"], th=r["th"], tw=r["tw"]), table=SCAN_TABLE),   # the band counts are a fixed set
    "scene-gather": Sweep("scene", draw_gather, sc.gather_case_of, valid_gather, lambda r: [sc.gather_instance_of(r)],
                          sizes=lambda r: dict(bands=r[2][0], H=r[2][1], W=r[2][2], th=r[4], tw=r[5]), table=list(sc.GATHER_ROWS.values())),
    "scene-mosaic": Sweep("scene", draw_mosaic, lambda r: sc.mosaic_case_of(r[:9], r[9], drawn_slots=True), valid_mosaic,
                          lambda r: [sc.mosaic_instance_of(r[:9])], sizes=lambda r: dict(H=r[1], W=r[2], th=r[3], tw=r[4]),
                          table=list(sc.MOSAIC_ROWS.values())),
    "scene-blend": Sweep("scene", draw_blend, lambda r: sc.blend_case_of(r, r["key"]), valid_blend, lambda r: [sc.blend_instance_of(r)],
                         sizes=lambda r: dict(H=r["H"], W=r["W"], th=r["th"], tw=r["tw"], sy=r["sy"], sx=r["sx"]),
                         table=list(sc.BLEND_ROWS.values())),
    "color-moments": Sweep("color", draw_moments, moments_case, valid_moments, moments_instances,
                           sizes=lambda r: dict(npix=r["npix"]), table=list(ac.MOMENT_ROWS.values())),
    "color-solve": Sweep("color", draw_solve, solve_case, valid_solve, lambda r: ["affine_reduce_solve_kernel"], admitted_solve,
                         sizes=lambda r: dict(n=r["n"], nslots=r.get("nslots", ac.slots(r["n"]))), table=list(ac.SOLVE_ROWS.values())),
    "color-apply": Sweep("color", draw_apply, lambda r: ac.apply_case_of(r, r["key"]), valid_apply,
                         lambda r: [ac.apply_instance(r)], sizes=lambda r: dict(npix=r["npix"]), table=list(ac.APPLY_ROWS.values())),
    "coreg-surface": Sweep("coreg", draw_surface, cc.surface_case_of, valid_surface, lambda r: [cc.surface_instance(r)], admitted_surface,
                           sizes=_surface_sizes, table=list(cc.SURFACE_ROWS.values())),
    "coreg-peaks": Sweep("coreg", draw_peaks, peaks_case, valid_peaks, lambda r: ["coreg_peaks_kernel"],
                         sizes=lambda r: dict(he=r["he"], we=r["we"], hs=r["hs"], ws=r["ws"], R=r["R"]),
                         table=[dict(cc.PEAK_SHAPES, R=cc.PEAK_R), dict(cc.PEAK_SHAPES_RECT, R=cc.PEAK_R)]
                         + [dict(_surface_sizes(r), R=r["R"]) for r in cc.SURFACE_ROWS.values()]),
    "coreg-model": Sweep("coreg", draw_model, model_case, valid_model, lambda r: ["coreg_fit_model_kernel"], admitted_model,
                         sizes=lambda r: dict(n=len(r["table"]), hs=r["hs"], ws=r["ws"]), table=list(cc.MODEL_ROWS_ALL.values())),
    "coreg-warp": Sweep("coreg", draw_warp, cc.warp_case_of, valid_warp,
                        lambda r: [cc.warp_instance(r["dtype"], r["bound"][1])], sizes=lambda r: dict(h=r["h"], w=r["w"]),
                        table=list(cc.WARP_ROWS.values())),
}


def draw(sweep, seed, index):
    """Row `index` of `sweep` under `seed`."""
    return SWEEPS[sweep].draw(seed, index)


def case(sweep, row):
    """The inputs and the reference of a drawn row, by the family's own case builder."""
    return SWEEPS[sweep].case(row)
