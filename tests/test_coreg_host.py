"""The co-registration family on the host side: include/hsr_coreg.h against nat.COREG_SIGNATURES and the library's exports; the
refusals of every entry and the launch record's contract, which need no device; hsr_coreg_fit_model_host against every model
case; tie_point_grid and the Python argument checks; what the case tables of tests/coreg_cases.py claim about their rows; and
the reference against the truth - on the generator's scenes the reference chain alone recovers the planted shift field and flags
the planted decoy window."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import coreg_cases as cc
import s2_emit
from conftest import ROOT
from s2_emit import _engine as eng
from s2_emit import _native as nat
from s2_emit import coreg

LAUNCH_PATH = ("hsr_coreg_surface", "hsr_coreg_peaks", "hsr_coreg_fit_model", "hsr_coreg_warp")
HOST_ONLY = ("hsr_coreg_fit_model_host", "hsr_coreg_last_launch", "hsr_coreg_instance_count", "hsr_coreg_instance_name")
INVALID = 1
TRUTH_CAP = 0.25                 # S2 pixels: the reference's error at an OK tie point (a cap, not a measurement)


def _header():
    text = open(os.path.join(ROOT, "include", "hsr_coreg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    return text, code, comments


def _doc_of(text, name):
    at = re.search(r"\n(?:int|size_t|const char\*) %s\(" % name, text).start()
    return text[text.rfind("/*", 0, at):at]


# ---- the header, the signature table, the exports ----------------------------------------------------------------------------------
def test_header_signatures_and_exports_agree():
    lib = nat.load()
    text, code, comments = _header()
    declared = sorted(set(re.findall(r"\b(hsr_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(nat.COREG_SIGNATURES) == sorted(LAUNCH_PATH + HOST_ONLY)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/hsr_coreg.h but not exported"
        assert getattr(lib, name).argtypes == nat.COREG_SIGNATURES[name][1] and getattr(lib, name).restype == nat.COREG_SIGNATURES[name][0]
        assert name in comments, f"{name} is not documented"
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        nargs = 0 if proto.strip() == "void" else proto.count(",") + 1
        assert nargs == len(nat.COREG_SIGNATURES[name][1]), (name, proto)
        if name in LAUNCH_PATH:
            assert proto.split(",")[-1].strip() == "hsr_stream_t stream", name                 # the stream is the last argument
            assert "arosics_coreg.py" in _doc_of(text, name), f"{name} cites no reference"
        else:
            assert "stream" not in proto
    assert '#include "hsr.h"' in code and "HSR_ABI_VERSION" not in code
    # a family of its own: hsr.h, hsr_color.h, SIGNATURES, the ABI version and the six other tables are what they were
    hsr_h = open(os.path.join(ROOT, "include", "hsr.h")).read() + open(os.path.join(ROOT, "include", "hsr_color.h")).read()
    for name in declared:
        assert name not in nat.SIGNATURES and name not in nat.COLOR_SIGNATURES and name not in hsr_h, name
    assert lib.hsr_abi_version() == 5 == nat.HSR_ABI_VERSION
    assert (lib.hsr_aux_instance_count(), lib.hsr_scene_instance_count(), lib.hsr_k4_instance_count(), lib.hsr_pairs_instance_count(),
            lib.hsr_ortho_instance_count(), lib.hsr_color_instance_count()) == (32, 20, 31, 12, 6, 20)
    assert nat.COREG_SIGNATURES["hsr_coreg_last_launch"] == nat.SIGNATURES["hsr_k4_last_launch"]
    assert nat.COREG_SIGNATURES["hsr_coreg_instance_name"] == nat.SIGNATURES["hsr_k4_instance_name"]
    for macro, value in (("HSR_COREG_RECORD", cc.REC), ("HSR_COREG_MODEL", cc.MODEL)):
        assert re.search(r"#define %s %d\b" % (macro, value), code) and getattr(nat, macro) == value
    for k, macro in enumerate(("OK", "OUTSIDE", "NO_SCORE", "BORDER", "LOW_SCORE", "OUTLIER")):
        assert re.search(r"#define HSR_COREG_%s %d\b" % (macro, k), code) and getattr(cc, macro) == k and coreg.STATUS[k] == macro


# ---- refusals and the record, without a device ---------------------------------------------------------------------------------------
def test_c_abi_refusals_need_no_device():
    lib = nat.load()
    p, q, null, st = C.c_void_p(1 << 20), C.c_void_p(1 << 30), C.c_void_p(0), C.c_void_p(0)
    lib.hsr_coreg_last_launch(None, 0)

    def refused(word, fn, *args):
        rc = fn(*args)
        text = lib.hsr_last_error().decode()
        assert rc == INVALID and word in text and fn.__name__ in text, (fn.__name__, args, rc, text)

    def surface(emit=p, ers=16, he=16, we=16, mask=null, mrs=0, s2=p, dt=0, srs=96, hs=96, ws=96, orig=p, n=1, w=8, f=6, R=3, mv=1,
                surf=p):
        return lib.hsr_coreg_surface, emit, ers, he, we, mask, mrs, s2, dt, srs, hs, ws, 0, 0.0, orig, n, w, f, R, mv, surf, st

    for kw in (dict(emit=null), dict(s2=null), dict(orig=null), dict(surf=null)):
        refused("NULL", *surface(**kw))
    for dt in (-1, 2):
        refused("s2_dtype", *surface(dt=dt))
    for kw in (dict(w=3), dict(w=65), dict(w=0)):
        refused("window", *surface(**kw))
    for kw in (dict(f=0), dict(f=9), dict(f=-6)):
        refused("factor", *surface(**kw))
    for kw in (dict(R=0), dict(R=25), dict(R=-1)):
        refused("max_shift", *surface(**kw))
    refused("min_valid", *surface(mv=0))
    refused("npoints", *surface(n=-1))
    for kw in (dict(ers=15), dict(srs=95), dict(he=0), dict(ws=0), dict(mask=p, mrs=15)):
        refused("stride", *surface(**kw))
    assert surface(n=0)[0](*surface(n=0)[1:]) == 0                                            # no point: succeeds, launches nothing

    def peaks(surf=p, orig=p, n=1, w=8, f=6, R=3, he=16, we=16, hs=96, ws=96, table=p):
        return lib.hsr_coreg_peaks, surf, orig, n, w, f, R, he, we, hs, ws, 0.6, table, st

    for kw in (dict(surf=null), dict(orig=null), dict(table=null)):
        refused("NULL", *peaks(**kw))
    for word, kw in (("window", dict(w=3)), ("window", dict(w=65)), ("factor", dict(f=0)), ("factor", dict(f=9)),
                     ("max_shift", dict(R=0)), ("max_shift", dict(R=25)), ("npoints", dict(n=-1)), ("extent", dict(hs=0))):
        refused(word, *peaks(**kw))
    assert peaks(n=0)[0](*peaks(n=0)[1:]) == 0

    def fit(fn, table=p, n=4, kind=1, mp=1, rej=1.0, hs=96, ws=96, model=p):
        return (fn, table, n, kind, mp, rej, hs, ws, model) + ((st,) if fn is lib.hsr_coreg_fit_model else ())

    for fn in (lib.hsr_coreg_fit_model, lib.hsr_coreg_fit_model_host):
        d = (C.c_double * 8)()
        ok = dict(table=d, model=(C.c_double * 10)()) if fn is lib.hsr_coreg_fit_model_host else {}
        refused("NULL", *fit(fn, **dict(ok, table=None if ok else null)))
        refused("NULL", *fit(fn, **dict(ok, model=None if ok else null)))
        for word, kw in (("npoints", dict(n=-1)), ("kind", dict(kind=2)), ("kind", dict(kind=-1)), ("min_points", dict(mp=-1)),
                         ("reject_px", dict(rej=0.0)), ("reject_px", dict(rej=float("nan"))), ("extent", dict(hs=0)), ("extent", dict(ws=0))):
            refused(word, *fit(fn, **dict(ok, **kw)))

    def warp(s2=p, dt=0, b=2, h=10, w=12, ibs=120, irs=12, model=p, shift=1.0, slope=0.0, out=q, obs=120, ors=12, status=p):
        return lib.hsr_coreg_warp, s2, dt, b, h, w, ibs, irs, model, 0, 0.0, 0.0, shift, slope, out, obs, ors, status, st

    for kw in (dict(s2=null), dict(model=null), dict(out=null), dict(status=null)):
        refused("NULL", *warp(**kw))
    refused("s2_dtype", *warp(dt=2))
    for kw in (dict(b=0), dict(h=0), dict(w=-1)):
        refused("extent", *warp(**kw))
    for kw in (dict(irs=11), dict(ors=11), dict(ibs=119), dict(obs=119)):
        refused("strides", *warp(**kw))
    for kw in (dict(shift=-1.0), dict(slope=-0.1), dict(shift=float("nan")), dict(slope=float("nan"))):
        refused("bound", *warp(**kw))
    base = 1 << 20
    for out in (base, base + 4, base + 4 * 239, base - 4 * 239):                            # in place, and overlapping at both ends
        refused("aliases", *warp(out=C.c_void_p(out)))
    refused("aliases", *warp(dt=1, out=C.c_void_p(base + 2 * 239)))
    buf = C.create_string_buffer(64)
    assert lib.hsr_coreg_last_launch(buf, 64) == 0 and buf.value == b""                     # refused calls leave no record


def test_instance_table_and_record_contract():
    lib = nat.load()
    n = lib.hsr_coreg_instance_count()
    table = [lib.hsr_coreg_instance_name(i).decode() for i in range(n)]
    assert n == 8 == len(set(table)) and table == cc.all_instances()
    for bad in (-1, n):
        assert lib.hsr_coreg_instance_name(bad) is None
        assert b"hsr_coreg_instance_name" in lib.hsr_last_error() and str(bad).encode() in lib.hsr_last_error()
    _, _, comments = _header()
    assert "hsr_coreg_instance_count = 8" in comments and "8 most recent" in comments and "hsr_aux_last_launch" in comments
    buf = C.create_string_buffer(64)
    buf.value = b"junk"
    lib.hsr_coreg_last_launch(None, 0)
    assert lib.hsr_coreg_last_launch(buf, 0) == 0 and buf.value == b"junk"
    assert lib.hsr_coreg_last_launch(buf, 64) == 0 and buf.value == b""
    assert lib.hsr_coreg_last_launch(None, 64) == 0


def test_public_surface():
    new = ["coregister_scene", "match_windows", "fit_shift_model", "warp_scene", "tie_point_grid", "closest_band", "TiePoints",
           "ShiftModel", "CoregOutput"]
    at = s2_emit.__all__.index(new[0])                         # after the reference's 13 names; where, other tests leave open
    assert at >= 13 and s2_emit.__all__[at:at + len(new)] == new and all(hasattr(s2_emit, n) for n in new)
    sig = inspect.signature(s2_emit.tie_point_grid)
    assert [(k, v.default) for k, v in sig.parameters.items()][4:] == [("window", 32), ("step", None), ("factor", 6), ("max_shift", 12),
                                                                        ("max_points", 500)]
    sig = inspect.signature(s2_emit.match_windows).parameters
    assert [sig[k].default for k in ("grid", "emit_mask", "s2_nodata", "min_valid_frac", "min_score")] == [None, None, None, 0.75, 0.6]
    sig = inspect.signature(s2_emit.fit_shift_model).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("model", "affine"), ("reject_px", 1.0), ("min_points", 1)]
    sig = inspect.signature(s2_emit.warp_scene).parameters
    assert [(k, v.default) for k, v in sig.items()][2:] == [("nodata", None), ("fill", None), ("out", None)]
    sig = inspect.signature(s2_emit.coregister_scene).parameters
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("emit_band", "s2_band"))
    assert s2_emit.TiePoints._fields[:3] == ("table", "surface", "origins") and s2_emit.CoregOutput._fields == ("s2", "model", "tie_points")
    assert "arosics_coreg.py" in coreg.__doc__ and "NOT reproduced" in coreg.__doc__
    assert "842" in s2_emit.coregister_scene.__doc__ and "665" in s2_emit.coregister_scene.__doc__


# ---- tie_point_grid, closest_band, the Python argument checks ----------------------------------------------------------------------------
def test_tie_point_grid():
    g = s2_emit.tie_point_grid(1242, 1280, 7452, 7680)                                      # the flagship scene
    assert g.dtype == np.int32 and g.shape == (500, 2) and len(np.unique(g, axis=0)) == 500
    full = s2_emit.tie_point_grid(1242, 1280, 7452, 7680, max_points=10 ** 6)
    assert full.shape == (38 * 39, 2) and full.min() == 2 and (np.diff(np.unique(full[:, 0])) == 32).all()
    assert {tuple(r) for r in g} <= {tuple(r) for r in full}
    assert (np.diff(np.flatnonzero((full[:, None] == g[None]).all(-1).any(1))) >= 2).all()   # thinned evenly: no two neighbours kept
    for he, we, f, w, R, step in ((24, 24, 6, 8, 6, 1), (40, 30, 2, 9, 7, 4), (120, 130, 1, 64, 24, 3), (16, 16, 6, 4, 1, 5)):
        g = s2_emit.tie_point_grid(he, we, he * f, we * f, window=w, step=step, factor=f, max_shift=R, max_points=10 ** 6)
        assert len(g) and all(cc.region_inside(i, j, w, f, R, he, we, he * f, we * f) for i, j in g)
        lo, hi = g.min(axis=0), g.max(axis=0)
        assert (lo == -(-R // f)).all()                                                     # set in by ceil(R / f)
        for (i, j) in ((lo[0] - 1, lo[1]), (lo[0], lo[1] - 1)):
            assert not cc.region_inside(i, j, w, f, R, he, we, he * f, we * f)
        if step == 1:
            assert not cc.region_inside(hi[0] + 1, lo[1], w, f, R, he, we, he * f, we * f)
            assert not cc.region_inside(lo[0], hi[1] + 1, w, f, R, he, we, he * f, we * f)
    # an S2 scene shorter than factor x EMIT limits the grid; scenes too small for one window give none
    g = s2_emit.tie_point_grid(48, 48, 200, 288, window=8, step=8, factor=6, max_shift=6)
    assert g[:, 0].max() == 17 and cc.region_inside(17, 1, 8, 6, 6, 48, 48, 200, 288) and not cc.region_inside(25, 1, 8, 6, 6, 48, 48, 200, 288)
    for shape in ((8, 8, 48, 48), (33, 4, 198, 24), (1, 1, 6, 6), (0, 0, 0, 0)):
        g = s2_emit.tie_point_grid(*shape, window=8, factor=6, max_shift=6)
        assert g.shape == (0, 2) and g.dtype == np.int32
    assert s2_emit.tie_point_grid(64, 64, 384, 384, max_points=1).shape == (1, 2)
    for kw in (dict(window=3), dict(window=65), dict(factor=0), dict(factor=9), dict(max_shift=0), dict(max_shift=25), dict(step=0),
               dict(max_points=0), dict(window=8.0)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            s2_emit.tie_point_grid(64, 64, 384, 384, **kw)


def test_closest_band_and_argument_checks():
    w = [380.0, 650.0, 668.0, 670.0, 842.0, 2500.0]
    assert [s2_emit.closest_band(w, t) for t in (842, 665, 669, 100, 9999)] == [4, 2, 2, 0, 5]
    assert s2_emit.closest_band([600.0, 700.0], 650.0) == 0                                  # the first of equally close bands
    with pytest.raises(ValueError, match="empty"):
        s2_emit.closest_band([], 842)
    tp = s2_emit.TiePoints(np.zeros((0, 8)), None, None, (96, 96), 3)
    for kw, word in ((dict(model="cubic"), "model"), (dict(reject_px=0), "reject_px"), (dict(min_points=-1), "min_points")):
        with pytest.raises(ValueError, match=word):
            s2_emit.fit_shift_model(tp, **kw)
    sm = s2_emit.fit_shift_model(tp)                                                         # array records: the host twin, no device
    assert sm.params[9] == -1 and not sm.params[:9].any() and sm.max_abs_shift == 4.0


# ---- the fit's host twin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.MODEL_ROWS_ALL))
def test_fit_model_host(name):
    r = cc.MODEL_ROWS_ALL[name]
    hs, ws = r["hs"], r["ws"]
    want_t, want_m, coef, bar = cc.model_ref(r["table"], r["kind"], r["min_points"], r["reject_px"], hs, ws)
    t, m = eng.coreg_fit_model_host(r["table"], r["kind"], r["min_points"], r["reject_px"], (hs, ws))
    assert np.array_equal(t[:, 7], want_t[:, 7]) and np.array_equal(t[:, 2:4], want_t[:, 2:4])
    assert (m[9], m[8]) == (want_m[9], want_m[8]) == (r["kind_used"], r["n_used"])
    diff = np.abs(cc.scaled_coefficients(m, hs, ws) - coef).max()
    print(f"{name}: diff {diff:.3g}, bar {bar:.3g}, |err| / bar {diff / bar if bar else 0.0:.3g}")
    assert diff <= bar
    if m[9] < 0:
        assert not m[:9].any()
    else:
        assert (m[6], m[7]) == (0.5 * (ws - 1), 0.5 * (hs - 1))
    if m[9] < 1:
        assert not m[[1, 2, 4, 5]].any()


@pytest.mark.parametrize("name", list(cc.MODEL_ROWS_ALL))
def test_model_row_claims(name):
    r = cc.MODEL_ROWS_ALL[name]
    hs, ws = r["hs"], r["ws"]
    t, m, coef, bar = cc.model_ref(r["table"], r["kind"], r["min_points"], r["reject_px"], hs, ws)
    assert list(np.flatnonzero(t[:, 7] == cc.OUTLIER)) == r["outliers"] and (m[9], m[8]) == (r["kind_used"], r["n_used"])
    assert not t[t[:, 7] != cc.OK, 2:4].any()
    if "outlier-outside" in name or "outlier-inside" in name:
        # the pushed record's residual after the first fit lies within 1e-3 of reject_px, on the side the name says
        first = cc._fit_ref(np.array(r["table"]), r["kind"], 1, hs, ws)[0]
        rec = r["table"][7]
        dy, dx = cc.shift_field(first, rec[0], rec[1])
        res = np.hypot(rec[2] - dy, rec[3] - dx)
        assert abs(res / r["reject_px"] - 1) < 2e-3 and (res > r["reject_px"]) == name.endswith("outlier-outside")
    if "collinear" in name:
        use, X, _ = cc._design(np.array(r["table"]), hs, ws)
        ev = np.linalg.eigvalsh(X.T @ X)
        assert ev[0] < 1e-12 * ev[-1] and use.sum() >= 3
    if name.startswith("rect-"):
        # the same truths as the square row, the table rebuilt at the rectangular shape
        sq = cc.MODEL_ROWS[name[5:]]
        assert (hs, ws) == cc.MODEL_RECT and all(r[k] == sq[k] for k in ("kind", "kind_used", "n_used", "outliers", "min_points"))
        assert len(r["table"]) == len(sq["table"]) and np.array_equal(r["table"][:, 7], sq["table"][:, 7])
        if r["kind_used"] == 1:
            # a fit that exchanged hs and ws leaves the bar: the reference of the exchanged shape, in this shape's scaled coefficients
            _, swapped, _, _ = cc.model_ref(r["table"], r["kind"], r["min_points"], r["reject_px"], ws, hs)
            off = np.abs(cc.scaled_coefficients(swapped, hs, ws) - coef).max()
            assert off > 1e6 * bar and (swapped[6], swapped[7]) == (m[7], m[6]) != (m[6], m[7])
    if name.startswith("clamp-"):
        xc, yc = 0.5 * (ws - 1), 0.5 * (hs - 1)
        assert min(xc, yc) <= 1.0 and (m[6], m[7]) == (xc, yc) and m[[1, 2, 4, 5]].all()
        _, X, (_, _, hx, hy) = cc._design(np.array(r["table"]), hs, ws)
        assert (hx, hy) == (max(xc, 1.0), max(yc, 1.0)) and 1.0 in (hx, hy) and np.ptp(X[:, 1]) > 0 and np.ptp(X[:, 2]) > 0


def test_model_rows_cover_the_classes():
    R = cc.MODEL_ROWS
    assert {r["kind_used"] for r in R.values()} == {-1, 0, 1} and {r["kind"] for r in R.values()} == {0, 1}
    assert {int((r["table"][:, 7] == cc.OK).sum()) if len(r["table"]) else 0 for r in R.values()} >= {0, 1, 2, 3, 25}
    assert any(r["outliers"] and r["kind_used"] == k for r in R.values() for k in (-1, 0, 1))
    assert {"outlier-inside", "outlier-outside", "collinear", "min-points-unmet", "no-records"} <= set(R)
    A = cc.MODEL_ROWS_ALL
    assert all((r["hs"], r["ws"]) == (cc.MODEL_HS, cc.MODEL_WS) for r in R.values()) and all(A[n] is R[n] for n in R)
    assert {n[5:] for n in A if n.startswith("rect-")} == set(R) and cc.MODEL_RECT[0] != cc.MODEL_RECT[1]
    assert all(abs(v - round(v)) == 0.5 for v in (0.5 * (cc.MODEL_RECT[0] - 1), 0.5 * (cc.MODEL_RECT[1] - 1)))      # xc != yc, hx != hy
    clamp = {(r["hs"], r["ws"]) for n, r in A.items() if n.startswith("clamp-")}
    assert clamp == {(200, 1), (200, 3), (2, 344), (2, 1)}                # xc = 0 and xc = 1 (the clamp's edge), yc = 0.5, both axes
    assert any(r["outliers"] for n, r in A.items() if n.startswith("clamp-"))
    assert len(A) == 2 * len(R) + 2 * len(clamp)


# ---- the surface table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.SURFACE_ROWS))
def test_surface_row_conditions(name):
    """Every finite entry's bar <= 1e-8; the peak's margin over every other entry >= 1e-4; which rows claim which status."""
    r, c = cc.SURFACE_ROWS[name], cc.surface_case(name)
    ref, bar = c["ref"], c["bar"]
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(bar)) and (bar[fin] <= cc.BAR_CAP).all() and (np.abs(ref[fin]) <= 1.0).all()
    inside = np.array([cc.region_inside(i, j, r["w"], r["f"], r["R"], r["he"], r["we"], c["hs"], c["ws"]) for i, j in c["origins"]])
    assert not fin[~inside].any()
    margins = [cc.peak_margin(s) for s in ref if np.isfinite(s).any()]
    assert all(m >= cc.MARGIN for m in margins), margins
    table = cc.peaks_ref(ref, c["origins"], r["w"], r["f"], r["R"], r["he"], r["we"], c["hs"], c["ws"], 0.6)
    status = table[:, 7].astype(int)
    assert (status[~inside] == cc.OUTSIDE).all() and (status[inside] != cc.OUTSIDE).all()
    if name == "edges":
        assert list(inside) == cc.EDGES_INSIDE and (status[inside] == cc.OK).all()
    elif r["inside"] is not None:
        # origins on both sides of the region test: the test says what the row says, and the inside ones recover the planted shift
        assert list(inside) == r["inside"] and fin[inside].all() and (status[inside] == cc.OK).all()
        assert (np.abs(table[inside, 2:4] - np.array(r["truth"])) <= 0.5).all(), table[inside, 2:4]
    elif r["mask"] == "all" or r["const"]:
        assert not fin.any() and (status == cc.NO_SCORE).all()
    elif name == "min-valid-missed":
        cnt, _ = cc.surface_ref_counts(c["emit"], c["mask"], c["s2"], c["nodata"], c["origins"], r["w"], r["f"], r["R"])
        assert np.array_equal(fin, cnt >= c["min_valid"]) and (cnt == c["min_valid"] - 1).any() and fin.any() and not fin.all()
    else:
        assert fin[inside].all() and (status == cc.OK).all(), status
        # the reference finds the planted shift: within half a pixel even at w = 4
        truth = np.array(r["truth"])
        assert (np.abs(table[:, 2:4] - truth) <= 0.5).all(), table[:, 2:4]
    if name == "min-valid-met":
        cnt, _ = cc.surface_ref_counts(c["emit"], c["mask"], c["s2"], c["nodata"], c["origins"], r["w"], r["f"], r["R"])
        assert cnt.min() == c["min_valid"] and fin.all() and cnt.min() < r["w"] ** 2
    if r["mask"] == "part":
        assert c["mask"].min() == 0 and c["mask"].max() > 1 and (~cc.s2_valid(c["s2"], c["nodata"])).sum() > 100
    if r["extra"]:
        assert c["emit_rs"] > r["we"] and c["s2_rs"] > c["ws"] and np.array_equal(c["s2_back"][:, :c["ws"]], c["s2"])
    assert (c["hs"], c["ws"]) == c["s2"].shape == (r["hs"], r["ws"]) and c["emit"].shape == (r["he"], r["we"])
    assert (c["emit_rs"], c["s2_rs"]) == (r["we"] + r["pads"][0], r["ws"] + r["pads"][1])
    if c["mask"] is not None:
        assert c["mask_rs"] == r["we"] + r["pads"][2] and np.array_equal(c["mask_back"][:, :r["we"]], c["mask"])


OWN_STRIDES = [n for n, r in cc.SURFACE_ROWS.items() if len(set(r["pads"])) == 3 and 0 not in r["pads"]]
STRADDLING = ("edges-rect", "s2-short-wide", "s2-tall-narrow")


@pytest.mark.parametrize("name", STRADDLING)
def test_region_rows_see_swapped_extents(name):
    """The inside list of these rows changes when he <-> we, and when hs <-> ws, are exchanged in the region test."""
    r = cc.SURFACE_ROWS[name]
    assert len({r["he"], r["we"], r["hs"] // r["f"], r["ws"] // r["f"]}) == 4

    def inside(he, we, hs, ws):
        return [cc.region_inside(i, j, r["w"], r["f"], r["R"], he, we, hs, ws) for i, j in r["origins"]]

    assert inside(r["he"], r["we"], r["hs"], r["ws"]) == r["inside"] and True in r["inside"] and False in r["inside"]
    assert inside(r["we"], r["he"], r["hs"], r["ws"]) != r["inside"]
    assert inside(r["he"], r["we"], r["ws"], r["hs"]) != r["inside"]
    if name != "edges-rect":
        # which of the two bounds decides: on one axis an origin passes the EMIT bound and fails the S2 bound, on the other the reverse
        big = 10 ** 6
        emit_only, s2_only = inside(r["he"], r["we"], big, big), inside(big, big, r["hs"], r["ws"])
        a, b = r["origins"][3], r["origins"][6]                    # the first outside origin along each axis, the other coordinate at 4
        assert (a[0] == 4) != (a[1] == 4) and (b[0] == 4) != (b[1] == 4) and (a[0] == 4) != (b[0] == 4)
        assert {(emit_only[3], s2_only[3]), (emit_only[6], s2_only[6])} == {(True, False), (False, True)}


def _restrided(back, rs, shape, sentinel):
    """The (h, w) plane that a reader with row stride `rs` sees at the base of `back` (past its end: `sentinel`)."""
    flat = back.reshape(-1)
    need = (shape[0] - 1) * rs + shape[1]
    if need > flat.size:
        flat = np.concatenate([flat, np.full(need - flat.size, sentinel, flat.dtype)])
    return np.lib.stride_tricks.as_strided(flat, shape, (rs * flat.itemsize, flat.itemsize), writeable=False)


@pytest.mark.parametrize("name", OWN_STRIDES)
def test_stride_rows_see_exchanged_strides(name):
    """The reference from the backing arrays under exchanged row strides - the mask read with emit_rs; emit_rs <-> s2_rs - leaves
    the bar of the row's own reference somewhere (or its NaN pattern)."""
    r, c = cc.SURFACE_ROWS[name], cc.surface_case(name)
    assert c["mask"] is not None and len({c["emit_rs"] - r["we"], c["s2_rs"] - r["ws"], c["mask_rs"] - r["we"]}) == 3
    assert len(set(r["offs"])) == 3
    eshape, sshape = c["emit"].shape, c["s2"].shape
    nan, seven, one = np.float32(np.nan), c["s2"].dtype.type(7), np.uint8(1)

    def ref(ers, srs, mrs):
        return cc.surface_ref(_restrided(c["emit_back"], ers, eshape, nan), _restrided(c["mask_back"], mrs, eshape, one),
                              _restrided(c["s2_back"], srs, sshape, seven), c["nodata"], c["origins"], r["w"], r["f"], r["R"], c["min_valid"])[0]

    def differs(got):
        fin = np.isfinite(c["ref"])
        if not np.array_equal(np.isfinite(got), fin):
            return True
        return bool((np.abs(got[fin] - c["ref"][fin]) > c["bar"][fin]).any())

    assert not differs(ref(c["emit_rs"], c["s2_rs"], c["mask_rs"]))                              # the backing arrays hold the case
    assert differs(ref(c["emit_rs"], c["s2_rs"], c["emit_rs"]))                                  # the mask indexed with emit_rs
    assert differs(ref(c["s2_rs"], c["emit_rs"], c["mask_rs"]))                                  # emit_rs <-> s2_rs
    assert differs(ref(c["s2_rs"], c["s2_rs"], c["mask_rs"])) and differs(ref(c["emit_rs"], c["emit_rs"], c["mask_rs"]))


def test_surface_rows_cover_the_bounds():
    R = cc.SURFACE_ROWS.values()
    assert {r["w"] for r in R} == {4, 8, 9, 32, 64} and {r["R"] for r in R} == {1, 3, 4, 5, 6, 7, 8, 9, 12, 24}
    assert {r["f"] for r in R} == {1, 2, 3, 4, 5, 6, 7, 8}
    rect = [r for r in R if r["he"] != r["we"]]
    assert {r["f"] for r in rect} == {3, 4, 5, 6, 7, 8} and {r["dtype"] for r in rect} == {"f32", "u16"}
    assert any(r["he"] > r["we"] for r in rect) and any(r["he"] < r["we"] for r in rect) and {r["w"] for r in rect} == {8, 9}
    assert {(r["R"] < r["f"], r["R"] == r["f"], r["R"] > r["f"]) for r in rect} == {(True, False, False), (False, True, False), (False, False, True)}
    assert any((r["f"], r["R"]) == (8, 24) for r in rect)
    assert len(OWN_STRIDES) >= 2 and {cc.SURFACE_ROWS[n]["dtype"] for n in OWN_STRIDES} == {"f32", "u16"}
    off_f = [r for r in R if (r["hs"], r["ws"]) != (r["he"] * r["f"], r["we"] * r["f"])]
    assert any(r["hs"] < r["he"] * r["f"] and r["ws"] > r["we"] * r["f"] for r in off_f)
    assert any(r["hs"] > r["he"] * r["f"] and r["ws"] < r["we"] * r["f"] for r in off_f)
    assert all(r["hs"] <= 384 and r["ws"] <= 384 for r in R)
    assert all(abs(t % 1.0 - 0.5) > 0.05 for r in rect for t in r["truth"])                      # no planted shift at x.5: two candidates tie
    assert {len(r["origins"]) for r in R} >= {1, 2, 65}
    assert {(r["R"] < r["f"], r["R"] == r["f"], r["R"] > r["f"]) for r in R} == {(True, False, False), (False, True, False), (False, False, True)}
    assert {r["dtype"] for r in R} == {"f32", "u16"} and {r["mask"] for r in R} == {"none", "part", "all"}
    assert any(r["extra"] for r in R) and any(r["const"] for r in R)
    # a 64-wide window has no search region inside a 64 x 64 EMIT scene: those rows' EMIT scenes are larger, their S2 scenes are not
    assert all(r["he"] <= 64 or r["w"] == 64 for r in R) and all(r["he"] * r["f"] <= 384 and r["we"] * r["f"] <= 384 for r in R)
    assert {cc.surface_instance(r) for r in R} == set(cc.all_instances()[:2])


# ---- the peak table --------------------------------------------------------------------------------------------------------------------
def test_peak_rows_claim_their_status():
    names, surf, origins, want = cc.peak_case()
    table = cc.peaks_ref(surf, origins, cc.PEAK_W, cc.PEAK_F, cc.PEAK_R, min_score=cc.PEAK_MIN_SCORE, **cc.PEAK_SHAPES)
    assert np.array_equal(table[:, 7], want), dict(zip(names, table[:, 7]))
    assert set(want) == {cc.OK, cc.OUTSIDE, cc.NO_SCORE, cc.BORDER, cc.LOW_SCORE}
    rec = dict(zip(names, table))
    assert tuple(rec["tie"][2:4]) == (-1.0, -1.0)                                             # the first of two equal maxima
    assert rec["tie-neighbour"][3] == 0.5 and rec["row-tie"][3] == 0.5 - 1.0                  # r == c: exactly +0.5 from the first
    assert rec["den-zero"][3] == 0.0 and rec["den-zero"][4] == 1.0
    assert -0.5 <= rec["clip-minus"][3] < -0.49 and 0.49 < rec["clip-plus"][2] <= 0.5
    assert np.isnan(rec["sharpness-none"][5]) and rec["sharpness-none"][6] == 9 and np.isnan(rec["all-nan"][4])
    assert rec["score-at-min"][4] == cc.PEAK_MIN_SCORE and rec["score-below-min"][4] < cc.PEAK_MIN_SCORE
    assert rec["inf-entry"][6] == 48 and rec["nan-diagonal"][7] == cc.OK
    assert not table[want != cc.OK, 2:4].any()
    assert (table[:, 0] == cc.PEAK_F * (origins[:, 0] + cc.PEAK_W / 2) - 0.5).all()


def test_rect_peak_rows_claim_their_status():
    """The crafted surfaces on a rectangular pair of planes: the same records but for cy, cx; one OUTSIDE record per axis and side,
    each outside on that axis alone; cy follows i0 and cx follows j0 on origins with i0 != j0."""
    names, surf, origins, want = cc.peak_case(rect=True)
    sq_names, _, sq_origins, _ = cc.peak_case()
    sh = cc.PEAK_SHAPES_RECT
    assert len({sh["he"], sh["we"], sh["hs"] // cc.PEAK_F, sh["ws"] // cc.PEAK_F}) == 4
    table = cc.peaks_ref(surf, origins, cc.PEAK_W, cc.PEAK_F, cc.PEAK_R, min_score=cc.PEAK_MIN_SCORE, **sh)
    assert np.array_equal(table[:, 7], want), dict(zip(names, table[:, 7]))
    assert (origins[:, 0] != origins[:, 1]).all()
    assert (table[:, 0] == cc.PEAK_F * (origins[:, 0] + cc.PEAK_W / 2) - 0.5).all()
    assert (table[:, 1] == cc.PEAK_F * (origins[:, 1] + cc.PEAK_W / 2) - 0.5).all() and (table[:, 0] != table[:, 1]).all()
    square = dict(zip(sq_names, cc.peaks_ref(cc.peak_case()[1], sq_origins, cc.PEAK_W, cc.PEAK_F, cc.PEAK_R, min_score=cc.PEAK_MIN_SCORE,
                                             **cc.PEAK_SHAPES)))
    for n, rec in zip(names, table):
        if n not in cc.PEAK_OUTSIDE_RECT:
            assert np.array_equal(rec[2:], square[n][2:], equal_nan=True), n

    def inside(i0, j0, **kw):
        return cc.region_inside(i0, j0, cc.PEAK_W, cc.PEAK_F, cc.PEAK_R, **dict(sh, **kw))

    assert set(cc.PEAK_OUTSIDE_RECT) == {"outside-top", "outside-bottom", "outside-left", "outside-right"}
    for n, (i0, j0) in cc.PEAK_OUTSIDE_RECT.items():
        rows = n in ("outside-top", "outside-bottom")
        assert not inside(i0, j0) and inside(5, j0) == rows and inside(i0, 5) == (not rows) and inside(5, 5)
        step = -1 if n in ("outside-bottom", "outside-right") else 1
        assert inside(i0 + step, j0) if rows else inside(i0, j0 + step)                         # the first origin past the bound
    # the bottom bound is the S2 plane's, the right one the EMIT plane's: exchanged extents admit or refuse other origins
    assert inside(15, 5, hs=10 ** 6) and not inside(15, 5, he=10 ** 6) and inside(5, 23, we=10 ** 6) and not inside(5, 23, ws=10 ** 6)
    assert inside(15, 5, hs=sh["ws"], ws=sh["hs"]) and inside(5, 23, he=sh["we"], we=sh["he"]) is False


# ---- the warp table --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.WARP_ROWS))
def test_warp_row_claims(name):
    r, c = cc.WARP_ROWS[name], cc.warp_case(name)
    scene, ref, raw, m = c["scene"], c["ref"], c["raw"], c["model"]
    assert ref.shape == scene.shape and ref.dtype == scene.dtype
    h, w = scene.shape[1:]
    corners = np.array([cc.shift_field(m, y, x) for y in (0, h - 1) for x in (0, w - 1)])
    respected = bool((np.abs(corners) <= r["bound"][0]).all() and (np.abs(m[[1, 2, 4, 5]]) <= r["bound"][1]).all())
    assert respected == (r["status"] == 0)
    valid = cc.s2_valid(scene, c["nodata"])
    integer = not m[[1, 2, 4, 5]].any() and m[0] == np.floor(m[0]) and m[3] == np.floor(m[3])
    if integer and np.isfinite(m[0]):
        # a bit-exact shifted copy; an invalid sample costs exactly its own pixel
        dy, dx = int(m[0]), int(m[3])
        want = np.full(scene.shape, ref.dtype.type(c["fill"]) if scene.dtype == np.float32 else np.uint16(c["fill"]))
        ys, xs = np.arange(h), np.arange(w)
        oky, okx = (ys + dy >= 0) & (ys + dy <= h - 1), (xs + dx >= 0) & (xs + dx <= w - 1)
        src = scene[:, np.clip(ys + dy, 0, h - 1)][:, :, np.clip(xs + dx, 0, w - 1)]
        sv = valid[:, np.clip(ys + dy, 0, h - 1)][:, :, np.clip(xs + dx, 0, w - 1)]
        take = sv & oky[None, :, None] & okx[None, None, :]
        want[take] = src[take]
        assert np.array_equal(want.view(np.uint32 if scene.dtype == np.float32 else np.uint16),
                              ref.view(np.uint32 if scene.dtype == np.float32 else np.uint16))
    if r["bad"] != "none":
        assert (~valid).sum() > 10 and np.isnan(raw).sum() >= (~valid).sum() * (1 if integer else 4)
    if name == "half-u16-rounding":
        frac = raw[np.isfinite(raw)] % 1.0
        halves = raw[np.isfinite(raw)][frac == 0.5]
        assert (np.rint(halves) > halves).any() and (np.rint(halves) < halves).any()           # half to even, both ways
        assert (raw[np.isfinite(raw)] < 0).any() and (raw[np.isfinite(raw)] > 65535).any() and ref.min() == 0 and ref.max() == 65535
    if name.startswith("past-"):
        fill = np.isnan(raw[0])
        assert fill[0].all() != fill[-1].all() and fill[:, 0].all() != fill[:, -1].all() and not fill.all()
    if name in ("wholly-outside", "nan-model"):
        assert np.isnan(raw).all()
    if name in ("affine", "affine-u16", "direct", "direct-u16", "strides-direct", "strides-u16-direct") or name.startswith("off-centre"):
        assert m[[1, 2, 4, 5]].any()
    if r["centre"] is not None:
        # a warp that took the centre from the scene it warps gives another output
        assert (m[6], m[7]) == r["centre"] != (0.5 * (w - 1), 0.5 * (h - 1)) and m[[1, 2, 4, 5]].all()
        own = cc.make_model(h, w, **r["model"])
        other, _ = cc.warp_ref(scene, own, c["nodata"], c["fill"])
        assert (other != ref).mean() > 0.5 and np.isfinite(raw).mean() > 0.5
    else:
        assert (m[6], m[7]) == (0.5 * (w - 1), 0.5 * (h - 1)) or m[9] < 0
    if name.startswith("thin-"):
        assert min(h, w) < 4 and r["bad"] == "none"
        if name.endswith("-frac") or name.endswith("-direct"):
            assert np.isfinite(raw).any() and ((h, w) == (1, 1) or (not integer and np.isnan(raw).any()))
        if name.endswith("-outside"):
            assert np.isnan(raw).all() and r["status"] == 0


def test_warp_rows_cover_the_classes():
    R = cc.WARP_ROWS
    assert {cc.warp_instance(r["dtype"], r["bound"][1]) for r in R.values()} == set(cc.all_instances()[4:])
    assert {r["status"] for r in R.values()} == {0, 1}
    assert any(r["off"] % 16 for r in R.values()) and any(r["w"] % 2 for r in R.values()) and any(r["extra"] for r in R.values())
    assert {(r["dtype"], r["bad"]) for r in R.values()} >= {("f32", "nan"), ("f32", "nodata"), ("u16", "nodata"), ("f32", "none")}
    assert all(r["h"] <= 384 and r["w"] <= 384 for r in R.values())
    assert any(r["w"] > 2 * cc.TILE_W and r["h"] > 2 * cc.TILE_H for r in R.values())        # more than one tile each way
    inst = {n: cc.warp_instance(r["dtype"], r["bound"][1]).split(", ")[1][:-1] for n, r in R.items()}
    # strides of their own in and out: both dtypes on both instances; gaps between the bands on both sides in one row
    own = {n: r for n, r in R.items() if r["out_extra"] != r["extra"] and r["out_off"] != r["off"]
           and r["h"] * (r["w"] + r["extra"]) + r["in_gap"] != r["h"] * (r["w"] + r["out_extra"]) + r["out_gap"]}
    assert {(r["dtype"], inst[n]) for n, r in own.items()} == {(d, i) for d in ("f32", "u16") for i in ("LDS", "DIRECT")}
    assert any(r["in_gap"] and r["out_gap"] for r in own.values()) and all(r["bands"] > 1 and r["bad"] != "none" for r in own.values())
    assert all(r["in_gap"] or r["out_gap"] for r in own.values())
    # a model centred elsewhere, on both instances
    assert {inst[n] for n, r in R.items() if r["centre"] is not None} == {"LDS", "DIRECT"}
    # tile multiples, one less and one more, under a fractional shift with two bands
    tiles = [r for n, r in R.items() if n.startswith("tile-")]
    assert {r["w"] for r in tiles} == set(cc.WARP_TILE_W) == {cc.TILE_W - 1, cc.TILE_W, cc.TILE_W + 1, 2 * cc.TILE_W}
    assert {r["h"] for r in tiles} == set(cc.WARP_TILE_H) == {cc.TILE_H - 1, cc.TILE_H, cc.TILE_H + 1, 2 * cc.TILE_H}
    assert all(r["bands"] == 2 and r["model"]["dy0"] % 1 and r["model"]["dx0"] % 1 for r in tiles)
    assert {r["dtype"] for r in tiles} == {"f32", "u16"}
    # planes thinner than the four taps: a fractional and an integer shift on each
    for h, w in cc.WARP_THIN:
        assert {f"thin-{h}x{w}-frac", f"thin-{h}x{w}-int"} <= set(R)
    assert set(cc.WARP_THIN) == {(1, 1), (1, 70), (40, 1), (2, 3), (3, 2)}
    assert {inst[n] for n in R if n.startswith("thin-")} == {"LDS", "DIRECT"}
    # the Keys weights: a partition of unity, (0, 1, 0, 0) at t = 0
    for t in (0.0, 0.25, 0.5, 0.999):
        assert abs(sum(cc.keys(t)) - 1.0) < 1e-15
    assert [float(v) for v in cc.keys(0.0)] == [0.0, 1.0, 0.0, 0.0]


# ---- the reference against the truth ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "u16"])
@pytest.mark.parametrize("name", list(cc.E2E_MODELS))
def test_reference_recovers_the_truth(name, dtype):
    _reference_recovers_the_truth(name, dtype, False)


@pytest.mark.parametrize("dtype", ["f32", "u16"])
@pytest.mark.parametrize("name", list(cc.E2E_MODELS))
def test_reference_recovers_the_truth_rectangular(name, dtype):
    _reference_recovers_the_truth(name, dtype, True)


def _reference_recovers_the_truth(name, dtype, rect):
    c = cc.e2e_case(name, dtype, rect)
    p = c["params"]
    assert c["emit"].shape == (p["he"], p["we"]) and c["s2"].shape == (c["hs"], c["ws"]) and max(c["hs"], c["ws"]) <= 384
    if rect:
        assert p["he"] != p["we"] and 0 < c["hs"] - p["f"] * p["he"] < p["f"] and c["ws"] == p["f"] * p["we"]
        assert len(set(c["origins"][:, 0])) != len(set(c["origins"][:, 1]))
    assert np.array_equal(c["origins"], s2_emit.tie_point_grid(p["he"], p["we"], c["hs"], c["ws"], window=p["w"], step=p["step"],
                                                               factor=p["f"], max_shift=p["R"]))
    t0, t, truth = c["table0"], c["table"], c["truth"]
    assert (np.nanmax(c["bar"]) <= cc.BAR_CAP) and min(cc.peak_margin(s) for s in c["surface"]) >= cc.MARGIN
    assert t0[cc.DECOY, 7] == cc.OK and t0[cc.DECOY, 4] > 0.9                                  # a good match at the wrong place ...
    assert t[cc.DECOY, 7] == cc.OUTLIER and (np.delete(t[:, 7], cc.DECOY) == cc.OK).all()        # ... flagged by the fit, alone
    ok = t[:, 7] == cc.OK
    dy, dx = cc.shift_field(truth, t[ok, 0], t[ok, 1])
    err = np.maximum(np.abs(t[ok, 2] - dy), np.abs(t[ok, 3] - dx))
    print(f"{name} {dtype}: {int(ok.sum())} OK tie points, largest error {err.max():.3f} S2 pixels")
    assert err.max() <= TRUTH_CAP
    # the fitted field over the whole scene
    yy, xx = np.meshgrid(np.arange(0, c["hs"], 7.0), np.arange(0, c["ws"], 7.0), indexing="ij")
    fy, fx = cc.shift_field(c["model"], yy, xx)
    gy, gx = cc.shift_field(truth, yy, xx)
    assert max(np.abs(fy - gy).max(), np.abs(fx - gx).max()) <= TRUTH_CAP
    assert c["model"][9] == (1 if name == "affine" else 0) and c["model"][8] == ok.sum()
    _, den_min = cc.shift_bar(c["surface"], c["bar"], t0, c["params"]["R"])
    assert den_min.min() >= 1e-3                                                               # every row is admitted by the GPU test


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_masked_case_conditions(dtype):
    """The pair with an EMIT mask and S2 nodata: the bars and margins of the table hold, statuses other than OK occur, and both
    the mask and the nodata value change the reference."""
    c = cc.masked_case(dtype)
    p, surf = c["params"], c["surface"]
    fin = np.isfinite(surf)
    assert (c["bar"][fin] <= cc.BAR_CAP).all() and min(cc.peak_margin(s) for s in surf if np.isfinite(s).any()) >= cc.MARGIN
    status = c["table0"][:, 7].astype(int)
    assert set(status) == {cc.OK, cc.NO_SCORE} and (status != cc.OK).sum() >= 3 and (status == cc.OK).sum() >= 20
    per_point = fin.reshape(len(surf), -1).sum(axis=1)
    assert ((per_point > 0) & (per_point < fin[0].size)).any()                   # a surface with some candidates short of pairs
    assert c["mask"].dtype == np.uint8 and c["mask"].min() == 0 and c["mask"].max() > 1
    bad = ~cc.s2_valid(c["s2"], c["nodata"])
    assert bad.sum() > 1000 and (dtype == "u16" or (np.isnan(c["s2"]).any() and np.isinf(c["s2"]).any()))

    def ref(mask, nodata):
        return cc.surface_ref(c["emit"], mask, c["s2"], nodata, c["origins"], p["w"], p["f"], p["R"], c["min_valid"])[0]

    for other in (ref(None, c["nodata"]), ref(c["mask"], None)):
        assert not np.array_equal(np.isfinite(other), fin) or (np.abs(other - surf)[fin] > c["bar"][fin]).any()
