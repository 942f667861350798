"""The reprojection family on the host side: include/hsr_reproject.h against nat.REPROJECT_SIGNATURES and the library's exports; the
refusals of every entry and the launch record's contract, which need no device; the public surface; utm_params and
utm_target_grid on hand-computable cases; the series against two independent facts and the fixture against its generator (both
when mpmath is importable); the coefficients in the header and the source against the generator's rationals; the coordinate bar
on hsr_reproject_coords_host; what the case tables of tests/reproject_cases.py claim about their rows; and the sweep generator's
admission rate."""
import ctypes as C
import importlib.util
import inspect
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import reproject_cases as rc
import s2_emit
from conftest import ROOT
from s2_emit import _engine as eng
from s2_emit import _native as nat
from s2_emit import reproject

LAUNCH_PATH = ("hsr_reproject_coords", "hsr_reproject_warp")
HOST_ONLY = ("hsr_reproject_coords_host", "hsr_reproject_last_launch", "hsr_reproject_instance_count", "hsr_reproject_instance_name")
INVALID = 1


def _gen():
    spec = importlib.util.spec_from_file_location("gen_g18", os.path.join(ROOT, "tests", "golden", "gen_g18.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header():
    text = open(os.path.join(ROOT, "include", "hsr_reproject.h")).read()
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
    assert declared == sorted(nat.REPROJECT_SIGNATURES) == sorted(LAUNCH_PATH + HOST_ONLY)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/hsr_reproject.h but not exported"
        sig = nat.REPROJECT_SIGNATURES[name]
        assert getattr(lib, name).argtypes == sig[1] and getattr(lib, name).restype == sig[0]
        assert name in comments, f"{name} is not documented"
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        nargs = 0 if proto.strip() == "void" else proto.count(",") + 1
        assert nargs == len(sig[1]), (name, proto)
        if name in LAUNCH_PATH:
            assert proto.split(",")[-1].strip() == "hsr_stream_t stream", name                 # the stream is the last argument
            assert "emit_proj.py" in _doc_of(text, name), f"{name} cites no reference"
        else:
            assert "stream" not in proto
    assert '#include "hsr.h"' in code and "HSR_ABI_VERSION" not in code
    # a family of its own: the other headers, the other tables, the ABI version and the seven other records are what they were
    others = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("hsr.h", "hsr_color.h", "hsr_coreg.h"))
    for name in declared:
        assert name not in nat.SIGNATURES and name not in nat.COLOR_SIGNATURES and name not in nat.COREG_SIGNATURES, name
        assert name not in others, name
    assert lib.hsr_abi_version() == 5 == nat.HSR_ABI_VERSION
    assert (lib.hsr_aux_instance_count(), lib.hsr_scene_instance_count(), lib.hsr_k4_instance_count(), lib.hsr_pairs_instance_count(),
            lib.hsr_ortho_instance_count(), lib.hsr_color_instance_count(), lib.hsr_coreg_instance_count()) == (32, 20, 31, 12, 6, 20, 8)
    assert nat.REPROJECT_SIGNATURES["hsr_reproject_last_launch"] == nat.SIGNATURES["hsr_k4_last_launch"]
    assert nat.REPROJECT_SIGNATURES["hsr_reproject_instance_name"] == nat.SIGNATURES["hsr_k4_instance_name"]
    for macro, value in (("HSR_REPROJECT_STRICT", rc.STRICT), ("HSR_REPROJECT_RENORM", rc.RENORM), ("HSR_REPROJECT_TILE_W", rc.TILE_W),
                         ("HSR_REPROJECT_TILE_H", rc.TILE_H)):
        assert re.search(r"#define %s %d\b" % (macro, value), code) and getattr(nat, macro) == value
    # what the header must say about itself
    for phrase in ("antimeridian", "GDAL's bits", "minification", "-ffp-contract=off", "not consulted"):
        assert phrase in comments, phrase


def test_coefficients_in_header_and_source_are_the_generators():
    """The beta rationals, read out of the header's comment and out of the source's statements, against gen_g18's table (which the
    mpmath tests below hold to the two facts): exact, so a wrong beta4 .. beta6 - below the coordinate bar - shows here."""
    gen = _gen()
    _, _, comments = _header()
    src = open(os.path.join(ROOT, "hyperspectral_super-resolution_amd", "csrc", "hsr_reproject.hip")).read()
    term = re.compile(r"([+-]?)\s*(?:(\d+)(?:\.0)?\s*/\s*(\d+)(?:\.0)?\s*\*?\s*)?n\s*\^?\s*(\d?)(?:\s*/\s*(\d+)(?:\.0)?)?")

    def parse(expr):
        got = {}
        for sign, p, q, power, q2 in term.findall(expr):
            got[int(power or 1)] = Fraction(int(p or 1), int(q or q2 or 1)) * (-1 if sign == "-" else 1)
        return got

    for j, row in enumerate(gen.BETA, start=1):
        want = {k + 1: Fraction(p, q) for k, (p, q) in enumerate(row) if p}
        in_header = re.search(r"beta%d = ([^\n]*?)(?:\.\s|\n|$)" % j, comments).group(1).rstrip(".")
        assert parse(in_header) == want, (j, in_header)
        in_source = re.search(r"t\.beta\[%d\] = ([^;]*);" % (j - 1), src).group(1)
        assert parse(re.sub(r"\bn(\d)\b", r"n^\1", in_source)) == want, (j, in_source)
    # the Python restatement, both series, to the last bit but a few
    n = Fraction(1) / (2 * Fraction(gen.INV_F) - 1)
    _, _, _, alpha, beta = reproject._series(float(gen.A_WGS84), float(gen.INV_F))
    for rows, got in ((gen.ALPHA, alpha), (gen.BETA, beta)):
        for row, g in zip(rows, got):
            want = float(sum(Fraction(p, q) * n ** (k + 1) for k, (p, q) in enumerate(row)))
            assert abs(g - want) <= 4 * np.spacing(abs(want)), (row, g, want)


# ---- refusals and the record, without a device ---------------------------------------------------------------------------------------
def test_c_abi_refusals_need_no_device():
    lib = nat.load()
    p, q, k, null, st = C.c_void_p(1 << 20), C.c_void_p(1 << 30), C.c_void_p(1 << 40), C.c_void_p(0), C.c_void_p(0)
    lib.hsr_reproject_last_launch(None, 0)

    def refused(word, fn, *args):
        rc_ = fn(*args)
        text = lib.hsr_last_error().decode()
        assert rc_ == INVALID and word in text and fn.__name__ in text, (fn.__name__, args, rc_, text)

    geo = dict(e0=4e5, n0=3.9e6, dx=60.0, dy=60.0, h=4, w=5, lon0=-117.0, k0=0.9996, fe=5e5, fn=0.0, a=6378137.0, inv_f=298.257223563,
               g0=-118.0, g1=5e-4, g3=35.0, g5=-5e-4)

    def coords(entry, out=p, **kw):
        g = dict(geo, **kw)
        return (entry,) + tuple(g.values()) + (out,) + ((st,) if entry is lib.hsr_reproject_coords else ())

    for fn in (lib.hsr_reproject_coords, lib.hsr_reproject_coords_host):
        host = fn is lib.hsr_reproject_coords_host
        ok = (C.c_double * 40)() if host else p
        refused("NULL", *coords(fn, out=None if host else null))
        for kw in (dict(h=0), dict(w=0), dict(h=-3)):
            refused("extent", *coords(fn, out=ok, **kw))
        for key in geo:
            if key not in ("h", "w"):
                for bad in (float("nan"), float("inf"), float("-inf")):
                    refused("non-finite", *coords(fn, out=ok, **{key: bad}))
        for kw in (dict(dx=0.0), dict(dx=-60.0), dict(dy=0.0), dict(dy=-1.0), dict(g1=0.0), dict(g1=-5e-4), dict(g5=0.0), dict(g5=5e-4)):
            refused("north-up", *coords(fn, out=ok, **kw))
        for kw in (dict(a=0.0), dict(a=-1.0), dict(k0=0.0), dict(k0=-0.9996), dict(inv_f=1.0), dict(inv_f=0.5), dict(inv_f=-298.0)):
            refused("ellipsoid", *coords(fn, out=ok, **kw))

    def warp(src=p, b=2, hs=10, ws=12, sbs=120, srs=12, co=k, h=6, w=8, rule=1, mf=1.5, out=q, obs=48, ors=8, counts=null, status=p):
        return lib.hsr_reproject_warp, src, b, hs, ws, sbs, srs, co, h, w, 0, 0.0, -9999.0, rule, mf, out, obs, ors, counts, status, st

    for kw in (dict(src=null), dict(co=null), dict(out=null), dict(status=null)):
        refused("NULL", *warp(**kw))
    for rule in (-1, 2, 7):
        refused("rule", *warp(rule=rule))
    for kw in (dict(b=0), dict(hs=0), dict(ws=-1), dict(h=0), dict(w=0)):
        refused("extent", *warp(**kw))
    for kw in (dict(srs=11), dict(ors=7), dict(sbs=119), dict(obs=47)):
        refused("strides", *warp(**kw))
    for mf in (-1.0, float("nan"), -0.001):
        refused("max_footprint", *warp(mf=mf))
    base = 1 << 20
    for out in (base, base + 4, base + 4 * 239, base - 4 * 95):                              # in place, and overlapping at both ends
        refused("source", *warp(out=C.c_void_p(out)))
    cbase = 1 << 40
    for out in (cbase, cbase + 8 * 95, cbase - 4 * 95):
        refused("coordinate", *warp(out=C.c_void_p(out)))
    buf = C.create_string_buffer(64)
    assert lib.hsr_reproject_last_launch(buf, 64) == 0 and buf.value == b""                  # refused calls leave no record


def test_instance_table_and_record_contract():
    lib = nat.load()
    n = lib.hsr_reproject_instance_count()
    table = [lib.hsr_reproject_instance_name(i).decode() for i in range(n)]
    assert n == 5 == len(set(table)) and table == rc.all_instances()
    for bad in (-1, n):
        assert lib.hsr_reproject_instance_name(bad) is None
        assert b"hsr_reproject_instance_name" in lib.hsr_last_error() and str(bad).encode() in lib.hsr_last_error()
    _, _, comments = _header()
    assert "hsr_reproject_instance_count = 5" in comments and "8 most recent" in comments and "hsr_aux_last_launch" in comments
    buf = C.create_string_buffer(64)
    buf.value = b"junk"
    lib.hsr_reproject_last_launch(None, 0)
    assert lib.hsr_reproject_last_launch(buf, 0) == 0 and buf.value == b"junk"
    assert lib.hsr_reproject_last_launch(buf, 64) == 0 and buf.value == b""
    assert lib.hsr_reproject_last_launch(None, 64) == 0
    # the other families' tables are what they were
    assert (lib.hsr_aux_instance_count(), lib.hsr_scene_instance_count(), lib.hsr_k4_instance_count(), lib.hsr_pairs_instance_count(),
            lib.hsr_ortho_instance_count(), lib.hsr_color_instance_count(), lib.hsr_coreg_instance_count()) == (32, 20, 31, 12, 6, 20, 8)


def test_public_surface():
    new = ["reproject_scene", "remap_scene", "reproject_coords", "utm_target_grid", "utm_params", "tm_forward", "tm_inverse",
           "ReprojectOutput"]
    allv = s2_emit.__all__
    at = allv.index(new[0])
    assert allv[at:at + len(new)] == new and all(hasattr(s2_emit, n) for n in new)
    assert allv[at - 1] == "CoregOutput" and allv[at + len(new)] == "apply_glt"                # between the coreg and the ortho names
    assert len(set(allv)) == len(allv)
    sig = inspect.signature(s2_emit.utm_target_grid).parameters
    assert list(sig) == ["src_geotransform", "src_shape", "epsg", "s2_geotransform", "s2_shape", "res"] and sig["res"].default == 60.0
    assert list(inspect.signature(s2_emit.reproject_coords).parameters)[:3] == ["grid", "epsg", "src_geotransform"]
    sig = inspect.signature(s2_emit.remap_scene).parameters
    assert [(k, v.default) for k, v in sig.items()][2:6] == [("nodata", None), ("fill", -9999.0), ("rule", "renorm"), ("out", None)]
    assert all(v.kind is v.KEYWORD_ONLY for v in list(sig.values())[2:])
    sig = inspect.signature(s2_emit.reproject_scene).parameters
    assert [(k, v.default) for k, v in sig.items()][2:] == [("epsg", inspect.Parameter.empty), ("s2_geotransform", inspect.Parameter.empty),
                                                            ("s2_shape", inspect.Parameter.empty), ("res", 60.0), ("nodata", -9999.0),
                                                            ("fill", -9999.0), ("rule", "renorm"), ("coords", None), ("out", None)]
    assert all(v.kind is v.KEYWORD_ONLY for v in list(sig.values())[2:])
    assert s2_emit.ReprojectOutput._fields == ("scene", "geotransform", "grid", "counts", "coords")
    assert "emit_proj.py" in reproject.__doc__ and "NOT reproduced" in reproject.__doc__ and "antimeridian" in reproject.__doc__
    from s2_emit import ortho
    for doc in (ortho.__doc__, s2_emit.ortho_scene.__doc__, s2_emit.apply_glt.__doc__):
        assert "reproject_scene" in doc


def test_python_argument_checks():
    gt, s2gt = (-118.0, 5e-4, 0.0, 35.0, 0.0, -5e-4), (399960.0, 60.0, 0.0, 3900000.0, 0.0, -60.0)
    for bad, word in (((-118.0, 5e-4, 1e-6, 35.0, 0.0, -5e-4), "rotation"), ((-118.0, 5e-4, 0.0, 35.0, 0.0, 5e-4), "north-up"),
                      ((-118.0, 5e-4, 0.0, 35.0), "six")):
        with pytest.raises(ValueError, match=word):
            s2_emit.utm_target_grid(bad, (100, 100), 32611, s2gt, (1830, 1830))
    with pytest.raises(ValueError, match="res"):
        s2_emit.utm_target_grid(gt, (100, 100), 32611, s2gt, (1830, 1830), res=0.0)
    with pytest.raises(ValueError, match="grid"):
        s2_emit.reproject_coords((0.0, 0.0, 60.0, 60.0, 0, 1), 32611, gt)
    with pytest.raises(ValueError, match="rule"):
        s2_emit.remap_scene(None, None, rule="cubic")
    with pytest.raises(ValueError, match="rule"):
        s2_emit.reproject_scene(None, gt, epsg=32611, s2_geotransform=s2gt, s2_shape=(10, 10), rule="nearest")
    with pytest.raises(ValueError, match="GPU tensors"):
        s2_emit.remap_scene(np.zeros((1, 4, 4), np.float32), np.zeros((2, 2, 2)))


# ---- utm_params, utm_target_grid -------------------------------------------------------------------------------------------------------
def test_utm_params():
    for zone in range(1, 61):
        for south in (False, True):
            code = (32700 if south else 32600) + zone
            want = (6.0 * zone - 183.0, 0.9996, 500000.0, 1e7 if south else 0.0, 6378137.0, 298.257223563)
            assert s2_emit.utm_params(code) == want == s2_emit.utm_params(f"EPSG:{code}") == s2_emit.utm_params(str(code))
    assert s2_emit.utm_params(32611)[0] == -117.0 and s2_emit.utm_params(32731)[0] == 3.0
    for bad in (32600, 32661, 32700, 32761, 4326, 3857, 0, -32611, "EPSG:4326", "utm11", None, 32611.5):
        with pytest.raises(ValueError, match="epsg"):
            s2_emit.utm_params(bad)


def _src_bounds(gt, shape, epsg):
    l, t = gt[0], gt[3]
    r, b = l + gt[1] * shape[1], t + gt[5] * shape[0]
    X, Y = s2_emit.tm_forward([l, l, r, r], [b, t, b, t], s2_emit.utm_params(epsg))
    return X.min(), Y.min(), X.max(), Y.max()


def test_utm_target_grid():
    gt, shape, epsg = (-117.6, 0.000542, 0.0, 34.9, 0.0, -0.000542), (1800, 2200), 32611
    L, B, R, T = _src_bounds(gt, shape, epsg)
    # S2 inside the source: the S2 extent itself, which is on its own lattice
    x0, y0 = 60.0 * math.ceil(L / 60.0) + 6000.0, 60.0 * math.floor(T / 60.0) - 6000.0
    s2gt = (x0, 10.0, 0.0, y0, 0.0, -10.0)
    assert x0 + 3000 < R and y0 - 2400 > B
    assert s2_emit.utm_target_grid(gt, shape, epsg, s2gt, (240, 300)) == (x0, y0 - 2400.0, x0 + 3000.0, y0, 40, 50)
    assert s2_emit.utm_target_grid(gt, (285,) + shape, epsg, s2gt, (3, 240, 300)) == (x0, y0 - 2400.0, x0 + 3000.0, y0, 40, 50)
    assert s2_emit.utm_target_grid(gt, shape, epsg, s2gt, (240, 300), res=20.0) == (x0, y0 - 2400.0, x0 + 3000.0, y0, 120, 150)
    # an S2 extent that is no multiple of the step loses the part cell on the right and at the bottom
    assert s2_emit.utm_target_grid(gt, shape, epsg, s2gt, (245, 309)) == (x0, y0 - 2400.0, x0 + 3060.0, y0, 40, 51)
    # the eps of the reference: 1e-10 cells short of a lattice line still counts as on it, 1e-8 cells does not - right and bottom
    # through the S2 extent (one S2 cell as wide as the extent) ...
    for off, cols in ((-1e-10, 50), (1e-10, 50), (-1e-8, 49), (0.0, 50)):
        wide = (x0, 60.0 * (50 + off), 0.0, y0, 0.0, -60.0 * (40 + off))
        g = s2_emit.utm_target_grid(gt, shape, epsg, wide, (1, 1))
        assert g == (x0, y0 - 60.0 * (cols - 10), x0 + 60.0 * cols, y0, cols - 10, cols), (off, g)
    # ... left and top through the source's own bounds: the S2 origin m cells (+- off) to the left of and above them
    for off, first in ((-1e-10, 7), (1e-10, 7), (1e-8, 8), (0.0, 7)):
        ox, oy = L - 60.0 * (7 + off), T + 60.0 * (7 + off)
        g = s2_emit.utm_target_grid(gt, shape, epsg, (ox, 60.0, 0.0, oy, 0.0, -60.0), (100, 100))
        assert g[:2] + g[2:4] == (ox + 60.0 * first, oy - 6000.0, ox + 6000.0, oy - 60.0 * first) and g[4:] == (100 - first, 100 - first), (off, g)
    # the source inside S2: the largest lattice box inside the corners' bounding box
    big = (60.0 * math.floor(L / 60.0) - 60000.0, 60.0, 0.0, 60.0 * math.ceil(T / 60.0) + 60000.0, 0.0, -60.0)
    left, bottom, right, top, rows, cols = s2_emit.utm_target_grid(gt, shape, epsg, big, (4000, 5000))
    assert L <= left < L + 60 and R - 60 < right <= R and B <= bottom < B + 60 and T - 60 < top <= T
    assert (left - big[0]) % 60.0 == 0 and (big[3] - top) % 60.0 == 0 and (rows, cols) == (round((top - bottom) / 60), round((right - left) / 60))
    assert 1200 < rows < 1900 and 1200 < cols < 2300
    # touching extents and disjoint ones: no overlap; an overlap thinner than a cell: the snapped extent is empty
    for s2gt_bad in ((R, 60.0, 0.0, T, 0.0, -60.0), (L - 6000.0, 60.0, 0.0, T, 0.0, -60.0), (L, 60.0, 0.0, B, 0.0, -60.0), (R + 1e5, 60.0, 0.0, T, 0.0, -60.0)):
        with pytest.raises(ValueError, match="no overlap"):
            s2_emit.utm_target_grid(gt, shape, epsg, s2gt_bad, (100, 100))
    with pytest.raises(ValueError, match="empty"):
        s2_emit.utm_target_grid(gt, shape, epsg, (R - 30.0, 60.0, 0.0, T, 0.0, -60.0), (100, 100))
    # the southern hemisphere: false northing 1e7
    gts, epsgs = (18.2, 0.000542, 0.0, -33.1, 0.0, -0.000542), 32734
    Ls, Bs, Rs, Ts = _src_bounds(gts, shape, epsgs)
    assert 6.1e6 < Bs < Ts < 6.4e6
    s2s = (60.0 * math.floor(Ls / 60.0) - 600.0, 60.0, 0.0, 60.0 * math.ceil(Ts / 60.0) + 600.0, 0.0, -60.0)
    left, bottom, right, top, rows, cols = s2_emit.utm_target_grid(gts, shape, epsgs, s2s, (5000, 5000))
    assert Ls <= left < Ls + 60 and Rs - 60 < right <= Rs and Bs <= bottom < Bs + 60 and Ts - 60 < top <= Ts and rows > 1000 and cols > 1000


# ---- the series and the fixture --------------------------------------------------------------------------------------------------------
def test_series_facts_and_fixture_against_mpmath():
    """Needs mpmath; without it the committed fixture stands alone (the GPU tests never import mpmath)."""
    if importlib.util.find_spec("mpmath") is None:
        return
    gen = _gen()
    mp = gen._mp()
    # fact 1: on the central meridian the northing is k0 times the quadrature of the meridian arc
    for lat in (0.5, 10.0, 33.0, 45.0, 60.0, 75.0, 84.0):
        E, N = gen.forward(lat, -117.0, -117.0, 0)
        assert abs(E - gen.FE) < mp.mpf("1e-30") and abs(N - mp.mpf(gen.K0) * gen.meridian_arc(lat)) < mp.mpf("1e-12"), lat
    # fact 2: inverse(forward) is the identity, to the truncation of the series (n^7 ~ 4e-20 rad)
    for lat, lam in ((0.0, 0.0), (0.0, 3.0), (33.0, -2.5), (-45.0, 4.0), (70.0, 3.5), (84.0, -4.0), (-80.0, 1.0)):
        fn = 0 if lat >= 0 else 10 ** 7
        la, lo = gen.inverse(*gen.forward(lat, 21.0 + lam, 21.0, fn), 21.0, fn)
        assert abs(la - lat) < mp.mpf("1e-16") and abs(lo - 21.0 - lam) < mp.mpf("1e-16"), (lat, lam, la, lo)
    # the committed fixture is what the generator gives
    fresh, g = gen.generate(), rc.fixture()
    assert sorted(fresh) == sorted(g)
    for key in g:
        assert np.array_equal(fresh[key], g[key]), key


def test_fixture_covers_what_it_is_for():
    g = rc.fixture()
    n = len(g["E"])
    assert 380 <= n <= 420 and len(rc.fixture_groups()) == 8
    assert set(np.unique(g["FN"])) == {0.0, 1e7} and g["E"].min() <= 1e5 and g["E"].max() >= 9e5 and (g["E"] == 1e5).any() and (g["E"] == 9e5).any() and g["N"].max() >= 9.3e6
    lam = g["lon"] - g["lon0"]
    assert lam.min() <= -4.0 and lam.max() >= 4.0 and (lam == 0.0).sum() >= 30 and (g["lat"] == 0.0).sum() >= 30
    assert g["lat"].min() < -75.0 and g["lat"].max() > 83.0
    # the forward direction: the NumPy restatement against the fixture, to 1e-8 m (ulp(1e7 m) = 1.9e-9 m, a few dozen roundings)
    for lon0, fn, idx in rc.fixture_groups():
        p = (lon0, rc.WGS84[0], rc.WGS84[1], fn, rc.WGS84[2], rc.WGS84[3])
        E, N = s2_emit.tm_forward(g["lon"][idx], g["lat"][idx], p)
        assert np.abs(E - g["fwd_E"][idx]).max() <= 1e-8 and np.abs(N - g["fwd_N"][idx]).max() <= 3e-8
        assert np.abs(g["fwd_E"][idx] - g["E"][idx]).max() <= 1e-8 and np.abs(g["fwd_N"][idx] - g["N"][idx]).max() <= 3e-8


def test_coordinate_bar_host_twin():
    """hsr_reproject_coords_host and the NumPy restatement against the fixture: every point within the coordinate bar."""
    lib, g = nat.load(), rc.fixture()
    bar = rc.coord_bar(rc.EMIT_CELL)
    assert 1.3e-8 < bar < 1.4e-8
    worst = worst_np = 0.0
    out = (C.c_double * 2)()
    for i in range(len(g["E"])):
        args, (g0, g3) = rc.point_call(g["E"][i], g["N"][i], g["lon0"][i], g["FN"][i])
        assert lib.hsr_reproject_coords_host(*args, out) == 0, lib.hsr_last_error()
        want_sx, want_sy = (g["lon"][i] - g0) / rc.EMIT_CELL - 0.5, (g["lat"][i] - g3) / -rc.EMIT_CELL - 0.5
        worst = max(worst, abs(out[0] - want_sy), abs(out[1] - want_sx))
        p = (g["lon0"][i], rc.WGS84[0], rc.WGS84[1], g["FN"][i], rc.WGS84[2], rc.WGS84[3])
        lon, lat = s2_emit.tm_inverse(g["E"][i], g["N"][i], p)
        worst_np = max(worst_np, abs((lon - g0) / rc.EMIT_CELL - 0.5 - want_sx), abs((lat - g3) / -rc.EMIT_CELL - 0.5 - want_sy))
    print(f"coordinate error, source pixels: host twin {worst:.3g}, NumPy {worst_np:.3g}, bar {bar:.3g}")
    assert worst <= bar and worst_np <= bar
    # a whole grid through the Python wrapper: the twin against the NumPy restatement, cell by cell (each within the bar of the truth)
    gt, epsg = (-118.0, rc.EMIT_CELL, 0.0, 34.9, 0.0, -rc.EMIT_CELL), 32611
    grid = (431040.0, 3800040.0, 431040.0 + 60.0 * 23, 3800040.0 + 60.0 * 17, 17, 23)
    field = eng.reproject_coords_host(reproject._grid_cells(grid), s2_emit.utm_params(epsg), (gt[0], gt[1], gt[3], gt[5]))
    E, N = np.meshgrid(grid[0] + (np.arange(23) + 0.5) * 60.0, grid[3] - (np.arange(17) + 0.5) * 60.0)
    lon, lat = s2_emit.tm_inverse(E, N, s2_emit.utm_params(epsg))
    assert field.shape == (17, 23, 2)
    assert np.abs(field[..., 1] - ((lon - gt[0]) / gt[1] - 0.5)).max() <= 2 * bar and np.abs(field[..., 0] - ((lat - gt[3]) / gt[5] - 0.5)).max() <= 2 * bar
    assert 0 < field[..., 0].min() < field[..., 0].max() < 1800 and 0 < field[..., 1].min() < field[..., 1].max() < 2200


# ---- what the rows claim ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.WARP_ROWS))
def test_warp_row_claims(name):
    r, c = rc.WARP_ROWS[name], rc.warp_case(name)
    assert rc.valid(r) and (r["hs"], r["ws"]) != (r["h"], r["w"])
    assert c["ref"].shape == (r["bands"], r["h"], r["w"]) and c["ref"].dtype == np.float32
    inst, ntiles = rc.warp_instance(r["mf"], r["rule"]), -(-r["h"] // rc.TILE_H) * -(-r["w"] // rc.TILE_W)
    assert ("DIRECT" in inst) == ("direct" in name) and rc.RULE_NAMES[r["rule"]] in inst
    assert c["fits"] + c["falls"] <= ntiles and c["counts"][0] == (~c["inside"]).sum() and c["counts"][1] == c["filled"].sum()
    fill = np.float32(r["fill"])
    is_fill = np.isnan(c["ref"]) if np.isnan(fill) else c["ref"] == fill
    assert is_fill[:, ~c["inside"]].all() and is_fill[c["filled"]].all()
    if r["rule"] == rc.STRICT:
        assert np.array_equal(c["filled"], c["bad"])
    else:
        assert not (c["filled"] & ~c["bad"]).any()
    if name in rc.FALLBACK_ROWS:
        assert "LDS" in inst and c["falls"] >= 1 and c["status"] == 1
    if name in rc.FITTING_ROWS:
        assert "LDS" in inst and c["falls"] == 0 and c["fits"] == ntiles and c["status"] == 0
    if name.startswith("size-"):
        assert c["inside"].all() and c["fits"] == ntiles
    if name == "bands-285":
        assert r["bands"] == 285 and (r["h"], r["w"]) == (20, 12)
    if name == "identity":                                             # a copy, bits: and invalid neighbours under zero weights
        assert np.array_equal(c["ref"][~is_fill].view(np.uint32), c["src"][:, :r["h"], :r["w"]][~is_fill].view(np.uint32))
        assert c["zero_weight_invalid"].sum() > 100 and np.array_equal(c["bad"], ~rc.src_valid(c["src"][:, :r["h"], :r["w"]], r["nodata"]))
    if name.startswith("int-shift"):                                   # a shifted copy under both rules; t = 0: only the pixel itself counts
        cut = c["src"][:, 3:3 + r["h"], 5:5 + r["w"]]
        assert np.array_equal(c["bad"], ~rc.src_valid(cut, r["nodata"])) and c["zero_weight_invalid"].sum() > 1000
        assert np.array_equal(c["ref"][~c["bad"]].view(np.uint32), cut[~c["bad"]].view(np.uint32)) and np.array_equal(c["filled"], c["bad"])
    if name == "half-shift":
        assert not c["zero_weight_invalid"].any() and c["bad"].sum() > 4 * c["filled"].sum() > 0
    if name in ("minify-5", "minify-5-direct", "bound-3.6-lds", "bound-3.7-direct"):
        fw, fh = max(rc.tile_footprints(c["coords"], r["hs"], r["ws"]))
        assert fw > 2.5 * rc.TILE_W
    if name == "bound-3.6-lds":
        assert rc.boxes(3.6)[0] * rc.boxes(3.6)[1] * 4 <= rc.LDS_LIMIT < rc.boxes(3.7)[0] * rc.boxes(3.7)[1] * 4
    if name.startswith("special"):
        sy, sx = c["coords"][..., 0], c["coords"][..., 1]
        for v in rc.SPECIALS:
            assert any(np.array_equal(np.asarray(v).view(np.uint64), s.view(np.uint64)) for s in np.concatenate([sy.ravel(), sx.ravel()])), v
        assert c["counts"][0] >= 2 * len(rc.SPECIALS) - 2               # -0.0 is inside
    if name.startswith("edges"):
        sy, sx = c["coords"][..., 0], c["coords"][..., 1]
        for v, n in ((0.0, r["hs"]), (-1e-12, r["hs"]), (r["hs"] - 1.0, r["hs"]), (r["hs"] - 1.0 + 1e-12, r["hs"])):
            assert (sy == v).any() and ((sy == v) & (sx == 0.0)).any()
        assert c["inside"][(sy == 0.0) & (sx == r["ws"] - 1.0)].all() and not c["inside"][sy == -1e-12].any()
        assert not c["inside"][sx == r["ws"] - 1.0 + 1e-12].any() and c["inside"].sum() * 25 == 9 * c["inside"].size
    if name == "half-outside":
        tiles = [c["inside"][:rc.TILE_H, :rc.TILE_W], c["inside"][:rc.TILE_H, rc.TILE_W:]]
        assert 0 < tiles[0].sum() < tiles[0].size and tiles[1].all()
    if name == "wholly-outside":
        assert not c["inside"].any() and is_fill.all() and c["fits"] == c["falls"] == 0
    if name.startswith("one-invalid"):
        assert (~rc.src_valid(c["src"], r["nodata"])).sum() == 1 and c["bad"].sum() == 16
        assert c["filled"].sum() == (16 if r["rule"] == rc.STRICT else 1)
    if name == "nodata-is-a-value":
        assert (c["src"] == -9999.0).sum() > 5 and not c["bad"].any() and (c["ref"] < -100.0).any()
    if name == "nan-and-nodata":
        assert np.isnan(c["src"]).any() and (c["src"] == -9999.0).any() and np.isinf(c["src"]).any()
    if name == "nearest-invalid":
        assert c["filled"].sum() > 100 and (c["bad"] & ~c["filled"]).sum() > 100
    if name.startswith("all-invalid"):
        assert not rc.src_valid(c["src"], -9999.0).any() and is_fill.all() and c["counts"][1] == c["ref"].size
    if name == "fill-nan":
        assert np.isnan(fill) and is_fill.any() and not is_fill.all()


def test_renorm_is_strict_where_every_tap_is_valid():
    """The two rules on one case: bit-equal where no consulted tap is invalid, and RENORM's quotient lies between the valid taps."""
    r = rc.WARP_ROWS["affine"]
    c = rc.warp_case("affine")
    strict, counts, info = rc.warp_ref(c["src"], c["coords"], r["nodata"], r["fill"], rc.STRICT)
    clean = c["inside"][None] & ~c["bad"]
    assert np.array_equal(strict[clean].view(np.uint32), c["ref"][clean].view(np.uint32)) and np.array_equal(info["bad"], c["bad"])
    partial = c["bad"] & ~c["filled"]
    ok = c["src"][rc.src_valid(c["src"], r["nodata"])]
    assert partial.sum() > 1000 and (c["ref"][partial] > ok.min() - 1.0).all() and (c["ref"][partial] < ok.max() + 1.0).all()
    assert counts[1] == c["bad"].sum() > c["counts"][1]


# ---- the sweep's generator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", rc.SEEDS)
def test_sweep_generator(seed):
    rows = [rc.draw(seed, i) for i in range(rc.ROWS_PER_SEED)]
    assert all(rc.valid(r) for r in rows)
    again = rc.draw(seed, 7)
    assert again == rows[7] or (np.isnan(again["fill"]) and np.isnan(rows[7]["fill"]))       # rebuilt without drawing the others
    cases = [rc.warp_case_of(r) for r in rows]
    skipped = [i for i, (r, c) in enumerate(zip(rows, cases)) if not rc.admitted(r, c)]
    assert len(skipped) <= rc.MAX_SKIPPED * len(rows), skipped
    assert {rc.warp_instance(r["mf"], r["rule"]) for r in rows} == set(rc.all_instances()[1:])
    assert any(c["status"] for c in cases) and any(c["falls"] for r, c in zip(rows, cases) if "LDS" in rc.warp_instance(r["mf"], r["rule"]))
