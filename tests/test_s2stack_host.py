"""The S2 stack family on the host side: the NumPy statement of tests/s2stack_cases.py against an independent reference
(scipy.ndimage.map_coordinates) on clean planes; hsr_s2_stack_host - the tile code of the kernel compiled for the CPU - against the
statement on every row and on the sweep; every refusal with its text and without a record; include/hsr_s2stack.h against
nat.S2STACK_SIGNATURES, the library's exports and the Python constants; s2_crop_window against rows worked by hand from
s2_utils.py:649-696; the public surface, S2_STACK_BANDS and the 9-band rule.

rasterio is not installed here, so no fixture can be frozen from crop_s2_stack_to_te or from GDAL's warp: the window rows below are
worked by hand from the reference's lines, and GDAL's bits are not claimed."""
import ctypes as C
import inspect
import os
import re
import warnings

import numpy as np
import pytest

import s2_emit
import s2stack_cases as sc
from conftest import ROOT
from s2_emit import _native as nat
from s2_emit import s2stack
from s2_emit.scenes import Window

LAUNCH_PATH = ("hsr_s2_stack", "hsr_s2_expand_u8")
HOST_ONLY = ("hsr_s2_stack_host", "hsr_s2stack_last_launch", "hsr_s2stack_instance_count", "hsr_s2stack_instance_name")
INVALID, UNSUPPORTED = 1, 2
OTHER_COUNTS = (32, 20, 31, 12, 6, 20, 8, 5, 8)            # aux, scene, k4, pairs, ortho, color, coreg, reproject, scl


def _header():
    text = open(os.path.join(ROOT, "include", "hsr_s2stack.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    return text, code, comments


def _other_counts(lib):
    return (lib.hsr_aux_instance_count(), lib.hsr_scene_instance_count(), lib.hsr_k4_instance_count(), lib.hsr_pairs_instance_count(),
            lib.hsr_ortho_instance_count(), lib.hsr_color_instance_count(), lib.hsr_coreg_instance_count(),
            lib.hsr_reproject_instance_count(), lib.hsr_scl_instance_count())


# ---- the statement against an independent reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 45), (36, 44), (1, 1), (1, 9), (8, 1)])
def test_statement_equals_map_coordinates_on_clean_planes(shape):
    """Full grids, edges included: order-1 interpolation at ((Y + 0.5) / 2 - 0.5, (X + 0.5) / 2 - 0.5) with the edge clamp equals
    N / 16 in float64 with no tolerance - both are exact: every value is a multiple of 1 / 16 below 2^20."""
    ndimage = pytest.importorskip("scipy.ndimage")
    H, W = shape
    plane = np.random.default_rng(H * W).integers(0, 65536, size=shape).astype(np.uint16)
    for H10, W10 in ((2 * H, 2 * W), (2 * H - 1, 2 * W - 1)):
        if H10 < 1 or W10 < 1:
            continue
        Y, X = np.arange(H10, dtype=np.int64), np.arange(W10, dtype=np.int64)
        N = sum(wt * plane.astype(np.int64)[i][:, j] for i, j, wt in sc.taps_of(2, sc.BILINEAR, Y, X, H, W))
        yy, xx = np.meshgrid((Y + 0.5) / 2 - 0.5, (X + 0.5) / 2 - 0.5, indexing="ij")
        want = ndimage.map_coordinates(plane.astype(np.float64), [yy, xx], order=1, mode="nearest")
        assert np.array_equal(N / 16.0, want)
        out, invalid = sc.band_ref(plane, 2, sc.BILINEAR, 0, (0, 0, H10, W10), 0, 0, sc.STRICT, sc.F32, 0, np.nan, 1.0)
        assert invalid == 0 and np.array_equal(out, want.astype(np.float32))
        near, _ = sc.band_ref(plane, 2, sc.NEAREST, 0, (0, 0, H10, W10), 0, 0, sc.STRICT, sc.U16, 65535, np.nan, 1.0)
        assert np.array_equal(near, np.repeat(np.repeat(plane, 2, 0), 2, 1)[:H10, :W10].clip(0, 65534))


def test_statement_by_hand():
    """Four outputs of a 2 x 2 plane worked by hand, both rules, and the rounding and the clamp of the uint16 value."""
    p = np.array([[100, 200], [0, 401]], dtype=np.uint16)               # 0 is nodata
    kw = dict(window=(0, 0, 4, 4), has_nodata=1, nodata_in=0, nodata_out=0, fill=-1.0, quant=1.0)
    s, _ = sc.band_ref(p, 2, sc.BILINEAR, 0, rule=sc.STRICT, dtype=sc.F32, **kw)
    r, n = sc.band_ref(p, 2, sc.BILINEAR, 0, rule=sc.RENORM, dtype=sc.F32, **kw)
    # (Y, X) = (1, 1): taps 100 x9, 200 x3, 0 x3, 401 x1 - the weight-9 tap is valid
    assert s[1, 1] == -1.0 and r[1, 1] == np.float32((900 + 600 + 401) / 13)
    # (2, 0): rows 0 (weight 1) and 1 (weight 3), column -1 clamped onto column 0: the weight-9 tap is the nodata pixel
    assert s[2, 0] == -1.0 and r[2, 0] == -1.0
    # (0, 3): both rows clamp onto row 0 and both columns onto column 1: four taps of 200
    assert s[0, 3] == 200.0 and r[0, 3] == 200.0
    # the nodata footprint under RENORM is exactly the pixel's own four outputs
    assert n == 4 and np.array_equal(r == -1.0, np.repeat(np.repeat(p == 0, 2, 0), 2, 1))
    u, _ = sc.band_ref(p, 2, sc.BILINEAR, 0, rule=sc.RENORM, dtype=sc.U16, **kw)
    assert u[1, 1] == (2 * 1901 + 13) // 26 == 146 and u[2, 0] == 0                 # 146.23 -> 146
    p = np.array([[1, 2]], dtype=np.uint16)
    kw.update(window=(0, 0, 1, 4), has_nodata=0)
    u, _ = sc.band_ref(p, 2, sc.BILINEAR, 0, rule=sc.STRICT, dtype=sc.U16, **kw)
    assert u.tolist() == [[1, 1, 2, 2]]                                             # 1, 1.25, 1.75, 2: half up would show at .5
    p = np.array([[1, 3]], dtype=np.uint16)
    u, _ = sc.band_ref(p, 2, sc.BILINEAR, 0, rule=sc.STRICT, dtype=sc.U16, **kw)
    assert u.tolist() == [[1, 2, 3, 3]]                                             # 1.5 -> 2, 2.5 -> 3: round half up
    u, _ = sc.band_ref(p, 2, sc.BILINEAR, -1000, rule=sc.STRICT, dtype=sc.U16, **kw)
    assert u.tolist() == [[1, 1, 1, 1]]                                             # clamped off nodata_out = 0
    kw["nodata_out"] = 65535
    u, _ = sc.band_ref(p, 2, sc.BILINEAR, 65535, rule=sc.STRICT, dtype=sc.U16, **kw)
    assert u.tolist() == [[65534] * 4]


# ---- the host twin against the statement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.ALL_ROWS))
def test_stack_host_equals_the_statement(name):
    lib, r = nat.load(), sc.ALL_ROWS[name]
    srcs, nout, dst_off, dtype = sc.layout(name)
    holders, ptrs = [], []
    for flat, off in srcs:                                  # a plane `off` bytes past a 16-byte boundary
        raw = np.full(flat.nbytes + off + 32, sc.SENT, dtype=np.uint8)
        base = (-raw.ctypes.data) % 16 + off
        raw[base: base + flat.nbytes] = flat.view(np.uint8)
        holders.append((raw, base, flat))
        ptrs.append(raw.ctypes.data + base)
    item = np.dtype(dtype).itemsize
    oraw = np.full(nout * item + dst_off + 32, sc.SENT, dtype=np.uint8)
    obase = (-oraw.ctypes.data) % 16 + dst_off
    invalid = np.full(len(r["bands"]), -77, dtype=np.int64)
    table = sc.band_table(nat.S2Band, name, ptrs)
    args = sc.stack_args(name, table, C.c_void_p(oraw.ctypes.data + obase), C.c_void_p(invalid.ctypes.data) if r["count"] else None)
    assert lib.hsr_s2_stack_host(*args) == 0, lib.hsr_last_error()
    assert (oraw[:obase] == sc.SENT).all() and (oraw[obase + nout * item:] == sc.SENT).all()
    sc.check_output(name, oraw[obase: obase + nout * item].view(dtype), invalid if r["count"] else None)
    assert r["count"] or (invalid == -77).all()
    for raw, base, flat in holders:
        assert np.array_equal(raw[base: base + flat.nbytes], flat.view(np.uint8))


def test_rows_cover_what_they_are_for():
    rows = sc.ROWS
    assert nat.HSR_S2_TILE_H == sc.TILE_H and nat.HSR_S2_TILE_W == sc.TILE_W
    assert sc.GRIDS[0][0] % 2 and sc.GRIDS[0][1] % 2 and not sc.GRIDS[1][0] % 2 and not sc.GRIDS[1][1] % 2
    assert sc.GRIDS[2] == (sc.TILE_H + 1, sc.TILE_W + 3)
    for grid in sc.GRIDS:
        wins = sc.windows_of(*grid)
        assert {(r0 & 1, c0 & 1) for r0, c0, _, _ in wins.values()} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert all(r0 >= 0 and c0 >= 0 and h >= 1 and w >= 1 and r0 + h <= grid[0] and c0 + w <= grid[1] for r0, c0, h, w in wins.values())
        assert sum(1 for w in wins.values() if w[2:] == (1, 1)) == 4
    assert {(r["dtype"], r["rule"], m) for r in rows.values() for u, m, _ in r["bands"] if u == 2} == {(d, ru, m) for d in (0, 1) for ru in (0, 1) for m in (0, 1)}
    assert {len(r["bands"]) for r in rows.values()} >= {1, 9, 10, 16}
    assert {sc.stack_instance(r["dtype"], r["rule"]) for r in rows.values()} == set(sc.all_instances()[:4])
    assert {r["nodata_out"] for r in rows.values()} == {0, 65535} and any(r["fill"] == -9999.0 for r in rows.values())
    for name, r in rows.items():
        rs, ors, obs = sc.strides_of(name)
        _, _, h, w = r["window"]
        assert ors >= w and obs >= (h - 1) * ors + w and all(s >= p.shape[1] for s, p in zip(rs, sc.case(name)))
        out, invalid = sc.ref(name)
        if name.startswith("nodata-none") or name.startswith("value-"):
            assert not invalid.any()
        if name.startswith("nodata-all"):
            assert (invalid == h * w).all()
        if name.startswith("nodata-one") and "renorm" in name:
            assert invalid.tolist() == [4]                   # exactly the pixel's own four outputs
        if name.startswith("nodata-one") and "strict" in name:
            assert invalid.tolist() == [16]                  # eroded by one output pixel on every side
        if name.startswith("nodata-block") and "strict" in name:
            assert invalid.tolist() == [36]
        if name.startswith("nodata-clamped-0-0") and "strict" in name:
            assert invalid.tolist() == [9]
        if name.startswith("offset-0-u16"):
            assert out.min() == 1 and (out == 1).sum() > out.size // 4        # the clamp at the low end, never nodata_out
        if name.startswith("offset-65535-u16"):
            assert out.min() == 0
        if name.startswith("offset-up-u16"):
            assert out.max() == 65534 and (out == 65534).sum() > out.size // 4
    assert any(r["rs_pad"] == 5 and r["ors_pad"] == 3 and r["obs_pad"] == 7 for r in rows.values())
    assert len(sc.SWEEP_ROWS) >= 20 and {r["dtype"] for r in sc.SWEEP_ROWS.values()} == {0, 1}
    for name, r in sc.EXPAND_ROWS.items():
        p, rs, ors, want = sc.expand_case(name)
        assert want.shape == r["window"][2:] and rs >= p.shape[1] and ors >= r["window"][3]


# ---- refusals and the record, without a device ------------------------------------------------------------------------------------------
def test_c_abi_refusals_need_no_device():
    lib = nat.load()
    null, st = C.c_void_p(0), C.c_void_p(0)
    P, Q = 1 << 20, 1 << 30
    lib.hsr_s2stack_last_launch(None, 0)

    def refused(word, fn, *args, code=INVALID):
        rc_ = fn(*args)
        text = lib.hsr_last_error().decode()
        assert rc_ == code and word in text and fn.__name__ in text, (fn.__name__, rc_, text, word)

    def stack(fn, nbands=2, H10=40, W10=50, win=(2, 3, 30, 40), rule=0, dtype=0, out=Q, obs=None, ors=40, nodata_out=0, quant=10000.0,
              table="ok", **band):
        t = (nat.S2Band * 16)()
        for b in range(16):
            up = 1 + b % 2
            t[b].plane_dev, t[b].rs, t[b].H, t[b].W, t[b].up, t[b].method = P + b * (1 << 16), 50, -(-H10 // up), -(-W10 // up), up, b % 2
        for key, val in band.items():                       # what is wrong with band 1
            setattr(t[1], key, val)
        args = (None if table is None else t, nbands, H10, W10) + tuple(win) + (1, 0, rule, dtype, C.c_void_p(out),
                                                                                29 * ors + win[3] if obs is None else obs, ors, nodata_out,
                                                                                C.c_float(np.nan), C.c_double(quant), null)
        return (fn,) + args + ((st,) if fn is lib.hsr_s2_stack else ())

    for fn in (lib.hsr_s2_stack, lib.hsr_s2_stack_host):
        refused("NULL", *stack(fn, table=None))
        refused("NULL", *stack(fn, out=0))
        refused("NULL", *stack(fn, plane_dev=0))
        for n in (0, -1, 17):
            refused("nbands", *stack(fn, nbands=n))
        for kw in (dict(H10=0), dict(W10=-3), dict(win=(2, 3, 0, 40)), dict(win=(2, 3, 30, -1))):
            refused("extent", *stack(fn, **kw))
        for win in ((-1, 3, 30, 40), (2, -1, 30, 40), (11, 3, 30, 40), (2, 11, 30, 40), (2 ** 31 - 1, 0, 30, 40)):
            refused("leaves", *stack(fn, win=win))
        for kw in (dict(H=19), dict(W=26), dict(H=40, W=50)):
            refused("not the ceil", *stack(fn, **kw))
        refused("row stride", *stack(fn, rs=24))
        refused("strides", *stack(fn, ors=39))
        refused("strides", *stack(fn, obs=29 * 40 + 39))
        for m in (-1, 2):
            refused("method", *stack(fn, method=m))
        for ru in (-1, 2):
            refused("rule", *stack(fn, rule=ru))
        for d in (-1, 2):
            refused("out_dtype", *stack(fn, dtype=d))
        for nd in (1, -1, 65534, 65536):
            refused("nodata_out", *stack(fn, nodata_out=nd))
        for q in (0.0, -1.0, float("inf"), float("nan")):
            refused("quantification", *stack(fn, quant=q))
        plane1 = P + (1 << 16)
        for out in (plane1, plane1 + 2, plane1 + (19 * 50 + 25) * 2 - 2, plane1 - 2 * (29 * 40 + 40) * 2 + 2):
            refused("overlaps", *stack(fn, out=out))
        for up in (0, 3, 6, -2):
            refused("up=", *stack(fn, up=up), code=UNSUPPORTED)

    def expand(plane=P, H=20, W=25, rs=25, up=2, H10=40, W10=50, win=(2, 3, 30, 40), out=Q, ors=40):
        return (lib.hsr_s2_expand_u8, C.c_void_p(plane), H, W, rs, up, H10, W10) + tuple(win) + (C.c_void_p(out), ors, st)

    refused("NULL", *expand(plane=0))
    refused("NULL", *expand(out=0))
    for kw in (dict(H10=0), dict(win=(2, 3, 0, 40))):
        refused("extent", *expand(**kw))
    for win in ((-1, 3, 30, 40), (11, 3, 30, 40), (2, 11, 30, 40)):
        refused("leaves", *expand(win=win))
    for kw in (dict(H=19), dict(W=24), dict(up=1)):
        refused("not the ceil", *expand(**kw))
    refused("row stride", *expand(rs=24))
    refused("row stride", *expand(ors=39))
    for out in (P, P + 19 * 25 + 24, P - 29 * 40 - 39):
        refused("overlaps", *expand(out=out))
    for up in (0, 3):
        refused("up=", *expand(up=up), code=UNSUPPORTED)
    buf = C.create_string_buffer(64)
    assert lib.hsr_s2stack_last_launch(buf, 64) == 0 and buf.value == b""              # refused calls leave no record


def test_instance_table_and_record_contract():
    lib = nat.load()
    n = lib.hsr_s2stack_instance_count()
    table = [lib.hsr_s2stack_instance_name(i).decode() for i in range(n)]
    assert n == 6 == len(set(table)) and table == sc.all_instances()
    for bad in (-1, n):
        assert lib.hsr_s2stack_instance_name(bad) is None
        assert b"hsr_s2stack_instance_name" in lib.hsr_last_error() and str(bad).encode() in lib.hsr_last_error()
    _, _, comments = _header()
    assert "hsr_s2stack_instance_count = 6" in comments and "8 most recent" in comments and "hsr_aux_last_launch" in comments
    buf = C.create_string_buffer(64)
    buf.value = b"junk"
    lib.hsr_s2stack_last_launch(None, 0)
    assert lib.hsr_s2stack_last_launch(buf, 0) == 0 and buf.value == b"junk"
    assert lib.hsr_s2stack_last_launch(buf, 64) == 0 and buf.value == b""
    assert _other_counts(lib) == OTHER_COUNTS               # the other families' tables are what they were


def test_header_signatures_and_exports_agree():
    lib = nat.load()
    text, code, comments = _header()
    declared = sorted(set(re.findall(r"\b(hsr_s2[a-z0-9_]*)\s*\(", code)))
    assert declared == sorted(nat.S2STACK_SIGNATURES) == sorted(LAUNCH_PATH + HOST_ONLY)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/hsr_s2stack.h but not exported"
        sig = nat.S2STACK_SIGNATURES[name]
        assert getattr(lib, name).argtypes == sig[1] and getattr(lib, name).restype == sig[0]
        assert name in comments, f"{name} is not documented"
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        nargs = 0 if proto.strip() == "void" else proto.count(",") + 1
        assert nargs == len(sig[1]), (name, proto)
        if name in LAUNCH_PATH:
            assert proto.split(",")[-1].strip() == "hsr_stream_t stream", name
            at = re.search(r"\nint %s\(" % name, text).start()
            assert ".py:" in text[text.rfind("/*", 0, at):at], f"{name} cites no reference lines"
        else:
            assert "stream" not in proto
    assert '#include "hsr.h"' in code and "HSR_ABI_VERSION" not in code and lib.hsr_abi_version() == 5 == nat.HSR_ABI_VERSION
    others = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("hsr.h", "hsr_color.h", "hsr_coreg.h", "hsr_reproject.h", "hsr_scl.h"))
    for name in declared:                                   # a family of its own: in no other table and no other header
        for tab in (nat.SIGNATURES, nat.COLOR_SIGNATURES, nat.COREG_SIGNATURES, nat.REPROJECT_SIGNATURES, nat.SCL_SIGNATURES):
            assert name not in tab, name
        assert name not in others, name
    for macro, value in (("HSR_S2_MAX_BANDS", sc.MAX_BANDS), ("HSR_S2_NEAREST", sc.NEAREST), ("HSR_S2_BILINEAR", sc.BILINEAR),
                         ("HSR_S2_STRICT", sc.STRICT), ("HSR_S2_RENORM", sc.RENORM), ("HSR_S2_U16", sc.U16), ("HSR_S2_F32", sc.F32),
                         ("HSR_S2_TILE_H", sc.TILE_H), ("HSR_S2_TILE_W", sc.TILE_W)):
        assert re.search(r"#define %s %d\b" % (macro, value), code) and getattr(nat, macro) == value, macro
    fields = re.search(r"typedef struct \{(.*?)\} hsr_s2_band;", code, flags=re.S).group(1)
    assert [f for f in re.findall(r"(\w+)\s*[,;]", fields)] == [n for n, _ in nat.S2Band._fields_] and C.sizeof(nat.S2Band) == 40
    for phrase in ("s2_utils.py:505-614", "s2_utils.py:617-783", "never (y, x)", "weight 9", "round half up", "integer sums", "GDAL's bits",
                   "by value"):
        assert phrase in comments, phrase
    src = open(os.path.join(ROOT, "hyperspectral_super-resolution_amd", "csrc", "Makefile")).read()
    assert "hsr_s2stack.hip" in re.search(r"^SRCS\s*=(.*)$", src, flags=re.M).group(1) and "hsr_s2stack.h" in src.split("HDRS")[1].split("all:")[0]


# ---- s2_crop_window: rows worked by hand from s2_utils.py:649-696 ----------------------------------------------------------------------
GT = (600000.0, 10.0, 0.0, 4200000.0, 0.0, -10.0)             # a 100 x 120 raster: x 600000 .. 601200, y 4199000 .. 4200000
SHAPE = (10, 100, 120)
# te (left, bottom, right, top), snap, cover -> Window(col_off, row_off, width, height)
CROP_ROWS = [
    # on the grid already: columns 10 .. 30, rows 5 .. 25
    ((600100.0, 4199750.0, 600300.0, 4199950.0), True, True, Window(10, 5, 20, 20)),
    # snap half up on both axes: (x - x0) / dx = 10.5 -> 11, 30.5 -> 31; (y0 - y) / dy = 4.5 -> 5 (top), 24.5 -> 25 (bottom)
    ((600105.0, 4199755.0, 600305.0, 4199955.0), True, True, Window(11, 5, 20, 20)),
    # ... and just below the half: 10.4 -> 10, 30.4 -> 30, 4.4 -> 4, 24.4 -> 24
    ((600104.0, 4199756.0, 600304.0, 4199956.0), True, True, Window(10, 4, 20, 20)),
    # no snap, cover: floor(10.4) = 10, ceil(30.4) = 31, floor(4.4) = 4, ceil(24.4) = 25
    ((600104.0, 4199756.0, 600304.0, 4199956.0), False, True, Window(10, 4, 21, 21)),
    # no snap, round: round(10.4) = 10, round(20.0) = 20
    ((600104.0, 4199756.0, 600304.0, 4199956.0), False, False, Window(10, 4, 20, 20)),
    # no snap, round with Python's round-half-even on the offsets: 10.5 -> 10, 4.5 -> 4
    ((600105.0, 4199755.0, 600305.0, 4199955.0), False, False, Window(10, 4, 20, 20)),
    # the 1e-9 of the cover: 1e-10 past a grid line is that grid line
    ((600100.0 + 1e-9, 4199750.0, 600300.0 + 1e-9, 4199950.0), False, True, Window(10, 5, 20, 20)),
    # clipped on the left and at the top, on the right and at the bottom, and on all sides
    ((599900.0, 4199900.0, 600100.0, 4200100.0), True, True, Window(0, 0, 10, 10)),
    ((601100.0, 4198900.0, 601300.0, 4199100.0), True, True, Window(110, 90, 10, 10)),
    ((599000.0, 4198000.0, 602000.0, 4201000.0), True, True, Window(0, 0, 120, 100)),
    ((599900.0, 4199500.0, 600100.0, 4199600.0), True, True, Window(0, 40, 10, 10)),
    ((600500.0, 4199900.0, 600600.0, 4200100.0), True, True, Window(50, 0, 10, 10)),
    # an odd origin: the case fuse_scene_clear's 20 m SCL could not take
    ((600030.0, 4199870.0, 600250.0, 4199970.0), True, True, Window(3, 3, 22, 10)),
]


@pytest.mark.parametrize("te, snap, cover, want", CROP_ROWS)
def test_crop_window_rows_worked_by_hand(te, snap, cover, want):
    win, gt, info = s2_emit.s2_crop_window(te, GT, SHAPE, snap=snap, cover=cover)
    assert win == want and isinstance(win, Window)
    assert gt == (GT[0] + 10.0 * want.col_off, 10.0, 0.0, GT[3] - 10.0 * want.row_off, 0.0, -10.0)
    assert info["window"] == dict(col_off=want.col_off, row_off=want.row_off, width=want.width, height=want.height)
    assert (info["snapped_te"] is not None) == snap
    if snap:
        s = info["snapped_te"]
        assert all(float(v).is_integer() and v % 10.0 == 0.0 for v in s.values()) and info["te"] == s


def test_crop_window_errors():
    with pytest.raises(ValueError, match="Invalid TE after snapping"):      # both edges snap onto one grid line
        s2_emit.s2_crop_window((600101.0, 4199750.0, 600104.0, 4199950.0), GT, SHAPE)
    with pytest.raises(ValueError, match="Invalid TE after snapping"):
        s2_emit.s2_crop_window((600100.0, 4199751.0, 600300.0, 4199754.0), GT, SHAPE)
    for te in ((598000.0, 4199750.0, 599000.0, 4199950.0), (600100.0, 4201000.0, 600300.0, 4202000.0), (601200.0, 4199000.0, 601300.0, 4199100.0)):
        with pytest.raises(ValueError, match="Overlap window is empty"):
            s2_emit.s2_crop_window(te, GT, SHAPE)
    with pytest.raises(ValueError, match="Overlap window is empty"):        # without the snap a sliver rounds to nothing
        s2_emit.s2_crop_window((600101.0, 4199750.0, 600104.0, 4199950.0), GT, SHAPE, snap=False, cover=False)
    with pytest.raises(ValueError, match="north-up"):
        s2_emit.s2_crop_window((0, 0, 1, 1), (0.0, 10.0, 1.0, 0.0, 0.0, -10.0), SHAPE)
    src = inspect.getsource(s2stack.s2_crop_window)
    assert "math.floor(((x - x0) / dx) + 0.5)" in src and "1e-9" in src and "round(" in src


# ---- the public surface -------------------------------------------------------------------------------------------------------------------
def test_public_surface_and_defaults():
    new = ["assemble_s2_stack", "s2_crop_window", "S2StackOutput"]
    allv = s2_emit.__all__
    at = allv.index(new[0])
    assert allv[at:at + 3] == new and allv[at + 3] == "find_valid_paired_tiles" and all(callable(getattr(s2_emit, n)) for n in new)
    assert "S2_STACK_BANDS" not in allv and len(set(allv)) == len(allv)
    assert allv[:13] == s2_emit._REFERENCE_SURFACE and allv[-5:] == ["apply_glt", "ortho_scene", "glt_from_xy", "quality_mask", "OrthoOutput"]
    assert allv[allv.index("SceneOutput") + 1] == "fuse_scene_clear" and allv[allv.index("ClearSceneOutput") + 1] == "coregister_scene"
    assert allv[allv.index("CoregOutput") + 1] == "reproject_scene"
    # s2_utils.py:567-586, value for value
    assert s2_emit.S2_STACK_BANDS == (("B02_blue", "blue", "nearest"), ("B03_green", "green", "nearest"), ("B04_red", "red", "nearest"),
                                      ("B08_nir", "nir", "nearest"), ("B05_rededge1", "rededge1", "bilinear"),
                                      ("B06_rededge2", "rededge2", "bilinear"), ("B07_rededge3", "rededge3", "bilinear"),
                                      ("B8A_nir08", "nir08", "bilinear"), ("B11_swir16", "swir16", "bilinear"),
                                      ("B12_swir22", "swir22", "bilinear"))
    assert s2_emit.S2StackOutput._fields == ("stack", "names", "window", "scl", "invalid")
    d = [(k, v.default) for k, v in inspect.signature(s2_emit.assemble_s2_stack).parameters.items()]
    assert d[0] == ("bands", inspect.Parameter.empty) and d[1:4] == [("window", None), ("out_dtype", "uint16"), ("rule", "strict")]
    assert d[4:7] == [("nodata", 0), ("add_offset", 0), ("quantification", 10000.0)] and d[7][0] == "fill" and np.isnan(d[7][1])
    assert d[8:] == [("nodata_out", 0), ("scl", None), ("out", None), ("count_invalid", False)]
    params = list(inspect.signature(s2_emit.assemble_s2_stack).parameters.values())
    assert all(p.kind is p.KEYWORD_ONLY for p in params[1:])
    d = [(k, v.default) for k, v in inspect.signature(s2_emit.s2_crop_window).parameters.items()]
    assert d[3:] == [("snap", True), ("cover", True)] and [k for k, _ in d[:3]] == ["te", "geotransform", "shape"]
    for w in ("s2_utils.py", "NOT reproduced", "GDAL's bits", "nothing is reprojected"):
        assert w in s2stack.__doc__, w


def _bands(H=18, W=22, nir08="20m", drop=()):
    full, half = np.ones((H, W), np.uint16), np.ones(((H + 1) // 2, (W + 1) // 2), np.uint16)
    b = {k: full for k in ("blue", "green", "red", "nir")}
    b.update({k: half for k in ("rededge1", "rededge2", "rededge3", "swir16", "swir22")})
    if nir08:
        b["nir08"] = half if nir08 == "20m" else full
    return {k: v for k, v in b.items() if k not in drop}


def test_plan_the_nine_band_rule_and_argument_checks():
    """Everything assemble_s2_stack decides before it touches a device (s2stack._stack_plan)."""
    plan = lambda b, **kw: s2stack._stack_plan(b, kw.get("window"), kw.get("out_dtype", "uint16"), kw.get("rule", "strict"),  # noqa: E731
                                               kw.get("nodata", 0), kw.get("add_offset", 0), kw.get("quantification", 10000.0),
                                               kw.get("nodata_out", 0))
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # ten bands: no warning
        rows, grid, win, dt, rl, nodata, quant = plan(_bands())
    assert [r[0] for r in rows] == [d for d, _, _ in s2_emit.S2_STACK_BANDS] and grid == (18, 22) and win == Window(0, 0, 22, 18)
    assert [r[2] for r in rows] == [1] * 4 + [2] * 6 and [r[3] for r in rows] == [0] * 4 + [1] * 6 and (dt, rl, nodata, quant) == (0, 0, 0, 10000.0)
    for b in (_bands(nir08=None), _bands(nir08="10m")):     # s2_utils.py:560-590: missing, or the resolution of nir
        with pytest.warns(UserWarning, match="9 bands"):
            rows = plan(b)[0]
        assert [r[0] for r in rows] == [d for d, k, _ in s2_emit.S2_STACK_BANDS if k != "nir08"]
    rows = plan(_bands(), add_offset={"blue": -1000, "swir22": 7})[0]
    assert [r[4] for r in rows] == [-1000] + [0] * 8 + [7]
    assert [r[4] for r in plan(_bands(), add_offset=-1000)[0]] == [-1000] * 10
    assert plan(_bands(), window=Window(3, 1, 5, 7))[2] == Window(3, 1, 5, 7) and plan(_bands(), nodata=None)[5] is None
    assert plan(_bands(17, 21))[1] == (17, 21)              # odd grids: the 20 m planes are the ceil
    with pytest.raises(ValueError, match="Missing required assets"):
        plan(_bands(drop=("red", "swir16")))
    bad = _bands()
    bad["swir16"] = np.ones((9, 12), np.uint16)
    with pytest.raises(ValueError, match="neither"):
        plan(bad)
    bad["swir16"] = np.ones((9, 11), np.float32)
    with pytest.raises(ValueError, match="uint16"):
        plan(bad)
    for kw, word in ((dict(out_dtype="float64"), "out_dtype"), (dict(rule="x"), "rule"), (dict(nodata=-1), "nodata"), (dict(nodata=70000), "nodata"),
                     (dict(nodata_out=1), "nodata_out"), (dict(quantification=0), "quantification"), (dict(quantification="a"), "quantification"),
                     (dict(add_offset=1.5), "add_offset"), (dict(add_offset={"blue": "x"}), "add_offset"),
                     (dict(window=(0, 0, 23, 18)), "window"), (dict(window=(-1, 0, 5, 5)), "window"), (dict(window=(0, 0, 0, 5)), "window"),
                     (dict(window=(20, 15, 3, 3)), "window")):
        with pytest.raises(ValueError, match=word):
            plan(_bands(), **kw)
    with pytest.raises(ValueError, match="mapping"):
        plan([np.ones((4, 4), np.uint16)])
    with pytest.raises(ValueError, match="out"):
        s2_emit.assemble_s2_stack(_bands(), out=np.zeros((10, 18, 22), np.uint16))
    with pytest.raises(ValueError, match="neither"):
        s2_emit.assemble_s2_stack(_bands(), scl=np.zeros((5, 5), np.uint8))
