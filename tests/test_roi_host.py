"""The polygon family on the host side: hsr_roi_rasterize_host, hsr_roi_glt_clip_host and hsr_roi_glt_reindex_host - the element
functions of the kernels compiled for the CPU - against the NumPy statement of tests/roi_cases.py on every row of the table and of
the seeded sweep, under both rules; the statement AND the host twin against two references that share no code with them
(matplotlib's point-in-path test for the centre rule, exact rationals for the touched rule); the ties worked by hand; every refusal
with its error text; include/hsr_roi.h against nat.ROI_SIGNATURES and the constants; the Python planners.  Every comparison of
values is an equality.

rasterio, shapely and GDAL are not installed here: nothing is compared with the reference's own run, and neither GDAL's bits nor
rasterio's window rounding are claimed (include/hsr_roi.h)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import roi_cases as rc
import s2_emit
from conftest import ROOT
from s2_emit import _native as nat
from s2_emit import reproject, roi

INVALID, UNSUPPORTED = 1, 2
SENT = 0xA5


def _gt(gt):
    return (C.c_double * 6)(*gt)


def run_host(r, rule, inside=1, outside=0):
    """The row through hsr_roi_rasterize_host into a guarded buffer with the row's stride -> (h, w) uint8."""
    lib = nat.load()
    verts, offs = rc.flatten(r["rings"])
    r0, c0, h, w = rc.window_of(r)
    rs = w + r["pad"]
    raw = np.full(64 + r["off"] + h * rs, SENT, np.uint8)
    lo = 32 + r["off"]
    code = lib.hsr_roi_rasterize_host(verts.ctypes.data, offs.ctypes.data, len(offs) - 1, len(verts), _gt(r["gt"]), r["H"], r["W"], rule, r0, c0,
                                      h, w, inside, outside, C.c_void_p(raw.ctypes.data + lo), rs)
    assert code == 0, lib.hsr_last_error()
    body = raw[lo: lo + (h - 1) * rs + w]
    assert (raw[:lo] == SENT).all() and (raw[lo + (h - 1) * rs + w:] == SENT).all()
    full = np.full(h * rs, SENT, np.uint8)
    full[: body.size] = body
    full = full.reshape(h, rs)
    assert (full[:, w:] == SENT).all()                                    # the stride's padding
    return full[:, :w]


# ---- the host twin against the statement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", list(rc.RULES))
@pytest.mark.parametrize("name", list(rc.ROWS))
def test_host_twin_equals_the_statement(name, rule):
    got = run_host(rc.ROWS[name], rc.RULES[rule])
    np.testing.assert_array_equal(got, rc.case(name, rc.RULES[rule]).astype(np.uint8))


@pytest.mark.parametrize("name", list(rc.SWEEP))
def test_host_twin_equals_the_statement_on_the_sweep(name):
    r = rc.SWEEP[name]
    for rule in (rc.CENTER, rc.TOUCHED):
        ref = rc.rasterize_ref(r["rings"], r["gt"], (r["H"], r["W"]), rule, r["window"])
        np.testing.assert_array_equal(run_host(r, rule), ref.astype(np.uint8))


def test_values_and_the_window_is_the_slice():
    r = rc.ROWS["holed"]
    for rule in (rc.CENTER, rc.TOUCHED):
        full = rc.case("holed", rule)
        np.testing.assert_array_equal(run_host(r, rule, 0, 1), (~full).astype(np.uint8))
        np.testing.assert_array_equal(run_host(r, rule, 7, 200), np.where(full, 7, 200).astype(np.uint8))
        for win in ((0, 0, 90, 140), (1, 0, 5, 7), (0, 1, 89, 139), (13, 77, 64, 63), (89, 139, 1, 1)):
            got = run_host(dict(r, window=win), rule)
            np.testing.assert_array_equal(got, full[win[0]: win[0] + win[2], win[1]: win[1] + win[3]].astype(np.uint8))


# ---- what the statement says on cases worked by hand -----------------------------------------------------------------------------------
def _px(rings, shape, rule):
    return rc.rasterize_ref(rings, (0.0, 1.0, 0.0, 0.0, 0.0, 1.0), shape, rule)


def test_statement_by_hand():
    # a 2 x 2 square on lattice lines: centre rule the four cells; touched rule also the row and column its closing edges OPEN
    sq = [np.array([[1.0, 1.0], [3.0, 1.0], [3.0, 3.0], [1.0, 3.0]])]
    c, t = _px(sq, (5, 5), rc.CENTER), _px(sq, (5, 5), rc.TOUCHED)
    want = np.zeros((5, 5), bool)
    want[1:3, 1:3] = True
    np.testing.assert_array_equal(c, want)
    want[1:4, 1:4] = True                                                 # floor: the edges on v = 3 and u = 3 touch row 3 and column 3
    np.testing.assert_array_equal(t, want)
    # a vertex exactly on a centre, edges to opposite sides: one crossing on that line, and a crossing AT pu is not right of it
    tri = [np.array([[2.5, 0.5], [4.5, 2.5], [0.5, 2.5]])]
    c = _px(tri, (4, 6), rc.CENTER)
    assert c[0].tolist() == [False] * 6                                   # the apex row: va <= pv for the apex only -> both edges cross at 2.5
    assert c[1].tolist() == [False, True, True, False, False, False]      # crossings at 1.5 and 3.5: pu = 1.5 is inside (not < 1.5), pu = 3.5 is not
    assert c[2].tolist() == [False] * 6                                   # the horizontal edge lies ON the line: it never crosses
    # a diagonal through lattice corners: the cells it crosses and (r - 1, c), (r, c) at every corner
    diag = [np.array([[0.5, 0.5], [2.5, 2.5], [0.5, 2.5]])]
    t = _px(diag, (3, 4), rc.TOUCHED)
    assert t.astype(int).tolist() == [[1, 1, 0, 0], [1, 1, 1, 0], [1, 1, 1, 0]]
    # overlapping parts cancel: even-odd over all rings, not a union
    two = [np.array([[0.0, 0.0], [3.0, 0.0], [3.0, 3.0], [0.0, 3.0]]), np.array([[1.0, 1.0], [4.0, 1.0], [4.0, 4.0], [1.0, 4.0]])]
    c = _px(two, (4, 4), rc.CENTER)
    assert not c[1:3, 1:3].any() and c[0, 0] and c[3, 3] and not c[0, 3]


# ---- two references that share no code with the statement ------------------------------------------------------------------------------
def test_centre_rule_against_matplotlib():
    """120 seeded polygon sets of one to three rings in general position on grids up to 40 x 60: no edge within 1e-6 pixel of a cell
    centre, so matplotlib's point-in-path test (XOR over the rings) has no tie to decide differently.  Every cell of every set is
    compared; no case is dropped.  The generator's redraw rate, measured here: 0 redraws in 240 rings (the chance of one is about
    2e-6 x the summed edge length per unit cell, some 1e-3 a ring); the test fails above 2 %."""
    rng = np.random.default_rng(27)
    drawn = redraws = 0
    for k in range(120):
        H, W = int(rng.integers(1, 41)), int(rng.integers(1, 61))
        rings = []
        for _ in range(1 + k % 3):
            ring, again = rc.general_polygon(rng, H, W)
            rings.append(ring)
            drawn, redraws = drawn + 1, redraws + again
        ref = rc.contains_points_ref(rings, H, W)
        gt = rc.GT_UTM if k % 2 else rc.GT_UP
        row = dict(H=H, W=W, gt=gt, rings=[rc.to_world(r, gt) for r in rings], window=None, pad=0, off=0)
        # the world coordinates round: the edges move by some 1e-10 pixel, far inside the margin
        np.testing.assert_array_equal(rc.rasterize_ref(row["rings"], gt, (H, W), rc.CENTER), ref)
        np.testing.assert_array_equal(run_host(row, rc.CENTER), ref.astype(np.uint8))
    print("general_polygon: %d redraws in %d rings" % (redraws, drawn))
    assert redraws <= 0.02 * drawn


def test_touched_rule_against_exact_rationals():
    """40 seeded polygon sets of one or two rings with vertices k / 16, k odd, on grids up to 12 x 14: "the boundary meets the closed
    cell or the centre is inside" in fractions.Fraction.  A ring is redrawn when an exact crossing of a lattice row line lies within
    1e-9 of a lattice column line (an edge through a lattice corner, where the closed cell and the header's floor differ), or an
    exact crossing of a centre line within 1e-9 of a centre.  Every cell of every set is compared.  Redraw rate measured here: 7
    redraws in 60 rings - vertices on a 1/16 lattice meet corners often; the test fails above 50 %."""
    rng = np.random.default_rng(28)
    drawn = redraws = 0
    gt = (0.0, 1.0, 0.0, 0.0, 0.0, 1.0)                                   # pixel coordinates: the dyadic vertices are exact
    for k in range(40):
        H, W = int(rng.integers(1, 13)), int(rng.integers(1, 15))
        rings = []
        for _ in range(1 + k % 2):
            ring, again = rc.dyadic_polygon(rng, H, W)
            rings.append(ring)
            drawn, redraws = drawn + 1, redraws + again
        ref = rc.touched_exact_ref(rings, H, W)
        world = [np.array([[float(u), float(v)] for u, v in ring]) for ring in rings]
        np.testing.assert_array_equal(rc.rasterize_ref(world, gt, (H, W), rc.TOUCHED), ref)
        row = dict(H=H, W=W, gt=gt, rings=world, window=None, pad=0, off=0)
        np.testing.assert_array_equal(run_host(row, rc.TOUCHED), ref.astype(np.uint8))
    print("dyadic_polygon: %d redraws in %d rings" % (redraws, drawn))
    assert redraws <= 0.5 * drawn


# ---- the GLT clip and re-index ------------------------------------------------------------------------------------------------------------
def run_clip_host(r, glt):
    lib = nat.load()
    verts, offs = rc.flatten(r["rings"])
    r0, c0, h, w = rc.bbox_window(r["rings"], r["gt"], (r["H"], r["W"]))
    out = np.full((h, w, 2), -77, np.int32)
    rec = np.full(rc.RECORD, -77, np.int32)
    code = lib.hsr_roi_glt_clip_host(verts.ctypes.data, offs.ctypes.data, len(offs) - 1, len(verts), _gt(r["gt"]), r["H"], r["W"], glt.ctypes.data,
                                     r0, c0, h, w, out.ctypes.data, rec.ctypes.data)
    assert code == 0, lib.hsr_last_error()
    return out, rec, (r0, c0, h, w)


CLIP_ROWS = ["triangle", "holed", "two-parts-up", "cross-tiles", "comb-1500", "off-left", "off-bottom", "huge-1e300", "tie-lattice-rectangle",
             "zero-area", "covering"]


@pytest.mark.parametrize("name", CLIP_ROWS)
def test_glt_clip_and_reindex_host(name):
    r = rc.ROWS[name]
    glt = rc.glt_of(r["H"], r["W"], 211, 97, seed=len(name))
    out, rec, win = run_clip_host(r, glt)
    mask = rc.rasterize_ref(r["rings"], r["gt"], (r["H"], r["W"]), rc.TOUCHED, win)
    want, wrec = rc.glt_clip_ref(glt, mask, win)
    np.testing.assert_array_equal(out, want)
    assert rec.tolist() == wrec.tolist()
    assert nat.load().hsr_roi_glt_reindex_host(out.ctypes.data, win[2], win[3], rec.ctypes.data) == 0
    np.testing.assert_array_equal(out, rc.glt_reindex_ref(want, wrec))
    if wrec[4]:
        assert out[..., 0].max() == wrec[3] - wrec[2] + 1 and out[..., 1].max() == wrec[1] - wrec[0] + 1 and out.min() == 0


def test_glt_clip_empty_range():
    r = rc.ROWS["triangle"]
    glt = np.zeros((r["H"], r["W"], 2), np.int32)
    glt[..., 1] = -5
    out, rec, win = run_clip_host(r, glt)
    assert rec.tolist() == [rc.I32_MAX, -1, rc.I32_MAX, -1, 0, 0, 0, 0] and rec[0] > rec[1]
    assert nat.load().hsr_roi_glt_reindex_host(out.ctypes.data, win[2], win[3], rec.ctypes.data) == 0
    assert not out.any()
    extreme = np.full((1, 1, 2), np.iinfo(np.int32).min, np.int32)         # INT32_MIN - INT32_MAX: the difference is taken in 64 bits
    assert nat.load().hsr_roi_glt_reindex_host(extreme.ctypes.data, 1, 1, rec.ctypes.data) == 0 and not extreme.any()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_their_texts():
    lib = nat.load()
    tri, offs = rc.flatten([[(1.0, 1.0), (9.0, 2.0), (4.0, 8.0)]])
    out = np.zeros((10, 10), np.uint8)
    gt = (0.0, 1.0, 0.0, 0.0, 0.0, 1.0)

    def call(v=tri, o=offs, nr=1, nv=3, g=gt, H=10, W=10, rule=0, win=(0, 0, 10, 10), dst=out, rs=10):
        return lib.hsr_roi_rasterize_host(None if v is None else v.ctypes.data, None if o is None else o.ctypes.data, nr, nv,
                                          None if g is None else _gt(g), H, W, rule, *win, 1, 0, None if dst is None else C.c_void_p(dst.ctypes.data), rs)

    def refused(code, text, **kw):
        assert call(**kw) == code and text in lib.hsr_last_error().decode(), (kw, lib.hsr_last_error())
        assert not out.any()                                              # nothing was written, nothing truncated

    assert call() == 0 and out.any()
    out[:] = 0
    two, offs2 = rc.flatten([[(1.0, 1.0), (9.0, 2.0), (4.0, 8.0)], [(2.0, 2.0), (3.0, 3.0)]])
    refused(INVALID, "a ring has at least 3 vertices", v=two, o=offs2, nr=2, nv=5)
    refused(INVALID, "5 vertices for 2 rings", v=two, o=np.array([0, 3, 5], np.int32), nr=2, nv=5)
    six, _ = rc.flatten([[(1.0, 1.0), (9.0, 2.0), (4.0, 8.0)]] * 2)
    refused(INVALID, "ring 1 has 2 vertices", v=six, o=np.array([0, 4, 6], np.int32), nr=2, nv=6)
    refused(INVALID, "ring_offsets run from 1", v=six, o=np.array([1, 3, 6], np.int32), nr=2, nv=6)
    refused(INVALID, "ring 0 has", v=six, o=np.array([0, -3, 6], np.int32), nr=2, nv=6)
    for bad in (np.nan, np.inf, -np.inf):
        nan = tri.copy()
        nan[1, 1] = bad
        refused(INVALID, "vertex 1 has a non-finite coordinate", v=nan)
    n = nat.HSR_ROI_MAX_EDGES + 1
    t = 2 * np.pi * np.arange(n) / n
    many = np.ascontiguousarray(np.stack([5 + 4 * np.cos(t), 5 + 4 * np.sin(t)], axis=1))
    refused(INVALID, "more than HSR_ROI_MAX_EDGES = 8192", v=many, o=np.array([0, n], np.int32), nv=n)
    assert call(v=many[:-1].copy(), o=np.array([0, n - 1], np.int32), nv=n - 1) == 0          # the limit itself is legal
    out[:] = 0
    refused(INVALID, "nrings=0", nr=0)
    refused(INVALID, "NULL polygon arrays", v=None)
    refused(INVALID, "NULL polygon arrays", o=None)
    refused(INVALID, "NULL geotransform", g=None)
    refused(UNSUPPORTED, "rotation terms", g=(0.0, 1.0, 0.1, 0.0, 0.0, 1.0))
    refused(UNSUPPORTED, "rotation terms", g=(0.0, 1.0, 0.0, 0.0, -0.1, 1.0))
    refused(INVALID, "pixel size of 0", g=(0.0, 0.0, 0.0, 0.0, 0.0, 1.0))
    refused(INVALID, "pixel size of 0", g=(0.0, 1.0, 0.0, 0.0, 0.0, 0.0))
    refused(INVALID, "term 3 is not finite", g=(0.0, 1.0, 0.0, np.nan, 0.0, 1.0))
    refused(INVALID, "an extent < 1", H=0)
    refused(INVALID, "an extent < 1", win=(0, 0, 0, 10))
    refused(INVALID, "leaves the 10 x 10 grid", win=(1, 0, 10, 10))
    refused(INVALID, "leaves the 10 x 10 grid", win=(0, -1, 5, 5))
    refused(UNSUPPORTED, "more than 2^30 a side", W=(1 << 30) + 1)
    refused(INVALID, "rule=2", rule=2)
    refused(INVALID, "NULL output", dst=None)
    refused(INVALID, "row stride 9 below w=10", rs=9)
    # the launch-path entries refuse what the counts show before they touch a device
    p = C.c_void_p(tri.ctypes.data)
    assert lib.hsr_roi_rasterize(p, p, 0, 3, _gt(gt), 10, 10, 0, 0, 0, 10, 10, 1, 0, p, 10, None) == INVALID
    assert lib.hsr_roi_rasterize(p, p, 1, 2, _gt(gt), 10, 10, 0, 0, 0, 10, 10, 1, 0, p, 10, None) == INVALID
    assert lib.hsr_roi_rasterize(p, p, 1, n, _gt(gt), 10, 10, 0, 0, 0, 10, 10, 1, 0, p, 10, None) == INVALID and b"HSR_ROI_MAX_EDGES" in lib.hsr_last_error()
    assert lib.hsr_roi_class_counts(p, p, 1, 3, _gt(gt), 10, 10, 0, 0, 0, 10, 10, p, 9, p, p, None) == INVALID and b"row stride" in lib.hsr_last_error()
    assert lib.hsr_roi_class_counts(p, p, 1, 3, _gt(gt), 10, 10, 0, 0, 0, 10, 10, None, 10, p, p, None) == INVALID
    assert lib.hsr_roi_glt_clip(p, p, 1, 3, _gt(gt), 10, 10, p, 0, 0, 10, 10, p, p, None) == INVALID and b"overlaps" in lib.hsr_last_error()
    assert lib.hsr_roi_glt_clip(p, p, 1, 3, _gt(gt), 10, 10, None, 0, 0, 10, 10, p, p, None) == INVALID
    assert lib.hsr_roi_glt_reindex(None, 1, 1, p, None) == INVALID and lib.hsr_roi_glt_reindex(p, 0, 1, p, None) == INVALID
    assert lib.hsr_roi_glt_reindex_host(None, 1, 1, None) == INVALID
    assert lib.hsr_roi_check_host(tri.ctypes.data, offs.ctypes.data, 1, 3) == 0
    assert lib.hsr_roi_check_host(two.ctypes.data, offs2.ctypes.data, 2, 5) == INVALID and b"hsr_roi_check_host" in lib.hsr_last_error()
    buf = C.create_string_buffer(64)
    assert lib.hsr_roi_last_launch(buf, 64) == 0 and buf.value == b""     # nothing was launched


def test_last_launch_is_empty_before_any_launch():
    buf = C.create_string_buffer(b"\x7f" * 63, 64)
    assert nat.load().hsr_roi_last_launch(buf, 64) == 0 and buf.value == b""


# ---- what the tables claim ---------------------------------------------------------------------------------------------------------------
def test_tables_hold_what_they_claim():
    rows = rc.ROWS
    wins = [rc.window_of(r) for r in rows.values()]
    assert {w[3] for w in wins} >= {1, rc.RUN - 1, rc.RUN, rc.RUN + 1, rc.TILE_W - 1, rc.TILE_W, rc.TILE_W + 1}
    assert {w[2] for w in wins} >= {1, rc.TILE_H - 1, rc.TILE_H, rc.TILE_H + 1}
    assert any(w[2] > 2 * rc.TILE_H and w[3] > 2 * rc.TILE_W for w in wins)
    assert {r["gt"][5] > 0 for r in rows.values()} == {True, False}
    assert any(r["pad"] for r in rows.values()) and any(r["off"] for r in rows.values())
    assert any((w[3] + r["pad"]) % 16 == 0 and r["off"] == 0 and w[3] % 16 for w, r in zip(wins, rows.values()))   # 16-byte stores with a tail
    heads = {(r["off"] + y * (w[3] + r["pad"])) % 16 for w, r in zip(wins, rows.values()) if w[3] >= 48 for y in range(w[2])}
    assert heads == set(range(16))                                        # rows of three runs and more start at every offset from a 16-byte boundary
    assert {(r["window"][0] % 2, r["window"][1] % 2) for r in rows.values() if r["window"]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(r["window"] and r["window"][0] >= rc.TILE_H and r["window"][1] >= rc.TILE_W for r in rows.values())
    assert len(rc.flatten(rows["comb-1500"]["rings"])[0]) == 1500 and len(rc.flatten(rows["ripple-1500"]["rings"])[0]) == 1500
    # every row of the comb between its teeth holds more than a thousand crossings
    ua, va, ub, vb = rc.pixel_edges(rows["comb-1500"]["rings"], rows["comb-1500"]["gt"])
    assert (((va <= 20.5) != (vb <= 20.5)).sum()) > 1000
    assert not rc.case("outside", rc.TOUCHED).any() and rc.case("covering", rc.CENTER).all()
    for name in ("off-left", "off-right", "off-top", "off-bottom"):
        m = rc.case(name, rc.CENTER)
        assert m.any() and not m.all()
    assert np.abs(rc.flatten(rows["huge-1e300"]["rings"])[0]).max() == 1e300 and rc.case("huge-1e300", rc.CENTER).any()
    assert not rc.case("zero-area", rc.CENTER).any() and rc.case("zero-area", rc.TOUCHED).any()
    assert rc.case("zero-area-point", rc.TOUCHED).sum() == 1
    assert not rc.case("overlapping", rc.CENTER)[45:60, 70:90].any()       # the overlap is outside
    for name in rows:
        if name.startswith("tie-"):
            c, t = rc.case(name, rc.CENTER), rc.case(name, rc.TOUCHED)
            assert (name == "tie-grid-edges" or (t & ~c).any()) and not (c & ~t).any()
    assert set(rc.EXTREME_ROWS) <= set(rows)


# ---- the header, the bindings, the package --------------------------------------------------------------------------------------------------
def test_header_bindings_and_constants():
    text = open(os.path.join(ROOT, "include", "hsr_roi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hsr_\w+)\s*\(", code))
    assert declared == set(nat.ROI_SIGNATURES) and not declared & set(nat.SIGNATURES)
    lib = nat.load()
    assert all(hasattr(lib, n) for n in declared)
    for n, (_, args) in nat.ROI_SIGNATURES.items():
        proto = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % n, code, flags=re.S).group(1)
        assert len([a for a in proto.split(",") if a.strip() != "void"]) == len(args), n
    defines = {k: int(v) for k, v in re.findall(r"#define (HSR_ROI_\w+) (\d+)", text)}
    assert defines == {k: getattr(nat, k) for k in defines} and len(defines) == 7
    assert (rc.MAX_EDGES, rc.TILE_H, rc.TILE_W, rc.RUN, rc.RECORD) == (nat.HSR_ROI_MAX_EDGES, nat.HSR_ROI_TILE_H, nat.HSR_ROI_TILE_W,
                                                                         nat.HSR_ROI_RUN, nat.HSR_ROI_RECORD)
    assert nat.HSR_ROI_MAX_EDGES >= 4096 and roi.MAX_EDGES == nat.HSR_ROI_MAX_EDGES
    assert lib.hsr_abi_version() == 5 and nat.HSR_ABI_VERSION == 5 and lib.hsr_roi_instance_count() == rc.INSTANCE_COUNT
    names = [lib.hsr_roi_instance_name(i).decode() for i in range(rc.INSTANCE_COUNT)]
    assert names == rc.INSTANCES
    assert lib.hsr_roi_instance_name(rc.INSTANCE_COUNT) is None and lib.hsr_roi_instance_name(-1) is None
    assert "NOT claimed" in text and "not a union" in text and "EVEN-ODD" in text and "Ties, decided" in text
    mk = open(os.path.join(ROOT, "hyperspectral_super-resolution_amd", "csrc", "Makefile")).read()
    assert "hsr_roi.hip" in mk and "hsr_roi.h" in mk and "roi-ubsan" in mk


def test_public_surface():
    for n in ("rasterize_roi", "scl_metrics_roi", "count_cloud_pixels_roi", "spatial_subset", "clip_cube", "SubsetOutput"):
        assert n in s2_emit.__all__ and callable(getattr(s2_emit, n)) and getattr(s2_emit, n) is getattr(roi, n)
    assert all(callable(getattr(s2_emit, n)) for n in s2_emit.__all__)


# ---- the planners ------------------------------------------------------------------------------------------------------------------------------
def test_polygon_rings_forms():
    a = np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 4.0], [0.0, 4.0]])
    hole = np.array([[1.0, 1.0], [2.0, 1.0], [2.0, 2.0]])
    closed = np.concatenate([a, a[:1]])
    same = lambda got, want: len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))  # noqa: E731
    assert same(roi.polygon_rings(a), [a]) and same(roi.polygon_rings([a, hole]), [a, hole])
    assert same(roi.polygon_rings([(a, hole), [hole + 10]]), [a, hole, hole + 10])
    assert same(roi.polygon_rings([a.tolist(), hole.tolist()]), [a, hole])
    assert same(roi.polygon_rings({"type": "Polygon", "coordinates": [closed.tolist(), hole.tolist()]}), [a, hole])
    multi = {"type": "MultiPolygon", "coordinates": [[closed.tolist(), hole.tolist()], [(hole + 10).tolist()]]}
    assert same(roi.polygon_rings(multi), [a, hole, hole + 10])
    z = {"type": "Polygon", "coordinates": [[p + [7.0] for p in closed.tolist()]]}                # positions with a height
    assert same(roi.polygon_rings(z), [a])

    class Geo:
        __geo_interface__ = multi

    assert same(roi.polygon_rings(Geo()), [a, hole, hole + 10])
    for bad in ({"type": "Point", "coordinates": [0, 0]}, 5, [], [np.zeros((3, 1))], {"type": "Polygon", "coordinates": 3}):
        with pytest.raises(ValueError):
            roi.polygon_rings(bad)


def test_plan_roi_and_the_bounding_window():
    tri = [np.array([[600025.0, 4099975.0], [600395.0, 4099915.0], [600105.0, 4099605.0]])]
    p = roi._plan_roi(tri, rc.GT_UTM, (50, 60))
    assert p.offsets.tolist() == [0, 3] and p.verts.dtype == np.float64 and p.gt == rc.GT_UTM and p.shape == (50, 60)
    assert roi._bbox_window(p.verts, p.gt, p.shape) == (2, 2, 38, 38) == rc.bbox_window(tri, rc.GT_UTM, (50, 60))
    assert roi._bbox_window(p.verts, p.gt, (20, 30)) == (2, 2, 18, 28)                              # clamped to the grid
    assert roi._bbox_window(p.verts + 1e6, p.gt, p.shape) is None                                   # misses the grid
    up = roi._plan_roi(tri, (600000.0, 10.0, 0.0, 4099500.0, 0.0, 10.0), (50, 60))
    assert roi._bbox_window(up.verts, up.gt, up.shape) == (10, 2, 38, 38)
    huge = roi._plan_roi([np.array([[-1e300, -1e300], [1e300, 0.0], [0.0, 1e300]])], (0.0, 1e-9, 0.0, 0.0, 0.0, -1e-9), (7, 9))
    assert roi._bbox_window(huge.verts, huge.gt, huge.shape) == (0, 0, 7, 9)
    for name, r in rc.ROWS.items():
        v, _ = rc.flatten(r["rings"])
        assert roi._bbox_window(v, r["gt"], (r["H"], r["W"])) == rc.bbox_window(r["rings"], r["gt"], (r["H"], r["W"])), name
    with pytest.raises(nat.HsrError, match="at least 3 vertices"):
        roi._plan_roi([np.zeros((2, 2))], rc.GT_UTM, (5, 5))
    with pytest.raises(nat.HsrError, match="non-finite"):
        roi._plan_roi([np.array([[0.0, 0.0], [1.0, np.nan], [2.0, 2.0]])], rc.GT_UTM, (5, 5))
    with pytest.raises(nat.HsrError, match="HSR_ROI_MAX_EDGES"):
        roi._plan_roi([np.random.default_rng(0).random((8193, 2))], rc.GT_UTM, (5, 5))
    for kw, msg in ((dict(transform=(0, 1, 0.5, 0, 0, 1)), "rotation"), (dict(transform=(0, 0, 0, 0, 0, 1)), "dx and dy"),
                    (dict(transform=(0, 1, 0, 0, 0)), "geotransform"), (dict(shape=(0, 5)), "shape"), (dict(crs="utm"), "crs"),
                    (dict(crs="wgs84"), "utm="), (dict(utm=32611), "crs='wgs84'")):
        args = dict(polygons=tri, transform=rc.GT_UTM, shape=(5, 5))
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            roi._plan_roi(**args)
    assert roi._window(None, (5, 6)) == (0, 0, 5, 6) and roi._window((1, 2, 3, 4), (5, 6)) == (1, 2, 3, 4)
    for bad in ((0, 0, 6, 6), (-1, 0, 2, 2), (0, 0, 0, 1), (0, 0, 1), 3):
        with pytest.raises(ValueError):
            roi._window(bad, (5, 6))


def test_lon_lat_vertices_go_through_tm_forward():
    lonlat = np.array([[-117.2, 34.1], [-117.0, 34.15], [-117.1, 34.3]])
    params = reproject.utm_params(32611)
    e, n = reproject.tm_forward(lonlat[:, 0], lonlat[:, 1], params)
    for utm in (32611, "EPSG:32611", params):
        p = roi._plan_roi({"type": "Polygon", "coordinates": [lonlat.tolist() + lonlat[:1].tolist()]}, (470000.0, 10.0, 0.0, 3800000.0, 0.0, -10.0),
                          (3000, 3000), crs="wgs84", utm=utm)
        np.testing.assert_array_equal(p.verts, np.stack([e, n], axis=1))                            # the vertices, and only the vertices
    assert roi._bbox_window(p.verts, p.gt, p.shape) is not None


def test_entry_points_need_a_gpu_only_after_planning():
    with pytest.raises(nat.HsrError, match="at least 3 vertices"):
        s2_emit.rasterize_roi([np.zeros((2, 2))], rc.GT_UTM, (5, 5))
    with pytest.raises(ValueError, match="glt"):
        s2_emit.spatial_subset(np.zeros((4, 4)), rc.GT_UTM, [np.zeros((3, 2))])
    with pytest.raises(ValueError, match="cube"):
        s2_emit.clip_cube(np.zeros((2, 4, 4), np.float32), [np.zeros((3, 2))], rc.GT_UTM)
    import torch
    tri = [np.array([[600005.0, 4099995.0], [600045.0, 4099985.0], [600015.0, 4099955.0]])]
    with pytest.raises(ValueError, match="cube: a non-empty .* device tensor"):                    # a host tensor never reaches a kernel
        s2_emit.clip_cube(torch.zeros((2, 5, 5), dtype=torch.float32), tri, rc.GT_UTM)
    with pytest.raises(ValueError, match="out: a device tensor"):
        s2_emit.rasterize_roi(tri, rc.GT_UTM, (5, 5), out=torch.zeros((5, 5), dtype=torch.uint8))
    with pytest.raises(ValueError, match="out: a \\(5, 5\\) uint8"):
        s2_emit.rasterize_roi(tri, rc.GT_UTM, (5, 5), out=torch.zeros((5, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="scl"):
        s2_emit.scl_metrics_roi(np.zeros((4, 4), np.float32), [np.zeros((3, 2))], rc.GT_UTM)
