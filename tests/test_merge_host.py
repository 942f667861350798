"""The scene-merging family on the host side: the planners' refusals; merge_grid (hsr_merge_grid) against the float64 statement of
tests/merge_cases.py and against grids worked by hand - offsets, union, bounds, residuals, a source offset by exactly half a pixel,
negative and positive dy, the refused pixel-size mismatch; hsr_merge_scenes_host - the per-element function of the kernels compiled
for the CPU - against the statement on every row of the table, in both layouts' strides and with the source plane; every refusal of
the C entries that needs no device; what the case tables claim; include/hsr_merge.h against nat.MERGE_SIGNATURES and the constants.
Every comparison of values is an equality on uint32 bits.

rioxarray, rasterio and xarray are not installed here: nothing is compared with the reference's own run, and rasterio's window
rounding is not claimed (include/hsr_merge.h)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import merge_cases as mc
import ortho_cases as oc
import s2_emit
from conftest import ROOT
from s2_emit import _native as nat
from s2_emit import merge

INVALID, UNSUPPORTED = 1, 2
SENT = 0xA5


def _table(arrays, offsets, bands, layout):
    rows = []
    for a, (oy, ox) in zip(arrays, offsets):
        h, w = a.shape[:2] if layout == mc.BIP else a.shape[1:]
        rows.append(nat.MergeScene(a.ctypes.data, h, w, oy, ox, bands, 0))
    return (nat.MergeScene * len(rows))(*rows)


def _run_host(name, source=True, reverse=False):
    lib, r, c = nat.load(), mc.ROWS[name], mc.case(name)
    scenes = [mc.in_layout(s, r["layout"]) for s in c["scenes"]]
    offsets = list(c["offsets"])
    if reverse:
        scenes, offsets = scenes[::-1], offsets[::-1]
    n_out = r["H"] * r["W"] * r["bands"]
    raw = np.full(n_out * 4 + 64, SENT, np.uint8)
    plane = np.full(r["H"] * r["W"] + 64, SENT, np.uint8)
    out = raw[32: 32 + 4 * n_out].view(np.float32)
    rc = lib.hsr_merge_scenes_host(_table(scenes, offsets, r["bands"], r["layout"]), len(scenes), r["layout"], r["H"], r["W"],
                                   C.c_float(r["nodata"]), int(r["nan"]), C.c_void_p(out.ctypes.data),
                                   C.c_void_p(plane.ctypes.data + 32) if source else None)
    assert rc == 0, lib.hsr_last_error()
    assert (raw[:32] == SENT).all() and (raw[32 + 4 * n_out:] == SENT).all()
    assert (plane[:32] == SENT).all() and (plane[32 + r["H"] * r["W"]:] == SENT).all()
    assert source or (plane == SENT).all()
    return out.view(np.uint32).reshape(c["ref"].shape), plane[32: 32 + r["H"] * r["W"]].reshape(r["H"], r["W"])


# ---- the host twin against the statement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mc.ROWS))
def test_host_twin_equals_the_statement(name):
    c = mc.case(name)
    got, plane = _run_host(name)
    np.testing.assert_array_equal(got, c["ref"])
    np.testing.assert_array_equal(plane, c["source"])


def test_host_twin_without_a_source_plane_and_order_dependence():
    for name in ("identical-bip", "identical-bsq"):
        r, c = mc.ROWS[name], mc.case(name)
        got, _ = _run_host(name, source=False)
        np.testing.assert_array_equal(got, c["ref"])
        swapped, plane = _run_host(name, reverse=True)
        ref_bip, src = mc.merge_ref(c["scenes"][::-1], c["offsets"][::-1], (r["H"], r["W"]), r["nodata"])
        np.testing.assert_array_equal(swapped, mc.in_layout(ref_bip, r["layout"]))
        np.testing.assert_array_equal(plane, src)
        assert (swapped != got).any()                                   # the other source's bits


# ---- what the statement says on cases worked by hand -------------------------------------------------------------------------------
def test_statement_by_hand():
    nd = np.float32(-9999.0)
    a = np.array([[[1.0, nd], [nd, nd], [np.nan, 4.0]]], np.float32)               # (1, 3, 2)
    b = np.array([[[7.0, 8.0], [9.0, nd], [5.0, 6.0], [nd, -0.0]]], np.float32)    # (1, 4, 2) one cell to the right
    out, src = mc.merge_ref([a, b], [(0, 0), (0, 1)], (1, 5))
    want = np.array([[[1.0, nd], [7.0, 8.0], [np.nan, 4.0], [5.0, 6.0], [nd, -0.0]]], np.float32)
    np.testing.assert_array_equal(out, want.view(np.uint32))
    assert src.tolist() == [[0, 1, 0, 1, 1]]
    out, src = mc.merge_ref([a, b], [(0, 0), (0, 1)], (1, 5), nan_is_nodata=True)
    want[0, 2, 0] = 9.0
    np.testing.assert_array_equal(out, want.view(np.uint32))
    out, src = mc.merge_ref([b, a], [(0, 1), (0, 0)], (1, 5))
    assert out.view(np.float32)[0, 2].tolist() == [9.0, 4.0] and src.tolist() == [[1, 0, 0, 0, 0]]
    # -0.0 is empty under nodata = 0 and the output then holds the bits of nodata, +0.0
    z = np.array([[[-0.0, 2.0]]], np.float32)
    out, src = mc.merge_ref([z], [(0, 0)], (1, 1), nodata=0.0)
    assert out.tolist() == [[[0, np.float32(2.0).view(np.uint32)]]]


# ---- merge_grid --------------------------------------------------------------------------------------------------------------------
GT_A = (600000.0, 60.0, 0.0, 4100040.0, 0.0, -60.0)


def _same_grid(got, want):
    assert got.geotransform == want[0] and got.shape == want[1] and got.offsets == want[2]
    assert got.residuals == want[3]                                      # float64, operation for operation


def test_merge_grid_union_offsets_and_residuals():
    gts = [GT_A, (600000.0 - 3 * 60.0, 60.0, 0.0, 4100040.0 - 1242 * 60.0, 0.0, -60.0), (600000.0 + 7 * 60.0 + 15.0, 60.0, 0.0, 4100040.0 + 600.0, 0.0, -60.0)]
    shapes = [(1280, 1242), (1280, 1242), (100, 50)]
    g = merge.merge_grid(gts, shapes)
    _same_grid(g, mc.merge_grid_ref(gts, shapes))
    assert g.geotransform == (600000.0 - 180.0, 60.0, 0.0, 4100040.0 + 600.0, 0.0, -60.0)
    assert g.offsets == ((10, 3), (1252, 0), (0, 10)) and g.shape == (1252 + 1280, 3 + 1242)
    assert g.residuals == ((0.0, 0.0), (0.0, 0.0), (0.0, 0.25))
    one = merge.merge_grid([GT_A], [(7, 9)])
    assert one.geotransform == GT_A and one.shape == (7, 9) and one.offsets == ((0, 0),) and one.residuals == ((0.0, 0.0),)


def test_merge_grid_half_a_pixel_goes_to_the_next_cell():
    gts = [GT_A, (600000.0 + 2.5 * 60.0, 60.0, 0.0, 4100040.0 - 1.5 * 60.0, 0.0, -60.0), (600000.0 + 60.0 * 0.49, 60.0, 0.0, 4100040.0, 0.0, -60.0)]
    g = merge.merge_grid(gts, [(4, 4)] * 3)
    assert g.offsets == ((0, 0), (2, 3), (0, 0)) and g.residuals[1] == (-0.5, -0.5) and abs(g.residuals[2][1] - 0.49) < 1e-12
    assert g.shape == (6, 7)
    _same_grid(g, mc.merge_grid_ref(gts, [(4, 4)] * 3))


def test_merge_grid_positive_dy_and_geographic_steps():
    up = [(10.0, 0.5, 0.0, 50.0, 0.0, 0.5), (11.0, 0.5, 0.0, 48.0, 0.0, 0.5)]
    g = merge.merge_grid(up, [(4, 4), (6, 2)])
    assert g.geotransform == (10.0, 0.5, 0.0, 48.0, 0.0, 0.5) and g.offsets == ((4, 0), (0, 2)) and g.shape == (8, 4)
    step = 0.000542232520256367                                           # EMIT's GLT grid step: offsets from inexact quotients
    geo = [(-118.5, step, 0.0, 35.25, 0.0, -step), (-118.5 + 37 * step, step, 0.0, 35.25 - 1100 * step, 0.0, -step)]
    g = merge.merge_grid(geo, [(1280, 1500), (1280, 1500)])
    _same_grid(g, mc.merge_grid_ref(geo, [(1280, 1500), (1280, 1500)]))
    assert g.offsets == ((0, 0), (1100, 37)) and max(abs(v) for r in g.residuals for v in r) < 1e-6


def test_merge_grid_bounds():
    gts = [GT_A, (600000.0 + 600.0, 60.0, 0.0, 4100040.0 - 6000.0, 0.0, -60.0)]
    shapes = [(120, 50), (120, 50)]
    bounds = (600000.0 + 130.0, 4100040.0 - 9000.0, 600000.0 + 130.0 + 20 * 60.0 + 29.0, 4100040.0 - 1000.0 + 31.0)
    g = merge.merge_grid(gts, shapes, bounds)
    _same_grid(g, mc.merge_grid_ref(gts, shapes, bounds))
    assert g.geotransform == (bounds[0], 60.0, 0.0, bounds[3], 0.0, -60.0)
    assert g.shape == (134, 20)                                           # floor(8031 / 60 + 0.5), floor(1229 / 60 + 0.5)
    # the top lies 969 m below source 0's edge: 969 / -60 = -16.15 -> -16; source 1: 5031 / 60 = 83.85 -> 84; -130 / 60 -> -2, 470 / 60 -> 8
    assert g.offsets == ((-16, -2), (84, 8))
    assert abs(g.residuals[0][0] + 0.15) < 1e-9 and abs(g.residuals[1][0] + 0.15) < 1e-9
    assert abs(g.residuals[0][1] - (-130.0 / 60.0 + 2)) < 1e-12
    tiny = merge.merge_grid(gts, shapes, (0.0, 0.0, 1.0, 1.0))
    assert tiny.shape == (1, 1)


@pytest.mark.parametrize("gt,code", [
    ((600000.0, 60.0, 0.5, 4100040.0, 0.0, -60.0), UNSUPPORTED), ((600000.0, 60.0, 0.0, 4100040.0, -0.5, -60.0), UNSUPPORTED),
    ((600000.0, 60.0 * (1 + 0.011 / 100), 0.0, 4100040.0, 0.0, -60.0), UNSUPPORTED), ((600000.0, 60.0, 0.0, 4100040.0, 0.0, 60.0), UNSUPPORTED),
    ((600000.0, 60.0, 0.0, 4100040.0, 0.0, -60.0 * (1 - 0.011 / 100)), UNSUPPORTED),
    ((float("nan"), 60.0, 0.0, 4100040.0, 0.0, -60.0), INVALID), ((600000.0, 60.0, 0.0, float("inf"), 0.0, -60.0), INVALID),
    ((600000.0 + 60.0 * 2.0 ** 31, 60.0, 0.0, 4100040.0, 0.0, -60.0), INVALID)])
def test_merge_grid_refusals(gt, code):
    with pytest.raises(nat.HsrError, match=r"code %d\): hsr_merge_grid:" % code):
        merge.merge_grid([GT_A, gt], [(100, 100), (100, 100)])


def test_merge_grid_accepts_a_pixel_size_within_the_hundredth():
    near = (600000.0, 60.0 * (1 + 0.009 / 100), 0.0, 4100040.0, 0.0, -60.0 * (1 - 0.009 / 100))
    assert merge.merge_grid([GT_A, near], [(100, 100), (100, 100)]).offsets == ((0, 0), (0, 0))
    for bad in ([(600000.0, 0.0, 0.0, 0.0, 0.0, -60.0)], [(600000.0, -60.0, 0.0, 0.0, 0.0, -60.0)], [(600000.0, 60.0, 0.0, 0.0, 0.0, 0.0)]):
        with pytest.raises(nat.HsrError, match=r"code 1\)"):
            merge.merge_grid(bad, [(4, 4)])
    with pytest.raises(nat.HsrError, match="bounds"):
        merge.merge_grid([GT_A], [(4, 4)], (5.0, 0.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        merge.merge_grid([GT_A], [(4, 4), (4, 4)])
    with pytest.raises(ValueError):
        merge.merge_grid([GT_A] * 9, [(4, 4)] * 9)
    with pytest.raises(ValueError):
        merge.merge_grid([GT_A[:5]], [(4, 4)])
    with pytest.raises(nat.HsrError, match=r"code 1\)"):
        merge.merge_grid([GT_A], [(0, 4)])
    lib = nat.load()
    assert lib.hsr_merge_grid(None, None, 1, None, None, None, None, None) == INVALID


# ---- the C entries' refusals that need no device --------------------------------------------------------------------------------------
def test_merge_scenes_host_refusals():
    lib = nat.load()
    a = np.zeros((2, 3, 4), np.float32)
    out = np.zeros((2, 3, 4), np.float32)
    plane = np.zeros((2, 3), np.uint8)

    def call(tab, n=1, layout=0, H=2, W=3, o=out, p=None):
        return lib.hsr_merge_scenes_host(tab, n, layout, H, W, C.c_float(-9999.0), 0, None if o is None else C.c_void_p(o.ctypes.data),
                                         None if p is None else C.c_void_p(p.ctypes.data))

    good = _table([a], [(0, 0)], 4, mc.BIP)
    assert call(good) == 0 and call(good, p=plane) == 0
    assert call(good, n=0) == INVALID and call(good, n=9) == INVALID and call(None) == INVALID and call(good, o=None) == INVALID
    assert call(good, layout=2) == INVALID and call(good, H=0) == INVALID and call(good, W=-1) == INVALID
    assert call(_table([a], [(0, 0)], 0, mc.BIP)) == INVALID
    assert call(_table([a], [(0, 0)], 513, mc.BIP)) == UNSUPPORTED
    two = _table([a, a], [(0, 0), (0, 1)], 4, mc.BIP)
    two[1].bands = 3
    assert call(two, n=2) == INVALID and b"bands" in lib.hsr_last_error()
    null = _table([a], [(0, 0)], 4, mc.BIP)
    null[0].scene_dev = None
    assert call(null) == INVALID
    zero = _table([a], [(0, 0)], 4, mc.BIP)
    zero[0].h = 0
    assert call(zero) == INVALID
    assert call(good, o=a) == INVALID and b"overlaps" in lib.hsr_last_error()       # the output is the input
    assert call(good, H=1 << 16, W=1 << 16) == UNSUPPORTED
    # the device entries refuse the same way before any launch (no device is touched)
    assert lib.hsr_merge_scenes(good, 0, 0, 2, 3, C.c_float(-9999.0), 0, C.c_void_p(out.ctypes.data), None, None) == INVALID
    sw = nat.MergeSwath(a.ctypes.data, a.ctypes.data, None, None, 2, 3, 2, 3, 0, 0, 0, 4)
    tab = (nat.MergeSwath * 2)(sw, sw)

    def ortho(n=1, layout=0, H=2, W=3, o=out.ctypes.data):
        return lib.hsr_ortho_merge(tab, n, 0, layout, H, W, C.c_float(-9999.0), C.c_float(-9999.0), C.c_void_p(o), None, None, None)

    assert ortho(n=0) == INVALID and ortho(n=9) == INVALID and ortho(layout=3) == INVALID and ortho(H=0) == INVALID
    assert ortho(o=None) == INVALID and ortho(o=a.ctypes.data) == INVALID
    tab[1].bands = 5
    assert ortho(n=2) == INVALID and b"bands" in lib.hsr_last_error()
    tab[1].bands, tab[0].bands = 513, 513
    assert ortho(n=2) == UNSUPPORTED
    tab[0].bands = tab[1].bands = 4
    tab[1].bmask_dev, tab[1].bmask_bytes = plane.ctypes.data, 0
    assert ortho(n=2) == INVALID and b"bmask_bytes" in lib.hsr_last_error()
    tab[1].bmask_dev, tab[1].glt_dev = None, None
    assert ortho(n=2) == INVALID
    buf = C.create_string_buffer(64)
    assert lib.hsr_merge_last_launch(buf, 64) == 0 and buf.value == b""          # nothing was launched


# ---- the planners --------------------------------------------------------------------------------------------------------------------
def test_plan_merge():
    a, b = np.zeros((5, 3, 4), np.float32), np.zeros((5, 2, 6), np.float32)
    p = merge._plan_merge([a, b], [(0, 0), (1, 2)])
    assert (p.n, p.bands, p.layout, p.sizes, p.offsets, p.shape, p.out_shape) == (2, 5, "bsq", ((3, 4), (2, 6)), ((0, 0), (1, 2)), (3, 8), (5, 3, 8))
    assert (p.nodata, p.nan, p.source) == (-9999.0, False, False)
    p = merge._plan_merge([np.zeros((3, 4, 5)), np.zeros((2, 6, 5), np.int16)], [(0, 0), (-1, -2)], layout="bip", shape=(2, 2), source=True, nan_is_nodata=1)
    assert (p.shape, p.out_shape, p.source, p.nan) == ((2, 2), (2, 2, 5), True, True)
    g = merge.merge_grid([GT_A, (GT_A[0] + 120.0, 60.0, 0.0, GT_A[3] - 60.0, 0.0, -60.0)], [(3, 4), (2, 6)])
    p = merge._plan_merge([a, b], grid=g)
    assert p.offsets == ((0, 0), (1, 2)) and p.shape == (3, 8)
    for kw, msg in ((dict(scenes=[]), "sources"), (dict(scenes=[a] * 9), "sources"), (dict(scenes=[a, np.zeros((4, 2, 6), np.float32)]), "bands"),
                    (dict(scenes=[np.zeros((3, 4), np.float32)]), "3-D"), (dict(scenes=[a], layout="bil"), "layout"),
                    (dict(scenes=[np.zeros((513, 2, 2), np.float32)]), "at most 512"), (dict(scenes=[a, b], offsets=[(0, 0)]), "offsets"),
                    (dict(scenes=[a], offsets=[(0.5, 0)]), "integer"), (dict(scenes=[a], grid=g), "MergeGrid"),
                    (dict(scenes=[a, b], grid=g, shape=(3, 8)), "not both"), (dict(scenes=[a], shape=(0, 4)), "shape"),
                    (dict(scenes=[a], offsets=[(-5, 0)]), "shape="), (dict(scenes=[a], nodata="x"), "nodata"),
                    (dict(scenes=[a], out=np.zeros((5, 3, 4), np.float32)), "out"), (dict(scenes=[np.zeros((5, 3, 4), bool)]), "numeric"),
                    (dict(scenes=[a], shape=(1 << 16, 1 << 16)), "2\\^31"), (dict(scenes=5), "sequence")):
        with pytest.raises(ValueError, match=msg):
            merge._plan_merge(**kw)


def test_plan_ortho_merge():
    sw = [np.zeros((4, 5, 7), np.float32), np.zeros((6, 5, 7), np.float32)]
    glt = [np.ones((3, 9, 2), np.int32), np.ones((2, 4, 2), np.int64)]
    p = merge._plan_ortho_merge(sw, glt, offsets=[(0, 0), (2, 8)], qmasks=[None, np.zeros((6, 5), np.uint8)],
                                band_masks=[np.zeros((4, 5, 2), np.uint8), None])
    assert (p.n, p.bands, p.shape, p.out_shape, p.offsets) == (2, 7, (4, 12), (7, 4, 12), ((0, 0), (2, 8)))
    assert (p.nodata, p.masked, p.glt_nodata, p.geotransform) == (-9999.0, -9999.0, 0, None)
    assert [q.bmask_bytes for q in p.plans] == [2, 0]
    g = merge.merge_grid([GT_A, (GT_A[0] + 8 * 60.0, 60.0, 0.0, GT_A[3] - 120.0, 0.0, -60.0)], [(3, 9), (2, 4)])
    p = merge._plan_ortho_merge(sw, glt, grid=g, layout="bip", nodata=-1.0, masked_value=-2.0, source=True)
    assert (p.shape, p.out_shape, p.geotransform, p.nodata, p.masked, p.source) == ((4, 12), (4, 12, 7), GT_A, -1.0, -2.0, True)
    for kw, msg in ((dict(swaths=sw, glts=glt[:1]), "glts"), (dict(swaths=[sw[0], np.zeros((4, 5, 6), np.float32)], glts=glt), "bands"),
                    (dict(swaths=sw, glts=glt, qmasks=[None]), "qmasks"), (dict(swaths=sw, glts=glt, band_masks=[None, np.zeros((6, 5), np.uint8)]), "band_mask"),
                    (dict(swaths=sw, glts=[glt[0], np.ones((2, 4, 2), np.float32)]), "integer"), (dict(swaths=[], glts=[]), "sources"),
                    (dict(swaths=sw * 5, glts=glt * 5), "sources"), (dict(swaths=sw, glts=glt, offsets=[(0, 0)] * 3), "offsets"),
                    (dict(swaths=sw, glts=glt, grid=g, offsets=[(0, 0)] * 2), "not both"), (dict(swaths=sw, glts=glt, layout="x"), "layout"),
                    (dict(swaths=sw, glts=glt, out=np.zeros((7, 3, 9), np.float32)), "out"),
                    (dict(swaths=[np.zeros((4, 5, 513), np.float32)], glts=glt[:1]), "at most 512")):
        with pytest.raises(ValueError, match=msg):
            merge._plan_ortho_merge(**kw)


def test_entry_points_need_a_gpu_only_after_planning():
    with pytest.raises(ValueError, match="bands"):
        s2_emit.merge_scenes([np.zeros((5, 3, 4), np.float32), np.zeros((4, 3, 4), np.float32)])
    with pytest.raises(ValueError, match="glts"):
        s2_emit.ortho_merge([np.zeros((4, 5, 7), np.float32)], [])


def test_is_adjacent():
    names = ["EMIT_L2A_RFL_001_20230401T203751_2309114_%03d.nc" % k for k in (2, 3, 4)]
    assert s2_emit.is_adjacent(names[0], names) is True and s2_emit.is_adjacent(names[0], names[::2]) is False
    assert s2_emit.is_adjacent("x", names[:1]) is True and s2_emit.is_adjacent("x", names[::-1]) is False


# ---- what the tables claim ------------------------------------------------------------------------------------------------------------
def test_tables_hold_what_they_claim():
    rows = mc.ROWS
    assert {r["W"] for r in rows.values()} >= {1, 63, 64, 65, 129} and {r["H"] for r in rows.values()} >= {1, 3}
    for layout in (mc.BIP, mc.BSQ):
        mine = [r for r in rows.values() if r["layout"] == layout]
        assert {r["bands"] for r in mine} >= {1, 3, 4, 5, 8, 285, 512}
        assert {len(r["sources"]) for r in mine} >= {1, 2, 3, 8}
        assert any(r["out_off"] % 16 for r in mine) and any(s["off"] % 16 for r in mine for s in r["sources"])
        assert any(s["oy"] < 0 and s["ox"] < 0 for r in mine for s in r["sources"])
    assert set(mc.all_instances()) == {mc.ortho_instance_of(rows[n]) for n in mc.ORTHO_ROWS} | set(mc.merge_scenes_instances(True))
    assert len(set(mc.all_instances())) == mc.INSTANCE_COUNT
    for ln in ("bip", "bsq"):
        r, c = rows[f"outside-{ln}"], mc.case(f"outside-{ln}")
        outside = [k for k, s in enumerate(r["sources"]) if s["oy"] + s["gh"] <= 0 or s["ox"] >= r["W"]]
        assert outside == [1, 2] and not np.isin(c["source"], outside).any() and [c["dropped"][k] for k in outside] == [0, 0]
        r = rows[f"identical-{ln}"]
        assert len({(s["gh"], s["gw"], s["oy"], s["ox"]) for s in r["sources"]}) == 1
        r = rows[f"one-row-{ln}"]
        assert r["sources"][0]["oy"] + r["sources"][0]["gh"] - r["sources"][1]["oy"] == 1
        r = rows[f"one-col-{ln}"]
        assert r["sources"][0]["ox"] + r["sources"][0]["gw"] - r["sources"][1]["ox"] == 1
        # a run boundary of merge_scenes inside a source's edge: the row has more than RUN elements and an edge beyond the first run
        r = rows[f"run-{ln}"]
        per = r["bands"] if r["layout"] == mc.BIP else 1
        assert r["W"] * per > mc.RUN and any(s["ox"] * per < mc.RUN < (s["ox"] + s["gw"]) * per for s in r["sources"])
        assert any(0 < (s["ox"] + s["gw"]) * per - mc.RUN < 64 for s in r["sources"])
        # empty elements in the overlap are filled from the second source: its index appears, and so do both in one pixel's bands
        for kind in ("bmask", "qmask", "planted"):
            r, c = rows[f"empty-{kind}-{ln}"], mc.case(f"empty-{kind}-{ln}")
            first = mc.merge_ref(c["scenes"][:1], c["offsets"][:1], (r["H"], r["W"]), r["nodata"])[0]
            overlap = np.s_[:, 15:50]
            changed = (first[overlap] != c["ref_bip"][overlap])
            assert changed.any() and (c["source"][overlap] == 0).any()
            if kind != "qmask":
                assert (changed.any(-1) & ~changed.all(-1)).any()          # single bands of a pixel, not whole pixels
            else:
                assert (c["source"][overlap] == 1).any()
        c = mc.case(f"all-empty-{ln}")
        assert (c["source"] == mc.NO_SOURCE).all() and (c["ref"] == oc.f32_bits(mc.NODATA)).all()
        r, c = rows[f"n3-dropped-{ln}"], mc.case(f"n3-dropped-{ln}")
        assert min(c["dropped"]) > 0 and len(set(c["dropped"])) == 3
        assert all((g == oc.I32_MIN).any() for g in c["glts"])               # the INT32_MIN entry, in every table
        # NaN wins with nan_is_nodata off and falls through with it on
        r, c = rows[f"nan-falls-{ln}"], mc.case(f"nan-falls-{ln}")
        off = mc.merge_ref(c["scenes"], c["offsets"], (r["H"], r["W"]), r["nodata"], False)[0]
        nan_off, nan_on = np.isnan(off.view(np.float32)), np.isnan(c["ref_bip"].view(np.float32))
        assert nan_off[:, 15:50].any() and (nan_off & ~nan_on)[:, 15:50].any()
        c = mc.case(f"masked-wins-{ln}")
        assert (c["ref"] == oc.f32_bits(-7777.5)).any()
        c = mc.case(f"nan-nodata-{ln}")
        assert (c["ref"] == oc.f32_bits(float("nan"))).any() and (c["source"] != mc.NO_SOURCE).all()
        r, c = rows[f"n1-identity-{ln}"], mc.case(f"n1-identity-{ln}")
        np.testing.assert_array_equal(c["ref_bip"], c["scenes"][0].view(np.uint32))   # one source at offset 0: hsr_ortho_glt's bits
    assert not [n for n in mc.ORTHO_ROWS if mc.ROWS[n]["nan"]]


# ---- the header, the bindings, the package ----------------------------------------------------------------------------------------------
def test_header_bindings_and_constants():
    text = open(os.path.join(ROOT, "include", "hsr_merge.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hsr_\w+)\s*\(", code))
    assert declared == set(nat.MERGE_SIGNATURES)
    lib = nat.load()
    assert all(hasattr(lib, n) for n in declared)
    for n, (_, args) in nat.MERGE_SIGNATURES.items():
        proto = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % n, code, flags=re.S).group(1)
        assert len([a for a in proto.split(",") if a.strip() != "void"]) == len(args), n
    defines = {k: int(v) for k, v in re.findall(r"#define (HSR_MERGE_\w+) (\d+)", text)}
    assert defines == {k: getattr(nat, k) for k in defines} and len(defines) == 4
    assert (mc.MAX_SOURCES, mc.MAX_BANDS, mc.RUN, mc.NO_SOURCE) == (nat.HSR_MERGE_MAX_SOURCES, nat.HSR_MERGE_MAX_BANDS, nat.HSR_MERGE_RUN,
                                                                     nat.HSR_MERGE_NO_SOURCE)
    assert lib.hsr_abi_version() == 5 and lib.hsr_merge_instance_count() == mc.INSTANCE_COUNT
    names = {lib.hsr_merge_instance_name(i).decode() for i in range(mc.INSTANCE_COUNT)}
    assert names == set(mc.all_instances())
    assert lib.hsr_merge_instance_name(mc.INSTANCE_COUNT) is None and lib.hsr_merge_instance_name(-1) is None
    assert "NOT claimed" in text and "per ELEMENT" in text
    mk = open(os.path.join(ROOT, "hyperspectral_super-resolution_amd", "csrc", "Makefile")).read()
    assert "hsr_merge.hip" in mk and "hsr_merge.h" in mk and "hsr_ortho_dev.h" in mk


def test_public_surface():
    for n in ("merge_grid", "merge_scenes", "ortho_merge", "is_adjacent", "merge_emit", "MergeGrid", "MergeOutput", "OrthoMergeOutput"):
        assert n in s2_emit.__all__ and callable(getattr(s2_emit, n)) and getattr(s2_emit, n) is getattr(merge, n)
