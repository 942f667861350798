"""s2_emit.ortho and hsr_ortho_glt on the host side: fixture g16 (the reference's apply_glt) against the NumPy reference of
tests/ortho_cases.py bit for bit; the refusals of _plan_ortho and of the C entry point, which need no device; glt_from_xy and
quality_mask against the fixture; the ortho launch record's table and exports; and what the case table claims about its rows."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ortho_cases as oc
import s2_emit
from conftest import load_golden
from s2_emit import ortho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("hsr_ortho_glt", "hsr_ortho_last_launch", "hsr_ortho_instance_count", "hsr_ortho_instance_name")


def _lib():
    from s2_emit import _native as nat
    return nat.load()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- fixture g16 --------------------------------------------------------------------------------------------------------------------
def test_g16_against_the_numpy_reference():
    g = load_golden("g16_ortho")
    s285, s3, q, b = g["swath285"], g["swath3"], g["qmask"], g["bmask"]
    assert s285.shape == (6, 5, 285) and s3.shape == (6, 5, 3) and b.shape == (6, 5, 36) and g["glt_mixed"].shape == (9, 11, 2)
    for tag, qm, bm in (("plain", None, None), ("q", q, None), ("b", None, b), ("qb", q, b)):
        ref, dropped = oc.ortho_ref(s285, g["glt_mixed"], qmask=qm, bmask=bm)
        np.testing.assert_array_equal(ref, _bits(g[f"out285_{tag}"]), err_msg=tag)
        assert dropped == 0
    np.testing.assert_array_equal(oc.ortho_ref(s3, g["glt_mixed"])[0], _bits(g["out3_plain"]))
    np.testing.assert_array_equal(oc.ortho_ref(s3, g["glt_mixed"], qmask=q)[0], _bits(g["out3_q"]))
    ref, dropped = oc.ortho_ref(s285, g["glt_nodata"])
    np.testing.assert_array_equal(ref, _bits(g["out285_nodata"]))
    assert dropped == 0 and (ref == oc.f32_bits(-9999.0)).all()
    ref, dropped = oc.ortho_ref(s285, g["glt_valid"])
    np.testing.assert_array_equal(ref, _bits(g["out285_valid"]))
    assert dropped == 0
    ref, dropped = oc.ortho_ref(s285, g["glt_drop"])
    np.testing.assert_array_equal(ref, _bits(g["out285_drop"]))
    assert dropped == int(g["dropped_drop"]) == 10
    for k, win in enumerate(g["windows"]):
        ref, dropped = oc.ortho_ref(s285, g["glt_drop"], window=tuple(int(v) for v in win), qmask=q, bmask=b)
        np.testing.assert_array_equal(ref, _bits(g[f"out285_win{k}"]))
        assert dropped == int(g[f"dropped_win{k}"]) > 0
    # what the fixture holds: payloads and signed zeros survive, == 1 alone masks, the pad bits mask nothing
    plain = _bits(g["out285_plain"])
    for s in (0x7fc12345, 0xffc00001, 0x80000000, 1, 0x7f800000):
        assert (plain == s).any(), hex(s)
    glt = g["glt_mixed"].astype(np.int64)
    valid = (glt != 0).all(axis=-1)
    qv = np.zeros(valid.shape, np.uint8)
    qv[valid] = q[glt[valid][:, 1] - 1, glt[valid][:, 0] - 1]
    qout = _bits(g["out285_q"])
    assert set(np.unique(qv[valid])) == {0, 1, 2, 255}
    assert (qout[valid & (qv == 1)] == oc.f32_bits(-9999.0)).all()
    np.testing.assert_array_equal(qout[valid & (qv != 1)], plain[valid & (qv != 1)])
    every = (glt[..., 0] == 4) & (glt[..., 1] == 6)                       # swath pixel (5, 3): every bit of its mask is set
    diff = _bits(g["out285_b"]) != plain
    changed = diff[~every].any(axis=0)
    assert set(np.flatnonzero(changed)) <= {0, 7, 8, 15, 283, 284} and changed[[0, 7, 8, 15, 283, 284]].all()
    assert every.any() and (_bits(g["out285_b"])[every] == oc.f32_bits(-9999.0)).all()
    assert (np.unpackbits(b, axis=-1)[:, :, 285:] == 1).any()


def test_glt_from_xy_and_quality_mask_against_g16():
    g = load_golden("g16_ortho")
    got = s2_emit.glt_from_xy(g["glt_x"], g["glt_y"])
    assert got.dtype == np.int32 and got.shape == (9, 11, 2)
    np.testing.assert_array_equal(got, g["glt_mixed"])
    other = s2_emit.glt_from_xy(g["glt_x"], g["glt_y"], nodata=-5)
    assert ((other == -5) == np.isnan(np.stack([g["glt_x"], g["glt_y"]], axis=-1))).all()
    np.testing.assert_array_equal(s2_emit.glt_from_xy(g["glt_mixed"][..., 0], g["glt_mixed"][..., 1]), g["glt_mixed"])   # integers
    with pytest.raises(ValueError):
        s2_emit.glt_from_xy(g["glt_x"], g["glt_y"][:, :5])
    import torch
    t = s2_emit.glt_from_xy(torch.from_numpy(g["glt_x"]), torch.from_numpy(g["glt_y"]))
    assert t.dtype == torch.int32 and np.array_equal(t.numpy(), g["glt_mixed"])
    qm = s2_emit.quality_mask(g["mask_cube"], [int(v) for v in g["quality_bands"]])
    assert qm.dtype == g["qmask_cube"].dtype
    np.testing.assert_array_equal(qm, g["qmask_cube"])
    assert set(np.unique(qm)) == {0.0, 1.0}
    np.testing.assert_array_equal(s2_emit.quality_mask(torch.from_numpy(g["mask_cube"]), [0, 1, 3, 4]).numpy(), g["qmask_cube"])
    for bad in ([5], [0, 6], [5, 6]):
        with pytest.raises(AttributeError):
            s2_emit.quality_mask(g["mask_cube"], bad)


# ---- _plan_ortho --------------------------------------------------------------------------------------------------------------------
def test_plan_ortho():
    swath, glt = np.zeros((6, 5, 285), np.float32), np.zeros((9, 11, 2), np.int32)
    p = ortho._plan_ortho(swath, glt)
    assert (p.rows, p.cols, p.bands, p.glt_h, p.glt_w) == (6, 5, 285, 9, 11) and p.window == (0, 0, 9, 11)
    assert p.layout == "bsq" and p.out_shape == (285, 9, 11) and p.bmask_bytes == 0 and (p.fill, p.masked, p.nodata) == (-9999.0, -9999.0, 0)
    p = ortho._plan_ortho(swath, glt.astype(np.int64), window=(1, 2, 5, 7), layout="bip", band_mask=np.zeros((6, 5, 40), np.uint8))
    assert p.out_shape == (5, 7, 285) and p.bmask_bytes == 40 and p.window == (1, 2, 5, 7)
    assert ortho._plan_ortho(swath[:, :, 0], glt, layout="bip").out_shape == (9, 11, 1)          # 2-d: one band
    assert ortho._plan_ortho(swath.astype(np.float64), glt, qmask=np.zeros((6, 5), np.float64)).bands == 285
    assert ortho._plan_ortho(np.zeros((2, 2, ortho.MAX_BANDS), np.float32), glt).bands == oc.MAX_BANDS == ortho.MAX_BANDS

    def refused(text, *a, **kw):
        with pytest.raises(ValueError, match=text):
            ortho._plan_ortho(*a, **kw)

    refused("swath", [[1.0]], glt)
    refused("swath", np.zeros((6, 5, 2, 2), np.float32), glt)
    refused("swath", np.zeros((0, 5, 3), np.float32), glt)
    refused("swath is bool", np.zeros((6, 5, 3), bool), glt)
    refused("bands", np.zeros((2, 2, ortho.MAX_BANDS + 1), np.float32), glt)
    refused("glt", swath, np.zeros((9, 11), np.int32))
    refused("glt", swath, np.zeros((9, 11, 3), np.int32))
    refused("integer", swath, np.zeros((9, 11, 2), np.float32))
    for win in ((0, 0, 10, 11), (0, 0, 9, 12), (-1, 0, 2, 2), (0, -1, 2, 2), (8, 0, 2, 1), (0, 10, 1, 2), (0, 0, 0, 1), (0, 0, 1, 0)):
        refused("leaves", swath, glt, window=win)
    refused("window", swath, glt, window=(0, 0, 9))
    refused("window", swath, glt, window=(0, 0, 9.0, 11))
    refused("window", swath, glt, window=5)
    refused("layout", swath, glt, layout="bil")
    refused("qmask", swath, glt, qmask=np.zeros((5, 6), np.uint8))
    refused("band_mask", swath, glt, band_mask=np.zeros((6, 5, 36), np.int8))
    refused("band_mask", swath, glt, band_mask=np.zeros((6, 5), np.uint8))
    refused("band_mask", swath, glt, band_mask=np.zeros((6, 4, 36), np.uint8))
    refused("36", swath, glt, band_mask=np.zeros((6, 5, 35), np.uint8))
    refused("numbers", swath, glt, fill_value="x")
    refused("glt_nodata", swath, glt, glt_nodata=1 << 31)
    refused("glt_nodata", swath, glt, glt_nodata=0.0)
    refused("out", swath, glt, out=np.zeros((285, 9, 11), np.float32))                         # not a device tensor
    import torch
    refused("out", swath, glt, out=torch.zeros((9, 11, 285)))                                   # the bip shape for a bsq call
    refused("out", swath, glt, out=torch.zeros((285, 9, 11), dtype=torch.float64))
    refused("contiguous", swath, glt, layout="bip", out=torch.zeros((285, 11, 9)).permute(2, 1, 0))
    assert ortho._plan_ortho(swath, glt, out=torch.zeros((285, 9, 11))).out_shape == (285, 9, 11)


def test_public_surface():
    assert s2_emit.__all__[-5:] == ["apply_glt", "ortho_scene", "glt_from_xy", "quality_mask", "OrthoOutput"]
    import inspect
    sig = inspect.signature(s2_emit.apply_glt)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [("ds_array", inspect.Parameter.empty), ("glt_array", inspect.Parameter.empty),
                                                                   ("fill_value", -9999), ("GLT_NODATA_VALUE", 0)]
    sig = inspect.signature(s2_emit.ortho_scene)
    assert [k for k, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY] == ["qmask", "band_mask", "window", "layout", "fill_value",
                                                                                 "masked_value", "glt_nodata", "out"]
    assert sig.parameters["layout"].default == "bsq" and sig.parameters["masked_value"].default == -9999.0
    assert s2_emit.OrthoOutput._fields == ("scene", "dropped", "window")
    for fn in (s2_emit.apply_glt, s2_emit.ortho_scene):
        assert "NOT" in fn.__doc__ or "not on" in fn.__doc__                                 # says what the result is not
    assert "gdalwarp" in ortho.__doc__


# ---- the C entry point's refusals ---------------------------------------------------------------------------------------------------
def test_c_abi_refusals_need_no_device():
    lib = _lib()
    p, null, st = C.c_void_p(64), C.c_void_p(0), C.c_void_p(0)
    lib.hsr_ortho_last_launch(None, 0)

    def call(swath=p, rows=6, cols=5, bands=285, glt=p, gh=9, gw=11, nodata=0, r0=0, c0=0, h=9, w=11, q=null, b=null, bbytes=0,
             layout=0, out=p, dropped=null):
        rc = lib.hsr_ortho_glt(swath, rows, cols, bands, glt, gh, gw, nodata, r0, c0, h, w, q, b, bbytes, -9999.0, -9999.0, layout, out,
                               dropped, st)
        return rc, lib.hsr_last_error().decode()

    INVALID, UNSUPPORTED = 1, 2
    for kw in (dict(swath=null), dict(glt=null), dict(out=null)):
        rc, text = call(**kw)
        assert rc == INVALID and "NULL" in text, (kw, rc, text)
    for kw in (dict(rows=0), dict(cols=-1), dict(bands=0), dict(gh=0), dict(gw=0), dict(h=0), dict(w=-3)):
        rc, text = call(**kw)
        assert rc == INVALID and "bad shape" in text, (kw, rc, text)
    for kw in (dict(r0=-1), dict(c0=-1), dict(r0=1), dict(c0=1), dict(h=10), dict(w=12), dict(r0=I32, h=1), dict(c0=I32, w=1)):
        rc, text = call(**kw)
        assert rc == INVALID and "leaves" in text, (kw, rc, text)
    rc, text = call(b=p, bbytes=35)
    assert rc == INVALID and "bmask_bytes=35" in text
    rc, text = call(b=p, bbytes=0, bands=1)
    assert rc == INVALID and "bmask_bytes" in text
    for layout in (-1, 2):
        rc, text = call(layout=layout)
        assert rc == INVALID and "layout" in text
    rc, text = call(bands=oc.MAX_BANDS + 1)
    assert rc == UNSUPPORTED and str(oc.MAX_BANDS) in text
    rc, text = call(rows=1 << 16, cols=1 << 15)
    assert rc == UNSUPPORTED and "swath" in text
    rc, text = call(gh=1 << 16, gw=1 << 15, h=1 << 16, w=1 << 15)
    assert rc == UNSUPPORTED and "window" in text
    buf = C.create_string_buffer(64)
    assert lib.hsr_ortho_last_launch(buf, 64) == 0 and buf.value == b""      # a refused call leaves no record


I32 = (1 << 31) - 1


# ---- the record and its exports -----------------------------------------------------------------------------------------------------
def test_instance_table_and_exports():
    from s2_emit import _native as nat
    lib = nat.load()
    n = lib.hsr_ortho_instance_count()
    table = [lib.hsr_ortho_instance_name(i).decode() for i in range(n)]
    assert n == oc.INSTANCE_COUNT == len(set(table))
    assert sorted(oc.all_instances()) == sorted(table)
    for bad in (-1, n):
        assert lib.hsr_ortho_instance_name(bad) is None
        assert b"hsr_ortho_instance_name" in lib.hsr_last_error() and str(bad).encode() in lib.hsr_last_error()
    text = open(os.path.join(ROOT, "include", "hsr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    for name in EXPORTS:
        assert hasattr(lib, name) and name in nat.SIGNATURES and name in comments
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/hsr.h"
    assert nat.SIGNATURES["hsr_ortho_last_launch"] == nat.SIGNATURES["hsr_scene_last_launch"]
    assert nat.SIGNATURES["hsr_ortho_instance_name"] == nat.SIGNATURES["hsr_scene_instance_name"]
    # a table of its own: the ABI version and the four other tables are what they were
    assert lib.hsr_abi_version() == 5 == nat.HSR_ABI_VERSION
    assert (lib.hsr_aux_instance_count(), lib.hsr_scene_instance_count(), lib.hsr_k4_instance_count(),
            lib.hsr_pairs_instance_count()) == (32, 20, 31, 12)
    buf = C.create_string_buffer(64)
    buf.value = b"junk"
    lib.hsr_ortho_last_launch(None, 0)
    assert lib.hsr_ortho_last_launch(buf, 0) == 0 and buf.value == b"junk"
    assert lib.hsr_ortho_last_launch(buf, 64) == 0 and buf.value == b""


# ---- the case table -----------------------------------------------------------------------------------------------------------------
def test_rows_claim_every_instance():
    lib = _lib()
    table = {lib.hsr_ortho_instance_name(i).decode() for i in range(lib.hsr_ortho_instance_count())}
    claimed = {oc.row_instance(n) for n in oc.ROWS}
    assert claimed == table, (sorted(table - claimed), sorted(claimed - table))
    for name, r in oc.ROWS.items():                                       # the predicate, restated on the row
        mask = r["q"] or r["bbytes"] > 0
        want = (f"ortho_bip_kernel<{str(mask).lower()}, "
                f"{str(r['bands'] % 4 == 0 and r['swath_off'] % 16 == 0 and r['out_off'] % 16 == 0).lower()}>"
                if r["layout"] == oc.BIP else f"ortho_bsq_kernel<{str(mask).lower()}>")
        assert oc.row_instance(name) == want, name


def test_rows_cover_the_shapes():
    R = oc.ROWS
    assert (oc.PX, oc.PX_WAVE, oc.AHEAD, oc.PX_WAVE_BSQ) == (64, 16, 4, 8)
    for layout in (oc.BIP, oc.BSQ):
        rows = [r for r in R.values() if r["layout"] == layout]
        assert {(r["bands"], r["window"][3]) for r in rows} >= {(b, w) for b in oc.BANDS for w in oc.WIDTHS}
        assert {r["window"][2] for r in rows} >= {1, 3}
        assert {(r["q"], r["bbytes"] > 0) for r in rows if r["bands"] == 285} == {(a, b) for a in (False, True) for b in (False, True)}
        assert {r["grid"] for r in rows} == {"mixed", "nodata", "valid", "dropped"}
        assert any(r["window"][1] % oc.PX and r["window"][3] > 1 for r in rows) and any(r["window"][2:] == (1, 1) for r in rows)
        assert any(not r["count"] for r in rows)
        assert any(r["bbytes"] > (r["bands"] + 7) // 8 for r in rows) and any(r["bbytes"] == 36 and r["bands"] == 285 for r in rows)
        assert {r["swath_off"] % 16 for r in rows} == {0, 4, 8, 12} == {r["out_off"] % 16 for r in rows}
    vec4 = {(r["swath_off"], r["out_off"]) for n, r in R.items() if n.startswith("align-b4-bip")}
    assert vec4 == {(s, o) for s in (0, 4, 8, 12) for o in (0, 4, 8, 12)}
    assert oc.row_instance("align-b4-bip-s0-o0").endswith("true>") and oc.row_instance("align-b64-bip-16-on").endswith("true, true>")
    assert all(oc.row_instance(f"align-b4-bip-s{s}-o{o}").endswith("false>") for s in (0, 4, 8, 12) for o in (0, 4, 8, 12) if s or o)


@pytest.mark.parametrize("name", list(oc.ROWS))
def test_row_references(name):
    """What a row is there for shows in its reference."""
    r, c = oc.ROWS[name], oc.case(name)
    _, _, h, w = r["window"]
    ref, bip = c["ref"], c["ref_bip"]
    assert ref.shape == ((h, w, r["bands"]) if r["layout"] == oc.BIP else (r["bands"], h, w))
    np.testing.assert_array_equal(ref if r["layout"] == oc.BIP else ref.transpose(1, 2, 0), bip)       # bsq = bip permuted
    assert c["glt"].shape == (r["gh"], r["gw"], 2) and c["glt"].dtype == np.int32
    fill = oc.f32_bits(r["fill"])
    allfill = (bip == fill).all(axis=-1)
    if r["grid"] == "nodata":
        assert c["dropped"] == 0 and allfill.all()
    elif r["grid"] == "dropped":
        assert c["dropped"] == h * w and allfill.all()
    elif r["grid"] == "valid":
        assert c["dropped"] == 0 and (r["bands"] < 3 or not allfill.any())
    elif h * w >= 60:
        assert 0 < c["dropped"] < h * w and allfill.any() and not allfill.all()
        g = c["glt"]
        assert (g == oc.I32_MIN).any() and (g == oc.I32_MAX).any() and (g < 0).any()
        nd = g == r["nodata"]
        assert (nd[..., 0] & ~nd[..., 1]).any() and (~nd[..., 0] & nd[..., 1]).any() and (nd[..., 0] & nd[..., 1]).any()
    if r["bbytes"]:
        un = np.unpackbits(c["bmask"], axis=-1)
        assert c["bmask"].shape[2] == r["bbytes"] and (r["bbytes"] * 8 == r["bands"] or (un[:, :, r["bands"]:] == 1).any())
    if r["q"]:
        assert set(np.unique(c["qmask"])) == {0, 1, 2, 255}
    if name.startswith("nodata-7"):
        assert (c["glt"] == 0).any() and (c["glt"] == 7).any()
