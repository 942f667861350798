"""The affine colour family on the host side: include/hsr_color.h against nat.COLOR_SIGNATURES and the library's exports; the
refusals and the launch record's contract, which need no device; hsr_affine_solve_host against np.linalg.lstsq on every solve
row; fixture g17 (the notebook's fit_ot_affine_rgb / apply_affine_rgb) against the NumPy restatements of tests/affine_cases.py;
and what the case tables claim about their rows."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import affine_cases as ac
import s2_emit
from conftest import ROOT, load_golden
from s2_emit import _engine as eng
from s2_emit import _native as nat

LAUNCH_PATH = ("hsr_affine_moments", "hsr_affine_moments_f64", "hsr_affine_reduce_solve", "hsr_affine_apply")
HOST_ONLY = ("hsr_affine_partial_slots", "hsr_affine_partials_bytes", "hsr_affine_solve_host", "hsr_color_last_launch",
             "hsr_color_instance_count", "hsr_color_instance_name")
INVALID = 1


def _header():
    text = open(os.path.join(ROOT, "include", "hsr_color.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    return text, code, comments


# ---- the header, the signature table, the exports ----------------------------------------------------------------------------------
def test_header_signatures_and_exports_agree():
    lib = nat.load()
    text, code, comments = _header()
    declared = sorted(set(re.findall(r"\b(hsr_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(nat.COLOR_SIGNATURES) == sorted(LAUNCH_PATH + HOST_ONLY)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/hsr_color.h but not exported"
        assert getattr(lib, name).argtypes == nat.COLOR_SIGNATURES[name][1] and getattr(lib, name).restype == nat.COLOR_SIGNATURES[name][0]
        assert name in comments, f"{name} is not documented"
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        nargs = 0 if proto.strip() == "void" else proto.count(",") + 1
        assert nargs == len(nat.COLOR_SIGNATURES[name][1]), (name, proto)
        if name in LAUNCH_PATH:
            assert proto.split(",")[-1].strip() == "hsr_stream_t stream", name                 # the stream is the last argument
            assert re.search(r"(color\.py:\d+|notebook|Pairs_EMIT_S2_demo-2)", _doc_of(text, name)), f"{name} cites no reference lines"
        else:
            assert "stream" not in proto
    assert '#include "hsr.h"' in code and "HSR_ABI_VERSION" not in code
    # a family of its own: hsr.h, SIGNATURES, the ABI version and the five other tables are what they were
    hsr_h = open(os.path.join(ROOT, "include", "hsr.h")).read()
    for name in declared:
        assert name not in nat.SIGNATURES and name not in hsr_h, name
    assert lib.hsr_abi_version() == 5 == nat.HSR_ABI_VERSION
    assert (lib.hsr_aux_instance_count(), lib.hsr_scene_instance_count(), lib.hsr_k4_instance_count(), lib.hsr_pairs_instance_count(),
            lib.hsr_ortho_instance_count()) == (32, 20, 31, 12, 6)
    assert nat.COLOR_SIGNATURES["hsr_color_last_launch"] == nat.SIGNATURES["hsr_k4_last_launch"]
    assert nat.COLOR_SIGNATURES["hsr_color_instance_name"] == nat.SIGNATURES["hsr_k4_instance_name"]
    for macro, value in (("HSR_AFFINE_MOMENTS", ac.NMOM), ("HSR_AFFINE_MAX_SLOTS", ac.MAX_SLOTS), ("HSR_AFFINE_SLOT_PIXELS", ac.SLOT_PIXELS)):
        assert re.search(r"#define %s %d\b" % (macro, value), code) and getattr(nat, macro) == value


def _doc_of(text, name):
    """The comment that precedes the declaration of `name`."""
    at = re.search(r"\n(?:int|size_t|const char\*) %s\(" % name, text).start()
    return text[text.rfind("/*", 0, at):at]


def test_sizing_helpers():
    lib = nat.load()
    for npix in (0, 1, ac.SLOT_PIXELS, ac.SLOT_PIXELS + 1, 66001, ac.SLOT_PIXELS * ac.MAX_SLOTS, ac.SLOT_PIXELS * ac.MAX_SLOTS + 1, 1 << 40):
        assert lib.hsr_affine_partial_slots(npix) == ac.slots(npix), npix
    assert ac.slots(0) == 1 and ac.slots(1 << 40) == ac.MAX_SLOTS
    assert lib.hsr_affine_partial_slots(-1) == -1 and b"npix" in lib.hsr_last_error()
    assert lib.hsr_affine_partials_bytes() == ac.MAX_SLOTS * ac.NMOM * 8


# ---- refusals and the record, without a device ---------------------------------------------------------------------------------------
def test_c_abi_refusals_need_no_device():
    lib = nat.load()
    p, null, st = C.c_void_p(64), C.c_void_p(0), C.c_void_p(0)
    lib.hsr_color_last_launch(None, 0)

    def refused(word, fn, *args):
        rc = fn(*args)
        text = lib.hsr_last_error().decode()
        assert rc == INVALID and word in text, (fn.__name__, args, rc, text)

    def moments(x=p, xbs=1, xps=3, y=p, ybs=1, yps=4, npix=10, part=p):
        return lib.hsr_affine_moments, x, xbs, xps, y, ybs, yps, null, npix, null, null, part, None, st

    for kw in (dict(x=null), dict(y=null), dict(part=null)):
        refused("NULL", *moments(**kw))
    refused("npix", *moments(npix=-1))
    for kw in (dict(xps=2), dict(xbs=2, xps=3), dict(xbs=9, xps=1), dict(ybs=1, yps=1), dict(ybs=0, yps=1), dict(xbs=-1, xps=3), dict(yps=-4)):
        refused("strides", *moments(**kw))                                        # rows that overlap
    refused("NULL", lib.hsr_affine_moments_f64, null, 3, p, 3, 10, p, None, st)
    refused("NULL", lib.hsr_affine_moments_f64, p, 3, null, 3, 10, p, None, st)
    refused("NULL", lib.hsr_affine_moments_f64, p, 3, p, 3, 10, null, None, st)
    refused("npix", lib.hsr_affine_moments_f64, p, 3, p, 3, -1, p, None, st)
    refused("overlap", lib.hsr_affine_moments_f64, p, 2, p, 3, 10, p, None, st)
    refused("overlap", lib.hsr_affine_moments_f64, p, 3, p, 0, 10, p, None, st)
    for a in ((null, 1, 0, p, p), (p, 1, 0, null, p), (p, 1, 0, p, null)):
        refused("NULL", lib.hsr_affine_reduce_solve, *a, st)
    for slots in (0, -1, ac.MAX_SLOTS + 1):
        refused("slots", lib.hsr_affine_reduce_solve, p, slots, 0, p, p, st)

    def apply(x=p, xbs=1, xps=3, At=p, npix=10, clip=1, out=p, obs=1, ops=4):
        return lib.hsr_affine_apply, x, xbs, xps, null, At, npix, null, clip, out, obs, ops, st

    for kw in (dict(x=null), dict(At=null), dict(out=null)):
        refused("NULL", *apply(**kw))
    refused("npix", *apply(npix=-1))
    for clip in (-1, 3):
        refused("clip_mode", *apply(clip=clip))
    for kw in (dict(xps=2), dict(obs=1, ops=2), dict(obs=9, ops=1), dict(xbs=3, xps=3)):
        refused("strides", *apply(**kw))
    assert lib.hsr_affine_apply(p, 1, 3, null, p, 0, null, 1, p, 1, 3, st) == 0          # npix == 0: succeeds, launches nothing
    assert lib.hsr_affine_solve_host(None, 0, (C.c_double * 12)()) == INVALID and b"NULL" in lib.hsr_last_error()
    assert lib.hsr_affine_solve_host((C.c_double * 22)(), 0, None) == INVALID
    buf = C.create_string_buffer(64)
    assert lib.hsr_color_last_launch(buf, 64) == 0 and buf.value == b""      # refused calls (and npix == 0) leave no record


def test_instance_table_and_record_contract():
    lib = nat.load()
    n = lib.hsr_color_instance_count()
    table = [lib.hsr_color_instance_name(i).decode() for i in range(n)]
    assert n == 20 == len(set(table)) and table == ac.all_instances()                     # unique, and in this order
    for bad in (-1, n):
        assert lib.hsr_color_instance_name(bad) is None
        assert b"hsr_color_instance_name" in lib.hsr_last_error() and str(bad).encode() in lib.hsr_last_error()
    _, _, comments = _header()
    assert "hsr_color_instance_count = 20" in comments and "8 most recent" in comments and "hsr_aux_last_launch" in comments
    buf = C.create_string_buffer(64)
    buf.value = b"junk"
    lib.hsr_color_last_launch(None, 0)
    assert lib.hsr_color_last_launch(buf, 0) == 0 and buf.value == b"junk"
    assert lib.hsr_color_last_launch(buf, 64) == 0 and buf.value == b""
    assert lib.hsr_color_last_launch(None, 64) == 0


def test_public_surface():
    assert s2_emit.__all__[13:18] == ["fit_ot_poly_rgb", "apply_poly_rgb", "fit_ot_affine_rgb", "apply_affine_rgb", "fit_affine_rgb"]
    sig = inspect.signature(s2_emit.fit_ot_affine_rgb)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [
        ("src_rgb", inspect.Parameter.empty), ("ref_rgb", inspect.Parameter.empty), ("mask", inspect.Parameter.empty),
        ("n_samples", 5000), ("reg", 0.05), ("numItermax", 300), ("stopThr", 1e-6), ("seed", 0)]
    sig = inspect.signature(s2_emit.apply_affine_rgb)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [("rgb", inspect.Parameter.empty), ("A", inspect.Parameter.empty),
                                                                   ("t", inspect.Parameter.empty), ("mask", None)]
    sig = inspect.signature(s2_emit.fit_affine_rgb)
    assert [(k, v.default) for k, v in sig.parameters.items()][3:] == [("min_count", 200), ("lohi_src", None), ("lohi_ref", None)]
    mp = list(inspect.signature(s2_emit.match_pair).parameters.items())
    assert mp[-1][0] == "model" and mp[-1][1].default == "poly" and mp[-2][0] == "as_numpy"
    with pytest.raises(ValueError, match="model"):
        s2_emit.match_pair(None, None, {}, None, None, model="cubic")                        # refused before anything else


# ---- the solve's host twin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ac.SOLVE_ROWS))
def test_solve_host_against_lstsq(name):
    r, c = ac.SOLVE_ROWS[name], ac.solve_case(name)
    At = eng.affine_solve_host(c["mom"].astype(np.float64), r["min_count"])
    if c["identity"]:
        assert np.array_equal(At, np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])) and np.array_equal(c["W"][:3], np.eye(3))
        return
    diff = ac.grid_diff(At, c["W"])
    print(f"{name}: diff {diff:.3g}, kappa {c['kappa']:.3g}, ratio {diff * 64 / c['bar']:.2f} of 64")
    assert diff <= c["bar"], (name, diff, c["bar"])


@pytest.mark.parametrize("name", list(ac.SOLVE_ROWS))
def test_solve_rows_claims(name):
    """Rank, count against min_count, and the condition that keeps a row out of the zone where lstsq keeps a direction that
    rounded moments cannot resolve: every eigenvalue of the Gram is >= 1e-9 of the largest or <= EPS of it."""
    r, c = ac.SOLVE_ROWS[name], ac.solve_case(name)
    assert len(c["xs"]) == r["n"] == int(c["mom"][9]) and c["identity"] == (r["n"] < max(r["min_count"], 1))
    if r["n"] == 0:
        assert not c["mom"].any()
        return
    ev = ac.spectrum(c["xs"])
    rel = ev / ev.max()
    assert ((rel >= 1e-9) | (rel <= ac.EPS)).all(), rel
    assert int((rel >= 1e-9).sum()) == r["rank"] == len(ac.kept(ev, r["n"])), rel
    assert np.linalg.matrix_rank(np.concatenate([c["xs"], np.ones((r["n"], 1))], axis=1)) == r["rank"]
    assert (c["xs"] == c["xs"].astype(np.float32)).all()                                     # float32-valued, as the image kernels see them
    if name == "narrow":
        assert c["kappa"] > 1e5 and c["xs"].min() >= 0.79 and c["xs"].max() <= 0.81
    if r["min_count"] > 1:
        assert r["n"] in (r["min_count"] - 1, r["min_count"])


def test_solve_rows_cover_the_classes():
    R = ac.SOLVE_ROWS
    assert {r["rank"] for r in R.values()} == {0, 1, 2, 3, 4} and {r["n"] for r in R.values()} >= {0, 1, 2, 3, ac.MIN_COUNT - 1, ac.MIN_COUNT}
    assert {r["kind"] for r in R.values()} == {"full", "equal-channels", "gray", "constant", "narrow"}


# ---- fixture g17 ----------------------------------------------------------------------------------------------------------------------
def test_g17_against_the_numpy_restatements():
    g = load_golden("g17_affine")
    src, ref, mask = g["src"], g["ref"], g["mask"]
    assert src.shape == ref.shape == (40, 36, 3) and src.dtype == np.float32 and mask.dtype == np.bool_ and 0.8 < mask.mean() < 0.9
    assert np.isnan(src[mask]).any() and np.isinf(src[mask]).any() and (src[np.isfinite(src)] < 0).any() and (src[np.isfinite(src)] > 1).any()
    assert np.array_equal(g["A_one"], np.eye(3)) and not g["t_one"].any() and g["mask_one"].sum() == 1
    rows = src.reshape(-1, 3)
    x64 = np.abs(np.nan_to_num(rows.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0))
    for tag, At in (("fit", np.concatenate([g["A"].reshape(-1), g["t"]])), ("hand", g["At_hand"])):
        for mtag, m in (("mask", mask.reshape(-1)), ("nomask", None)):
            got = ac.apply_ref(rows, At, m, None, 1).reshape(40, 36, 3)
            want = g[f"out_{tag}_{mtag}"]
            assert want.dtype == np.float32 and np.array_equal(np.isnan(got), np.isnan(want)), (tag, mtag)
            # the notebook's matmul may add in another order: two float32 roundings of values in [0, 1] + the float64 reordering
            bound = 2.0 ** -24 + 8 * ac.EPS * (x64 @ np.abs(At[:9].reshape(3, 3)) + np.abs(At[9:])).reshape(40, 36, 3)
            ok = ~np.isnan(want)
            assert (np.abs(got.astype(np.float64) - want)[ok] <= bound[ok]).all(), (tag, mtag)
            if m is not None:
                assert np.array_equal(want[~mask].view(np.uint32), src[~mask].view(np.uint32))     # outside: untouched, unclipped
    assert (g["At_hand"] == 0).any() and np.isnan(g["out_hand_mask"][np.isinf(src).any(axis=2) & mask]).any()      # inf * 0
    # the gray image: lstsq's minimum-norm solution from the host twin on long-double moments
    gray = np.repeat(src[..., :1], 3, axis=2).reshape(-1, 3)
    ok = ac.usable(gray, ref.reshape(-1, 3), mask.reshape(-1))
    xs, ys = gray[ok].astype(np.float64), ref.reshape(-1, 3)[ok].astype(np.float64)
    np.testing.assert_allclose(ac.lstsq_ref(xs, ys, 0), g["W_gray"], rtol=0, atol=1e-12)
    mom, _ = ac.moments_ld(xs, ys)
    bar, kappa = ac.solve_bar(xs, g["W_gray"])
    assert len(ac.kept(ac.spectrum(xs), len(xs))) == 2
    assert ac.grid_diff(eng.affine_solve_host(mom.astype(np.float64), 0), g["W_gray"]) <= bar


# ---- the moment and apply tables --------------------------------------------------------------------------------------------------------
def test_rows_claim_every_instance():
    lib = nat.load()
    table = {lib.hsr_color_instance_name(i).decode() for i in range(lib.hsr_color_instance_count())}
    claimed = ({ac.moments_instance(r) for r in ac.MOMENT_ROWS.values()} | {ac.apply_instance(r) for r in ac.APPLY_ROWS.values()}
               | {"affine_moments_f64_kernel", "affine_reduce_solve_kernel"})
    assert claimed == table, (sorted(table - claimed), sorted(claimed - table))
    assert (ac.mode(ac.PADDED, 0), ac.mode(ac.PACKED, 0), ac.mode(ac.PLANAR, 0)) == (1, 2, 0)
    assert all(ac.mode(l, off) == 0 for l in (ac.PADDED, ac.PACKED, ac.PLANAR) for off in (4, 8, 12))


def test_rows_cover_the_bounds():
    for table, key in ((ac.MOMENT_ROWS, "y"), (ac.APPLY_ROWS, "out")):
        sizes = {r["npix"] for r in table.values()}
        assert sizes >= {1, ac.GROUP - 1, ac.GROUP, ac.GROUP + 1, ac.PASS - 1, ac.PASS, ac.PASS + 1}
        assert max(sizes) <= 70000
        for side in ("x", key):
            assert {(r[side][0], r[side][1] % 16 == 0) for r in table.values()} == {(l, a) for l in (ac.PADDED, ac.PACKED, ac.PLANAR)
                                                                                      for a in (True, False)}
        assert {r["mask"] for r in table.values()} == {"none", "all", "part", "clear"}
    M = ac.MOMENT_ROWS
    assert {r["npix"] for r in M.values()} >= {ac.SLOT_PIXELS - 1, ac.SLOT_PIXELS, ac.SLOT_PIXELS + 1}
    assert {ac.slots(r["npix"]) for r in M.values()} >= {1, 2, 3, 33}
    ragged = [r["npix"] for r in M.values() if ac.slots(r["npix"]) > 1 and r["npix"] % ac.slot_rows(r["npix"], ac.slots(r["npix"]))]
    assert ragged and any(n % ac.GROUP for n in ragged)
    assert {r["bad"] for r in M.values()} == {"none", "x", "y", "both"}
    assert any(r["lohi_x"] is not None and r["lohi_y"] is not None for r in M.values())
    assert any(r["lohi_x"] is ac.LOHI_FLAT for r in M.values()) and (ac.LOHI_FLAT[:, 0] == ac.LOHI_FLAT[:, 1]).any()
    A = ac.APPLY_ROWS
    assert {(r["mask"] != "none", r["clip"]) for r in A.values()} == {(m, c) for m in (False, True) for c in (0, 1, 2)}
    assert any(r["lohi"] is not None for r in A.values()) and any(r["lohi"] is None for r in A.values())
    assert {(r["npix"] + ac.PASS - 1) // ac.PASS for r in A.values()} >= {1, 2, 3, 65}


@pytest.mark.parametrize("name", list(ac.MOMENT_ROWS))
def test_moment_row_references(name):
    r, c = ac.MOMENT_ROWS[name], ac.moment_case(name)
    assert c["ref"][9] == c["n"] == len(c["xs"])
    x_bad, y_bad = ~np.isfinite(c["x"]).all(axis=1), ~np.isfinite(c["y"]).all(axis=1)
    if r["npix"] >= 100:
        assert x_bad.any() == (r["bad"] in ("x", "both")) and y_bad.any() == (r["bad"] in ("y", "both"))
        if r["bad"] != "none":
            both = np.concatenate([c["x"][x_bad].reshape(-1), c["y"][y_bad].reshape(-1)])
            assert np.isnan(both).any() and (np.isposinf(both).any() or np.isneginf(both).any())
        if r["mask"] == "part":
            assert 0 < c["n"] < r["npix"] and (c["mask"] == 0).any() and (c["mask"] > 1).any()
    if r["mask"] == "clear":
        assert c["n"] == 0 and not c["ref"].any()
    if r["lohi_x"] is not None and r["npix"] >= 100:
        assert c["xs"].min() == 0.0 and c["xs"].max() == 1.0                                  # the clip acts on both sides
    if r["lohi_x"] is ac.LOHI_FLAT:
        assert set(np.unique(c["xs"][:, 1])) <= {0.0, 1.0}                                    # hi == lo: the 1e-12 decides


@pytest.mark.parametrize("name", list(ac.APPLY_ROWS))
def test_apply_row_references(name):
    r, c = ac.APPLY_ROWS[name], ac.apply_case(name)
    ref, x = c["ref"], c["x"]
    assert ref.shape == x.shape and ref.dtype == np.float32
    m = np.ones(len(x), bool) if c["mask"] is None else c["mask"] != 0
    fin = np.isfinite(ref)
    if r["clip"] == 2:
        assert ref[fin].min() >= 0 and ref[fin].max() <= 1
    if r["clip"] == 1 and m.any():
        assert ref[m][np.isfinite(ref[m])].min() >= 0 and ref[m][np.isfinite(ref[m])].max() <= 1
    if r["clip"] != 2 and r["lohi"] is None and not m.all():
        np.testing.assert_array_equal(ref[~m].view(np.uint32), x[~m].view(np.uint32))       # passes through
    if r["At"] is ac.AT_WIDE and r["npix"] >= 100 and m.any():
        raw = ac.apply_ref(x, r["At"], c["mask"], r["lohi"], 0)[m]
        assert (raw[np.isfinite(raw)] < 0).any() and (raw[np.isfinite(raw)] > 1).any()          # out of range on both sides
    if r["At"] is ac.AT_ZEROS:
        inf_rows = np.isinf(x).any(axis=1)
        assert inf_rows.any() and np.isnan(ref[inf_rows]).any() and (r["At"] == 0).any()          # inf * 0
    if r["bad"] and r["npix"] >= 100:
        assert np.isnan(ref).any()
