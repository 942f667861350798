"""Runners of the kernel families' case rows: a row and its case (inputs and reference, from the family's *_cases.py) marshalled
into one C-ABI call on guarded buffers (Buf of gpu_harness.py).  Every runner takes (torch, row, case, log): `log` is the calling
module's LaunchLog, which checks the launch record against the instance the family's mirror expects and collects the names seen.
A runner checks what holds for every row - nothing written outside a payload, inputs as they were, paddings and gaps as they were -
and returns the outputs; comparing them with the reference is the caller's.  Not a test module.

Used by the instance modules (tests/test_gpu_{scene,ortho,color,coreg}_instances.py) with their tables' named rows and their own
LaunchLog, and by tests/test_gpu_family_sweeps.py and tools/dbg/stress_families.py with the drawn rows of tests/sweep_cases.py: the
judge_* functions at the end hold a drawn row to what the instance modules assert of a table row."""
import ctypes as C

import numpy as np

import affine_cases as ac
import coreg_cases as cc
import ortho_cases as oc
import scene_cases as sc
from gpu_harness import FILL, SENT16, SENT32, Buf, bits_equal, same_bits
from gpu_harness import lib as _lib, stream as _stream

SENT64 = np.frombuffer(bytes([FILL] * 8), np.uint64)[0]


def untouched(buf, back):
    np.testing.assert_array_equal(buf.get(np.uint8), np.ascontiguousarray(back).reshape(-1).view(np.uint8))


# ---- ortho -------------------------------------------------------------------------------------------------------------------------
def run_ortho(torch, r, c, log, layout=None, count=None):
    """The ortho row `r` (optionally in the other layout) -> (output bits in that layout's shape, dropped or None)."""
    layout = r["layout"] if layout is None else layout
    count = r["count"] if count is None else count
    swath, glt = c["swath"], c["glt"]
    r0, c0, h, w = r["window"]
    sb = Buf(torch, swath.nbytes, r["swath_off"], swath)
    gb = Buf(torch, glt.nbytes, 0, glt)
    qb = Buf(torch, c["qmask"].nbytes, 0, c["qmask"]) if r["q"] else None
    bb = Buf(torch, c["bmask"].nbytes, 0, c["bmask"]) if r["bbytes"] else None
    db = Buf(torch, 8, 8) if count else None                              # holds the sentinel: the call has to zero it
    ob = Buf(torch, h * w * r["bands"] * 4, r["out_off"])
    expect = oc.instance(layout, r["bands"], r["q"] or r["bbytes"] > 0, r["swath_off"], r["out_off"])
    log.call(expect, _lib().hsr_ortho_glt, sb.ptr, r["rows"], r["cols"], r["bands"], gb.ptr, r["gh"], r["gw"], r["nodata"], r0, c0, h, w,
             qb.ptr if qb else None, bb.ptr if bb else None, r["bbytes"], r["fill"], r["masked"], layout, ob.ptr,
             db.ptr if db else None, _stream(torch))
    got = ob.get(np.uint32).reshape((h, w, r["bands"]) if layout == oc.BIP else (r["bands"], h, w))
    for b in (sb, gb, qb, bb):                                            # the inputs and their guards are as they were
        if b is not None:
            b.get(np.uint8)
    np.testing.assert_array_equal(sb.get(np.float32).view(np.uint32), swath.view(np.uint32).reshape(-1))
    return got, (int(db.get(np.int64)[0]) if db else None)


# ---- co-registration ---------------------------------------------------------------------------------------------------------------
def run_surface(torch, r, c, log):
    """The surface row `r` -> the (P, 2R+1, 2R+1) float64 surfaces."""
    P, D = len(c["origins"]), 2 * r["R"] + 1
    eb = Buf(torch, c["emit_back"].nbytes, r["offs"][0], c["emit_back"])
    sb = Buf(torch, c["s2_back"].nbytes, r["offs"][1], c["s2_back"])
    mb = Buf(torch, c["mask_back"].nbytes, r["offs"][2], c["mask_back"]) if c["mask"] is not None else None
    ob = Buf(torch, c["origins"].nbytes, 0, c["origins"])
    out = Buf(torch, P * D * D * 8, 8)
    nd = c["nodata"]
    log.call([cc.surface_instance(r)], _lib().hsr_coreg_surface, eb.ptr, c["emit_rs"], r["he"], r["we"], mb.ptr if mb else None,
             c["mask_rs"], sb.ptr, 1 if r["dtype"] == "u16" else 0, c["s2_rs"], c["hs"], c["ws"], 0 if nd is None else 1,
             0.0 if nd is None else float(nd), ob.ptr, P, r["w"], r["f"], r["R"], c["min_valid"], out.ptr, _stream(torch))
    got = out.get(np.float64).reshape(P, D, D)
    untouched(eb, c["emit_back"])
    untouched(sb, c["s2_back"])
    untouched(ob, c["origins"])
    if mb:
        untouched(mb, c["mask_back"])
    return got


def run_peaks(torch, r, c, log):
    """A peaks job: r = dict(w, f, R, he, we, hs, ws, min_score), c = dict(surface (P, D, D) float64, origins (P, 2)) -> the (P, 8)
    records, every double of them written."""
    S, org = c["surface"], np.ascontiguousarray(c["origins"], np.int32)
    P = len(org)
    sb, ob = Buf(torch, S.nbytes, 8, S), Buf(torch, org.nbytes, 4, org)
    tb = Buf(torch, P * cc.REC * 8, 8)
    log.call(["coreg_peaks_kernel"], _lib().hsr_coreg_peaks, sb.ptr, ob.ptr, P, r["w"], r["f"], r["R"], r["he"], r["we"], r["hs"], r["ws"],
             r["min_score"], tb.ptr, _stream(torch))
    got = tb.get(np.float64).reshape(P, cc.REC)
    assert (got.view(np.uint64) != SENT64).all()
    untouched(sb, S)
    untouched(ob, org)
    return got


def run_model(torch, r, c, log):
    """The model row `r` (its table is the case: c is unused and may be None) -> (records after the call, model)."""
    table = np.array(r["table"], np.float64)
    tb = Buf(torch, max(table.nbytes, 8), 8, table if table.size else None)
    mb = Buf(torch, cc.MODEL * 8, 8)
    log.call(["coreg_fit_model_kernel"], _lib().hsr_coreg_fit_model, tb.ptr, len(table), r["kind"], r["min_points"], r["reject_px"],
             r["hs"], r["ws"], mb.ptr, _stream(torch))
    return tb.get(np.float64)[:table.size].reshape(-1, cc.REC), mb.get(np.float64)


def run_warp(torch, r, c, log):
    """The warp row `r` -> (output without its padding, status word).  The input and the output have their own row padding, gap
    after every band and base offset; all of it must stay as it was."""
    scene = c["scene"]
    bands, h, w = scene.shape
    u16 = r["dtype"] == "u16"
    inb = cc.pack_scene(scene, r["extra"], scene.dtype.type(3), r["in_gap"])
    irs, ors = w + r["extra"], w + r["out_extra"]
    ibs, obs = h * irs + r["in_gap"], h * ors + r["out_gap"]
    assert inb.shape == (bands, ibs)
    ib = Buf(torch, inb.nbytes, r["off"], inb)
    ob = Buf(torch, bands * obs * scene.dtype.itemsize, r["out_off"])
    mb, sb = Buf(torch, cc.MODEL * 8, 8, c["model"]), Buf(torch, 4, 4)
    nd = c["nodata"]
    log.call([cc.warp_instance(r["dtype"], r["bound"][1])], _lib().hsr_coreg_warp, ib.ptr, 1 if u16 else 0, bands, h, w, ibs, irs, mb.ptr,
             0 if nd is None else 1, 0.0 if nd is None else float(nd), c["fill"], r["bound"][0], r["bound"][1], ob.ptr, obs, ors, sb.ptr,
             _stream(torch))
    out, outside = cc.unpack_scene(ob.get(scene.dtype).reshape(bands, obs), h, w, r["out_extra"])
    raw = ob.get(np.uint16 if u16 else np.uint32).reshape(bands, obs)
    sent = np.frombuffer(bytes([FILL] * scene.dtype.itemsize), raw.dtype)[0]
    assert outside.sum() == bands * (h * r["out_extra"] + r["out_gap"]) and (raw[outside] == sent).all()   # row padding and band gaps
    untouched(ib, inb)
    untouched(mb, c["model"])
    return out, int(sb.get(np.int32)[0])


# ---- scene -------------------------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def scan_call(torch, sb, scene, th, tw, log, nodata=None, masked_val=-0.01, nodata_atol=1e-3, zero_atol=1e-6, passed=0.0):
    """hsr_scene_black_counts on the scene in Buf `sb` -> the (H // th, W // tw) counts.  The counts start 4 bytes past a 256-byte
    boundary - 4-byte but not 16-byte aligned - and hold the sentinel, which the call has to zero."""
    bands, H, W = scene.shape
    ny, nx = H // th, W // tw
    cb = Buf(torch, ny * nx * 4, 4)
    use, nd = (0, passed) if nodata is None else (1, nodata)
    log.call(sc.scan_instance(scene.dtype), _lib().hsr_scene_black_counts, sb.ptr, sc.DT_CODE[scene.dtype], bands, H, W, th, tw, use, nd,
             masked_val, nodata_atol, zero_atol, cb.ptr, _stream(torch))
    return cb.get(np.int32).reshape(ny, nx)


def run_scan(torch, r, c, log):
    """The scan row `r` on its scene -> the window counts."""
    scene = c["scene"]
    sb = Buf(torch, scene.nbytes, 0, scene)
    got = scan_call(torch, sb, scene, r["th"], r["tw"], log, passed=r["passed"], **sc.scan_settings(r))
    untouched(sb, scene)
    return got


def run_gather(torch, row, c, log):
    """The gather row -> the (P, bands, th, tw) tiles; the slice of a window outside the scene must hold the sentinel still."""
    dtype, encode, shape, org, th, tw, off = row
    scene, want, inside = c["scene"], c["want"], c["inside"]
    bands, H, W = shape
    sb, gb = Buf(torch, scene.nbytes, 0, scene), Buf(torch, org.nbytes, 0, org)
    ob = Buf(torch, want.nbytes, off)
    scale, has_nd, nd, nd16 = encode if encode else (1.0, 0, 0.0, 65535)
    log.call(sc.gather_instance_of(row), _lib().hsr_scene_gather_tiles, sb.ptr, sc.DT_CODE[dtype], bands, H, W, gb.ptr, len(org), th, tw,
             int(encode is not None), scale, has_nd, nd, nd16, ob.ptr, _stream(torch))
    got = ob.get(want.dtype).reshape(want.shape)
    sentinel = SENT32 if want.dtype == np.float32 else SENT16
    assert (bits(got[~inside]) == sentinel).all(), "a window outside the scene was written"
    sb.get(np.uint8)
    return got


def run_mosaic(torch, row, c, log, fill, fill_rest):
    """The mosaic row under one (fill, fill_rest) -> the (T, H, W) output as uint32 bits, sentinel where nothing was written."""
    T, H, W, th, tw, P, out_off, cubes_off, _ = row
    cubes, slot = c
    cb = Buf(torch, cubes.nbytes, cubes_off, cubes) if P else None
    sl = Buf(torch, slot.nbytes, 0, slot)
    ob = Buf(torch, T * H * W * 4, out_off)
    log.call(sc.mosaic_instance_of(row), _lib().hsr_scene_mosaic, cb.ptr if P else None, P, T, th, tw, ob.ptr, H, W, sl.ptr,
             slot.shape[0], slot.shape[1], float(fill), int(fill_rest), _stream(torch))
    got = ob.get(np.uint32).reshape(T, H, W)
    if P:
        cb.get(np.uint8)
    return got


def run_blend(torch, r, c, log, fill):
    """The blend row under `fill` -> the (T, H, W) float32 output."""
    cubes, start = c["cubes"], c["start"]
    P, T, th, tw = cubes.shape
    cb, sb = Buf(torch, cubes.nbytes, r["cubes_off"], cubes), Buf(torch, start.nbytes, 0, start)
    ob = Buf(torch, T * r["H"] * r["W"] * 4, r["out_off"])
    log.call(sc.blend_instance_of(r), _lib().hsr_scene_mosaic_blend, cb.ptr, P, T, th, tw, r["sy"], r["sx"], sb.ptr, start.shape[0],
             start.shape[1], ob.ptr, r["H"], r["W"], float(fill), _stream(torch))
    return ob.get(np.float32).reshape(T, r["H"], r["W"])


# ---- colour ------------------------------------------------------------------------------------------------------------------------
REDUCE = "affine_reduce_solve_kernel"
IDENTITY_AT = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])


def color_image(torch, rows, place):
    layout, off = place
    flat = ac.pack(rows, layout)
    return Buf(torch, flat.nbytes, off, flat), flat


def same_words(buf, flat):
    np.testing.assert_array_equal(buf.get(np.uint32), flat.view(np.uint32))


def lohi_buf(torch, lohi):
    return Buf(torch, 48, 0, np.ascontiguousarray(lohi, np.float64)) if lohi is not None else None


def ptr_of(b):
    return b.ptr if b is not None else None


def run_moments(torch, r, c, log):
    """The moment row's launch + reduce (min_count above every count: the solve is the identity) -> (22 moments, partials)."""
    npix = r["npix"]
    xb, xflat = color_image(torch, c["x"], r["x"])
    yb, yflat = color_image(torch, c["y"], r["y"])
    mb = Buf(torch, npix, 1, c["mask"]) if c["mask"] is not None else None            # the mask needs no alignment: 1 byte off
    lx, ly = lohi_buf(torch, r["lohi_x"]), lohi_buf(torch, r["lohi_y"])
    nslots = ac.slots(npix)
    pb = Buf(torch, nslots * ac.NMOM * 8, 0)
    slots = C.c_int32(-1)
    xbs, xps, _ = ac.strides(r["x"][0], npix)
    ybs, yps, _ = ac.strides(r["y"][0], npix)
    log.call([ac.moments_instance(r)], _lib().hsr_affine_moments, xb.ptr, xbs, xps, yb.ptr, ybs, yps, ptr_of(mb), npix, ptr_of(lx), ptr_of(ly),
             pb.ptr, C.byref(slots), _stream(torch))
    assert slots.value == nslots == _lib().hsr_affine_partial_slots(npix)
    partials = pb.get(np.uint64)
    assert (partials != SENT64).all()                                                          # every partial is written
    mo, at = Buf(torch, ac.NMOM * 8, 0), Buf(torch, 96, 0)
    log.call([REDUCE], _lib().hsr_affine_reduce_solve, pb.ptr, nslots, 1 << 40, mo.ptr, at.ptr, _stream(torch))
    same_words(xb, xflat)
    same_words(yb, yflat)
    if mb is not None:
        np.testing.assert_array_equal(mb.get(np.uint8), c["mask"])
    assert np.array_equal(at.get(np.float64), IDENTITY_AT)
    return mo.get(np.float64), partials.view(np.float64).reshape(nslots, ac.NMOM)


def run_moments_f64(torch, r, c, log, min_count=1 << 40, rs=(3, 3)):
    """float64 rows c["xs"], c["ys"] (n, 3), in device rows of rs doubles, through hsr_affine_moments_f64 + the reduce and solve
    under `min_count` -> (22 moments, At, partials)."""
    n = len(c["xs"])
    xh, yh = np.full((max(n, 1), rs[0]), 7.5), np.full((max(n, 1), rs[1]), 7.5)
    xh[:n, :3], yh[:n, :3] = c["xs"], c["ys"]
    xb, yb = Buf(torch, xh.nbytes, 0, xh), Buf(torch, yh.nbytes, 8, yh)
    nslots = ac.slots(n)
    pb, mo, at = Buf(torch, nslots * ac.NMOM * 8, 0), Buf(torch, ac.NMOM * 8, 0), Buf(torch, 96, 0)
    log.call(["affine_moments_f64_kernel"], _lib().hsr_affine_moments_f64, xb.ptr, rs[0], yb.ptr, rs[1], n, pb.ptr, None, _stream(torch))
    log.call([REDUCE], _lib().hsr_affine_reduce_solve, pb.ptr, nslots, min_count, mo.ptr, at.ptr, _stream(torch))
    partials = pb.get(np.uint64)
    assert (partials != SENT64).all()
    untouched(xb, xh)
    untouched(yb, yh)
    return mo.get(np.float64), at.get(np.float64), partials.view(np.float64).reshape(nslots, ac.NMOM)


def run_reduce_solve(torch, partials, min_count, log):
    """Hand-built partials (slots, 22) through hsr_affine_reduce_solve -> (22 moments, At)."""
    partials = np.ascontiguousarray(partials, np.float64)
    pb, mo, at = Buf(torch, partials.nbytes, 0, partials), Buf(torch, ac.NMOM * 8, 8), Buf(torch, 96, 0)
    log.call([REDUCE], _lib().hsr_affine_reduce_solve, pb.ptr, len(partials), min_count, mo.ptr, at.ptr, _stream(torch))
    untouched(pb, partials)
    return mo.get(np.float64), at.get(np.float64)


def run_apply(torch, r, c, log):
    """The apply row `r` -> the (npix, 3) output rows; what lies beside them - the fourth float of a padded row (written, +0.0), the
    gap between planes (not written) - the input and the mask are checked here."""
    npix = r["npix"]
    xb, xflat = color_image(torch, c["x"], r["x"])
    mb = Buf(torch, npix, 3, c["mask"]) if c["mask"] is not None else None
    at = Buf(torch, 96, 0, np.ascontiguousarray(r["At"], np.float64))
    lo = lohi_buf(torch, r["lohi"])
    olayout, ooff = r["out"]
    obs, ops, ofloats = ac.strides(olayout, npix)
    ob = Buf(torch, ofloats * 4, ooff)
    xbs, xps, _ = ac.strides(r["x"][0], npix)
    log.call([ac.apply_instance(r)], _lib().hsr_affine_apply, xb.ptr, xbs, xps, ptr_of(mb), at.ptr, npix, ptr_of(lo), r["clip"], ob.ptr,
             obs, ops, _stream(torch))
    rows, beside = ac.unpack(ob.get(np.float32), olayout, npix)                               # get(): the guard zones are intact
    if olayout == ac.PADDED:
        assert (beside.view(np.uint32) == 0).all()                                             # the fourth float: written, +0.0
    elif olayout == ac.PLANAR:
        assert (beside.view(np.uint32) == SENT32).all()                                        # the gap between planes: not written
    same_words(xb, xflat)
    if mb is not None:
        np.testing.assert_array_equal(mb.get(np.uint8), c["mask"])
    return np.ascontiguousarray(rows)


# ---- a drawn row against its family's reference and bar ----------------------------------------------------------------------------
def judge_ortho(torch, r, c, log):
    got, dropped = run_ortho(torch, r, c, log)
    np.testing.assert_array_equal(got, c["ref"])
    assert dropped == (c["dropped"] if r["count"] else None)
    return 0.0


def judge_surface(torch, r, c, log):
    """What test_surface_rows asserts of a table row; -> worst |err| / bar."""
    got = run_surface(torch, r, c, log)
    assert (got.view(np.uint64) != SENT64).all()                                              # every entry is written
    assert np.array_equal(np.isnan(got), np.isnan(c["ref"])), (int(np.isnan(got).sum()), int(np.isnan(c["ref"]).sum()))
    fin = np.isfinite(c["ref"])
    assert np.isfinite(got[fin]).all()
    err = np.abs(got[fin] - c["ref"][fin])
    worst = float(np.max(err / c["bar"][fin])) if fin.any() else 0.0
    assert (err <= c["bar"][fin]).all(), worst
    same_bits(run_surface(torch, r, c, log), got, "second run")                               # fixed order: bit-equal runs
    return worst


def judge_peaks(torch, r, c, log):
    same_bits(run_peaks(torch, r, c, log), c["ref"], "peak records")
    return 0.0


def judge_model(torch, r, c, log):
    """What test_model_rows asserts of a table row, the row's claims replaced by the reference's own answer; -> |err| / bar."""
    t, m = run_model(torch, r, None, log)
    hs, ws = r["hs"], r["ws"]
    same_bits(t, c["table"], "records after the rejection pass")
    assert (m[9], m[8]) == (c["model"][9], c["model"][8]), (m[8:], c["model"][8:])
    diff = np.abs(cc.scaled_coefficients(m, hs, ws) - c["coef"]).max()
    assert diff <= c["bar"], (diff, c["bar"])
    assert (m[6], m[7]) == ((0.5 * (ws - 1), 0.5 * (hs - 1)) if m[9] >= 0 else (0.0, 0.0))
    return float(diff / c["bar"]) if c["bar"] else 0.0


def judge_warp(torch, r, c, log):
    got, status = run_warp(torch, r, c, log)
    assert status == r["status"]
    if r["dtype"] == "u16":
        bad = got != c["ref"]
        assert not bad.any(), f"{int(bad.sum())} of {bad.size} elements differ, first {got[bad][:4]} vs {c['ref'][bad][:4]}"
    else:
        bits_equal(got, c["ref"], "warp")
    return 0.0


def judge_moments(torch, r, c, log):
    """What test_moment_rows asserts of a table row, for either entry point; -> worst |err| / bar."""
    def once():
        if r["entry"] == "f64":
            mom, _, partials = run_moments_f64(torch, r, c, log, rs=r["rs"])
            return mom, partials
        return run_moments(torch, r, c, log)
    got, partials = once()
    assert got[9] == c["n"] == partials[:, 9].sum()                                              # the count is exact
    err = np.abs(got.astype(ac.LD) - c["ref"]).astype(np.float64)
    bar = ac.moments_bar(c["n"], c["mag"])
    assert (err <= bar).all(), (err, bar)
    same_bits(once()[0], got, "second run")                                                     # fixed order: bit-equal runs
    return float(np.max(err / np.where(bar > 0, bar, 1.0)))


def judge_solve(torch, r, c, log):
    """Hand-built partials through the reduce and the solve: the reduced moments within (slots + 2) EPS sum |partial| of their
    long-double sum (moments_bar with the slots as the terms), the count exact; then what test_solve_rows asserts."""
    from s2_emit import _engine as eng
    mom, At = run_reduce_solve(torch, c["partials"], r["min_count"], log)
    assert mom[9] == r["n"]
    err = np.abs(mom.astype(ac.LD) - c["mom_ref"]).astype(np.float64)
    assert (err <= ac.moments_bar(r["nslots"], c["mom_mag"])).all(), err
    same_bits(At, eng.affine_solve_host(mom, r["min_count"]), "host twin on the device's moments")
    if c["identity"]:
        assert np.array_equal(At, IDENTITY_AT)
        return 0.0
    diff = ac.grid_diff(At, c["W"])
    assert diff <= c["bar"], (diff, c["bar"], c["kappa"])
    return diff / c["bar"]


def judge_apply(torch, r, c, log):
    same_bits(run_apply(torch, r, c, log), c["ref"], "apply")
    return 0.0


def judge_scan(torch, r, c, log):
    np.testing.assert_array_equal(run_scan(torch, r, c, log), c["ref"])
    return 0.0


def judge_gather(torch, row, c, log):
    got = run_gather(torch, row, c, log)
    np.testing.assert_array_equal(bits(got[c["inside"]]), bits(c["want"][c["inside"]]))
    return 0.0


def judge_mosaic(torch, row, c, log):
    row = row[:9]                                          # a drawn row carries its draw key behind the table's nine fields
    T, H, W, th, tw, *_, fills = row
    pre = np.frombuffer(bytes([FILL]) * (T * H * W * 4), np.float32).reshape(T, H, W)
    for fill, fill_rest in fills:
        got = run_mosaic(torch, row, c, log, fill, fill_rest)
        np.testing.assert_array_equal(got, bits(sc.assemble(c[0], c[1], pre, th, tw, fill, fill_rest)))
    return 0.0


def judge_blend(torch, r, c, log):
    """check_blend of tests/test_scene_blend_host.py, under the row's fill; -> the largest error over the bound."""
    from test_scene_blend_host import check_blend
    return check_blend(run_blend(torch, r, c, log, r["fill"]), c["ref"], c["K"], r["fill"])


# sweep -> judge(torch, row, case, log) -> worst |err| / bar (0.0 where the bar is bit equality)
JUDGES = {"ortho": judge_ortho, "scene-scan": judge_scan, "scene-gather": judge_gather, "scene-mosaic": judge_mosaic,
          "scene-blend": judge_blend, "color-moments": judge_moments, "color-solve": judge_solve, "color-apply": judge_apply,
          "coreg-surface": judge_surface, "coreg-peaks": judge_peaks, "coreg-model": judge_model, "coreg-warp": judge_warp}
# family -> (its launch-record reader, whether the record is a list of names)
LAUNCH_READERS = {"scene": ("hsr_scene_last_launch", False), "ortho": ("hsr_ortho_last_launch", False),
                  "color": ("hsr_color_last_launch", True), "coreg": ("hsr_coreg_last_launch", True)}
