"""Every kernel instance of csrc/hsr_coreg.hip - score surfaces, peak records, the shift model, the cubic warp - on an MI355X, row
by row of the tables of tests/coreg_cases.py, against their references.

The entry points of include/hsr_coreg.h are called through ctypes.  Planes, scenes and outputs lie in buffers filled with a
sentinel byte between two guard zones (Buf of gpu_harness.py), some `off` bytes past a 256-byte boundary and with row strides
larger than their width - for the rows that say so each operand with a padding and an offset of its own, the warp's output with
another row stride, band stride (gaps between the bands) and offset than its input: nothing outside a payload may be written,
the padding of an output row and the gap after a band stay as they were, inputs stay as they were, and every output element the
contract names must be written.  After every call the launch record
(hsr_coreg_last_launch) is compared with the instance the tables expect.  Bars: the header of coreg_cases.py - surfaces within
their bars with NaN in the same places, peak records and warp outputs bit-equal, models within the model bar with equal
statuses.  The last test checks that the rows reached every name hsr_coreg_instance_name enumerates."""
import numpy as np
import pytest

import coreg_cases as cc
from gpu_harness import FILL, Buf, LaunchLog, bits_equal, same_bits, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from gpu_harness import lib as _lib, stream as _stream

pytestmark = pytest.mark.gpu

LOG = LaunchLog("hsr_coreg_last_launch", joined=True)
SENT64 = np.frombuffer(bytes([FILL] * 8), np.uint64)[0]


def _untouched(buf, back):
    np.testing.assert_array_equal(buf.get(np.uint8), np.ascontiguousarray(back).reshape(-1).view(np.uint8))


def _surface(torch, name):
    r, c = cc.SURFACE_ROWS[name], cc.surface_case(name)
    P, D = len(c["origins"]), 2 * r["R"] + 1
    eb = Buf(torch, c["emit_back"].nbytes, r["offs"][0], c["emit_back"])
    sb = Buf(torch, c["s2_back"].nbytes, r["offs"][1], c["s2_back"])
    mb = Buf(torch, c["mask_back"].nbytes, r["offs"][2], c["mask_back"]) if c["mask"] is not None else None
    ob = Buf(torch, c["origins"].nbytes, 0, c["origins"])
    out = Buf(torch, P * D * D * 8, 8)
    nd = c["nodata"]
    LOG.call([cc.surface_instance(r)], _lib().hsr_coreg_surface, eb.ptr, c["emit_rs"], r["he"], r["we"], mb.ptr if mb else None,
             c["mask_rs"], sb.ptr, 1 if r["dtype"] == "u16" else 0, c["s2_rs"], c["hs"], c["ws"], 0 if nd is None else 1,
             0.0 if nd is None else float(nd), ob.ptr, P, r["w"], r["f"], r["R"], c["min_valid"], out.ptr, _stream(torch))
    got = out.get(np.float64).reshape(P, D, D)
    _untouched(eb, c["emit_back"])
    _untouched(sb, c["s2_back"])
    _untouched(ob, c["origins"])
    if mb:
        _untouched(mb, c["mask_back"])
    return got


@pytest.mark.parametrize("name", list(cc.SURFACE_ROWS))
def test_surface_rows(torch_gpu, name):
    c = cc.surface_case(name)
    got = _surface(torch_gpu, name)
    assert (got.view(np.uint64) != SENT64).all()                                              # every entry is written
    assert np.array_equal(np.isnan(got), np.isnan(c["ref"])), (name, int(np.isnan(got).sum()), int(np.isnan(c["ref"]).sum()))
    fin = np.isfinite(c["ref"])
    assert np.isfinite(got[fin]).all()
    err = np.abs(got[fin] - c["ref"][fin])
    worst = float(np.max(err / c["bar"][fin])) if fin.any() else 0.0
    print(f"{name}: {int(fin.sum())} finite entries, worst |err| / bar {worst:.3g}, largest bar {np.max(c['bar'][fin]) if fin.any() else 0:.3g}")
    assert (err <= c["bar"][fin]).all(), (name, worst)
    same_bits(_surface(torch_gpu, name), got, name + ": second run")                           # fixed order: bit-equal runs


def test_peak_rows(torch_gpu):
    """Crafted surfaces, and the reference surfaces of every surface row: records bit-equal to the NumPy restatement."""
    torch = torch_gpu
    names, surf, origins, want = cc.peak_case()
    jobs = [("crafted", surf, origins, cc.PEAK_W, cc.PEAK_F, cc.PEAK_R, cc.PEAK_SHAPES, cc.PEAK_MIN_SCORE)]
    _, rsurf, rorigins, rwant = cc.peak_case(rect=True)
    jobs.append(("crafted-rect", rsurf, rorigins, cc.PEAK_W, cc.PEAK_F, cc.PEAK_R, cc.PEAK_SHAPES_RECT, cc.PEAK_MIN_SCORE))
    for name, r in cc.SURFACE_ROWS.items():
        c = cc.surface_case(name)
        jobs.append((name, c["ref"], c["origins"], r["w"], r["f"], r["R"], dict(he=r["he"], we=r["we"], hs=c["hs"], ws=c["ws"]), 0.6))
    for tag, S, org, w, f, R, sh, min_score in jobs:
        P = len(org)
        sb, ob = Buf(torch, S.nbytes, 8, S), Buf(torch, org.nbytes, 4, np.ascontiguousarray(org, np.int32))
        tb = Buf(torch, P * cc.REC * 8, 8)
        LOG.call(["coreg_peaks_kernel"], _lib().hsr_coreg_peaks, sb.ptr, ob.ptr, P, w, f, R, sh["he"], sh["we"], sh["hs"], sh["ws"],
                 min_score, tb.ptr, _stream(torch))
        got = tb.get(np.float64).reshape(P, cc.REC)
        assert (got.view(np.uint64) != SENT64).all()
        same_bits(got, cc.peaks_ref(S, org, w, f, R, min_score=min_score, **sh), "peaks " + tag)
        _untouched(sb, S)
        if tag == "crafted":
            assert np.array_equal(got[:, 7], want)
        if tag == "crafted-rect":
            assert np.array_equal(got[:, 7], rwant) and (got[:, 0] != got[:, 1]).all()
            assert np.array_equal(got[:, 0], f * (org[:, 0] + w / 2) - 0.5) and np.array_equal(got[:, 1], f * (org[:, 1] + w / 2) - 0.5)


def _fit(torch, r):
    table = np.array(r["table"], np.float64)
    tb = Buf(torch, max(table.nbytes, 8), 8, table if table.size else None)
    mb = Buf(torch, cc.MODEL * 8, 8)
    LOG.call(["coreg_fit_model_kernel"], _lib().hsr_coreg_fit_model, tb.ptr, len(table), r["kind"], r["min_points"], r["reject_px"],
             r["hs"], r["ws"], mb.ptr, _stream(torch))
    return tb.get(np.float64)[:table.size].reshape(-1, cc.REC), mb.get(np.float64)


@pytest.mark.parametrize("name", list(cc.MODEL_ROWS_ALL))
def test_model_rows(torch_gpu, name):
    from s2_emit import _engine as eng
    r = cc.MODEL_ROWS_ALL[name]
    hs, ws = r["hs"], r["ws"]
    want_t, want_m, coef, bar = cc.model_ref(r["table"], r["kind"], r["min_points"], r["reject_px"], hs, ws)
    t, m = _fit(torch_gpu, r)
    same_bits(t, want_t, name + ": records after the rejection pass")
    assert (m[9], m[8]) == (r["kind_used"], r["n_used"])
    diff = np.abs(cc.scaled_coefficients(m, hs, ws) - coef).max()
    print(f"{name}: diff {diff:.3g}, bar {bar:.3g}, |err| / bar {diff / bar if bar else 0.0:.3g}")
    assert diff <= bar
    assert (m[6], m[7]) == ((0.5 * (ws - 1), 0.5 * (hs - 1)) if m[9] >= 0 else (0.0, 0.0))
    _, host = eng.coreg_fit_model_host(r["table"], r["kind"], r["min_points"], r["reject_px"], (hs, ws))
    assert np.abs(cc.scaled_coefficients(host, hs, ws) - cc.scaled_coefficients(m, hs, ws)).max() <= bar
    assert np.array_equal(host[6:], m[6:])


def _warp(torch, name, row=None):
    """The warp of case `name` (under the bound of `row`, when given) -> (output without its padding, status word).  The input
    and the output have their own row padding, gap after every band and base offset; all of it must stay as it was."""
    r, c = row or cc.WARP_ROWS[name], cc.warp_case(name)
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
    LOG.call([cc.warp_instance(r["dtype"], r["bound"][1])], _lib().hsr_coreg_warp, ib.ptr, 1 if u16 else 0, bands, h, w, ibs, irs, mb.ptr,
             0 if nd is None else 1, 0.0 if nd is None else float(nd), c["fill"], r["bound"][0], r["bound"][1], ob.ptr, obs, ors, sb.ptr,
             _stream(torch))
    out, outside = cc.unpack_scene(ob.get(scene.dtype).reshape(bands, obs), h, w, r["out_extra"])
    raw = ob.get(np.uint16 if u16 else np.uint32).reshape(bands, obs)
    sent = np.frombuffer(bytes([FILL] * scene.dtype.itemsize), raw.dtype)[0]
    assert outside.sum() == bands * (h * r["out_extra"] + r["out_gap"]) and (raw[outside] == sent).all()   # row padding and band gaps
    _untouched(ib, inb)
    _untouched(mb, c["model"])
    return out, int(sb.get(np.int32)[0])


@pytest.mark.parametrize("name", list(cc.WARP_ROWS))
def test_warp_rows(torch_gpu, name):
    r, c = cc.WARP_ROWS[name], cc.warp_case(name)
    got, status = _warp(torch_gpu, name)
    assert status == r["status"]
    if r["dtype"] == "u16":
        bad = got != c["ref"]
        assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} elements differ, first {got[bad][:4]} vs {c['ref'][bad][:4]}"
    else:
        bits_equal(got, c["ref"], name)


def test_warp_instances_agree(torch_gpu):
    """The direct-gather instance and the LDS instance give the same bits on the same scene and model."""
    for name, bound in (("affine", (80.0, 2.0)), ("frac-u16", (40.0, 2.0))):
        row = dict(cc.WARP_ROWS[name], bound=bound)
        assert cc.warp_instance(row["dtype"], cc.WARP_ROWS[name]["bound"][1]).endswith("LDS>")
        assert cc.warp_instance(row["dtype"], bound[1]).endswith("DIRECT>")
        a, _ = _warp(torch_gpu, name)
        b, _ = _warp(torch_gpu, name, row)
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), name


def test_refusals_leave_no_record(torch_gpu):
    torch = torch_gpu
    lib, st = _lib(), _stream(torch)
    b = Buf(torch, 4096)
    LOG.refused(lib.hsr_coreg_surface, b.ptr, 16, 16, 16, None, 0, b.ptr, 0, 96, 96, 96, 0, 0.0, b.ptr, 1, 3, 6, 3, 1, b.ptr, st)
    LOG.refused(lib.hsr_coreg_peaks, b.ptr, b.ptr, 1, 8, 9, 3, 16, 16, 96, 96, 0.6, b.ptr, st)
    LOG.refused(lib.hsr_coreg_fit_model, b.ptr, 4, 2, 1, 1.0, 96, 96, b.ptr, st)
    LOG.refused(lib.hsr_coreg_warp, b.ptr, 0, 1, 8, 8, 64, 8, b.ptr, 0, 0.0, 0.0, 1.0, 0.0, b.ptr, 64, 8, b.ptr, st)      # in place
    LOG.call(None, lib.hsr_coreg_surface, b.ptr, 16, 16, 16, None, 0, b.ptr, 0, 96, 96, 96, 0, 0.0, b.ptr, 0, 8, 6, 3, 1, b.ptr, st)
    LOG.call(None, lib.hsr_coreg_peaks, b.ptr, b.ptr, 0, 8, 6, 3, 16, 16, 96, 96, 0.6, b.ptr, st)
    assert (b.get(np.uint8) == FILL).all()


def test_every_instance_was_launched():
    table = {_lib().hsr_coreg_instance_name(i).decode() for i in range(_lib().hsr_coreg_instance_count())}
    assert LOG.seen == table, (sorted(table - LOG.seen), sorted(LOG.seen - table))
