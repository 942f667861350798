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
from family_runners import SENT64, run_model, run_peaks, run_surface, run_warp

pytestmark = pytest.mark.gpu

LOG = LaunchLog("hsr_coreg_last_launch", joined=True)


def _surface(torch, name):
    return run_surface(torch, cc.SURFACE_ROWS[name], cc.surface_case(name), LOG)


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
        got = run_peaks(torch, dict(sh, w=w, f=f, R=R, min_score=min_score), dict(surface=S, origins=org), LOG)
        same_bits(got, cc.peaks_ref(S, org, w, f, R, min_score=min_score, **sh), "peaks " + tag)
        if tag == "crafted":
            assert np.array_equal(got[:, 7], want)
        if tag == "crafted-rect":
            assert np.array_equal(got[:, 7], rwant) and (got[:, 0] != got[:, 1]).all()
            assert np.array_equal(got[:, 0], f * (org[:, 0] + w / 2) - 0.5) and np.array_equal(got[:, 1], f * (org[:, 1] + w / 2) - 0.5)


def _fit(torch, r):
    return run_model(torch, r, None, LOG)


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
    return run_warp(torch, row or cc.WARP_ROWS[name], cc.warp_case(name), LOG)


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
