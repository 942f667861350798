"""Every kernel instance of csrc/hsr_resize.hip - the staged kernel for both layouts and the gather kernel, each for the five dtype
pairs - on an MI355X, row by row of the tables of tests/resize_cases.py and of its seeded sweep: the instance by name (the family's
launch record), every output element equal to the NumPy statement of include/hsr_resize.h and to the host twin's, the invalid
counts, guard bytes and the gaps between rows, pixels and planes intact, inputs unchanged.  Every comparison is an equality."""
import ctypes as C

import numpy as np
import pytest

import resize_cases as rc
from gpu_harness import FILL, Buf, LaunchLog, lib, stream, torch_gpu  # noqa: F401  (torch_gpu: the fixture)

pytestmark = pytest.mark.gpu

LOG = LaunchLog("hsr_resize_last_launch", joined=True)
assert FILL == rc.SENT


def _host(name, flat, nout):
    """The host twin on 16-byte aligned copies with the row's offsets -> (output as its dtype, counts)."""
    r = rc.ALL_ROWS[name]
    _, soff, _, _, doff, _ = rc.layout(name)
    item = np.dtype(r["out"]).itemsize
    sraw = np.full(flat.nbytes + soff + 48, rc.SENT, np.uint8)
    sbase = (-sraw.ctypes.data) % 16 + soff
    sraw[sbase: sbase + flat.nbytes] = flat.view(np.uint8)
    oraw = np.full(nout * item + doff + 48, rc.SENT, np.uint8)
    obase = (-oraw.ctypes.data) % 16 + doff
    inv = np.zeros(r["C"], np.int64)
    args = rc.call_args(name, C.c_void_p(sraw.ctypes.data + sbase), C.c_void_p(oraw.ctypes.data + obase), C.c_void_p(inv.ctypes.data))
    assert lib().hsr_area_resample_host(*args) == 0, lib().hsr_last_error()
    return oraw[obase: obase + nout * item].view(r["out"]).copy(), inv


@pytest.mark.parametrize("name", list(rc.ALL_ROWS))
def test_row(torch_gpu, name):
    torch, r = torch_gpu, rc.ALL_ROWS[name]
    flat, soff, _, nout, doff, _ = rc.layout(name)
    item = np.dtype(r["out"]).itemsize
    src = Buf(torch, flat.nbytes, soff, flat)
    out = Buf(torch, nout * item, doff)
    invalid = Buf(torch, 8 * r["C"], 8)
    args = rc.call_args(name, src.ptr, out.ptr, invalid.ptr)
    LOG.call([rc.instance_name(name)], lib().hsr_area_resample, *args, stream(torch))
    got = out.get(r["out"])
    rc.check_output(name, got, invalid.get(np.int64) if r["count"] else None)
    if not r["count"]:
        assert (invalid.get(np.uint8) == rc.SENT).all()
    assert np.array_equal(src.get(np.uint8), flat.view(np.uint8))
    hout, hinv = _host(name, flat, nout)
    assert np.array_equal(got.view(np.uint8), hout.view(np.uint8)), f"{name}: device bits != host bits"
    if r["count"]:
        assert np.array_equal(invalid.get(np.int64), hinv)


def test_every_instance_was_launched():
    """Runs last: every name of the instance table was recorded by some row above."""
    assert LOG.seen == set(rc.all_instances()), sorted(set(rc.all_instances()) - LOG.seen)
