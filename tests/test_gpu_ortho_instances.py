"""Every kernel instance of csrc/hsr_ortho.hip - the swath -> scene gather, band-interleaved and band-sequential, with and without
masks - on an MI355X, row by row of the table of tests/ortho_cases.py, against its NumPy reference.

hsr_ortho_glt is called through ctypes.  The swath and the output lie `off` bytes past a 256-byte boundary in buffers filled with
a sentinel byte, between two guard zones (Buf of gpu_harness.py): nothing outside the output may be written, and every byte of
it must be.  After every call the library's launch record (hsr_ortho_last_launch) is compared with the instance the row expects,
computed by ortho_cases' mirror of the selection rule.  Outputs are compared as uint32 bits; the dropped count is exact.  The last
test checks that the rows reached every name hsr_ortho_instance_name enumerates."""
import ctypes as C

import numpy as np
import pytest

import ortho_cases as oc
from gpu_harness import FILL, Buf, LaunchLog, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from gpu_harness import lib as _lib, stream as _stream
from family_runners import run_ortho

pytestmark = pytest.mark.gpu

LOG = LaunchLog("hsr_ortho_last_launch")


def _run(torch, name, layout=None, count=None):
    """The row `name` (optionally in the other layout) -> (output bits in that layout's shape, dropped or None)."""
    return run_ortho(torch, oc.ROWS[name], oc.case(name), LOG, layout=layout, count=count)


@pytest.mark.parametrize("name", list(oc.ROWS))
def test_rows(torch_gpu, name):
    r, c = oc.ROWS[name], oc.case(name)
    got, dropped = _run(torch_gpu, name)
    np.testing.assert_array_equal(got, c["ref"])
    assert dropped == (c["dropped"] if r["count"] else None)


@pytest.mark.parametrize("name", [n for n in oc.ROWS if n.startswith(("mask-", "window-", "nodata-b", "dropped-b", "valid-b", "align-b3",
                                                                      "max-bands", "nan-fill")) or n.endswith(("w65", "w130"))])
def test_bsq_bits_are_bip_bits_permuted(torch_gpu, name):
    """The row in the OTHER layout than its own: the same bits, permuted; with and without the counter."""
    r, c = oc.ROWS[name], oc.case(name)
    other = oc.BSQ if r["layout"] == oc.BIP else oc.BIP
    got, dropped = _run(torch_gpu, name, layout=other, count=not r["count"])
    np.testing.assert_array_equal(got if other == oc.BIP else got.transpose(1, 2, 0), c["ref_bip"])
    assert dropped == (None if r["count"] else c["dropped"])


def test_refused_calls_launch_nothing(torch_gpu):
    torch = torch_gpu
    r, c = oc.ROWS["b3-bip-w3"], oc.case("b3-bip-w3")
    sb, gb = Buf(torch, c["swath"].nbytes, 0, c["swath"]), Buf(torch, c["glt"].nbytes, 0, c["glt"])
    ob, mb = Buf(torch, 3 * 3 * 3 * 4, 0), Buf(torch, 64, 0)
    st, f = _stream(torch), _lib().hsr_ortho_glt
    ok = [sb.ptr, r["rows"], r["cols"], 3, gb.ptr, r["gh"], r["gw"], 0, 0, 0, r["gh"], r["gw"], None, None, 0, -9999.0, -9999.0, 0,
          ob.ptr, None, st]
    for at, bad in ((0, None), (4, None), (18, None), (1, 0), (3, 0), (10, 0), (8, 1), (9, -1), (11, r["gw"] + 1), (17, 2), (3, oc.MAX_BANDS + 1)):
        args = list(ok)
        args[at] = bad
        LOG.refused(f, *args)
    args = list(ok)
    args[13], args[14] = mb.ptr, 0                                        # a band mask of too few bytes a pixel
    LOG.refused(f, *args)
    assert (ob.get(np.uint8) == FILL).all()
    LOG.call(oc.instance(oc.BIP, 3, False), f, *ok)


def test_rows_reach_every_instance(torch_gpu):
    lib = _lib()
    n = lib.hsr_ortho_instance_count()
    assert n == oc.INSTANCE_COUNT
    table = {lib.hsr_ortho_instance_name(i).decode() for i in range(n)}
    assert len(table) == n
    assert LOG.seen == table, (sorted(table - LOG.seen), sorted(LOG.seen - table))
    print("ortho instances seen: %d of %d" % (len(LOG.seen & table), len(table)))
