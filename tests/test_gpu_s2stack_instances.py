"""Every kernel instance of csrc/hsr_s2stack.hip - the stack kernel for both output types and both nodata rules, the byte plane
under a window at both resolutions - on an MI355X, row by row of the tables of tests/s2stack_cases.py and of its seeded sweep: the
instance by name (the family's launch record), every output element equal to the NumPy statement of include/hsr_s2stack.h, the
invalid counts, guard bytes and the gaps between rows and bands intact, inputs unchanged.  Every comparison is an equality."""
import numpy as np
import pytest

import s2stack_cases as sc
from gpu_harness import Buf, LaunchLog, lib, stream, torch_gpu  # noqa: F401  (torch_gpu: the fixture)

pytestmark = pytest.mark.gpu

LOG = LaunchLog("hsr_s2stack_last_launch", joined=True)


@pytest.mark.parametrize("name", list(sc.ALL_ROWS))
def test_stack(torch_gpu, name):
    from s2_emit import _native as nat
    torch, r = torch_gpu, sc.ALL_ROWS[name]
    srcs, nout, dst_off, dtype = sc.layout(name)
    planes = [Buf(torch, flat.nbytes, off, flat) for flat, off in srcs]
    out = Buf(torch, nout * np.dtype(dtype).itemsize, dst_off)
    invalid = Buf(torch, 8 * len(r["bands"]), 8)
    table = sc.band_table(nat.S2Band, name, [p.ptr.value for p in planes])
    args = sc.stack_args(name, table, out.ptr, invalid.ptr if r["count"] else None)
    LOG.call([sc.stack_instance(r["dtype"], r["rule"])], lib().hsr_s2_stack, *args, stream(torch))
    sc.check_output(name, out.get(dtype), invalid.get(np.int64) if r["count"] else None)
    if not r["count"]:
        assert (invalid.get(np.uint8) == sc.SENT).all()
    for p, (flat, _) in zip(planes, srcs):
        assert np.array_equal(p.get(np.uint16), flat)


@pytest.mark.parametrize("name", list(sc.EXPAND_ROWS))
def test_expand(torch_gpu, name):
    torch, r = torch_gpu, sc.EXPAND_ROWS[name]
    p, rs, ors, want = sc.expand_case(name)
    H, W = p.shape
    row0, col0, h, w = r["window"]
    src = Buf(torch, (H - 1) * rs + W, r["src_off"], sc.strided(p, rs, 200))
    out = Buf(torch, (h - 1) * ors + w, r["dst_off"])
    LOG.call(["s2_expand_kernel<UP%d>" % r["up"]], lib().hsr_s2_expand_u8, src.ptr, H, W, rs, r["up"], r["grid"][0], r["grid"][1], row0, col0,
             h, w, out.ptr, ors, stream(torch))
    got, gaps = sc.unstrided3(out.get(np.uint8), 1, h, w, 0, ors)
    np.testing.assert_array_equal(got[0], want)
    assert (gaps == sc.SENT).all()
    assert np.array_equal(src.get(np.uint8), sc.strided(p, rs, 200))


def test_every_instance_was_launched():
    """Runs last: every name of the instance table was recorded by some row above."""
    assert LOG.seen == set(sc.all_instances()), sorted(set(sc.all_instances()) - LOG.seen)
