"""Every kernel instance of csrc/hsr_reproject.hip - the coordinate field and the cubic remap under both sample rules, staged and
direct - on an MI355X, row by row of the tables of tests/reproject_cases.py, against their references.

The entry points of include/hsr_reproject.h are called through ctypes.  Scenes and outputs lie in buffers filled with a sentinel
byte between two guard zones (Buf of gpu_harness.py), some bytes past a 256-byte boundary, with row strides larger than their
width and gaps between the bands, the output with a layout of its own: nothing outside a payload may be written, the padding of an
output row and the gap after a band stay as they were, inputs stay as they were, and every output element must be written.
After every call the launch record (hsr_reproject_last_launch) is compared with the instance the tables expect.  Bars: the header
of reproject_cases.py - the remap bit-equal to the NumPy statement with equal counts and status word, the coordinates within the
coordinate bar of the mpmath fixture.  The last test checks that the rows reached every name hsr_reproject_instance_name
enumerates."""
import ctypes as C

import numpy as np
import pytest

import reproject_cases as rc
from gpu_harness import FILL, SENT32, Buf, LaunchLog, same_bits, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from gpu_harness import lib as _lib, stream as _stream

pytestmark = pytest.mark.gpu

LOG = LaunchLog("hsr_reproject_last_launch", joined=True)
SENT64 = np.frombuffer(bytes([FILL] * 8), np.uint64)[0]


def run_warp(torch, r, c, log=LOG, mf=None):
    """The remap of row `r` on case `c` -> (output without its padding, counts (2,), status word)."""
    lib, st = _lib(), _stream(torch)
    bands, h, w, hs, ws = r["bands"], r["h"], r["w"], r["hs"], r["ws"]
    sent = np.frombuffer(bytes([FILL] * 4), np.float32)[0]
    src_back = rc.pack(c["src"], r["src_pad"], sent)
    src = Buf(torch, src_back.nbytes, r["src_pad"][0], src_back)
    coords = Buf(torch, c["coords"].nbytes, 0, c["coords"])
    out_back = rc.pack(np.zeros((bands, h, w), np.float32), r["out_pad"], sent)
    out = Buf(torch, out_back.nbytes, r["out_pad"][0])
    counts, status = Buf(torch, 16, 8), Buf(torch, 4, 4)
    srs, ors = ws + r["src_pad"][1], w + r["out_pad"][1]
    mf = r["mf"] if mf is None else mf
    log.call([rc.warp_instance(mf, r["rule"])], lib.hsr_reproject_warp, src.ptr, bands, hs, ws, hs * srs + r["src_pad"][2], srs, coords.ptr,
             h, w, 0 if r["nodata"] is None else 1, 0.0 if r["nodata"] is None else r["nodata"], r["fill"], r["rule"], mf, out.ptr,
             h * ors + r["out_pad"][2], ors, counts.ptr, status.ptr, st)
    got_back = out.get(np.float32).reshape(out_back.shape)
    got, outside = rc.unpack(got_back, h, w, r["out_pad"])
    assert (got_back.view(np.uint32)[outside] == SENT32).all(), "the output's row padding or band gap was written"
    assert (np.ascontiguousarray(got).view(np.uint32) != SENT32).all(), "an output element was not written"
    assert np.array_equal(src.get(np.uint8), src_back.reshape(-1).view(np.uint8)) and np.array_equal(coords.get(np.float64).view(np.uint64),
                                                                                                    c["coords"].reshape(-1).view(np.uint64))
    return np.ascontiguousarray(got), counts.get(np.int64), int(status.get(np.int32)[0])


def _judge(name, r, c, got, counts, status):
    same_bits(got, c["ref"], name)
    assert np.array_equal(counts, c["counts"]), (name, counts, c["counts"])
    assert status == c["status"], (name, status, c["status"])


@pytest.mark.parametrize("name", list(rc.WARP_ROWS))
def test_warp_rows(torch_gpu, name):
    r, c = rc.WARP_ROWS[name], rc.warp_case(name)
    _judge(name, r, c, *run_warp(torch_gpu, r, c))


def test_warp_without_counts(torch_gpu):
    """counts_dev NULL: the same output and status."""
    torch, lib, st = torch_gpu, _lib(), _stream(torch_gpu)
    r, c = rc.WARP_ROWS["affine-strict"], rc.warp_case("affine-strict")
    src, coords = Buf(torch, c["src"].nbytes, 0, c["src"]), Buf(torch, c["coords"].nbytes, 0, c["coords"])
    out, status = Buf(torch, c["ref"].nbytes), Buf(torch, 4)
    LOG.call([rc.warp_instance(r["mf"], r["rule"])], lib.hsr_reproject_warp, src.ptr, r["bands"], r["hs"], r["ws"], r["hs"] * r["ws"], r["ws"],
             coords.ptr, r["h"], r["w"], 1, r["nodata"], r["fill"], r["rule"], r["mf"], out.ptr, r["h"] * r["w"], r["w"], None, status.ptr, st)
    same_bits(out.get(np.float32).reshape(c["ref"].shape), c["ref"], "no counts")
    assert int(status.get(np.int32)[0]) == c["status"]


def test_warp_instances_agree(torch_gpu):
    """The direct-gather instance and the staged one give the same bits, counts included, on the same scene and field."""
    for name in ("affine", "half-outside", "nearest-invalid", "minify-5"):
        r, c = rc.WARP_ROWS[name], rc.warp_case(name)
        assert "LDS" in rc.warp_instance(r["mf"], r["rule"]) and "DIRECT" in rc.warp_instance(64.0, r["rule"])
        a, ca, _ = run_warp(torch_gpu, r, c)
        b, cb, sb = run_warp(torch_gpu, r, c, mf=64.0)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(ca, cb) and sb == 0, name


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_warp_sweep(torch_gpu, seed):
    skipped = 0
    for index in range(rc.ROWS_PER_SEED):
        r = rc.draw(seed, index)
        c = rc.warp_case_of(r)
        assert rc.valid(r)
        if not rc.admitted(r, c):
            skipped += 1
            continue
        _judge(f"sweep {seed}/{index}", r, c, *run_warp(torch_gpu, r, c))
    assert skipped <= rc.MAX_SKIPPED * rc.ROWS_PER_SEED


def test_coordinate_bar(torch_gpu):
    """reproject_coords_kernel against the mpmath fixture, one 1 x 1 grid per point, and a whole grid against the host twin."""
    torch, lib, st, g = torch_gpu, _lib(), _stream(torch_gpu), rc.fixture()
    n = len(g["E"])
    out = Buf(torch, n * 16)
    want = np.empty((n, 2))
    for i in range(n):
        args, (g0, g3) = rc.point_call(g["E"][i], g["N"][i], g["lon0"][i], g["FN"][i])
        call = (lib.hsr_reproject_coords, *args, C.c_void_p(out.ptr.value + 16 * i), st)
        if i % 50 == 0:
            LOG.call(["reproject_coords_kernel"], *call)
        else:
            assert call[0](*call[1:]) == 0, lib.hsr_last_error()
        want[i] = (g["lat"][i] - g3) / -rc.EMIT_CELL - 0.5, (g["lon"][i] - g0) / rc.EMIT_CELL - 0.5
    got = out.get(np.float64).reshape(n, 2)
    bar, worst = rc.coord_bar(rc.EMIT_CELL), float(np.abs(got - want).max())
    print(f"coordinate error, source pixels: kernel {worst:.3g}, bar {bar:.3g}")
    assert worst <= bar
    # a grid that is no multiple of the workgroup: every element written once, nothing else, and the host twin within twice the bar
    geo = [431040.0, 3801060.0, 60.0, 60.0, 19, 27, -117.0, *rc.WGS84[:2], 0.0, *rc.WGS84[2:], -118.0, rc.EMIT_CELL, 34.9, -rc.EMIT_CELL]
    field = Buf(torch, 19 * 27 * 16, 8)
    LOG.call(["reproject_coords_kernel"], lib.hsr_reproject_coords, *geo, field.ptr, st)
    dev = field.get(np.float64).reshape(19, 27, 2)
    assert (dev.view(np.uint64) != SENT64).all()
    host = np.empty((19, 27, 2))
    assert lib.hsr_reproject_coords_host(*geo, host.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert np.abs(dev - host).max() <= 2 * bar and 0 < dev.min() and dev[..., 0].max() < 1800 and dev[..., 1].max() < 2200
    assert (np.diff(dev[..., 0], axis=0) > 0.9).all() and (np.diff(dev[..., 1], axis=1) > 0.9).all()


def test_refusals_leave_no_record(torch_gpu):
    torch = torch_gpu
    lib, st = _lib(), _stream(torch)
    b, o = Buf(torch, 4096), Buf(torch, 4096)
    geo = [4e5, 3.9e6, 60.0, 60.0, 4, 5, -117.0, 0.9996, 5e5, 0.0, 6378137.0, 298.257223563, -118.0, 5e-4, 35.0, -5e-4]
    LOG.refused(lib.hsr_reproject_coords, *(geo[:2] + [0.0] + geo[3:]), o.ptr, st)
    LOG.refused(lib.hsr_reproject_coords, *(geo[:11] + [1.0] + geo[12:]), o.ptr, st)
    LOG.refused(lib.hsr_reproject_warp, b.ptr, 1, 8, 8, 64, 8, b.ptr, 4, 4, 0, 0.0, 0.0, 2, 1.5, o.ptr, 16, 4, None, o.ptr, st)        # rule
    LOG.refused(lib.hsr_reproject_warp, b.ptr, 1, 8, 8, 64, 8, o.ptr, 4, 4, 0, 0.0, 0.0, 1, 1.5, b.ptr, 16, 4, None, o.ptr, st)        # in place
    LOG.refused(lib.hsr_reproject_warp, b.ptr, 1, 8, 8, 64, 8, o.ptr, 4, 4, 0, 0.0, 0.0, 1, 1.5, o.ptr, 16, 4, None, b.ptr, st)        # on the field
    assert (b.get(np.uint8) == FILL).all() and (o.get(np.uint8) == FILL).all()


def test_every_instance_was_launched():
    table = {_lib().hsr_reproject_instance_name(i).decode() for i in range(_lib().hsr_reproject_instance_count())}
    assert LOG.seen == table, (sorted(table - LOG.seen), sorted(LOG.seen - table))
