"""Every kernel instance of csrc/hsr_color.hip - the affine moments of an image pair and of float64 rows, the reduce + solve, the
apply - on an MI355X, row by row of the tables of tests/affine_cases.py, against their references.

The entry points of include/hsr_color.h are called through ctypes.  Images, masks and outputs lie `off` bytes past a 256-byte
boundary in buffers filled with a sentinel byte between two guard zones (Buf of gpu_harness.py): nothing outside a payload may be
written, inputs stay as they were, and every output byte the contract names must be written.  After every call the launch record
(hsr_color_last_launch) is compared with the instance that affine_cases' mirror of the host predicate expects.  Bars are those in
the header of affine_cases.py.  The last test checks that the rows reached every name hsr_color_instance_name enumerates."""
import ctypes as C

import numpy as np
import pytest

import affine_cases as ac
from gpu_harness import FILL, Buf, LaunchLog, same_bits, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from gpu_harness import lib as _lib, stream as _stream
from family_runners import REDUCE, color_image as _image, lohi_buf as _lohi, ptr_of as _ptr, run_apply, run_moments, run_moments_f64

pytestmark = pytest.mark.gpu

LOG = LaunchLog("hsr_color_last_launch", joined=True)


def _moments(torch, name):
    """The row's moments launch + reduce (min_count above every count: the solve is the identity) -> (22 moments, slots)."""
    return run_moments(torch, ac.MOMENT_ROWS[name], ac.moment_case(name), LOG)


@pytest.mark.parametrize("name", list(ac.MOMENT_ROWS))
def test_moment_rows(torch_gpu, name):
    c = ac.moment_case(name)
    got, partials = _moments(torch_gpu, name)
    assert got[9] == c["n"] == partials[:, 9].sum()                                              # the count is exact
    err = np.abs(got.astype(ac.LD) - c["ref"]).astype(np.float64)
    bar = ac.moments_bar(c["n"], c["mag"])
    worst = float(np.max(err / np.where(bar > 0, bar, 1.0)))
    print(f"{name}: n {c['n']}, worst |err| / bar {worst:.3g}")
    assert (err <= bar).all(), (name, err, bar)
    again, _ = _moments(torch_gpu, name)
    same_bits(again, got, name + ": second run")                                                # fixed order: bit-equal runs


def test_layout_does_not_change_the_bits(torch_gpu):
    """The summation order depends on (npix, slots) only: one image pair through every (x, y) placement, off-alignment arms
    included, gives the same 22 x 64 bits."""
    torch = torch_gpu
    name = "layout-packed-packed"
    r, c = ac.MOMENT_ROWS[name], ac.moment_case(name)
    first = None
    for xp in ((ac.PACKED, 0), (ac.PADDED, 0), (ac.PLANAR, 0), (ac.PACKED, 4)):
        for yp in ((ac.PACKED, 0), (ac.PADDED, 0), (ac.PLANAR, 0), (ac.PADDED, 12)):
            got = _moments_of(torch, c["x"], c["y"], c["mask"], dict(r, x=xp, y=yp))
            first = got if first is None else first
            same_bits(got, first, f"{xp} {yp}")


def _moments_of(torch, x, y, mask, r):
    npix = r["npix"]
    xb, _ = _image(torch, x, r["x"])
    yb, _ = _image(torch, y, r["y"])
    mb = Buf(torch, npix, 0, mask) if mask is not None else None
    lx, ly = _lohi(torch, r["lohi_x"]), _lohi(torch, r["lohi_y"])
    nslots = ac.slots(npix)
    pb, mo, at = Buf(torch, nslots * ac.NMOM * 8, 0), Buf(torch, ac.NMOM * 8, 0), Buf(torch, 96, 0)
    xbs, xps, _ = ac.strides(r["x"][0], npix)
    ybs, yps, _ = ac.strides(r["y"][0], npix)
    LOG.call([ac.moments_instance(r)], _lib().hsr_affine_moments, xb.ptr, xbs, xps, yb.ptr, ybs, yps, _ptr(mb), npix, _ptr(lx), _ptr(ly),
             pb.ptr, None, _stream(torch))
    LOG.call([REDUCE], _lib().hsr_affine_reduce_solve, pb.ptr, nslots, 0, mo.ptr, at.ptr, _stream(torch))
    return mo.get(np.float64)


def test_zero_pixels(torch_gpu):
    """npix == 0: the moments write one slot of zeros (and record their launch), the solve gives the identity, the apply launches
    nothing and writes nothing."""
    torch = torch_gpu
    xb, pb, mo, at = Buf(torch, 64, 0), Buf(torch, ac.NMOM * 8, 0), Buf(torch, ac.NMOM * 8, 0), Buf(torch, 96, 0)
    slots = C.c_int32(-1)
    LOG.call(["affine_moments_kernel<2, 1>"], _lib().hsr_affine_moments, xb.ptr, 1, 3, xb.ptr, 1, 4, None, 0, None, None, pb.ptr,
             C.byref(slots), _stream(torch))
    assert slots.value == 1 and not pb.get(np.float64).any()
    db = Buf(torch, 64, 0)
    LOG.call(["affine_moments_f64_kernel"], _lib().hsr_affine_moments_f64, db.ptr, 3, db.ptr, 3, 0, pb.ptr, None, _stream(torch))
    assert not pb.get(np.float64).any()
    LOG.call([REDUCE], _lib().hsr_affine_reduce_solve, pb.ptr, 1, 1, mo.ptr, at.ptr, _stream(torch))
    assert not mo.get(np.float64).any() and np.array_equal(at.get(np.float64), np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]))
    ob = Buf(torch, 64, 0)
    LOG.call(None, _lib().hsr_affine_apply, xb.ptr, 1, 3, None, at.ptr, 0, None, 1, ob.ptr, 1, 3, _stream(torch))
    assert (ob.get(np.uint8) == FILL).all()


# ---- solve ------------------------------------------------------------------------------------------------------------------------------
def _solve_f64(torch, name):
    mom, at, _ = run_moments_f64(torch, ac.SOLVE_ROWS[name], ac.solve_case(name), LOG, min_count=ac.SOLVE_ROWS[name]["min_count"])
    return mom, at


@pytest.mark.parametrize("name", list(ac.SOLVE_ROWS))
def test_solve_rows(torch_gpu, name):
    """The float64 rows through hsr_affine_moments_f64 + hsr_affine_reduce_solve, against np.linalg.lstsq on the same rows; the
    host twin on the DEVICE's moments gives the device's bits."""
    r, c = ac.SOLVE_ROWS[name], ac.solve_case(name)
    mom, At = _solve_f64(torch_gpu, name)
    assert mom[9] == r["n"]
    err = np.abs(mom.astype(ac.LD) - c["mom"]).astype(np.float64)
    assert (err <= ac.moments_bar(r["n"], c["mag"])).all(), (name, err)
    from s2_emit import _engine as eng
    same_bits(At, eng.affine_solve_host(mom, r["min_count"]), name + ": host twin on the device's moments")
    if c["identity"]:
        assert np.array_equal(At, np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]))
        return
    diff = ac.grid_diff(At, c["W"])
    print(f"{name}: diff {diff:.3g}, kappa {c['kappa']:.3g}, ratio {diff * 64 / c['bar']:.2f} of 64")
    assert diff <= c["bar"], (name, diff, c["bar"])


def test_solve_through_the_image_kernel(torch_gpu):
    """The gray and the narrow rows as float32 IMAGES through hsr_affine_moments: the same bar against lstsq on the same rows."""
    torch = torch_gpu
    for name in ("gray", "narrow", "full-5000"):
        r, c = ac.SOLVE_ROWS[name], ac.solve_case(name)
        row = dict(npix=r["n"], x=(ac.PADDED, 0), y=(ac.PACKED, 0), lohi_x=None, lohi_y=None)
        mom = _moments_of(torch, c["xs"].astype(np.float32), c["ys"].astype(np.float32), None, row)
        from s2_emit import _engine as eng
        diff = ac.grid_diff(eng.affine_solve_host(mom, 0), c["W"])
        print(f"{name} (image kernel): ratio {diff * 64 / c['bar']:.2f} of 64")
        assert mom[9] == r["n"] and diff <= c["bar"], (name, diff, c["bar"])


# ---- apply ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ac.APPLY_ROWS))
def test_apply_rows(torch_gpu, name):
    same_bits(run_apply(torch_gpu, ac.APPLY_ROWS[name], ac.apply_case(name), LOG), ac.apply_case(name)["ref"], name)


def test_refused_calls_launch_nothing(torch_gpu):
    torch = torch_gpu
    xb, ob, at, pb = Buf(torch, 4096, 0), Buf(torch, 4096, 0), Buf(torch, 96, 0, np.zeros(12)), Buf(torch, ac.NMOM * 8, 0)
    st, lib = _stream(torch), _lib()
    LOG.refused(lib.hsr_affine_apply, xb.ptr, 1, 3, None, at.ptr, 10, None, 3, ob.ptr, 1, 3, st)
    LOG.refused(lib.hsr_affine_apply, xb.ptr, 1, 2, None, at.ptr, 10, None, 1, ob.ptr, 1, 3, st)
    LOG.refused(lib.hsr_affine_apply, xb.ptr, 1, 3, None, at.ptr, -1, None, 1, ob.ptr, 1, 3, st)
    LOG.refused(lib.hsr_affine_apply, xb.ptr, 1, 3, None, None, 10, None, 1, ob.ptr, 1, 3, st)
    LOG.refused(lib.hsr_affine_moments, xb.ptr, 1, 3, xb.ptr, 5, 1, None, 10, None, None, pb.ptr, None, st)
    LOG.refused(lib.hsr_affine_moments, xb.ptr, 1, 3, None, 1, 3, None, 10, None, None, pb.ptr, None, st)
    LOG.refused(lib.hsr_affine_moments_f64, xb.ptr, 2, xb.ptr, 3, 10, pb.ptr, None, st)
    LOG.refused(lib.hsr_affine_reduce_solve, pb.ptr, 0, 0, pb.ptr, at.ptr, st)
    LOG.refused(lib.hsr_affine_reduce_solve, pb.ptr, ac.MAX_SLOTS + 1, 0, pb.ptr, at.ptr, st)
    assert (ob.get(np.uint8) == FILL).all() and (pb.get(np.uint8) == FILL).all()


def test_record_keeps_the_eight_most_recent(torch_gpu):
    torch = torch_gpu
    xb, ob, at = Buf(torch, 4096, 0, np.zeros(1024, np.float32)), Buf(torch, 4096, 0), Buf(torch, 96, 0, np.zeros(12))
    st, lib = _stream(torch), _lib()
    LOG.clear()
    for k in range(10):                                  # ten launches, alternating two instances
        assert lib.hsr_affine_apply(xb.ptr, 1, 3 + k % 2, None, at.ptr, 16, None, 0, ob.ptr, 1, 3, st) == 0
    got = LOG.read()
    assert got == [f"affine_apply_kernel<{2 - k % 2}, 2>" for k in range(2, 10)], got
    assert LOG.read() is None
    ob.get(np.uint8)


def test_rows_reach_every_instance(torch_gpu):
    lib = _lib()
    n = lib.hsr_color_instance_count()
    table = {lib.hsr_color_instance_name(i).decode() for i in range(n)}
    assert len(table) == n == 20
    assert LOG.seen == table, (sorted(table - LOG.seen), sorted(LOG.seen - table))
    print("color instances seen: %d of %d" % (len(LOG.seen & table), len(table)))
