"""Every kernel instance of csrc/hsr_scl.hip - the class histograms, the buffered mask (lookup, disc, square), the mask on the EMIT
grid, the byte gather and the blanking of a cube - on an MI355X, row by row of the tables of tests/scl_cases.py: the instance by
name (the family's launch record), every output byte equal to the NumPy reference, guard bytes and row gaps intact, inputs
unchanged.  Every comparison is an equality."""
import ctypes as C

import numpy as np
import pytest

import scl_cases as sc
from gpu_harness import Buf, LaunchLog, bits_equal, lib, stream, torch_gpu  # noqa: F401  (torch_gpu: the fixture)

pytestmark = pytest.mark.gpu

LOG = LaunchLog("hsr_scl_last_launch", joined=True)


@pytest.mark.parametrize("name", list(sc.COUNT_ROWS))
def test_class_counts(torch_gpu, name):
    torch = torch_gpu
    H, W, rs, th, tw, off = sc.COUNT_ROWS[name]
    scl = sc.count_plane(name)
    src = Buf(torch, (H - 1) * rs + W, off, sc.strided(scl, rs, 9))
    ref = sc.counts_ref(scl, th, tw)
    out = Buf(torch, ref.size * 4)
    LOG.call(["scl_counts_kernel"], lib().hsr_scl_class_counts, src.ptr, H, W, rs, th, tw, out.ptr, stream(torch))
    np.testing.assert_array_equal(out.get(np.int32).reshape(ref.shape), ref)
    np.testing.assert_array_equal(sc.unstrided(src.get(np.uint8), H, W, rs)[0], scl)


@pytest.mark.parametrize("name", list(sc.MASK_ROWS))
def test_mask(torch_gpu, name):
    torch, r = torch_gpu, sc.MASK_ROWS[name]
    H, W, rs, mrs = r["H"], r["W"], r["rs"], r["mrs"]
    scl = sc.mask_plane(name)
    src = Buf(torch, (H - 1) * rs + W, r["off"], sc.strided(scl, rs, 9))     # the gaps hold a grow class: not part of the plane
    out = Buf(torch, (H - 1) * mrs + W, r["off"])
    LOG.call([sc.mask_instance(r["r"], r["shape"])], lib().hsr_scl_mask, src.ptr, H, W, rs, r["grow"], r["flat"], r["r"], r["shape"],
             out.ptr, mrs, stream(torch))
    got, gaps = sc.unstrided(out.get(np.uint8), H, W, mrs)
    np.testing.assert_array_equal(got, sc.mask_ref(name))
    assert (gaps == sc.SENT).all()
    np.testing.assert_array_equal(sc.unstrided(src.get(np.uint8), H, W, rs)[0], scl)


@pytest.mark.parametrize("name", list(sc.COARSE_ROWS))
def test_coarse(torch_gpu, name):
    torch, r = torch_gpu, sc.COARSE_ROWS[name]
    H, W, rs, k = r["H"], r["W"], r["rs"], r["k"]
    m = sc.coarse_plane(name)
    clear, bad, win = sc.coarse_ref(m, k, r["max_bad"], r["cell"])
    src = Buf(torch, (H - 1) * rs + W, 0, sc.strided(m, rs, 1))
    o_clear, o_bad = Buf(torch, clear.size), Buf(torch, bad.size, 3)
    o_win = Buf(torch, win.size * 4) if win is not None else None
    ch, cw = r["cell"] or (0, 0)
    LOG.call(["scl_coarse_kernel"], lib().hsr_scl_coarse, src.ptr, H, W, rs, k, r["max_bad"], o_clear.ptr, o_bad.ptr if r["cell_bad"] else None,
             ch, cw, o_win.ptr if o_win else None, stream(torch))
    np.testing.assert_array_equal(o_clear.get(np.uint8).reshape(clear.shape), clear)
    if r["cell_bad"]:
        np.testing.assert_array_equal(o_bad.get(np.uint8).reshape(bad.shape), bad)
    else:
        assert (o_bad.get(np.uint8) == sc.SENT).all()
    if win is not None:
        np.testing.assert_array_equal(o_win.get(np.int32).reshape(win.shape), win)


@pytest.mark.parametrize("name", list(sc.GATHER_ROWS))
def test_gather(torch_gpu, name):
    torch = torch_gpu
    H, W, rs, th, tw, origins = sc.GATHER_ROWS[name]
    plane = sc.gather_plane(name)
    ref = sc.gather_ref(plane, origins, th, tw)
    src = Buf(torch, (H - 1) * rs + W, 1, sc.strided(plane, rs))
    org = Buf(torch, len(origins) * 8, 0, np.array(origins, dtype=np.int64).astype(np.int32))
    out = Buf(torch, ref.size, 5)
    LOG.call(["scl_gather_kernel"], lib().hsr_scl_gather_tiles, src.ptr, H, W, rs, org.ptr, len(origins), th, tw, out.ptr, stream(torch))
    np.testing.assert_array_equal(out.get(np.uint8).reshape(ref.shape), ref)       # a skipped window keeps the sentinel


@pytest.mark.parametrize("name", list(sc.APPLY_ROWS))
def test_apply(torch_gpu, name):
    torch = torch_gpu
    T, H, W, rs, bs, up, fill, _ = sc.APPLY_ROWS[name]
    c = sc.apply_case(name)
    Hm, Wm = c["mask"].shape
    flat = np.full((T - 1) * bs + (H - 1) * rs + W, np.float32(123.5), dtype=np.float32)
    for t in range(T):
        for y in range(H):
            flat[t * bs + y * rs: t * bs + y * rs + W] = c["cube"][t, y]
    cube = Buf(torch, flat.size * 4, 0, flat)
    mask = Buf(torch, (Hm - 1) * c["mrs"] + Wm, 3, sc.strided(c["mask"], c["mrs"], 1))
    want = flat.copy()
    for t in range(T):
        for y in range(H):
            want[t * bs + y * rs: t * bs + y * rs + W] = c["ref"][t, y]
    for with_count in (True, False):
        cube.put(flat)
        count = Buf(torch, 8, 8)
        LOG.call(["scl_apply_kernel<UP%d>" % up], lib().hsr_scl_apply, cube.ptr, T, H, W, bs, rs, mask.ptr, Hm, Wm, c["mrs"], up,
                 C.c_float(fill), count.ptr if with_count else None, stream(torch))
        bits_equal(cube.get(np.float32), want, name)          # the filled elements, and every other element and gap bit for bit
        if with_count:
            assert int(count.get(np.int64)[0]) == c["count"]
        else:
            assert (count.get(np.uint8) == sc.SENT).all()


def test_every_instance_was_launched():
    """Runs last: every name of the instance table was recorded by some row above."""
    assert LOG.seen == set(sc.all_instances()), sorted(set(sc.all_instances()) - LOG.seen)
