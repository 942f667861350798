"""Every kernel instance of csrc/hsr_roi.hip - the rasteriser and the class histogram under the centre and the touched rule, the GLT
clip with its record and the re-index - on an MI355X, row by row of the table of tests/roi_cases.py, against the host twin and the
NumPy statement.

The entries are called through ctypes.  Every vertex array, plane, table and output lies `off` bytes past a 256-byte boundary in a
buffer filled with a sentinel byte, between two guard zones (Buf of gpu_harness.py): nothing outside an output may be written, and
every byte of it must be - also the padding of a row stride must keep the sentinel.  After every call the library's launch record
(hsr_roi_last_launch) is compared with the instances the entry must launch.  device == host twin == statement, as bytes and int32
bits.  The last test checks that the rows reached every name hsr_roi_instance_name enumerates."""
import ctypes as C

import numpy as np
import pytest

import roi_cases as rc
from gpu_harness import FILL, Buf, LaunchLog, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from gpu_harness import lib as _lib, stream as _stream
from test_roi_host import CLIP_ROWS, run_clip_host, run_host

pytestmark = pytest.mark.gpu

LOG = LaunchLog("hsr_roi_last_launch", joined=True)
RULE_NAMES = {rc.CENTER: "CENTER", rc.TOUCHED: "TOUCHED"}


def _gt(gt):
    return (C.c_double * 6)(*gt)


def poly_bufs(torch, rings):
    verts, offs = rc.flatten(rings)
    return Buf(torch, verts.nbytes, 0, verts), Buf(torch, offs.nbytes, 0, offs), len(offs) - 1, len(verts)


def strided(raw, h, w, rs):
    """The (h, w) part of a buffer of (h - 1) rs + w bytes, after checking that the stride's padding holds the sentinel."""
    full = np.full(h * rs, FILL, np.uint8)
    full[: raw.size] = raw
    full = full.reshape(h, rs)
    assert (full[:, w:] == FILL).all(), "write into the padding of the row stride"
    return full[:, :w]


def run_raster(torch, r, rule, inside=1, outside=0):
    vb, fb, nr, nv = poly_bufs(torch, r["rings"])
    r0, c0, h, w = rc.window_of(r)
    rs = w + r["pad"]
    ob = Buf(torch, (h - 1) * rs + w, r["off"])
    LOG.call(["roi_raster_kernel<%s>" % RULE_NAMES[rule]], _lib().hsr_roi_rasterize, vb.ptr, fb.ptr, nr, nv, _gt(r["gt"]), r["H"], r["W"], rule,
             r0, c0, h, w, inside, outside, ob.ptr, rs, _stream(torch))
    vb.get(np.uint8), fb.get(np.uint8)
    return strided(ob.get(np.uint8), h, w, rs)


def scl_plane(H, W, seed):
    """Every class value 0 .. 11 and values above, in patches and in noise."""
    rng = np.random.default_rng(seed)
    values = np.array(list(range(12)) + [12, 13, 200, 255], np.uint8)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    plane = values[((yy // 3) * 5 + xx // 4) % len(values)]
    noise = rng.random((H, W)) < 0.3
    plane[noise] = values[rng.integers(0, len(values), int(noise.sum()))]
    return plane


def run_counts(torch, r, rule, plane):
    vb, fb, nr, nv = poly_bufs(torch, r["rings"])
    r0, c0, h, w = rc.window_of(r)
    rs = r["W"] + r["pad"]
    host = np.full((r["H"] - 1) * rs + r["W"], FILL, np.uint8)
    for y in range(r["H"]):
        host[y * rs: y * rs + r["W"]] = plane[y]
    pb, cb, ib = Buf(torch, host.size, r["off"], host), Buf(torch, 64, 4), Buf(torch, 4, 4)      # the sentinel: the call has to zero them
    LOG.call(["roi_counts_kernel<%s>" % RULE_NAMES[rule]], _lib().hsr_roi_class_counts, vb.ptr, fb.ptr, nr, nv, _gt(r["gt"]), r["H"], r["W"],
             rule, r0, c0, h, w, pb.ptr, rs, cb.ptr, ib.ptr, _stream(torch))
    assert np.array_equal(pb.get(np.uint8), host)
    return cb.get(np.int32).astype(np.int64), int(ib.get(np.int32)[0])


@pytest.mark.parametrize("rule", list(rc.RULES))
@pytest.mark.parametrize("name", list(rc.ROWS))
def test_raster_rows(torch_gpu, name, rule):
    r, rule = rc.ROWS[name], rc.RULES[rule]
    got = run_raster(torch_gpu, r, rule)
    np.testing.assert_array_equal(got, run_host(r, rule))
    np.testing.assert_array_equal(got, rc.case(name, rule).astype(np.uint8))


@pytest.mark.parametrize("name", list(rc.SWEEP))
def test_raster_sweep(torch_gpu, name):
    r = rc.SWEEP[name]
    for rule in (rc.CENTER, rc.TOUCHED):
        got = run_raster(torch_gpu, r, rule, 0, 1)
        np.testing.assert_array_equal(got, run_host(r, rule, 0, 1))
        np.testing.assert_array_equal(got, (~rc.rasterize_ref(r["rings"], r["gt"], (r["H"], r["W"]), rule, r["window"])).astype(np.uint8))


def test_raster_values(torch_gpu):
    r = rc.ROWS["w256-aligned"]
    for rule in (rc.CENTER, rc.TOUCHED):
        ref = rc.case("w256-aligned", rule)
        np.testing.assert_array_equal(run_raster(torch_gpu, r, rule, 7, 200), np.where(ref, 7, 200).astype(np.uint8))
        np.testing.assert_array_equal(run_raster(torch_gpu, r, rule, 255, 255), np.full(ref.shape, 255, np.uint8))


@pytest.mark.parametrize("rule", list(rc.RULES))
@pytest.mark.parametrize("name", list(rc.ROWS))
def test_counts_rows(torch_gpu, name, rule):
    r, rule = rc.ROWS[name], rc.RULES[rule]
    plane = scl_plane(r["H"], r["W"], len(name))
    counts, inside = run_counts(torch_gpu, r, rule, plane)
    want, n = rc.class_counts_ref(plane, rc.case(name, rule), rc.window_of(r))
    assert counts.tolist() == want.tolist() and inside == n == int(counts.sum())
    assert counts[13:].tolist() == [0, 0, 0]


@pytest.mark.parametrize("name", CLIP_ROWS)
def test_glt_clip_and_reindex_rows(torch_gpu, name):
    torch, r = torch_gpu, rc.ROWS[name]
    glt = rc.glt_of(r["H"], r["W"], 211, 97, seed=len(name))
    want, wrec, win = run_clip_host(r, glt)
    r0, c0, h, w = win
    vb, fb, nr, nv = poly_bufs(torch, r["rings"])
    gb, ob, rb = Buf(torch, glt.nbytes, 8, glt), Buf(torch, h * w * 8, 8), Buf(torch, 4 * rc.RECORD, 4)
    LOG.call(["roi_record_init_kernel", "roi_glt_clip_kernel"], _lib().hsr_roi_glt_clip, vb.ptr, fb.ptr, nr, nv, _gt(r["gt"]), r["H"], r["W"],
             gb.ptr, r0, c0, h, w, ob.ptr, rb.ptr, _stream(torch))
    np.testing.assert_array_equal(ob.get(np.int32).reshape(h, w, 2), want)
    assert rb.get(np.int32).tolist() == wrec.tolist()
    mask = rc.rasterize_ref(r["rings"], r["gt"], (r["H"], r["W"]), rc.TOUCHED, win)
    sref, srec = rc.glt_clip_ref(glt, mask, win)
    np.testing.assert_array_equal(want, sref)
    assert wrec.tolist() == srec.tolist()
    LOG.call(["roi_glt_reindex_kernel"], _lib().hsr_roi_glt_reindex, ob.ptr, h, w, rb.ptr, _stream(torch))
    np.testing.assert_array_equal(ob.get(np.int32).reshape(h, w, 2), rc.glt_reindex_ref(sref, srec))
    assert rb.get(np.int32).tolist() == wrec.tolist()
    np.testing.assert_array_equal(gb.get(np.int32).reshape(glt.shape), glt)


def test_glt_clip_empty_range(torch_gpu):
    torch, r = torch_gpu, rc.ROWS["triangle"]
    glt = np.zeros((r["H"], r["W"], 2), np.int32)
    glt[..., 0] = np.iinfo(np.int32).min
    r0, c0, h, w = rc.bbox_window(r["rings"], r["gt"], (r["H"], r["W"]))
    vb, fb, nr, nv = poly_bufs(torch, r["rings"])
    gb, ob, rb = Buf(torch, glt.nbytes, 0, glt), Buf(torch, h * w * 8), Buf(torch, 4 * rc.RECORD)
    LOG.call(["roi_record_init_kernel", "roi_glt_clip_kernel"], _lib().hsr_roi_glt_clip, vb.ptr, fb.ptr, nr, nv, _gt(r["gt"]), r["H"], r["W"],
             gb.ptr, r0, c0, h, w, ob.ptr, rb.ptr, _stream(torch))
    assert rb.get(np.int32).tolist() == [rc.I32_MAX, -1, rc.I32_MAX, -1, 0, 0, 0, 0]
    LOG.call(["roi_glt_reindex_kernel"], _lib().hsr_roi_glt_reindex, ob.ptr, h, w, rb.ptr, _stream(torch))
    assert not ob.get(np.int32).any()                                     # INT32_MIN - INT32_MAX, in 64 bits: 0


def test_device_arrays_the_check_refuses_stay_inside_their_buffers(torch_gpu):
    """Offsets that name no ring and vertices that are not finite: every edge is dropped, the plane is outside everywhere, and
    nothing is read or written outside a buffer that would show here (the guards of the outputs)."""
    torch = torch_gpu
    verts = np.array([[1.0, 1.0], [9.0, 2.0], [4.0, 8.0], [np.nan, 2.0], [3.0, np.inf], [5.0, 5.0]])
    for offs, keep in ((np.array([0, 1 << 30, -5], np.int32), False), (np.array([7, 9, 6], np.int32), False), (np.array([0, 3, 6], np.int32), True)):
        vb, fb = Buf(torch, verts.nbytes, 0, verts), Buf(torch, offs.nbytes, 0, offs)
        ob = Buf(torch, 20 * 30, 3)
        LOG.call(["roi_raster_kernel<TOUCHED>"], _lib().hsr_roi_rasterize, vb.ptr, fb.ptr, 2, 6, _gt((0.0, 1.0, 0.0, 0.0, 0.0, 1.0)), 20, 30,
                 rc.TOUCHED, 0, 0, 20, 30, 1, 0, ob.ptr, 30, _stream(torch))
        got = ob.get(np.uint8).reshape(20, 30)
        if keep:                                                          # the finite ring as it is; of the other only the edge (5, 5) -> (nan, 2) - dropped
            np.testing.assert_array_equal(got, rc.rasterize_ref([verts[:3]], (0.0, 1.0, 0.0, 0.0, 0.0, 1.0), (20, 30), rc.TOUCHED).astype(np.uint8))
        else:
            assert not got.any()


def test_refused_calls_launch_nothing(torch_gpu):
    torch, r = torch_gpu, rc.ROWS["triangle"]
    vb, fb, nr, nv = poly_bufs(torch, r["rings"])
    ob = Buf(torch, r["H"] * r["W"] * 8)
    st = _stream(torch)
    f = _lib().hsr_roi_rasterize
    ok = [vb.ptr, fb.ptr, nr, nv, _gt(r["gt"]), r["H"], r["W"], 0, 0, 0, r["H"], r["W"], 1, 0, ob.ptr, r["W"], st]
    for at, bad in ((0, None), (1, None), (2, 0), (3, 2), (3, rc.MAX_EDGES + 1), (4, None), (4, _gt((0.0, 1.0, 0.5, 0.0, 0.0, 1.0))),
                    (4, _gt((0.0, 0.0, 0.0, 0.0, 0.0, 1.0))), (5, 0), (7, 2), (8, 1), (9, -1), (10, 0), (14, None), (15, r["W"] - 1)):
        args = list(ok)
        args[at] = bad
        LOG.refused(f, *args)
    g = _lib().hsr_roi_class_counts
    okc = ok[:12] + [ob.ptr, r["W"], vb.ptr, fb.ptr, st]
    for at, bad in ((12, None), (13, r["W"] - 1), (14, None), (15, None), (7, 5)):
        args = list(okc)
        args[at] = bad
        LOG.refused(g, *args)
    k = _lib().hsr_roi_glt_clip
    glt = Buf(torch, r["H"] * r["W"] * 8)
    okk = ok[:7] + [glt.ptr, 0, 0, r["H"], r["W"], ob.ptr, vb.ptr, st]
    for at, bad in ((7, None), (12, None), (13, None), (12, glt.ptr), (12, C.c_void_p(ob.ptr.value + 4)), (10, r["H"] + 1)):
        args = list(okk)
        args[at] = bad
        LOG.refused(k, *args)
    x = _lib().hsr_roi_glt_reindex
    for args in ((None, 3, 3, vb.ptr, st), (ob.ptr, 0, 3, vb.ptr, st), (ob.ptr, 3, 3, None, st), (C.c_void_p(ob.ptr.value + 4), 3, 3, vb.ptr, st)):
        LOG.refused(x, *args)
    assert (ob.get(np.uint8) == FILL).all() and (glt.get(np.uint8) == FILL).all()


def test_rows_reach_every_instance(torch_gpu):
    lib = _lib()
    n = lib.hsr_roi_instance_count()
    assert n == rc.INSTANCE_COUNT
    table = {lib.hsr_roi_instance_name(i).decode() for i in range(n)}
    assert len(table) == n
    assert LOG.seen == table, (sorted(table - LOG.seen), sorted(LOG.seen - table))
    print("roi instances seen: %d of %d" % (len(LOG.seen & table), len(table)))
