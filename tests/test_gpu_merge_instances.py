"""Every kernel instance of csrc/hsr_merge.hip - the merging gather of N swaths, band-interleaved and band-sequential, with and
without masks, and the streaming select over N scenes with its source plane - on an MI355X, row by row of the table of
tests/merge_cases.py, against its NumPy statement.

hsr_ortho_merge and hsr_merge_scenes are called through ctypes.  Every swath, scene and output lies `off` bytes past a 256-byte
boundary in a buffer filled with a sentinel byte, between two guard zones (Buf of gpu_harness.py): nothing outside an output may be
written, and every byte of it must be.  After every call the library's launch record (hsr_merge_last_launch) is compared with the
instances the row expects, computed by merge_cases' mirror of the selection rule.  Outputs are compared as uint32 bits; the dropped
counts are exact per source.  The last test checks that the rows reached every name hsr_merge_instance_name enumerates."""
import ctypes as C

import numpy as np
import pytest

import merge_cases as mc
from gpu_harness import FILL, Buf, LaunchLog, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from gpu_harness import lib as _lib, stream as _stream
from s2_emit import _native as nat

pytestmark = pytest.mark.gpu

LOG = LaunchLog("hsr_merge_last_launch", joined=True)


def _shape(r, layout=None):
    layout = r["layout"] if layout is None else layout
    return (r["H"], r["W"], r["bands"]) if layout == mc.BIP else (r["bands"], r["H"], r["W"])


def run_ortho_merge(torch, name, order=None, source=True):
    """The row through hsr_ortho_merge, its sources in `order` -> (bits in the row's layout, dropped per source or None, plane)."""
    r, c = mc.ROWS[name], mc.case(name)
    order = list(range(len(r["sources"]))) if order is None else order
    bufs, table = [], []
    for k in order:
        s, rows_cols = r["sources"][k], mc.swath_dims(k)
        sb, gb = Buf(torch, c["swaths"][k].nbytes, s["off"], c["swaths"][k]), Buf(torch, c["glts"][k].nbytes, 0, c["glts"][k])
        qb = Buf(torch, c["qmasks"][k].nbytes, 0, c["qmasks"][k]) if s["q"] else None
        bb = Buf(torch, c["bmasks"][k].nbytes, 0, c["bmasks"][k]) if s["bm"] else None
        bufs.append((sb, gb, qb, bb, c["swaths"][k]))
        table.append(nat.MergeSwath(sb.ptr, gb.ptr, qb.ptr if qb else None, bb.ptr if bb else None, rows_cols[0], rows_cols[1], s["gh"], s["gw"],
                                    s["oy"], s["ox"], c["bmasks"][k].shape[2] if s["bm"] else 0, r["bands"]))
    n = len(table)
    ob = Buf(torch, r["H"] * r["W"] * r["bands"] * 4, r["out_off"])
    db = Buf(torch, 8 * n, 8) if r["count"] else None                      # holds the sentinel: the call has to zero it
    pb = Buf(torch, r["H"] * r["W"], 1) if source else None
    expect = mc.ortho_merge_instance(r["layout"], r["bands"], mc.row_mask(r), [r["sources"][k]["off"] for k in order], r["out_off"])
    LOG.call([expect], _lib().hsr_ortho_merge, (nat.MergeSwath * n)(*table), n, 0, r["layout"], r["H"], r["W"], C.c_float(r["nodata"]),
             C.c_float(r["masked"]), ob.ptr, db.ptr if db else None, pb.ptr if pb else None, _stream(torch))
    got = ob.get(np.uint32).reshape(_shape(r))
    for sb, gb, qb, bb, swath in bufs:                                    # the inputs and their guards are as they were
        for b in (gb, qb, bb):
            if b is not None:
                b.get(np.uint8)
        np.testing.assert_array_equal(sb.get(np.float32).view(np.uint32), swath.view(np.uint32).reshape(-1))
    return got, (db.get(np.int64).tolist() if db else None), (pb.get(np.uint8).reshape(r["H"], r["W"]) if pb else None)


def run_merge_scenes(torch, name, order=None, source=True):
    """The row's per-source scenes (the statement's) through hsr_merge_scenes -> (bits in the row's layout, plane)."""
    r, c = mc.ROWS[name], mc.case(name)
    order = list(range(len(r["sources"]))) if order is None else order
    bufs, table = [], []
    for k in order:
        s, scene = r["sources"][k], mc.in_layout(c["scenes"][k], r["layout"])
        sb = Buf(torch, scene.nbytes, s["off"] + 4 * (k % 3), scene)       # scenes on and off 16 bytes
        bufs.append((sb, scene))
        table.append(nat.MergeScene(sb.ptr, s["gh"], s["gw"], s["oy"], s["ox"], r["bands"], 0))
    n = len(table)
    ob = Buf(torch, r["H"] * r["W"] * r["bands"] * 4, r["out_off"])
    pb = Buf(torch, r["H"] * r["W"], 1) if source else None
    LOG.call(mc.merge_scenes_instances(source), _lib().hsr_merge_scenes, (nat.MergeScene * n)(*table), n, r["layout"], r["H"], r["W"],
             C.c_float(r["nodata"]), int(r["nan"]), ob.ptr, pb.ptr if pb else None, _stream(torch))
    got = ob.get(np.uint32).reshape(_shape(r))
    for sb, scene in bufs:
        np.testing.assert_array_equal(sb.get(np.float32).view(np.uint32), scene.view(np.uint32).reshape(-1))
    return got, (pb.get(np.uint8).reshape(r["H"], r["W"]) if pb else None)


@pytest.mark.parametrize("name", mc.ORTHO_ROWS)
def test_ortho_merge_rows(torch_gpu, name):
    r, c = mc.ROWS[name], mc.case(name)
    got, dropped, plane = run_ortho_merge(torch_gpu, name)
    np.testing.assert_array_equal(got, c["ref"])
    assert dropped == (c["dropped"] if r["count"] else None)
    np.testing.assert_array_equal(plane, c["source"])


@pytest.mark.parametrize("name", list(mc.ROWS))
def test_merge_scenes_rows(torch_gpu, name):
    c = mc.case(name)
    got, plane = run_merge_scenes(torch_gpu, name)
    np.testing.assert_array_equal(got, c["ref"])
    np.testing.assert_array_equal(plane, c["source"])


@pytest.mark.parametrize("name", ["identical-bip", "identical-bsq", "n3-dropped-bip", "n8-bsq", "empty-bmask-bsq", "masked-wins-bip"])
def test_order_dependence_and_no_source_plane(torch_gpu, name):
    """The sources in reverse order: the other source's bits; without a source plane: the same scene."""
    r, c = mc.ROWS[name], mc.case(name)
    order = list(range(len(r["sources"])))[::-1]
    ref_bip, src = mc.merge_ref([c["scenes"][k] for k in order], [c["offsets"][k] for k in order], (r["H"], r["W"]), r["nodata"])
    ref = mc.in_layout(ref_bip, r["layout"])
    assert name.startswith("n3-dropped") or (ref != c["ref"]).any()         # n3-dropped: one source supplies everything; its counts swap
    got, dropped, plane = run_ortho_merge(torch_gpu, name, order, source=False)
    np.testing.assert_array_equal(got, ref)
    assert dropped == [c["dropped"][k] for k in order] and plane is None
    got, plane = run_merge_scenes(torch_gpu, name, order)
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(plane, src)
    got, plane = run_merge_scenes(torch_gpu, name, order, source=False)
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("name", [n for n in mc.ROWS if n.startswith("n1-")])
def test_one_source_at_the_origin_is_hsr_ortho_glt(torch_gpu, name):
    """The same buffers through hsr_ortho_glt: the scene and the count, bit for bit."""
    torch, r, c = torch_gpu, mc.ROWS[name], mc.case(name)
    s, (rows, cols) = r["sources"][0], mc.swath_dims(0)
    sb, gb = Buf(torch, c["swaths"][0].nbytes, s["off"], c["swaths"][0]), Buf(torch, c["glts"][0].nbytes, 0, c["glts"][0])
    qb = Buf(torch, c["qmasks"][0].nbytes, 0, c["qmasks"][0]) if s["q"] else None
    bb = Buf(torch, c["bmasks"][0].nbytes, 0, c["bmasks"][0]) if s["bm"] else None
    ob, db = Buf(torch, r["H"] * r["W"] * r["bands"] * 4, r["out_off"]), Buf(torch, 8, 8)
    rc = _lib().hsr_ortho_glt(sb.ptr, rows, cols, r["bands"], gb.ptr, s["gh"], s["gw"], 0, 0, 0, s["gh"], s["gw"], qb.ptr if qb else None,
                              bb.ptr if bb else None, c["bmasks"][0].shape[2] if s["bm"] else 0, r["nodata"], r["masked"], r["layout"], ob.ptr,
                              db.ptr, _stream(torch))
    assert rc == 0, _lib().hsr_last_error()
    got, dropped, _ = run_ortho_merge(torch, name)
    np.testing.assert_array_equal(got.reshape(-1), ob.get(np.uint32))
    assert dropped == db.get(np.int64).tolist()


def test_refused_calls_launch_nothing(torch_gpu):
    torch = torch_gpu
    r, c = mc.ROWS["nomask-b3-bip"], mc.case("nomask-b3-bip")
    n_out = r["H"] * r["W"] * r["bands"] * 4
    big = Buf(torch, 4 * n_out)                                            # output and "inputs" inside one allocation: overlaps on demand
    sb = [Buf(torch, c["swaths"][k].nbytes, 0, c["swaths"][k]) for k in range(2)]
    gb = [Buf(torch, c["glts"][k].nbytes, 0, c["glts"][k]) for k in range(2)]
    st = _stream(torch)

    def swaths(**kw):
        rows = []
        for k, s in enumerate(r["sources"]):
            f = dict(swath_dev=sb[k].ptr, glt_dev=gb[k].ptr, qmask_dev=None, bmask_dev=None, rows=mc.swath_dims(k)[0], cols=mc.swath_dims(k)[1],
                     glt_h=s["gh"], glt_w=s["gw"], off_y=s["oy"], off_x=s["ox"], bmask_bytes=0, bands=r["bands"])
            if k == 1:
                f.update(kw)
            rows.append(nat.MergeSwath(**f))
        return (nat.MergeSwath * 2)(*rows)

    f = _lib().hsr_ortho_merge
    ok = [swaths(), 2, 0, 0, r["H"], r["W"], C.c_float(-9999.0), C.c_float(-9999.0), big.ptr, None, None, st]
    inside = C.c_void_p(big.ptr.value + n_out - 4)
    for at, bad in ((0, None), (1, 0), (1, 9), (3, 2), (4, 0), (5, 0), (8, None), (0, swaths(bands=4)), (0, swaths(swath_dev=None)),
                    (0, swaths(glt_dev=None)), (0, swaths(rows=0)), (0, swaths(glt_w=0)), (0, swaths(bmask_dev=gb[0].ptr, bmask_bytes=0)),
                    (0, swaths(swath_dev=inside)), (0, swaths(glt_dev=inside)), (9, inside), (10, inside)):
        args = list(ok)
        args[at] = bad
        LOG.refused(f, *args)
    scenes = [mc.in_layout(s, mc.BIP) for s in c["scenes"]]
    cb = [Buf(torch, s.nbytes, 0, s) for s in scenes]

    def table(**kw):
        rows = []
        for k, s in enumerate(r["sources"]):
            fld = dict(scene_dev=cb[k].ptr, h=s["gh"], w=s["gw"], off_y=s["oy"], off_x=s["ox"], bands=r["bands"], reserved=0)
            if k == 1:
                fld.update(kw)
            rows.append(nat.MergeScene(**fld))
        return (nat.MergeScene * 2)(*rows)

    g = _lib().hsr_merge_scenes
    ok2 = [table(), 2, 0, r["H"], r["W"], C.c_float(-9999.0), 0, big.ptr, None, st]
    for at, bad in ((0, None), (1, 0), (1, 9), (2, 2), (3, 0), (4, -1), (7, None), (7, C.c_void_p(big.ptr.value + 2)), (0, table(bands=2)),
                    (0, table(scene_dev=None)), (0, table(h=0)), (0, table(scene_dev=inside)), (8, inside),
                    (0, table(scene_dev=C.c_void_p(cb[1].ptr.value + 1)))):
        args = list(ok2)
        args[at] = bad
        LOG.refused(g, *args)
    assert (big.get(np.uint8) == FILL).all()
    LOG.call([mc.ortho_merge_instance(mc.BIP, 3, False)], f, *ok)
    LOG.call(mc.merge_scenes_instances(False), g, *ok2)
    np.testing.assert_array_equal(big.get(np.uint32)[: n_out // 4], c["ref"].reshape(-1))


def test_rows_reach_every_instance(torch_gpu):
    lib = _lib()
    n = lib.hsr_merge_instance_count()
    assert n == mc.INSTANCE_COUNT
    table = {lib.hsr_merge_instance_name(i).decode() for i in range(n)}
    assert len(table) == n
    assert LOG.seen == table, (sorted(table - LOG.seen), sorted(LOG.seen - table))
    print("merge instances seen: %d of %d" % (len(LOG.seen & table), len(table)))
