"""Graph capture and reused buffers for the launch-path entries of include/hsr_roi.h, on an MI355X: the procedure of
tests/test_gpu_graph_capture.py, as tests/test_gpu_merge_capture.py applies it, on

    hsr_roi_rasterize (centre and touched rule)     hsr_roi_class_counts     hsr_roi_glt_clip -> hsr_roi_glt_reindex (a chain)

captured once on ONE side stream in global error mode (an allocation, a synchronisation, a host-to-device copy or a launch on another
stream fails the capture or shows in the sentinel), replayed over three input sets in the same buffers, then run big -> small -> big
in buffers sized for the big shape.  The polygon's vertex and offset arrays are DEVICE memory and its counts travel by value: what
changes between replays is the content of the vertex buffer - three polygon sets of two rings, five and four vertices each.  Set 0
is a quadrilateral footprint with a hole, set 1 two separate parts elsewhere on the grid, set 2 lies over the part of the lookup
table that holds no valid entry: the clip's record is the empty range there, the re-index launch - which reads the record from
device memory - zeroes the table, and the counts, which every call clears in-stream, must not add to what the last replay left.

The row protocol (Row, Chain) is capture_cases', the buffers gpu_harness', and the procedure itself is called, not restated.  Single
branch: no parallel branches.  The module sets no environment variable.  Bar: equality of every output with the statement of
tests/roi_cases.py."""
import contextlib
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

import capture_cases as cc
import roi_cases as rc
from gpu_harness import Buf, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from s2_emit import _native as nat
import test_gpu_graph_capture as gc
from test_gpu_graph_capture import side  # noqa: F401  (side: the fixture)
from test_gpu_roi_instances import scl_plane

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

Shape = namedtuple("Shape", "H W")
GT = rc.GT_UTM
SMALL, BIG = Shape(40, 70), Shape(150, 600)
OFFSETS = np.array([0, 5, 9], np.int32)
SWATH = (211, 97)


def _window(s):
    return (2, 3, s.H - 4, s.W - 5)


def _rings(s, k):
    """Two rings of five and four vertices, as fractions of the grid; set 2 lies in the eastern quarter."""
    f = lambda pts: rc.to_world(rc._frac(s.H, s.W, pts), GT)  # noqa: E731
    return ([f([(0.1, 0.05), (0.6, 0.02), (0.7, 0.5), (0.55, 0.97), (0.04, 0.8)]), f([(0.3, 0.3), (0.32, 0.6), (0.5, 0.62), (0.48, 0.28)])],
            [f([(0.02, 0.4), (0.2, 0.1), (0.35, 0.45), (0.3, 0.9), (0.1, 0.95)]), f([(0.45, 0.1), (0.72, 0.2), (0.7, 0.85), (0.5, 0.7)])],
            [f([(0.8, 0.1), (0.97, 0.05), (0.99, 0.6), (0.9, 0.95), (0.78, 0.7)]), f([(0.85, 0.3), (0.87, 0.5), (0.93, 0.52), (0.92, 0.28)])])[k]


def _glt(s):
    g = rc.glt_of(s.H, s.W, *SWATH, seed=s.H)
    g[:, (3 * s.W) // 4:] = np.where(g[:, (3 * s.W) // 4:] > 0, 0, g[:, (3 * s.W) // 4:])     # no valid entry in the eastern quarter
    return g


def _gt():
    return (C.c_double * 6)(*GT)


class _RoiChain(cc.Chain):
    def poly(self):
        return self.ins["verts"].ptr, self.ins["offsets"].ptr, 2, 9, _gt(), self.shape.H, self.shape.W


class RasterChain(_RoiChain):
    def allocate(self, s):
        self.ins = dict(verts=Buf(self.torch, 9 * 16), offsets=Buf(self.torch, 12))
        self.outs = dict(out=(Buf(self.torch, (s.H - 4) * (s.W - 5), 3), np.uint8))

    def used(self, name):
        return (self.shape.H - 4) * (self.shape.W - 5)

    def launch(self, st):
        s = self.shape
        return [self.lib.hsr_roi_rasterize(*self.poly(), self.row.rule, *_window(s), 1, 0, self.outs["out"][0].ptr, s.W - 5, st)]


class CountsChain(_RoiChain):
    def allocate(self, s):
        self.ins = dict(verts=Buf(self.torch, 9 * 16), offsets=Buf(self.torch, 12), plane=Buf(self.torch, s.H * s.W, 1))
        self.outs = dict(counts=(Buf(self.torch, 64, 4), np.int32), inside=(Buf(self.torch, 4, 4), np.int32))

    def used(self, name):
        return dict(counts=64, inside=4)[name]

    def launch(self, st):
        s = self.shape
        return [self.lib.hsr_roi_class_counts(*self.poly(), self.row.rule, *_window(s), self.ins["plane"].ptr, s.W, self.outs["counts"][0].ptr,
                                              self.outs["inside"][0].ptr, st)]


class ClipChain(_RoiChain):
    def allocate(self, s):
        self.ins = dict(verts=Buf(self.torch, 9 * 16), offsets=Buf(self.torch, 12), glt=Buf(self.torch, s.H * s.W * 8))
        self.outs = dict(glt_out=(Buf(self.torch, (s.H - 4) * (s.W - 5) * 8, 8), np.int32), record=(Buf(self.torch, 4 * rc.RECORD, 4), np.int32))

    def used(self, name):
        return dict(glt_out=(self.shape.H - 4) * (self.shape.W - 5) * 8, record=4 * rc.RECORD)[name]

    def launch(self, st):
        s = self.shape
        _, _, h, w = _window(s)
        out, rec = self.outs["glt_out"][0].ptr, self.outs["record"][0].ptr
        return [self.lib.hsr_roi_glt_clip(*self.poly(), self.ins["glt"].ptr, *_window(s), out, rec, st),
                self.lib.hsr_roi_glt_reindex(out, h, w, rec, st)]


class _RoiRow(cc.Row):
    log = ("hsr_roi_last_launch", True)
    rule = rc.CENTER

    def make_inputs(self, s, k):
        out = dict(verts=rc.flatten(_rings(s, k))[0], offsets=OFFSETS.copy())
        assert rc.flatten(_rings(s, k))[1].tolist() == OFFSETS.tolist()
        return out

    def mask(self, s, k):
        return rc.rasterize_ref(_rings(s, k), GT, (s.H, s.W), self.rule, _window(s))

    def check(self, got, s, k, worst):
        r = self.reference(s, k)
        for name in got:
            np.testing.assert_array_equal(got[name], r[name], err_msg=f"set {k} {name}")


class RasterRow(_RoiRow):
    chain = RasterChain

    def __init__(self, name, covers, small, big, rule):
        super().__init__(name, covers, small, big)
        self.rule = rule

    def instances(self, s):
        return ["roi_raster_kernel<%s>" % ("TOUCHED" if self.rule else "CENTER")]

    def make_reference(self, s, k):
        m = self.mask(s, k)
        assert m.any() and not m.all()
        return dict(out=m.astype(np.uint8).reshape(-1))


class CountsRow(_RoiRow):
    chain, rule = CountsChain, rc.TOUCHED

    def instances(self, s):
        return ["roi_counts_kernel<TOUCHED>"]

    def make_inputs(self, s, k):
        return dict(super().make_inputs(s, k), plane=np.roll(scl_plane(s.H, s.W, 4), 7 * k, axis=1).copy())

    def make_reference(self, s, k):
        counts, inside = rc.class_counts_ref(self.inputs(s, k)["plane"], self.mask(s, k), _window(s))
        return dict(counts=counts.astype(np.int32), inside=np.array([inside], np.int32))


class ClipRow(_RoiRow):
    chain, rule = ClipChain, rc.TOUCHED

    def instances(self, s):
        return ["roi_record_init_kernel", "roi_glt_clip_kernel", "roi_glt_reindex_kernel"]

    def make_inputs(self, s, k):
        return dict(super().make_inputs(s, k), glt=_glt(s))

    def make_reference(self, s, k):
        clipped, rec = rc.glt_clip_ref(_glt(s), self.mask(s, k), _window(s))
        assert (rec[4] == 0 and rec[0] > rec[1] and rec[2] > rec[3]) if k == 2 else rec[4] > 0     # set 2: the empty range
        return dict(glt_out=rc.glt_reindex_ref(clipped, rec).reshape(-1), record=rec)


ROWS = {
    "roi-rasterize-center": RasterRow("roi-rasterize-center", ("hsr_roi_rasterize",), SMALL, BIG, rc.CENTER),
    "roi-rasterize-touched": RasterRow("roi-rasterize-touched", ("hsr_roi_rasterize",), SMALL, BIG, rc.TOUCHED),
    "roi-class-counts": CountsRow("roi-class-counts", ("hsr_roi_class_counts",), SMALL, BIG),
    "roi-glt-clip-reindex": ClipRow("roi-glt-clip-reindex", ("hsr_roi_glt_clip", "hsr_roi_glt_reindex"), SMALL, BIG),
}


def test_rows_cover_the_launch_path_entries():
    covered = {n for r in ROWS.values() for n in r.covers}
    launch_path = {n for n, (_, args) in nat.ROI_SIGNATURES.items() if args and args[-1] is C.c_void_p and not n.endswith("_host")
                   and len(args) >= 5}
    assert covered == launch_path == {"hsr_roi_rasterize", "hsr_roi_class_counts", "hsr_roi_glt_clip", "hsr_roi_glt_reindex"}
    row = ROWS["roi-glt-clip-reindex"]
    recs = [row.reference(SMALL, k)["record"].tolist() for k in cc.SETS]
    assert recs[0] != recs[1] and recs[1] != recs[2] and recs[2][:5] == [rc.I32_MAX, -1, rc.I32_MAX, -1, 0]   # the record changes between replays
    tiles = lambda s: -(-(s.H - 4) // rc.TILE_H) * -(-(s.W - 5) // rc.TILE_W)  # noqa: E731
    assert tiles(SMALL) == 1 and tiles(BIG) >= 9


@contextlib.contextmanager
def _placed(name):
    """The procedure looks its row up in capture_cases.ROWS: the row stands there for the length of one call, so that the table
    other modules are parametrised and checked by is what it was before and after."""
    assert name not in cc.ROWS
    cc.ROWS[name] = ROWS[name]
    try:
        yield
    finally:
        del cc.ROWS[name]


@pytest.mark.parametrize("name", list(ROWS))
def test_capture_and_replay(torch_gpu, side, name):
    """Eager warm-up, capture on the side stream, replays over sets 0, 1, 2, 2."""
    with _placed(name):
        gc.test_capture_and_replay(torch_gpu, side, name)


@pytest.mark.parametrize("name", list(ROWS))
def test_small_after_big_in_the_same_buffers(torch_gpu, side, name):
    """Big, small, big, small, small in buffers sized for the big shape."""
    with _placed(name):
        gc.test_small_after_big_in_the_same_buffers(torch_gpu, side, name)
