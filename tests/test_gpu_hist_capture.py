"""Graph capture and a reused workspace for the histogram-matching chain (include/hsr_hist.h), on an MI355X: the procedure of
tests/test_gpu_graph_capture.py, as tests/test_gpu_s2stack_capture.py applies it, on

    hsr_hist_match      = keys -> 4 x (count, scan, scatter) -> pivots -> lookup: fifteen launches and one memset node
    hsr_hist_keys -> hsr_hist_sort -> hsr_hist_lookup      the same chain as three entries in buffers of the caller
    hsr_hist_keys -> 4 x hsr_hist_sort_pass -> hsr_hist_lookup      ... and with the sort as its four passes

captured once on ONE side stream in global error mode (an allocation, a synchronisation or a launch on another stream fails the
capture or shows in the sentinel), replayed over three input sets in the same buffers, then run big -> small -> big in a workspace
sized for the big shape.  The counts are device data: the sets' masks give different n - set 0 every pixel, set 1 about 40 % with
non-finite samples inside the mask, set 2 about 70 % and a channel whose reference is NaN throughout (n == 0: it passes through) -
and the pivot tables, the top level and every search bound follow them without a host round trip.  The counts are cleared in-stream
by every call: a replay after set 1 must not add to what set 1 left.

The row protocol (Row, Chain) is capture_cases', the buffers gpu_harness', and the procedure itself is called, not restated.  The
chain is a chain: no parallel branches.  The module sets no environment variable.  Bar: equality by value with the statement of
tests/hist_cases.py and bit equality with an eager call on fresh buffers."""
import contextlib
from collections import namedtuple

import numpy as np
import pytest

import capture_cases as cc
import hist_cases as hc
from gpu_harness import Buf, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
import test_gpu_graph_capture as gc
from test_gpu_graph_capture import side  # noqa: F401  (side: the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

Shape = namedtuple("Shape", "npix C")
SMALL, BIG = Shape(hc.PIVOT + 45, 3), Shape(2 * hc.TILE + 19, 3)


def _inputs(s, k):
    rng = np.random.default_rng(190 + 7 * k + s.npix)
    src = (rng.random((s.npix, s.C)) * 1.2 - 0.1).astype(np.float32)
    ref = (np.round(rng.random((s.npix, s.C)) ** 2 * 64) / 64).astype(np.float32)
    if k == 0:
        mask = np.ones(s.npix, np.uint8)
    elif k == 1:
        mask = (rng.random(s.npix) < 0.4).astype(np.uint8)
        src[3::17, 0], ref[5::19, 1] = np.nan, -np.inf
    else:
        mask = (rng.random(s.npix) < 0.7).astype(np.uint8)
        ref[:, 2] = np.nan
    return dict(src=src, ref=ref, mask=mask)


class HistChain(cc.Chain):
    def allocate(self, s):
        B = lambda n, off=0: Buf(self.torch, n, off)  # noqa: E731
        self.ins = dict(src=B(4 * s.npix * s.C), ref=B(4 * s.npix * s.C, 4), mask=B(s.npix, 1))
        self.outs = dict(out=(B(4 * s.npix * s.C, 4), np.float32), n_valid=(B(8 * s.C, 8), np.int64))
        self.work = dict(work=B(self.lib.hsr_hist_scratch_bytes(s.npix, s.C)))

    def used(self, name):
        return dict(out=4 * self.shape.npix * self.shape.C, n_valid=8 * self.shape.C)[name]

    def launch(self, st):
        s, i, o, lib = self.shape, self.ins, self.outs, self.lib
        work = self.work["work"]
        if not self.row.pieces:
            return [lib.hsr_hist_match(i["src"].ptr, 1, s.C, i["ref"].ptr, 1, s.C, i["mask"].ptr, s.npix, s.C, o["out"][0].ptr, 1, s.C,
                                       o["n_valid"][0].ptr, work.ptr, lib.hsr_hist_scratch_bytes(s.npix, s.C), st)]
        # the caller's own partition of the same workspace: keys, tmp, counters, pivots
        stride = lib.hsr_hist_plane_stride(s.npix)
        planes = 2 * s.C * stride * 4
        cbytes, pbytes = lib.hsr_hist_sort_bytes(s.npix, 2 * s.C), lib.hsr_hist_pivot_bytes(s.npix, s.C)
        base = work.ptr.value
        keys, tmp, counters, pivots = base, base + planes, base + 2 * planes, base + 2 * planes + cbytes
        assert 2 * planes + cbytes + pbytes <= work.nbytes
        rcs = [lib.hsr_hist_keys(i["src"].ptr, 1, s.C, i["ref"].ptr, 1, s.C, i["mask"].ptr, s.npix, s.C, keys, stride, o["n_valid"][0].ptr, st)]
        if self.row.pieces == "passes":
            for p, (a, b) in enumerate(((keys, tmp), (tmp, keys), (keys, tmp), (tmp, keys))):
                rcs.append(lib.hsr_hist_sort_pass(a, b, stride, s.npix, 2 * s.C, p, counters, cbytes, st))
        else:
            rcs.append(lib.hsr_hist_sort(keys, tmp, stride, s.npix, 2 * s.C, counters, cbytes, st))
        rcs.append(lib.hsr_hist_lookup(keys, stride, o["n_valid"][0].ptr, pivots, pbytes, i["src"].ptr, 1, s.C, i["ref"].ptr, 1, s.C, i["mask"].ptr,
                                       s.npix, s.C, o["out"][0].ptr, 1, s.C, st))
        return rcs


class HistRow(cc.Row):
    chain, log = HistChain, ("hsr_hist_last_launch", True)

    def __init__(self, name, covers, small, big, pieces):
        super().__init__(name, covers, small, big)
        self.pieces = pieces

    def instances(self, s):
        return ["hist_keys_kernel<PIXMAJOR>"] + hc.sort_record() + ["hist_pivots_kernel", "hist_lookup_kernel<PIXMAJOR>"]

    def make_inputs(self, s, k):
        return _inputs(s, k)

    def make_reference(self, s, k):
        i = self.inputs(s, k)
        out, counts = hc.match_planes(i["src"].T, i["ref"].T, i["mask"] != 0)
        return dict(out=np.ascontiguousarray(out.T), n_valid=counts)

    def check(self, got, s, k, worst):
        r = self.reference(s, k)
        n = r["n_valid"]
        # the sets do what they are for
        assert ((n == s.npix).all(), (n > 0).all() and (n < s.npix // 2).all() and len(set(n.tolist())) > 1, n[2] == 0 and (n[:2] > s.npix // 2).all())[k], (k, n)
        np.testing.assert_array_equal(got["n_valid"], n, err_msg=f"set {k} counts")
        hc.equal_by_value(got["out"].reshape(s.npix, s.C), r["out"], f"set {k} out")


ROWS = {"hist-match": HistRow("hist-match", ("hsr_hist_match",), SMALL, BIG, False),
        "hist-pieces": HistRow("hist-pieces", ("hsr_hist_keys", "hsr_hist_sort", "hsr_hist_lookup"), SMALL, BIG, "entries"),
        "hist-passes": HistRow("hist-passes", ("hsr_hist_keys", "hsr_hist_sort_pass", "hsr_hist_lookup"), SMALL, BIG, "passes")}


def test_rows_cover_the_launch_path_entries():
    from s2_emit import _native as nat
    covered = {n for r in ROWS.values() for n in r.covers}
    launch_path = {n for n, (_, args) in nat.HIST_SIGNATURES.items() if len(args) > 2 and not n.endswith("_host") and "last_launch" not in n}
    assert covered == launch_path == {"hsr_hist_keys", "hsr_hist_sort", "hsr_hist_sort_pass", "hsr_hist_lookup", "hsr_hist_match"}
    tiles = lambda s: -(-s.npix // hc.TILE)  # noqa: E731
    assert tiles(SMALL) == 1 and tiles(BIG) == 3 and SMALL.npix > hc.PIVOT          # the small shape has a pivot level at set 0 ...
    assert _inputs(SMALL, 1)["mask"].sum() < hc.PIVOT                                # ... and none at set 1: the top level follows n


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
    """Big, small, big, small, small in a workspace sized for the big shape."""
    with _placed(name):
        gc.test_small_after_big_in_the_same_buffers(torch_gpu, side, name)
