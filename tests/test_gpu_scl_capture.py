"""Graph capture and reused buffers for the scene-classification entries (include/hsr_scl.h), on an MI355X: the procedure of
tests/test_gpu_graph_capture.py on the chain

    hsr_scl_class_counts -> hsr_scl_mask -> hsr_scl_coarse -> hsr_scl_gather_tiles -> hsr_scl_apply

captured once on ONE side stream in global error mode (an allocation, a synchronisation or a launch on another stream fails the
capture or shows in the sentinel), replayed over three input sets in the same buffers, then run big -> small -> big in buffers
sized for the big shape.  The sets flip the chain's DEVICE-side decisions: 0 cloudy - workgroups with and without flags, cells
of both kinds, stores under the mask; 1 clear - every workgroup of the mask takes the early exit and the apply stores nothing;
2 everything bad - every cell counts and every element of the cube is filled.  The histogram, the window counts and the filled
count are cleared in-stream by every call: a replay after set 2 must not add to what set 2 left.

The row protocol (Row, Chain) is capture_cases', the buffers gpu_harness', and the procedure itself is called, not restated; the
row lives here because capture_cases' table is pinned to the entry points of hsr.h.  The chain is a chain: no parallel branches.
The module sets no environment variable.  Bar: equality of every output with tests/scl_cases.py's references."""
import contextlib
from collections import namedtuple

import numpy as np
import pytest

import capture_cases as cc
import scl_cases as sc
from gpu_harness import Buf, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
import test_gpu_graph_capture as gc
from test_gpu_graph_capture import side  # noqa: F401  (side: the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

Shape = namedtuple("Shape", "H W")
SMALL, BIG = Shape(45, 100), Shape(70, 150)
T, UP, K, MAX_BAD, CE, R, TH, TW, TILE = 2, 2, 3, 1, 4, 3, 4, 4, (8, 16)
NAMES = ["scl_counts_kernel", "scl_mask_kernel<DISC>", "scl_coarse_kernel", "scl_gather_kernel", "scl_apply_kernel<UP2>"]


def _dims(s):
    """(the cube's H, W), the clear grid, the window grid, the origins."""
    hc, wc = s.H // K, s.W // K
    origins = [(0, 0), (hc - TH, wc - TW), (3, 5), (3, 5), (hc - TH + 1, 0), (0, -1), (2, wc - TW)]
    return (2 * s.H - 1, 2 * s.W - 1), (hc, wc), (hc // CE, wc // CE), origins


def _inputs(s, k):
    rng = np.random.default_rng(60 + k)
    (ch, cw), _, _, origins = _dims(s)
    if k == 0:
        scl = np.where(rng.random((s.H, s.W)) < 0.03, rng.choice([8, 9, 10, 0, 1], size=(s.H, s.W)), rng.choice([4, 5, 6, 7, 11, 40], size=(s.H, s.W)))
        scl[:, s.W // 2:] = np.where(scl[:, s.W // 2:] > 7, 4, scl[:, s.W // 2:])          # the right half: flat classes only
    elif k == 1:
        scl = rng.choice([4, 5, 6], size=(s.H, s.W))
    else:
        scl = np.full((s.H, s.W), 9)
    return dict(scl=scl.astype(np.uint8), origins=np.array(origins, dtype=np.int32),
                cube=rng.standard_normal((T, ch, cw)).astype(np.float32))


class SclChain(cc.Chain):
    in_place = ("cube",)

    def allocate(self, s):
        B = lambda n, off=0: Buf(self.torch, n, off)  # noqa: E731
        (ch, cw), (hc, wc), (ny, nx), origins = _dims(s)
        self.ins = dict(scl=B(s.H * s.W), origins=B(len(origins) * 8), cube=B(T * ch * cw * 4))
        self.outs = dict(hist=(B((s.H // TILE[0]) * (s.W // TILE[1]) * 64), np.int32), mask=(B(s.H * s.W, 5), np.uint8),
                         clear=(B(hc * wc), np.uint8), cell_bad=(B(hc * wc, 1), np.uint8), win=(B(ny * nx * 4), np.int32),
                         tiles=(B(len(origins) * TH * TW, 3), np.uint8), cube=(self.ins["cube"], np.float32), count=(B(8, 8), np.int64))

    def used(self, name):
        s = self.shape
        (ch, cw), (hc, wc), (ny, nx), origins = _dims(s)
        return dict(hist=(s.H // TILE[0]) * (s.W // TILE[1]) * 64, mask=s.H * s.W, clear=hc * wc, cell_bad=hc * wc, win=ny * nx * 4,
                    tiles=len(origins) * TH * TW, cube=T * ch * cw * 4, count=8)[name]

    def launch(self, st):
        s, i, o, lib = self.shape, self.ins, self.outs, self.lib
        (ch, cw), (hc, wc), _, origins = _dims(s)
        return [lib.hsr_scl_class_counts(i["scl"].ptr, s.H, s.W, s.W, TILE[0], TILE[1], o["hist"][0].ptr, st),
                lib.hsr_scl_mask(i["scl"].ptr, s.H, s.W, s.W, sc.GROW, sc.FLAT, R, sc.DISC, o["mask"][0].ptr, s.W, st),
                lib.hsr_scl_coarse(o["mask"][0].ptr, s.H, s.W, s.W, K, MAX_BAD, o["clear"][0].ptr, o["cell_bad"][0].ptr, CE, CE,
                                   o["win"][0].ptr, st),
                lib.hsr_scl_gather_tiles(o["clear"][0].ptr, hc, wc, wc, i["origins"].ptr, len(origins), TH, TW, o["tiles"][0].ptr, st),
                lib.hsr_scl_apply(i["cube"].ptr, T, ch, cw, ch * cw, cw, o["mask"][0].ptr, s.H, s.W, s.W, UP, float("nan"),
                                  o["count"][0].ptr, st)]


class SclRow(cc.Row):
    chain, log = SclChain, ("hsr_scl_last_launch", True)

    def instances(self, s):
        return NAMES

    def make_inputs(self, s, k):
        return _inputs(s, k)

    def make_reference(self, s, k):
        i = self.inputs(s, k)
        mask = sc.dilate_ref(i["scl"], sc.GROW, sc.FLAT, R, sc.DISC)
        clear, bad, win = sc.coarse_ref(mask, K, MAX_BAD, (CE, CE))
        cube, count = sc.apply_ref(i["cube"], mask, UP, np.nan)
        return dict(hist=sc.counts_ref(i["scl"], *TILE), mask=mask, clear=clear, cell_bad=bad, win=win,
                    tiles=sc.gather_ref(clear, i["origins"].tolist(), TH, TW), cube=cube, count=count)

    def check(self, got, s, k, worst):
        r = self.reference(s, k)
        # the sets do what they are for
        frac = r["mask"].mean()
        assert (0.02 < frac < 0.6, frac == 0.0, frac == 1.0)[k], (k, frac)
        if k == 0:
            assert not r["mask"][:, -sc.TILE_W + R:].all() and 0 < r["clear"].sum() < r["clear"].size and r["win"].max() > 0
        assert r["count"] == (np.repeat(np.repeat(r["mask"], 2, 0), 2, 1)[:2 * s.H - 1, :2 * s.W - 1] != 0).sum()
        for name in ("hist", "mask", "clear", "cell_bad", "win", "tiles"):
            np.testing.assert_array_equal(got[name], r[name].reshape(-1), err_msg=f"set {k} {name}")
        g, w = got["cube"].view(np.uint32), np.ascontiguousarray(r["cube"]).reshape(-1).view(np.uint32)
        nan = np.isnan(r["cube"]).reshape(-1)
        assert np.array_equal(np.isnan(got["cube"]), nan) and np.array_equal(g[~nan], w[~nan]), f"set {k} cube"
        assert int(got["count"][0]) == r["count"]


ROWS = {"scl-chain": SclRow("scl-chain", ("hsr_scl_class_counts", "hsr_scl_mask", "hsr_scl_coarse", "hsr_scl_gather_tiles",
                                           "hsr_scl_apply"), SMALL, BIG)}


def test_rows_cover_the_launch_path_entries():
    from s2_emit import _native as nat
    covered = {n for r in ROWS.values() for n in r.covers}
    launch_path = {n for n in nat.SCL_SIGNATURES if "last_launch" not in n and "instance" not in n and not n.endswith("_host")}
    assert covered == launch_path
    for s in (SMALL, BIG):                                 # more than one mask tile either way
        assert s.W > sc.TILE_W and s.H > sc.TILE_H
    assert -(-BIG.W // sc.TILE_W) * -(-BIG.H // sc.TILE_H) > -(-SMALL.W // sc.TILE_W) * -(-SMALL.H // sc.TILE_H)
    origins = _dims(SMALL)[3]
    assert len(set(origins)) < len(origins) and any(c < 0 for _, c in origins)


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
