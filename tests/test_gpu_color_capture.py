"""Graph capture and reused scratch for the affine colour entries (include/hsr_color.h), on an MI355X: the procedure of
tests/test_gpu_graph_capture.py, steps 1 - 4, on two chains

    image   hsr_affine_moments -> hsr_affine_reduce_solve -> hsr_affine_apply
    rows    hsr_affine_moments_f64 -> hsr_affine_reduce_solve

Each is captured once on ONE side stream in global error mode (an allocation, a synchronisation or a launch on another stream fails
the capture or shows in the sentinel), replayed over three input sets in the same buffers, then run big -> small -> big in buffers
sized for the big shape.  The three sets flip the chain's DEVICE-side decisions: 0 full rank, 1 a gray source (rank 2: the
eigenvalue cut), 2 a count below min_count (the identity).  The big shape only changes the slot count (3 against 1).

The row protocol (Row, Chain) is capture_cases', the buffers gpu_harness', and the procedure itself - the two test bodies and the
side-stream fixture of test_gpu_graph_capture - is called, not restated; the rows live here because capture_cases' table is pinned
to the entry points of hsr.h.
Each chain is a chain: no parallel branches.  The module sets no environment variable.  Bars: affine_cases' header."""
import contextlib
from collections import namedtuple

import numpy as np
import pytest

import affine_cases as ac
import capture_cases as cc
from gpu_harness import Buf, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
import test_gpu_graph_capture as gc
from test_gpu_graph_capture import side  # noqa: F401  (side: the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

AffShape = namedtuple("AffShape", "npix")
MIN_COUNT = 200
SMALL, BIG = AffShape(1500), AffShape(2 * ac.SLOT_PIXELS + 1)
IDENTITY = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])


def _rows(npix, k, seed):
    """Set k of a shape: (x, y float32 rows, mask).  0 full rank; 1 gray; 2 fewer than MIN_COUNT rows inside the mask."""
    x, y = ac.image_pair(npix, seed + 10 * k)
    ac.poison(x, y, "both", seed + k)
    mask = ac.make_mask(npix, "part", seed + k)
    if k == 1:
        x[:, 1] = x[:, 0]
        x[:, 2] = x[:, 0]
    if k == 2:
        mask[MIN_COUNT - 50:] = 0
    return x, y, mask


def _check_fit(got, xs, ys, n, worst, tag):
    """moments within their bar, (A, t) within the solve bar of np.linalg.lstsq on the same rows - or exactly the identity."""
    ref, mag = ac.moments_ld(xs, ys)
    err = np.abs(got["moments"].astype(ac.LD) - ref).astype(np.float64)
    bar = ac.moments_bar(n, mag)
    assert got["moments"][9] == n and (err <= bar).all(), (tag, err, bar)
    cc._note(worst, tag + " moments", np.max(err / np.where(bar > 0, bar, 1.0)))
    if n < MIN_COUNT:
        assert np.array_equal(got["At"], IDENTITY), tag
        return
    W = ac.lstsq_ref(xs, ys, MIN_COUNT)
    sbar, _ = ac.solve_bar(xs, W)
    diff = ac.grid_diff(got["At"], W)
    assert diff <= sbar, (tag, diff, sbar)
    assert not np.array_equal(got["At"], IDENTITY)
    cc._note(worst, tag + " solve", diff / sbar)


class ImageChain(cc.Chain):
    def allocate(self, s):
        T = self.torch
        self.ins = dict(x=Buf(T, s.npix * 16), y=Buf(T, s.npix * 12), mask=Buf(T, s.npix, 1))
        self.work = dict(partials=Buf(T, ac.slots(s.npix) * ac.NMOM * 8))
        self.outs = dict(moments=(Buf(T, ac.NMOM * 8), np.float64), At=(Buf(T, 96), np.float64), out=(Buf(T, s.npix * 12), np.float32))

    def used(self, name):
        return {"moments": ac.NMOM * 8, "At": 96, "out": self.shape.npix * 12}[name]

    def launch(self, st):
        n, i, o, lib = self.shape.npix, self.ins, self.outs, self.lib
        return [lib.hsr_affine_moments(i["x"].ptr, 1, 4, i["y"].ptr, 1, 3, i["mask"].ptr, n, None, None, self.work["partials"].ptr, None, st),
                lib.hsr_affine_reduce_solve(self.work["partials"].ptr, ac.slots(n), MIN_COUNT, o["moments"][0].ptr, o["At"][0].ptr, st),
                lib.hsr_affine_apply(i["x"].ptr, 1, 4, i["mask"].ptr, o["At"][0].ptr, n, None, 1, o["out"][0].ptr, 1, 3, st)]


class ImageRow(cc.Row):
    chain, log = ImageChain, ("hsr_color_last_launch", True)

    def instances(self, s):
        return ["affine_moments_kernel<1, 2>", "affine_reduce_solve_kernel", "affine_apply_kernel<1, 2>"]

    def make_inputs(self, s, k):
        x, y, mask = _rows(s.npix, k, 40)
        return dict(x=ac.pack(x, ac.PADDED), y=ac.pack(y, ac.PACKED), mask=mask)

    def make_reference(self, s, k):
        x, y, mask = _rows(s.npix, k, 40)
        ok = ac.usable(x, y, mask)
        return dict(x=x, mask=mask, xs=x[ok].astype(np.float64), ys=y[ok].astype(np.float64), n=int(ok.sum()))

    def check(self, got, s, k, worst):
        r = self.reference(s, k)
        assert (r["n"] < MIN_COUNT) == (k == 2)
        _check_fit(got, r["xs"], r["ys"], r["n"], worst, f"image set {k}")
        want = ac.apply_ref(r["x"], got["At"], r["mask"], None, 1)                   # the apply with the DEVICE's (A, t): bit-equal
        assert np.array_equal(np.isnan(got["out"]), np.isnan(want.reshape(-1)))
        keep = ~np.isnan(want.reshape(-1))
        np.testing.assert_array_equal(got["out"].view(np.uint32)[keep], want.reshape(-1).view(np.uint32)[keep])


class RowsChain(cc.Chain):
    def allocate(self, s):
        T = self.torch
        self.ins = dict(x=Buf(T, s.npix * 24), y=Buf(T, s.npix * 24, 8))
        self.work = dict(partials=Buf(T, ac.slots(s.npix) * ac.NMOM * 8))
        self.outs = dict(moments=(Buf(T, ac.NMOM * 8), np.float64), At=(Buf(T, 96), np.float64))

    def used(self, name):
        return {"moments": ac.NMOM * 8, "At": 96}[name]

    def launch(self, st):
        n, i, o, lib = self.shape.npix, self.ins, self.outs, self.lib
        return [lib.hsr_affine_moments_f64(i["x"].ptr, 3, i["y"].ptr, 3, n, self.work["partials"].ptr, None, st),
                lib.hsr_affine_reduce_solve(self.work["partials"].ptr, ac.slots(n), MIN_COUNT, o["moments"][0].ptr, o["At"][0].ptr, st)]


class RowsRow(cc.Row):
    chain, log = RowsChain, ("hsr_color_last_launch", True)

    def instances(self, s):
        return ["affine_moments_f64_kernel", "affine_reduce_solve_kernel"]

    def make_inputs(self, s, k):
        x, y, mask = _rows(s.npix, k, 70)
        x, y = x.astype(np.float64), y.astype(np.float64) + 1e-9 * np.arange(3)             # float64 rows that are no float32 values
        x[mask == 0, 0] = np.nan                                                              # no mask here: the skipped rows are NaN rows
        return dict(x=x, y=y)

    def make_reference(self, s, k):
        i = self.inputs(s, k)
        ok = np.isfinite(i["x"]).all(axis=1) & np.isfinite(i["y"]).all(axis=1)
        return dict(xs=i["x"][ok], ys=i["y"][ok], n=int(ok.sum()))

    def check(self, got, s, k, worst):
        r = self.reference(s, k)
        assert (r["n"] < MIN_COUNT) == (k == 2)
        _check_fit(got, r["xs"], r["ys"], r["n"], worst, f"rows set {k}")


ROWS = {"affine-image": ImageRow("affine-image", ("hsr_affine_moments", "hsr_affine_reduce_solve", "hsr_affine_apply"), SMALL, BIG),
        "affine-rows": RowsRow("affine-rows", ("hsr_affine_moments_f64", "hsr_affine_reduce_solve"), SMALL, BIG)}


def test_rows_cover_the_launch_path_entries():
    covered = {n for r in ROWS.values() for n in r.covers}
    assert covered == {"hsr_affine_moments", "hsr_affine_moments_f64", "hsr_affine_reduce_solve", "hsr_affine_apply"}
    assert ac.slots(SMALL.npix) == 1 and ac.slots(BIG.npix) == 3


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
    """Steps 1 - 3: eager warm-up, capture on the side stream, replays over sets 0, 1, 2, 2."""
    with _placed(name):
        gc.test_capture_and_replay(torch_gpu, side, name)


@pytest.mark.parametrize("name", list(ROWS))
def test_small_after_big_in_the_same_buffers(torch_gpu, side, name):
    """Step 4: big, small, big, small, small in buffers sized for the big shape."""
    with _placed(name):
        gc.test_small_after_big_in_the_same_buffers(torch_gpu, side, name)
