"""Graph capture and reused buffers for the S2 stack entries (include/hsr_s2stack.h), on an MI355X: the procedure of
tests/test_gpu_graph_capture.py, as tests/test_gpu_scl_capture.py applies it, on the chain

    hsr_s2_stack -> hsr_s2_expand_u8

captured once on ONE side stream in global error mode (an allocation, a synchronisation, a host-to-device copy of the band table or
a launch on another stream fails the capture or shows in the sentinel), replayed over three input sets in the same buffers, then
run big -> small -> big in buffers sized for the big shape.  The sets: 0 clean planes - every thread of a bilinear band takes the
separable path and no output is invalid; 1 a nodata border - both paths in one launch; 2 everything nodata - every output is
invalid.  The counts are cleared in-stream by every call: a replay after set 2 must not add to what set 2 left.

The band table is host memory that the call copies into the kernel's arguments: the capture freezes it with the other arguments.
The row protocol (Row, Chain) is capture_cases', the buffers gpu_harness', and the procedure itself is called, not restated.  The
chain is a chain: no parallel branches.  The module sets no environment variable.  Bar: equality of every output with the
statement of tests/s2stack_cases.py."""
import contextlib
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

import capture_cases as cc
import s2stack_cases as sc
from gpu_harness import Buf, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
import test_gpu_graph_capture as gc
from test_gpu_graph_capture import side  # noqa: F401  (side: the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

Shape = namedtuple("Shape", "H10 W10")
SMALL, BIG = Shape(18, 50), Shape(sc.TILE_H + 19, sc.TILE_W + 18)
BANDS = ((1, sc.NEAREST, -1000), (2, sc.NEAREST, 0), (2, sc.BILINEAR, 0))
DTYPE, RULE, NODATA, QUANT, FILL, SCL_UP = sc.F32, sc.RENORM, 0, 10000.0, np.nan, 2
NAMES = [sc.stack_instance(DTYPE, RULE), "s2_expand_kernel<UP2>"]


def _window(s):
    return (1, 1, s.H10 - 2, s.W10 - 2)                    # an odd origin


def _plane_shapes(s):
    return [(sc.ceil_div(s.H10, up), sc.ceil_div(s.W10, up)) for up, _, _ in BANDS]


def _inputs(s, k):
    rng = np.random.default_rng(70 + k)
    out = {}
    for b, shape in enumerate(_plane_shapes(s)):
        p = rng.integers(1, 65536, size=shape)
        if k == 1:
            keep = np.zeros(shape, bool)
            keep[2:-2, 3:-3] = True
            p = np.where(keep, p, NODATA)
        elif k == 2:
            p = np.full(shape, NODATA)
        out[f"p{b}"] = p.astype(np.uint16)
    out["scl"] = rng.integers(0, 12, size=(sc.ceil_div(s.H10, SCL_UP), sc.ceil_div(s.W10, SCL_UP))).astype(np.uint8)
    return out


class S2Chain(cc.Chain):
    def allocate(self, s):
        B = lambda n, off=0: Buf(self.torch, n, off)  # noqa: E731
        _, _, h, w = _window(s)
        self.ins = {f"p{b}": B(2 * H * W) for b, (H, W) in enumerate(_plane_shapes(s))}
        self.ins["scl"] = B(sc.ceil_div(s.H10, SCL_UP) * sc.ceil_div(s.W10, SCL_UP))
        self.outs = dict(stack=(B(4 * len(BANDS) * h * w), np.float32), invalid=(B(8 * len(BANDS), 8), np.int64), scl10=(B(h * w, 5), np.uint8))

    def used(self, name):
        _, _, h, w = _window(self.shape)
        return dict(stack=4 * len(BANDS) * h * w, invalid=8 * len(BANDS), scl10=h * w)[name]

    def launch(self, st):
        from s2_emit import _native as nat
        s, i, o, lib = self.shape, self.ins, self.outs, self.lib
        row0, col0, h, w = _window(s)
        table = (nat.S2Band * len(BANDS))()
        for b, (e, (H, W), (up, method, off)) in enumerate(zip(table, _plane_shapes(s), BANDS)):
            e.plane_dev, e.rs, e.H, e.W, e.up, e.method, e.add_offset = i[f"p{b}"].ptr.value, W, H, W, up, method, off
        Hs, Ws = sc.ceil_div(s.H10, SCL_UP), sc.ceil_div(s.W10, SCL_UP)
        return [lib.hsr_s2_stack(table, len(BANDS), s.H10, s.W10, row0, col0, h, w, 1, NODATA, RULE, DTYPE, o["stack"][0].ptr, h * w, w, 0,
                                 C.c_float(FILL), C.c_double(QUANT), o["invalid"][0].ptr, st),
                lib.hsr_s2_expand_u8(i["scl"].ptr, Hs, Ws, Ws, SCL_UP, s.H10, s.W10, row0, col0, h, w, o["scl10"][0].ptr, w, st)]


class S2Row(cc.Row):
    chain, log = S2Chain, ("hsr_s2stack_last_launch", True)

    def instances(self, s):
        return NAMES

    def make_inputs(self, s, k):
        return _inputs(s, k)

    def make_reference(self, s, k):
        i = self.inputs(s, k)
        stack, invalid = sc.stack_ref([i[f"p{b}"] for b in range(len(BANDS))], BANDS, _window(s), 1, NODATA, RULE, DTYPE, 0, FILL, QUANT)
        return dict(stack=stack, invalid=invalid, scl10=sc.expand_ref(i["scl"], SCL_UP, _window(s)))

    def check(self, got, s, k, worst):
        r = self.reference(s, k)
        _, _, h, w = _window(s)
        # the sets do what they are for
        n = r["invalid"]
        assert ((n == 0).all(), (n > 0).all() and (n < h * w).all(), (n == h * w).all())[k], (k, n)
        want = r["stack"].reshape(-1)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got["stack"]), nan), f"set {k} stack"
        assert np.array_equal(got["stack"].view(np.uint32)[~nan], want.view(np.uint32)[~nan]), f"set {k} stack"
        np.testing.assert_array_equal(got["invalid"], n, err_msg=f"set {k} invalid")
        np.testing.assert_array_equal(got["scl10"], r["scl10"].reshape(-1), err_msg=f"set {k} scl10")


ROWS = {"s2stack-chain": S2Row("s2stack-chain", ("hsr_s2_stack", "hsr_s2_expand_u8"), SMALL, BIG)}


def test_rows_cover_the_launch_path_entries():
    from s2_emit import _native as nat
    covered = {n for r in ROWS.values() for n in r.covers}
    launch_path = {n for n in nat.S2STACK_SIGNATURES if "last_launch" not in n and "instance" not in n and not n.endswith("_host")}
    assert covered == launch_path
    tiles = lambda s: sc.ceil_div(s.H10 - 2, sc.TILE_H) * sc.ceil_div(s.W10 - 2, sc.TILE_W)  # noqa: E731
    assert tiles(SMALL) == 1 and tiles(BIG) == 6 and _window(SMALL)[0] % 2 and _window(SMALL)[1] % 2
    assert {(u, m) for u, m, _ in BANDS} == {(1, sc.NEAREST), (2, sc.NEAREST), (2, sc.BILINEAR)}


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
