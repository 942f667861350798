"""Graph capture and reused buffers for the area-resampling entry (include/hsr_resize.h), on an MI355X: the procedure of
tests/test_gpu_graph_capture.py, as tests/test_gpu_s2stack_capture.py applies it, on

    hsr_area_resample

captured once on ONE side stream in global error mode (an allocation, a synchronisation, a host-to-device copy of a tap table or a
launch on another stream fails the capture or shows in the sentinel), replayed over three input sets in the same buffers, then run
big -> small -> big in buffers sized for the big shape.  The sets: 0 a clean image - no output is invalid; 1 a border of invalid
samples - valid and invalid outputs in one launch; 2 every sample invalid - every output is invalid.  The counts are cleared
in-stream by every call: a replay after set 2 must not add to what set 2 left.

One row per kernel: the staged one (float32 planes, NaN) and the gather one (uint16 pixel-major at a scale past the LDS, nodata).
The row protocol (Row, Chain) is capture_cases', the buffers gpu_harness', and the procedure itself is called, not restated.  A
single launch: no parallel branches.  The module sets no environment variable.  Bar: equality of every output with the statement of
tests/resize_cases.py."""
import contextlib
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

import capture_cases as cc
import resize_cases as rc
from gpu_harness import Buf, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
import test_gpu_graph_capture as gc
from test_gpu_graph_capture import side  # noqa: F401  (side: the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

Shape = namedtuple("Shape", "h w H W")
Form = namedtuple("Form", "dtype out C pixmajor scale origin nodata rule mvf")
FORMS = {
    "area-staged": Form("float32", "float32", 2, False, (2.5, 3.25), (0.25, -0.5), None, rc.RENORM, 0.5),
    "area-gather": Form("uint16", "float32", 3, True, (12.5, 12.0), (-1.0, 0.5), 0, rc.STRICT, 0.0),
}
SHAPES = {
    "area-staged": (Shape(30, 50, 11, 15), Shape(70, 230, 27, 70)),
    "area-gather": (Shape(40, 50, 3, 4), Shape(230, 420, 18, 35)),
}
FILL_OUT = -3.0


def _strides(f, rows, cols):
    return (1, cols * f.C, f.C) if f.pixmajor else (rows * cols, cols, 1)


def _image(f, s, k):
    """(C, h, w)."""
    rng = np.random.default_rng(90 + k)
    bad = np.nan if f.nodata is None else f.nodata
    if f.dtype == "float32":
        img = rng.uniform(-1.0, 1.0, size=(f.C, s.h, s.w)).astype(np.float32)
    else:
        img = rng.integers(1, 65536, size=(f.C, s.h, s.w)).astype(f.dtype)
    if k == 1:
        keep = np.zeros((s.h, s.w), bool)
        keep[s.h // 4: -(s.h // 4), s.w // 4: -(s.w // 4)] = True
        img = np.where(keep[None], img, bad).astype(f.dtype)
    elif k == 2:
        img[:] = bad
    return img


class AreaChain(cc.Chain):
    def allocate(self, s):
        f = self.row.form
        self.ins = {"src": Buf(self.torch, f.C * s.h * s.w * np.dtype(f.dtype).itemsize)}
        self.outs = dict(image=(Buf(self.torch, 4 * f.C * s.H * s.W), np.float32), invalid=(Buf(self.torch, 8 * f.C, 8), np.int64))

    def used(self, name):
        f, s = self.row.form, self.shape
        return dict(image=4 * f.C * s.H * s.W, invalid=8 * f.C)[name]

    def launch(self, st):
        f, s, lib = self.row.form, self.shape, self.lib
        ss, ds = _strides(f, s.h, s.w), _strides(f, s.H, s.W)
        return [lib.hsr_area_resample(self.ins["src"].ptr, rc.CODES[f.dtype], f.C, s.h, s.w, ss[0], ss[1], ss[2], f.origin[0], f.origin[1],
                                      f.scale[0], f.scale[1], 0 if f.nodata is None else 1, float(f.nodata or 0), f.rule, f.mvf,
                                      self.outs["image"][0].ptr, rc.CODES[f.out], s.H, s.W, ds[0], ds[1], ds[2], C.c_float(1.0),
                                      C.c_float(FILL_OUT), 0, self.outs["invalid"][0].ptr, st)]


class AreaRow(cc.Row):
    chain, log = AreaChain, ("hsr_resize_last_launch", True)

    def __init__(self, name, covers, small, big):
        super().__init__(name, covers, small, big)
        self.form = FORMS[name]

    def instances(self, s):
        f = self.form
        ss = _strides(f, s.h, s.w)
        return [rc.instance_of(f.dtype, f.out, f.C, ss[0], ss[2], f.scale[0], f.scale[1])]

    def make_inputs(self, s, k):
        f = self.form
        img = _image(f, s, k)
        return {"src": np.ascontiguousarray(np.moveaxis(img, 0, -1) if f.pixmajor else img)}

    def make_reference(self, s, k):
        f = self.form
        out, inv = rc.area_ref(_image(f, s, k), (s.H, s.W), f.origin, f.scale, f.nodata, "strict" if f.rule == rc.STRICT else "renorm", f.mvf,
                               f.out, 1.0, FILL_OUT, 0)
        return dict(image=np.ascontiguousarray(np.moveaxis(out, 0, -1) if f.pixmajor else out), invalid=inv)

    def check(self, got, s, k, worst):
        r = self.reference(s, k)
        n, cells = r["invalid"], s.H * s.W
        assert ((n == 0).all(), (n > 0).all() and (n < cells).all(), (n == cells).all())[k], (k, n)      # the sets do what they are for
        rc.same(got["image"], r["image"].reshape(-1), f"set {k} image")
        np.testing.assert_array_equal(got["invalid"], n, err_msg=f"set {k} invalid")


ROWS = {name: AreaRow(name, ("hsr_area_resample",), *SHAPES[name]) for name in FORMS}


def test_rows_cover_the_launch_path_entry_and_both_kernels():
    from s2_emit import _native as nat
    covered = {n for r in ROWS.values() for n in r.covers}
    launch_path = {n for n, (_, args) in nat.RESIZE_SIGNATURES.items() if len(args) > 8 and not n.endswith("_host")}
    assert covered == launch_path == {"hsr_area_resample"}
    names = {name: [r.instances(s)[0] for s in r.shapes.values()] for name, r in ROWS.items()}
    assert names["area-staged"] == ["area_staged_kernel<F32, F32, PLANAR>"] * 2
    assert names["area-gather"] == ["area_gather_kernel<U16, F32>"] * 2
    tiles = lambda s: -(-s.H // rc.TILE_H) * -(-s.W // rc.TILE_W)  # noqa: E731
    for small, big in SHAPES.values():
        assert tiles(small) <= 2 < 6 <= tiles(big)
    # every cell of every shape lies inside the source: set 0 has no invalid output
    for name, f in FORMS.items():
        for s in SHAPES[name]:
            assert f.origin[0] + s.H * f.scale[0] <= s.h + f.scale[0] / 2 and f.origin[1] + s.W * f.scale[1] <= s.w + f.scale[1] / 2


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
