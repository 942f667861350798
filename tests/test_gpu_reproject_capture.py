"""Graph capture and reused buffers for the reprojection entries (include/hsr_reproject.h), on an MI355X: the procedure of
tests/test_gpu_graph_capture.py, steps 1 - 4, on the chain

    hsr_reproject_coords -> hsr_reproject_warp (under that field) -> hsr_reproject_warp (under a field from a buffer)

captured once on ONE side stream in global error mode (an allocation, a synchronisation or a launch on another stream fails the
capture or shows in the sentinel), replayed over three input sets in the same buffers, then run big -> small -> big in buffers
sized for the big shape.  The geometry of the first field is made of scalars, which a graph holds fixed; what a replay can change
is what lies in the buffers, so the third launch takes its field from one.  The three sets flip the remap's DEVICE-side
decisions: 0 every tile's footprint fits the staged box; 1 per-pixel random coordinates in some tiles, which fall back to the
direct gather and raise the status word; 2 every coordinate outside or non-finite - nothing is read and everything is fill.  The
source's invalid samples change with the set too.  The status word and the counts are cleared in-stream by every call: a replay
after set 1 must read 0 again.

The row protocol (Row, Chain) is capture_cases', the buffers gpu_harness', and the procedure itself is called, not restated; the
rows live here because capture_cases' table is pinned to the entry points of hsr.h.  The chain is a chain: no parallel branches.
The module sets no environment variable.  Bars: reproject_cases' header - the remaps bit-equal to the NumPy statement under the
field the DEVICE computed, that field within twice the coordinate bar of the NumPy restatement."""
import contextlib
from collections import namedtuple

import numpy as np
import pytest

import capture_cases as cc
import reproject_cases as rc
import s2_emit
from gpu_harness import Buf, same_bits, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
import test_gpu_graph_capture as gc
from test_gpu_graph_capture import side  # noqa: F401  (side: the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

Shape = namedtuple("Shape", "h w hs ws")
SMALL, BIG = Shape(20, 70, 40, 110), Shape(37, 135, 48, 172)
BANDS, NODATA, FILL_VALUE, MF = 2, -9999.0, -9999.0, 1.5
EPSG, E0, N0 = 32611, 431040.0, 3801060.0
NAMES = ["reproject_coords_kernel", "reproject_warp_kernel<LDS, RENORM>", "reproject_warp_kernel<LDS, STRICT>"]


def _geometry(s):
    """The 16 geometry arguments: a 60 m grid at (E0, N0) and an EMIT-like source whose origin lies 3 cells up and left of it."""
    lon, lat = s2_emit.tm_inverse(E0, N0, s2_emit.utm_params(EPSG))
    g0, g3 = float(lon) - 3 * rc.EMIT_CELL, float(lat) + 3 * rc.EMIT_CELL
    return [E0, N0, 60.0, 60.0, s.h, s.w, *s2_emit.utm_params(EPSG), g0, rc.EMIT_CELL, g3, -rc.EMIT_CELL]


def _inputs(s, k):
    r = rc.warp_row(BANDS, s.h, s.w, s.hs, s.ws, ("affine", 3.0, 0.8), bad=("nan", "mixed", "dense")[k], nodata=NODATA)
    src = rc.make_source(r, 40 + k)
    field = rc.make_field(r["field"], s.h, s.w, s.hs, s.ws, 40 + k).copy()
    if k == 1:                                            # the right-hand tiles: per-pixel random coordinates
        field[:, rc.TILE_W:] = rc.make_field(("random",), s.h, s.w - rc.TILE_W, s.hs, s.ws, 41)
    if k == 2:
        field[...] = np.where(np.arange(s.w)[None, :, None] % 3 == 0, np.nan, np.where(np.arange(s.w)[None, :, None] % 3 == 1, -1.0, 1e300))
    return dict(src=src, field=np.ascontiguousarray(field))


class ReprojectChain(cc.Chain):
    def allocate(self, s):
        T = self.torch
        self.ins = dict(src=Buf(T, BANDS * s.hs * s.ws * 4), field=Buf(T, s.h * s.w * 16))
        out = lambda: (Buf(T, BANDS * s.h * s.w * 4), np.float32)  # noqa: E731
        self.outs = dict(coords=(Buf(T, s.h * s.w * 16), np.float64), out_a=out(), counts_a=(Buf(T, 16), np.int64),
                         status_a=(Buf(T, 4, 4), np.int32), out_b=out(), counts_b=(Buf(T, 16, 8), np.int64), status_b=(Buf(T, 4), np.int32))

    def used(self, name):
        s = self.shape
        return {"coords": s.h * s.w * 16, "out_a": BANDS * s.h * s.w * 4, "out_b": BANDS * s.h * s.w * 4}.get(name, 16 if "counts" in name else 4)

    def launch(self, st):
        s, i, o, lib = self.shape, self.ins, self.outs, self.lib
        warp = lambda field, rule, tag: lib.hsr_reproject_warp(  # noqa: E731
            i["src"].ptr, BANDS, s.hs, s.ws, s.hs * s.ws, s.ws, field, s.h, s.w, 1, NODATA, FILL_VALUE, rule, MF, o["out_" + tag][0].ptr,
            s.h * s.w, s.w, o["counts_" + tag][0].ptr, o["status_" + tag][0].ptr, st)
        return [lib.hsr_reproject_coords(*_geometry(s), o["coords"][0].ptr, st), warp(o["coords"][0].ptr, rc.RENORM, "a"),
                warp(i["field"].ptr, rc.STRICT, "b")]


class ReprojectRow(cc.Row):
    chain, log = ReprojectChain, ("hsr_reproject_last_launch", True)

    def instances(self, s):
        return NAMES

    def make_inputs(self, s, k):
        return _inputs(s, k)

    def make_reference(self, s, k):
        i = self.inputs(s, k)
        E, N = np.meshgrid(E0 + (np.arange(s.w) + 0.5) * 60.0, N0 - (np.arange(s.h) + 0.5) * 60.0)
        lon, lat = s2_emit.tm_inverse(E, N, s2_emit.utm_params(EPSG))
        g = _geometry(s)
        field = np.stack([(lat - g[14]) / g[15] - 0.5, (lon - g[12]) / g[13] - 0.5], axis=-1)
        ref_b, counts_b, info = rc.warp_ref(i["src"], i["field"], NODATA, FILL_VALUE, rc.STRICT)
        status, fits, falls = rc.warp_status(i["field"], s.hs, s.ws, MF)
        return dict(field=field, out_b=ref_b, counts_b=counts_b, status_b=status, fits=fits, falls=falls, inside=info["inside"])

    def check(self, got, s, k, worst):
        r, i = self.reference(s, k), self.inputs(s, k)
        # the sets do what they are for
        assert (r["status_b"], r["falls"] > 0, bool(r["inside"].any())) == ((0, False, True), (1, True, True), (0, False, False))[k], (k, r["status_b"], r["falls"])
        assert r["fits"] > 0 or k == 2
        coords = got["coords"].reshape(s.h, s.w, 2)
        bar = rc.coord_bar(rc.EMIT_CELL)
        err = np.abs(coords - r["field"]).max()
        assert err <= 2 * bar
        cc._note(worst, f"set {k} coords / (2 bar)", err / (2 * bar))
        ref_a, counts_a, info_a = rc.warp_ref(i["src"], coords, NODATA, FILL_VALUE, rc.RENORM)      # under the DEVICE's field: bit-equal
        assert info_a["inside"].mean() > 0.8
        same_bits(got["out_a"].reshape(ref_a.shape), ref_a, f"set {k} remap under the computed field")
        assert np.array_equal(got["counts_a"], counts_a) and int(got["status_a"][0]) == 0
        same_bits(got["out_b"].reshape(r["out_b"].shape), r["out_b"], f"set {k} remap under the given field")
        assert np.array_equal(got["counts_b"], r["counts_b"]) and int(got["status_b"][0]) == r["status_b"]
        if k == 2:
            assert (got["out_b"] == np.float32(FILL_VALUE)).all() and got["counts_b"][0] == s.h * s.w and got["counts_b"][1] == 0


ROWS = {"reproject-chain": ReprojectRow("reproject-chain", ("hsr_reproject_coords", "hsr_reproject_warp"), SMALL, BIG)}


def test_rows_cover_the_launch_path_entries():
    from s2_emit import _native as nat
    covered = {n for r in ROWS.values() for n in r.covers}
    launch_path = {n for n in nat.REPROJECT_SIGNATURES if "last_launch" not in n and "instance" not in n and not n.endswith("_host")}
    assert covered == launch_path
    assert "LDS" in rc.warp_instance(MF, rc.RENORM)
    for s in (SMALL, BIG):                                 # more than one tile either way, and the shapes differ in tiles
        assert s.w > rc.TILE_W and s.h > rc.TILE_H
    assert -(-BIG.w // rc.TILE_W) * -(-BIG.h // rc.TILE_H) > -(-SMALL.w // rc.TILE_W) * -(-SMALL.h // rc.TILE_H)


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
