"""Graph capture and reused buffers for the launch-path entries of include/hsr_merge.h, on an MI355X: the procedure of
tests/test_gpu_graph_capture.py, as tests/test_gpu_resize_capture.py applies it, on

    hsr_ortho_merge        hsr_merge_scenes (with its source plane: two launches in a chain)

captured once on ONE side stream in global error mode (an allocation, a synchronisation, a host-to-device copy of the source table or
a launch on another stream fails the capture or shows in the sentinel), replayed over three input sets in the same buffers, then run
big -> small -> big in buffers sized for the big shape.  The source table is host memory that the call reads before it returns: the
structs travel in the kernel arguments, which the capture freezes; what changes between replays is the content of the buffers.
The sets flip which source wins the overlap: 0 both sources valid - source 0 wins; 1 source 0 has no data anywhere - source 1
wins; 2 a mixed table against one whose entries all point outside the swath - the dropped counts, which every call clears
in-stream, differ from set to set and a replay must not add to what the last one left.

The row protocol (Row, Chain) is capture_cases', the buffers gpu_harness', and the procedure itself is called, not restated.  Single
branch: no parallel branches.  The module sets no environment variable.  Bar: equality of every output with the statement of
tests/merge_cases.py."""
import contextlib
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

import capture_cases as cc
import merge_cases as mc
import ortho_cases as oc
from gpu_harness import Buf, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from s2_emit import _native as nat
import test_gpu_graph_capture as gc
from test_gpu_graph_capture import side  # noqa: F401  (side: the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

Shape = namedtuple("Shape", "bands layout H W")
GRIDS = (("valid", "valid"), ("nodata", "valid"), ("mixed", "dropped"))
NODATA, MASKED = -9999.0, -9999.0
SHAPES = {
    "ortho-merge-bip": (Shape(8, mc.BIP, 3, 65), Shape(8, mc.BIP, 6, 200)),
    "ortho-merge-bsq": (Shape(5, mc.BSQ, 3, 65), Shape(5, mc.BSQ, 6, 200)),
    "merge-scenes-bsq": (Shape(5, mc.BSQ, 3, 65), Shape(5, mc.BSQ, 4, 1100)),
    "merge-scenes-bip": (Shape(5, mc.BIP, 3, 65), Shape(5, mc.BIP, 6, 300)),
}


def _place(s):
    """Two sources: the western two thirds and the eastern two thirds of the output."""
    return ((s.H, max(1, 2 * s.W // 3), 0, 0), (s.H, s.W - s.W // 3, 0, s.W // 3))          # (gh, gw, off_y, off_x)


def _bmask_bytes(s):
    return (s.bands + 7) // 8 + 1


def _sources(s, k):
    """-> per source dict(swath, glt, qmask or None, bmask or None, scene (float32 bip: the statement's ortho rule))."""
    out = []
    for i, (gh, gw, _, _) in enumerate(_place(s)):
        rows, cols = mc.swath_dims(i)
        swath = np.roll(oc.swath_of(rows, cols, s.bands), k, axis=1).copy()
        glt = oc.glt_of(GRIDS[k][i], gh, gw, rows, cols).copy()
        q = np.roll(oc.qmask_of(rows, cols), k, axis=0).copy() if i == 0 else None
        bm = np.roll(oc.bmask_of(rows, cols, s.bands, _bmask_bytes(s)), k, axis=1).copy() if i == 1 else None
        bits, _ = oc.ortho_ref(swath, glt, None, q, bm, NODATA, MASKED, 0, mc.BIP)
        out.append(dict(swath=swath, glt=glt, qmask=q, bmask=bm, scene=bits.view(np.float32)))
    return out


class OrthoMergeChain(cc.Chain):
    def allocate(self, s):
        self.ins = {}
        for i, (gh, gw, _, _) in enumerate(_place(s)):
            rows, cols = mc.swath_dims(i)
            self.ins[f"swath{i}"] = Buf(self.torch, rows * cols * s.bands * 4)
            self.ins[f"glt{i}"] = Buf(self.torch, gh * gw * 8)
        self.ins["qmask0"] = Buf(self.torch, int(np.prod(mc.swath_dims(0))))
        self.ins["bmask1"] = Buf(self.torch, int(np.prod(mc.swath_dims(1))) * _bmask_bytes(s))
        self.outs = dict(out=(Buf(self.torch, s.H * s.W * s.bands * 4), np.uint32), dropped=(Buf(self.torch, 16, 8), np.int64),
                         source=(Buf(self.torch, s.H * s.W, 1), np.uint8))

    def used(self, name):
        s = self.shape
        return dict(out=s.H * s.W * s.bands * 4, dropped=16, source=s.H * s.W)[name]

    def launch(self, st):
        s, i = self.shape, self.ins
        rows = []
        for k, (gh, gw, oy, ox) in enumerate(_place(s)):
            r, c = mc.swath_dims(k)
            rows.append(nat.MergeSwath(i[f"swath{k}"].ptr, i[f"glt{k}"].ptr, i["qmask0"].ptr if k == 0 else None, i["bmask1"].ptr if k == 1 else None,
                                       r, c, gh, gw, oy, ox, _bmask_bytes(s) if k == 1 else 0, s.bands))
        return [self.lib.hsr_ortho_merge((nat.MergeSwath * 2)(*rows), 2, 0, s.layout, s.H, s.W, C.c_float(NODATA), C.c_float(MASKED),
                                         self.outs["out"][0].ptr, self.outs["dropped"][0].ptr, self.outs["source"][0].ptr, st)]


class MergeScenesChain(cc.Chain):
    def allocate(self, s):
        self.ins = {f"scene{i}": Buf(self.torch, gh * gw * s.bands * 4, 4 * i) for i, (gh, gw, _, _) in enumerate(_place(s))}
        self.outs = dict(out=(Buf(self.torch, s.H * s.W * s.bands * 4, 8), np.uint32), source=(Buf(self.torch, s.H * s.W, 1), np.uint8))

    def used(self, name):
        s = self.shape
        return dict(out=s.H * s.W * s.bands * 4, source=s.H * s.W)[name]

    def launch(self, st):
        s = self.shape
        rows = [nat.MergeScene(self.ins[f"scene{k}"].ptr, gh, gw, oy, ox, s.bands, 0) for k, (gh, gw, oy, ox) in enumerate(_place(s))]
        return [self.lib.hsr_merge_scenes((nat.MergeScene * 2)(*rows), 2, s.layout, s.H, s.W, C.c_float(NODATA), 0, self.outs["out"][0].ptr,
                                          self.outs["source"][0].ptr, st)]


class _MergeRow(cc.Row):
    log = ("hsr_merge_last_launch", True)

    def make_reference(self, s, k):
        src = _sources(s, k)
        place = _place(s)
        ref_bip, plane = mc.merge_ref([x["scene"] for x in src], [(p[2], p[3]) for p in place], (s.H, s.W), NODATA)
        dropped = [mc.dropped_inside(x["glt"], *mc.swath_dims(i), (p[2], p[3]), (s.H, s.W)) for i, (x, p) in enumerate(zip(src, place))]
        return dict(out=mc.in_layout(ref_bip, s.layout).reshape(-1), source=plane.reshape(-1), dropped=np.array(dropped, np.int64))

    def check(self, got, s, k, worst):
        r = self.reference(s, k)
        plane = r["source"].reshape(s.H, s.W)[:, s.W // 3: max(1, 2 * s.W // 3)]           # the overlap
        # the sets do what they are for: source 0 supplies most of the overlap (its quality mask leaves some cells to source 1) / none of it
        assert ((plane == 0).sum() > (plane != 0).sum(), (plane != 0).all() and (plane == 1).any(), (r["dropped"] > 0).all())[k], (k, r["dropped"])
        for name in got:
            np.testing.assert_array_equal(got[name], r[name], err_msg=f"set {k} {name}")


class OrthoMergeRow(_MergeRow):
    chain = OrthoMergeChain

    def instances(self, s):
        return [mc.ortho_merge_instance(s.layout, s.bands, True)]

    def make_inputs(self, s, k):
        out = {}
        for i, x in enumerate(_sources(s, k)):
            out[f"swath{i}"], out[f"glt{i}"] = x["swath"], x["glt"]
        out["qmask0"], out["bmask1"] = _sources(s, k)[0]["qmask"], _sources(s, k)[1]["bmask"]
        return out


class MergeScenesRow(_MergeRow):
    chain = MergeScenesChain

    def instances(self, s):
        return mc.merge_scenes_instances(True)

    def make_inputs(self, s, k):
        return {f"scene{i}": mc.in_layout(x["scene"], s.layout) for i, x in enumerate(_sources(s, k))}


ROWS = {name: (OrthoMergeRow if name.startswith("ortho") else MergeScenesRow)(name, ("hsr_" + name[:-4].replace("-", "_"),), *SHAPES[name])
        for name in SHAPES}


def test_rows_cover_the_launch_path_entries():
    covered = {n for r in ROWS.values() for n in r.covers}
    launch_path = {n for n, (_, args) in nat.MERGE_SIGNATURES.items() if len(args) > 8 and not n.endswith("_host")}
    assert covered == launch_path == {"hsr_ortho_merge", "hsr_merge_scenes"}
    assert ROWS["ortho-merge-bip"].instances(SHAPES["ortho-merge-bip"][0]) == ["ortho_merge_bip_kernel<true, true>"]
    assert ROWS["ortho-merge-bsq"].instances(SHAPES["ortho-merge-bsq"][0]) == ["ortho_merge_bsq_kernel<true>"]
    for small, big in SHAPES.values():
        blocks = lambda s: s.H * -(-s.W // mc.PX)  # noqa: E731
        assert blocks(small) <= 6 < 20 <= blocks(big)
    s = SHAPES["merge-scenes-bsq"][1]
    assert s.W > mc.RUN                                                    # the big shape has a second run in every row


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
