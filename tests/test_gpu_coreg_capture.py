"""Graph capture and reused scratch for the co-registration entries (include/hsr_coreg.h), on an MI355X: the procedure of
tests/test_gpu_graph_capture.py, steps 1 - 4, on the chain

    hsr_coreg_surface -> hsr_coreg_peaks -> hsr_coreg_fit_model -> hsr_coreg_warp

captured once on ONE side stream in global error mode (an allocation, a synchronisation or a launch on another stream fails the
capture or shows in the sentinel), replayed over three input sets in the same buffers, then run big -> small -> big in buffers
sized for the big shape.  The three sets flip the chain's DEVICE-side decisions: 0 every tie point OK; 1 a decoy window, rejected
as an outlier and the model refitted; 2 an EMIT scene without a valid pixel - no usable point, the zero model, the identity copy.
The big shape changes the number of tie points (25 against 9), of surface workgroups and of warp tiles.

The row protocol (Row, Chain) is capture_cases', the buffers gpu_harness', and the procedure itself - the two test bodies and the
side-stream fixture of test_gpu_graph_capture - is called, not restated; the rows live here because capture_cases' table is pinned
to the entry points of hsr.h.  The chain is a chain: no parallel branches.  The module sets no environment variable.
Bars: coreg_cases' header, as tests/test_gpu_coreg.py applies them."""
import contextlib
from collections import namedtuple

import numpy as np
import pytest

import capture_cases as cc
import coreg_cases as cg
from gpu_harness import Buf, bits_equal, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
import test_gpu_graph_capture as gc
from test_gpu_graph_capture import side  # noqa: F401  (side: the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

CoregShape = namedtuple("CoregShape", "he")
SMALL, BIG = CoregShape(32), CoregShape(48)
F, W, R, STEP, BANDS, MIN_POINTS, MIN_SCORE, REJECT = 6, 8, 6, 8, 2, 3, 0.6, 1.0
MIN_VALID = 48
TRUTH = dict(dy0=1.4, dx0=-2.2, dy_x=0.006, dy_y=-0.004, dx_x=0.005, dx_y=0.007)
NAMES = ["coreg_surface_kernel<float>", "coreg_peaks_kernel", "coreg_fit_model_kernel", "coreg_warp_kernel<float, LDS>"]


def _origins(he):
    ax = np.arange(1, min(he - W, (he * F - R - F * W) // F) + 1, STEP)
    return np.stack(np.meshgrid(ax, ax, indexing="ij"), axis=-1).reshape(-1, 2).astype(np.int32)


def _decoy(he):
    return len(_origins(he)) // 2


def _scene(he, k):
    """Set k of a shape: (emit (he, he), s2 (BANDS, hs, hs), origins)."""
    hs = he * F
    truth = cg.make_model(hs, hs, **TRUTH)
    emit, s2 = cg.scene_pair(he, he, F, truth, 60 + k)
    origins = _origins(he)
    if k == 1:
        i0, j0 = origins[_decoy(he)]
        off = cg.make_model(hs, hs, truth[0] - 4.0, truth[3] + 3.0, *truth[[1, 2, 4, 5]])
        emit[i0:i0 + W, j0:j0 + W] = cg.scene_pair(he, he, F, off, 60 + k)[0][i0:i0 + W, j0:j0 + W]
    if k == 2:
        emit[:] = np.nan
    return emit, np.stack([s2, np.roll(s2, 9, axis=0)]), origins


class CoregChain(cc.Chain):
    def allocate(self, s):
        T, hs, P, D = self.torch, s.he * F, len(_origins(s.he)), 2 * R + 1
        self.ins = dict(emit=Buf(T, s.he * s.he * 4), s2=Buf(T, BANDS * hs * hs * 4), origins=Buf(T, P * 8))
        self.outs = dict(surface=(Buf(T, P * D * D * 8), np.float64), table=(Buf(T, P * cg.REC * 8), np.float64),
                         model=(Buf(T, cg.MODEL * 8), np.float64), status=(Buf(T, 4, 4), np.int32),
                         out=(Buf(T, BANDS * hs * hs * 4), np.float32))

    def used(self, name):
        hs, P, D = self.shape.he * F, len(_origins(self.shape.he)), 2 * R + 1
        return {"surface": P * D * D * 8, "table": P * cg.REC * 8, "model": cg.MODEL * 8, "status": 4, "out": BANDS * hs * hs * 4}[name]

    def launch(self, st):
        he, i, o, lib = self.shape.he, self.ins, self.outs, self.lib
        hs, P = he * F, len(_origins(he))
        return [lib.hsr_coreg_surface(i["emit"].ptr, he, he, he, None, 0, i["s2"].ptr, 0, hs, hs, hs, 0, 0.0, i["origins"].ptr, P, W, F, R,
                                      MIN_VALID, o["surface"][0].ptr, st),
                lib.hsr_coreg_peaks(o["surface"][0].ptr, i["origins"].ptr, P, W, F, R, he, he, hs, hs, MIN_SCORE, o["table"][0].ptr, st),
                lib.hsr_coreg_fit_model(o["table"][0].ptr, P, 1, MIN_POINTS, REJECT, hs, hs, o["model"][0].ptr, st),
                lib.hsr_coreg_warp(i["s2"].ptr, 0, BANDS, hs, hs, hs * hs, hs, o["model"][0].ptr, 0, 0.0, float("nan"), R + 1.0, 0.05,
                                   o["out"][0].ptr, hs * hs, hs, o["status"][0].ptr, st)]


class CoregRow(cc.Row):
    chain, log = CoregChain, ("hsr_coreg_last_launch", True)

    def instances(self, s):
        return NAMES

    def make_inputs(self, s, k):
        emit, s2, origins = _scene(s.he, k)
        return dict(emit=emit, s2=s2, origins=origins)

    def make_reference(self, s, k):
        i, hs = self.inputs(s, k), s.he * F
        surf, bar = cg.surface_ref(i["emit"], None, i["s2"][0], None, i["origins"], W, F, R, MIN_VALID)
        table0 = cg.peaks_ref(surf, i["origins"], W, F, R, s.he, s.he, hs, hs, MIN_SCORE)
        table, model, coef, mbar = cg.model_ref(table0, 1, MIN_POINTS, REJECT, hs, hs)
        return dict(surface=surf, bar=bar, table0=table0, table=table, model=model, coef=coef, model_bar=mbar)

    def check(self, got, s, k, worst):
        r, i, hs = self.reference(s, k), self.inputs(s, k), s.he * F
        P = len(i["origins"])
        status = r["table"][:, 7]
        # the sets do what they are for
        want = np.zeros(P)
        if k == 1:
            want[_decoy(s.he)] = cg.OUTLIER
        if k == 2:
            want[:] = cg.NO_SCORE
        assert np.array_equal(status, want), (k, status)
        assert r["model"][9] == (-1 if k == 2 else 1) and r["model"][8] == (0, P, P - 1)[(k + 1) % 3]
        surf, table, model = got["surface"].reshape(r["surface"].shape), got["table"].reshape(P, cg.REC), got["model"]
        fin = np.isfinite(r["surface"])
        assert np.array_equal(np.isfinite(surf), fin) and np.isnan(surf[~fin]).all()
        if fin.any():
            err = np.abs(surf - r["surface"])[fin]
            assert (err <= r["bar"][fin]).all()
            cc._note(worst, f"set {k} surface", np.max(err / r["bar"][fin]))
            assert min(cg.peak_margin(x) for x in r["surface"]) >= cg.MARGIN and r["bar"][fin].max() <= cg.BAR_CAP
        assert np.array_equal(table[:, 7], status) and int(got["status"][0]) == 0
        assert (model[9], model[8]) == (r["model"][9], r["model"][8])
        if k < 2:
            bound, den_min = cg.shift_bar(r["surface"], r["bar"], r["table0"], R)
            ok = status == cg.OK
            assert den_min[ok].min() >= 1e-3
            err = np.abs(table[:, 2:4] - r["table"][:, 2:4])
            assert (err[ok] <= bound[ok]).all() and not table[~ok, 2:4].any()
            use, X, _ = cg._design(r["table"], hs, hs)
            Pm = np.abs(np.linalg.pinv(X))
            allowed = r["model_bar"] + np.stack([Pm @ bound[use, 0], Pm @ bound[use, 1]])
            diff = np.abs(cg.scaled_coefficients(model, hs, hs) - r["coef"])
            assert (diff <= allowed).all(), (diff, allowed)
            cc._note(worst, f"set {k} model", np.max(diff / allowed))
        else:
            assert not model[:9].any()
        ref, _ = cg.warp_ref(i["s2"], model, None, float("nan"))                 # the warp under the DEVICE's model: bit-equal
        out = got["out"].reshape(ref.shape)
        bits_equal(out, ref, f"set {k} warp")
        if k == 2:
            assert np.array_equal(out.view(np.uint32), i["s2"].view(np.uint32))   # the identity copy


ROWS = {"coreg-chain": CoregRow("coreg-chain", ("hsr_coreg_surface", "hsr_coreg_peaks", "hsr_coreg_fit_model", "hsr_coreg_warp"),
                                SMALL, BIG)}


def test_rows_cover_the_launch_path_entries():
    from s2_emit import _native as nat
    covered = {n for r in ROWS.values() for n in r.covers}
    launch_path = {n for n, (_, args) in nat.COREG_SIGNATURES.items() if n.startswith("hsr_coreg_") and "last_launch" not in n
                   and "instance" not in n and not n.endswith("_host")}
    assert covered == launch_path
    assert (len(_origins(SMALL.he)), len(_origins(BIG.he))) == (9, 25)
    assert MIN_VALID == int(np.ceil(0.75 * W * W))


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
