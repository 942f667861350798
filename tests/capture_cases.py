"""The table behind tests/test_gpu_graph_capture.py: chains of C-ABI calls as the Python drivers issue them, each with three input
sets of one shape that drive the chain's DEVICE-side decisions differently, the float64 / long double reference of every set and
the bar its family's instance suite already applies.  NumPy and ctypes marshalling only; not a test module.

What the table is for: include/hsr.h promises that every `*_dev` entry point allocates nothing, synchronises nothing and can be
captured in a hipGraph.  A captured chain freezes its host arguments; what may change between replays is the CONTENT of the buffers.
So a row is replayed over its three sets in the same buffers (a flag that sticks, a counter that does not rewind, gives set k + 1
the verdict of set k), and run big -> small -> big in buffers sized for the big shape (scratch a large call left behind).

A row (class Row) has
    covers      the hsr_* symbols its chain calls;
    shapes      {"small": ..., "big": ...}; the big one only as large as it takes to change the slot / chunk / workgroup count;
    reuse       True where the chain owns a work buffer or a device counter: the row takes part in the big -> small -> big step;
    log         (reader, joined) of the family's launch record, "srf" for K1's (SrfLog), or None where the family has none (OT);
    inputs(shape, k), reference(shape, k)          k = 0, 1, 2; cached, not to be written to;
    build(torch, alloc) -> Chain                   every buffer once, as gpu_harness.Buf, sized for `alloc`;
    check(got, shape, k, worst)                    the bar; `worst` collects observed error / bar of the bounded outputs.
A Chain has set_shape / refill(k) / restore() / sentinel() / launch(stream) / results().  launch allocates nothing and returns
the return codes of its calls.  In buffers sized for a larger shape the current shape's data is the contiguous prefix.

Every key of _native.SIGNATURES is in exactly one of: some row's covers, NOT_LAUNCH_PATH, EXCLUDED (name -> the reason, read from
the code).  EXCLUDED_FORMS names the one form of an entry WITH a row that is not capturable: the _apply launches given a job."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

import ortho_cases as oc
import ot_cases as otc
import scene_cases as sc
from gpu_harness import FILL, Buf, lib as _lib

LD = np.longdouble
U52 = 2.0 ** -52
SETS = (0, 1, 2)


# =============================================================================================================================
# the chain
# =============================================================================================================================
class Chain:
    """The device buffers of one row, sized for `alloc`.  ins / outs / work: name -> Buf; a name in both ins and outs is overwritten
    in place (in_place): restore() writes the current set into it again, sentinel() leaves it alone."""
    in_place = ()

    def __init__(self, torch, row, alloc):
        self.torch, self.row, self.lib, self.alloc = torch, row, _lib(), alloc
        self.ins, self.outs, self.work, self.k = {}, {}, {}, None
        self.allocate(alloc)
        self.set_shape(alloc)

    def set_shape(self, shape):
        self.shape = shape

    def refill(self, k):
        self.k = k
        for name, arr in self.row.inputs(self.shape, k).items():
            if name in self.ins:
                self.ins[name].put(arr)

    def restore(self):
        for name in self.in_place:
            self.ins[name].put(self.row.inputs(self.shape, self.k)[name])

    def sentinel(self):
        for name, (buf, _) in self.outs.items():
            if name not in self.in_place:
                buf.t[buf.lo: buf.lo + buf.nbytes] = FILL

    def reinit(self):
        """What include/hsr.h tells a caller to re-initialise between two calls on the same buffers: nothing, for every row so far."""

    def buffers(self):
        return list(self.ins.values()) + [b for b, _ in self.outs.values()] + list(self.work.values())

    def snapshot(self):
        """Every output and work buffer, raw."""
        snap = {name: buf.get(np.uint8) for name, (buf, _) in self.outs.items()}
        snap.update({"work:" + name: buf.get(np.uint8) for name, buf in self.work.items()})
        return snap

    def results(self):
        """name -> the current shape's part of every output (work buffers raw), after checking every guard zone, that the inputs
        are as they were and that an output's bytes past the current shape still hold the sentinel."""
        for b in self.buffers():
            b.get(np.uint8)
        want = self.row.inputs(self.shape, self.k)
        for name, buf in self.ins.items():
            if name not in self.in_place:
                raw = np.ascontiguousarray(want[name]).reshape(-1).view(np.uint8)
                assert np.array_equal(buf.get(np.uint8)[:raw.size], raw), f"input {name} was written to"
        out = {}
        for name, (buf, dtype) in self.outs.items():
            raw, used = buf.get(np.uint8), self.used(name)
            if name not in self.in_place:
                assert (raw[used:] == FILL).all(), f"{name}: write past the current shape's output"
            out[name] = raw[:used].view(dtype).copy()
        for name, buf in self.work.items():
            out[name] = buf.get(np.uint8)
        return out


class Row:
    reuse, log = True, None

    def __init__(self, name, covers, small, big):
        self.name, self.covers, self.shapes = name, tuple(covers), {"small": small, "big": big}

    def build(self, torch, alloc):
        return self.chain(torch, self, alloc)

    def instances(self, shape):
        """The launch record the chain must leave (as LaunchLog.read gives it), or None where it is not predicted here."""
        return None

    @functools.lru_cache(maxsize=None)
    def inputs(self, shape, k):
        out = self.make_inputs(shape, k)
        for a in out.values():
            a.setflags(write=False)
        return out

    @functools.lru_cache(maxsize=None)
    def reference(self, shape, k):
        return self.make_reference(shape, k)


def _note(worst, key, value):
    worst[key] = max(worst.get(key, 0.0), float(value))


# =============================================================================================================================
# hsr_ortho_glt: the dropped counter is zeroed in-stream by every call
# =============================================================================================================================
OrthoShape = namedtuple("OrthoShape", "bands rows cols gh gw layout q bm")
ORTHO_GRIDS = ("mixed", "valid", "dropped")             # dropped > 0, = 0, > 0
ORTHO_FILL, ORTHO_MASKED = -9999.0, -7777.5


class OrthoChain(Chain):
    def allocate(self, s):
        bb = (s.bands + 7) // 8 + 1 if s.bm else 0
        self.ins = dict(swath=Buf(self.torch, s.rows * s.cols * s.bands * 4), glt=Buf(self.torch, s.gh * s.gw * 8))
        if s.q:
            self.ins["qmask"] = Buf(self.torch, s.rows * s.cols)
        if s.bm:
            self.ins["bmask"] = Buf(self.torch, s.rows * s.cols * bb)
        self.outs = dict(out=(Buf(self.torch, s.gh * s.gw * s.bands * 4), np.uint32), dropped=(Buf(self.torch, 8, 8), np.int64))

    def used(self, name):
        return self.shape.gh * self.shape.gw * self.shape.bands * 4 if name == "out" else 8

    def launch(self, st):
        s, i = self.shape, self.ins
        bb = (s.bands + 7) // 8 + 1 if s.bm else 0
        return [self.lib.hsr_ortho_glt(i["swath"].ptr, s.rows, s.cols, s.bands, i["glt"].ptr, s.gh, s.gw, 0, 0, 0, s.gh, s.gw,
                                       i["qmask"].ptr if s.q else None, i["bmask"].ptr if s.bm else None, bb, ORTHO_FILL, ORTHO_MASKED,
                                       s.layout, self.outs["out"][0].ptr, self.outs["dropped"][0].ptr, st)]


class OrthoRow(Row):
    """Bar: bit equality of the output and the exact count (tests/test_gpu_ortho_instances.py::test_rows)."""
    chain, log = OrthoChain, ("hsr_ortho_last_launch", False)

    def instances(self, s):
        return oc.instance(s.layout, s.bands, s.q or s.bm)

    def make_inputs(self, s, k):
        bb = (s.bands + 7) // 8 + 1
        out = dict(swath=np.roll(oc.swath_of(s.rows, s.cols, s.bands), k, axis=1).copy(),
                   glt=oc.glt_of(ORTHO_GRIDS[k], s.gh, s.gw, s.rows, s.cols).copy())
        if s.q:
            out["qmask"] = np.roll(oc.qmask_of(s.rows, s.cols), k, axis=0).copy()
        if s.bm:
            out["bmask"] = np.roll(oc.bmask_of(s.rows, s.cols, s.bands, bb), k, axis=1).copy()
        return out

    def make_reference(self, s, k):
        i = self.inputs(s, k)
        ref, dropped = oc.ortho_ref(i["swath"], i["glt"], None, i.get("qmask"), i.get("bmask"), ORTHO_FILL, ORTHO_MASKED, 0, s.layout)
        return dict(out=ref.reshape(-1), dropped=dropped)

    def check(self, got, s, k, worst):
        ref = self.reference(s, k)
        np.testing.assert_array_equal(got["out"], ref["out"])
        assert int(got["dropped"][0]) == ref["dropped"], (int(got["dropped"][0]), ref["dropped"])


# =============================================================================================================================
# hsr_scene_black_counts: the counts are zeroed in-stream by every call
# =============================================================================================================================
SceneShape = namedtuple("SceneShape", "bands H W th tw")
SCAN_KW = dict(nodata=-9999.0, masked_val=-0.01, nodata_atol=1e-3, zero_atol=1e-6)


class ScanChain(Chain):
    def allocate(self, s):
        self.ins = dict(scene=Buf(self.torch, s.bands * s.H * s.W * 4))
        self.outs = dict(counts=(Buf(self.torch, (s.H // s.th) * (s.W // s.tw) * 4, 4), np.int32))

    def used(self, name):
        s = self.shape
        return (s.H // s.th) * (s.W // s.tw) * 4

    def launch(self, st):
        s = self.shape
        return [self.lib.hsr_scene_black_counts(self.ins["scene"].ptr, 0, s.bands, s.H, s.W, s.th, s.tw, 1, SCAN_KW["nodata"],
                                                SCAN_KW["masked_val"], SCAN_KW["nodata_atol"], SCAN_KW["zero_atol"],
                                                self.outs["counts"][0].ptr, st)]


class ScanRow(Row):
    """A black border, a clean scene, all black.  Bar: the exact counts (tests/test_gpu_scene_instances.py::test_scan_deciding_band)."""
    chain, log = ScanChain, ("hsr_scene_last_launch", False)

    def instances(self, s):
        return sc.scan_instance(np.float32)

    def make_inputs(self, s, k):
        rng = np.random.default_rng(100 + k)
        scene = (0.05 + rng.random((s.bands, s.H, s.W))).astype(np.float32)
        if k == 0:                                                        # a border of the three black values, one pixel inside too
            scene[:, :2, :], scene[:, -1, :], scene[:, :, :3], scene[:, :, -2:] = 0.0, -9999.0, -0.01, 0.0
            scene[:, s.H // 2, s.W // 2] = 0.0
            scene[0, 0, 0] = 0.5                                          # black in every band but one: not black
        elif k == 2:
            scene[:] = np.array([0.0, -9999.0, -0.01], np.float32)[rng.integers(0, 3, (s.H, s.W))]
        return dict(scene=scene)

    def make_reference(self, s, k):
        return dict(counts=sc.scan_ref(self.inputs(s, k)["scene"], s.th, s.tw, **SCAN_KW).reshape(-1))

    def check(self, got, s, k, worst):
        np.testing.assert_array_equal(got["counts"], self.reference(s, k)["counts"])


# =============================================================================================================================
# hsr_chol_solve_f64 / _batched: the bad-pivot status
# =============================================================================================================================
CholShape = namedtuple("CholShape", "n P nrhs")


def chol_layout(s):
    """(lda, ldb, pair stride of A, of B) in elements: padded rows, and pair strides that are no multiple of the rows."""
    lda, ldb = s.n + 1, s.nrhs + 2
    return lda, ldb, s.n * lda + (4 if s.P > 1 else 0), s.n * ldb + (6 if s.P > 1 else 0)


def chol_bad_pivot(s):
    """The pivot set 1 makes non-positive (0-based), in the last system: in the third 32-block of the small shape, the fifth of the big."""
    return s.n // 2 + 22


class CholChain(Chain):
    in_place = ("A", "B")

    def allocate(self, s):
        _, _, pa, pb = chol_layout(s)
        a, b = Buf(self.torch, s.P * pa * 8, 8), Buf(self.torch, s.P * pb * 8)
        self.ins = dict(A=a, B=b)
        self.outs = dict(A=(a, np.float64), B=(b, np.float64), info=(Buf(self.torch, 4 * s.P), np.int32))
        self.work = dict(work=Buf(self.torch, s.P * self.lib.hsr_chol_work_bytes(s.n)))

    def used(self, name):
        s = self.shape
        _, _, pa, pb = chol_layout(s)
        return dict(A=s.P * pa * 8, B=s.P * pb * 8, info=4 * s.P)[name]

    def launch(self, st):
        s = self.shape
        lda, ldb, pa, pb = chol_layout(s)
        a, b, info, work = self.ins["A"].ptr, self.ins["B"].ptr, self.outs["info"][0].ptr, self.work["work"].ptr
        if s.P == 1:
            return [self.lib.hsr_chol_solve_f64(a, lda, s.n, b, ldb, s.nrhs, work, info, st)]
        return [self.lib.hsr_chol_solve_f64_batched(a, lda, s.n, pa, b, ldb, s.nrhs, pb, work, info, s.P, st)]


class CholRow(Row):
    """Positive definite, a non-positive pivot in a later 32-block (last system), positive definite again.  Bars, of
    tests/test_gpu_k4_instances.py::test_chol on its well-conditioned class: L against numpy.linalg.cholesky at rtol 1e-10 /
    atol 1e-12, the solution against numpy.linalg.solve at rtol 1e-9 / atol 1e-11, LAPACK's two normwise ratios in long double
    <= 1; ::test_chol_bad_pivot: info = the pivot's 1-based index, the other systems' info 0."""
    chain, log = CholChain, ("hsr_k4_last_launch", True)

    def instances(self, s):
        return [("chol_factor_res_kernel" if s.n <= 288 else "chol_factor_kernel"), "chol_solve_kernel " + ("lds" if s.n <= 384 else "global")]

    def systems(self, s, k):
        """-> [(A, B, info)] of set k."""
        rng = np.random.default_rng(1000 * s.n + 10 * s.P + k)
        out = []
        for p in range(s.P):
            M = rng.standard_normal((s.n, s.n + 40))
            A = M @ M.T / s.n + 0.3 * np.eye(s.n)                          # test_gpu_k4_instances._spd "project": cond ~ 10
            info = 0
            if k == 1 and p == s.P - 1:
                kp = chol_bad_pivot(s)
                A[kp, kp] -= np.linalg.cholesky(A)[kp, kp] ** 2 + 1.0     # Schur pivot kp becomes -1
                info = kp + 1
            out.append((A, rng.standard_normal((s.n, s.nrhs)), info))
        return out

    def make_inputs(self, s, k):
        lda, ldb, pa, pb = chol_layout(s)
        A, B = np.full((s.P, pa), np.nan), np.full((s.P, pb), np.nan)     # gaps and the strict upper triangle: NaN
        for p, (a, b, _) in enumerate(self.systems(s, k)):
            a = a.copy()
            a[np.triu_indices(s.n, 1)] = np.nan
            A[p, :s.n * lda].reshape(s.n, lda)[:, :s.n] = a
            B[p, :s.n * ldb].reshape(s.n, ldb)[:, :s.nrhs] = b
        return dict(A=A, B=B)

    def make_reference(self, s, k):
        return [dict(info=info, L=np.linalg.cholesky(a), X=np.linalg.solve(a, b)) if info == 0 else dict(info=info)
                for a, b, info in self.systems(s, k)]

    def check(self, got, s, k, worst):
        lda, ldb, pa, pb = chol_layout(s)
        ref, given = self.reference(s, k), self.inputs(s, k)
        assert list(got["info"]) == [r["info"] for r in ref], (list(got["info"]), k)
        Ag, Bg = got["A"].reshape(s.P, pa), got["B"].reshape(s.P, pb)
        for p, (a, b, info) in enumerate(self.systems(s, k)):
            rows, brow = Ag[p, :s.n * lda].reshape(s.n, lda), Bg[p, :s.n * ldb].reshape(s.n, ldb)
            assert np.isnan(rows[:, s.n:]).all() and np.isnan(brow[:, s.nrhs:]).all() and np.isnan(Ag[p, s.n * lda:]).all(), "write into a gap"
            assert np.isnan(rows[:, :s.n][np.triu_indices(s.n, 1)]).all(), "write above the diagonal"         # n <= 288
            if info:
                continue
            L, X = np.tril(rows[:, :s.n]), brow[:, :s.nrhs]
            np.testing.assert_allclose(L, ref[p]["L"], rtol=1e-10, atol=1e-12)
            np.testing.assert_allclose(X, ref[p]["X"], rtol=1e-9, atol=1e-11)
            _note(worst, "chol factor vs numpy (rtol 1e-10 / atol 1e-12)", np.max(np.abs(L - ref[p]["L"]) / (1e-12 + 1e-10 * np.abs(ref[p]["L"]))))
            _note(worst, "chol solution vs numpy (rtol 1e-9 / atol 1e-11)", np.max(np.abs(X - ref[p]["X"]) / (1e-11 + 1e-9 * np.abs(ref[p]["X"]))))
            Al, Ll, Xl = a.astype(LD), L.astype(LD), X.astype(LD)
            anorm = np.abs(Al).sum(axis=1).max()
            r1 = np.abs(Ll @ Ll.T - Al).sum(axis=1).max() / (s.n * anorm * U52)
            r2 = np.abs(Al @ Xl - b.astype(LD)).sum(axis=0).max() / (s.n * anorm * np.abs(Xl).sum(axis=0).max() * U52)
            _note(worst, "chol factor ratio (<= 1)", r1)
            _note(worst, "chol solve ratio (<= 1)", r2)
            assert r1 <= 1 and r2 <= 1, (float(r1), float(r2))
        assert given["A"].shape == Ag.shape


# =============================================================================================================================
# OT: the OtState that makes later iterations no-ops after a stop or a breakdown
# =============================================================================================================================
OtShape = namedtuple("OtShape", "n m")
OT_REG, OT_ITMAX, OT_THR = 0.01, 40, 1e-9               # the settings of ot_cases' breakdown rows
OT_BREAK = {OtShape(97, 65): "break1-u", OtShape(130, 66): "break12-v"}    # found by tools/scan_ot_cases.py for ot_cases.ROWS


def ot_regions(n, m):
    off, cnt, out = C.c_int64(), C.c_int64(), []
    for which in range(8):
        assert _lib().hsr_ot_work_region(n, m, which, C.byref(off), C.byref(cnt)) == 0
        out.append((off.value, cnt.value))
    return out


def ot_state(raw):
    """(break_iter, conv_iter, checks) of 24 state bytes; None for 'never'."""
    i = raw[:12].view(np.int32)
    return (None if i[0] == otc.NEVER else int(i[0]), None if i[1] == otc.NEVER else int(i[1]), int(i[2]))


class OtChain(Chain):
    def allocate(self, s):
        self.ins = dict(X=Buf(self.torch, s.n * 24), Y=Buf(self.torch, s.m * 24))
        self.outs = dict(ybar=(Buf(self.torch, s.n * 24), np.float64), info=(Buf(self.torch, 24), np.uint8))
        self.work = dict(work=Buf(self.torch, self.lib.hsr_ot_work_bytes(s.n, s.m)))

    def used(self, name):
        return self.shape.n * 24 if name == "ybar" else 24

    def launch(self, st):
        s, lib = self.shape, self.lib
        x, y, w, ybar, info = self.ins["X"].ptr, self.ins["Y"].ptr, self.work["work"].ptr, self.outs["ybar"][0].ptr, self.outs["info"][0].ptr
        if self.row.staged:
            return [lib.hsr_ot_begin(x, s.n, y, s.m, OT_REG, w, st), lib.hsr_ot_iterate(s.n, s.m, 0, OT_ITMAX, OT_THR, w, info, st),
                    lib.hsr_ot_finish(y, s.n, s.m, OT_ITMAX, w, ybar, info, st)]
        return [lib.hsr_ot_sinkhorn_barycentric(x, s.n, y, s.m, OT_REG, OT_ITMAX, OT_THR, w, ybar, info, st)]


class OtRow(Row):
    """Set 0 uses all 40 iterations, set 1 breaks down (at iteration 1, small shape; 12, big), set 2 - every source point the
    same, so that K has equal rows and one iteration is exact - meets the stop rule at iteration 0.  Bars, of
    tests/test_gpu_ot_instances.py: the state (break_iter, conv_iter, checks) is the one of ot_cases.solve; K within
    ot_cases.kernel_matrix_bound; Ybar within ot_cases.projection's bound of the projection of the device's own (K, u, v) of the
    buffer ot_cases.final_buffer names."""
    chain = OtChain

    def __init__(self, name, covers, small, big, staged):
        super().__init__(name, covers, small, big)
        self.staged = staged

    def make_inputs(self, s, k):
        if k == 0:
            X, Y = otc.clouds(s.n, s.m, s.n + s.m)
        elif k == 1:
            X, Y = otc.inputs(OT_BREAK[s])
        else:
            rng = np.random.default_rng(s.n)
            X, Y = np.full((s.n, 3), 0.5), 0.4 + 0.2 * rng.random((s.m, 3))
        return dict(X=np.ascontiguousarray(X, np.float64).copy(), Y=np.ascontiguousarray(Y, np.float64).copy())

    def make_reference(self, s, k):
        i = self.inputs(s, k)
        return otc.solve(i["X"], i["Y"], OT_REG, OT_ITMAX, OT_THR)

    def check(self, got, s, k, worst):
        i, ref = self.inputs(s, k), self.reference(s, k)
        want = (ref["break_iter"], ref["conv_iter"], ref["checks"])
        assert ot_state(got["info"]) == want, (ot_state(got["info"]), want)
        part = [got["work"][o: o + 8 * c] for o, c in ot_regions(s.n, s.m)]
        assert ot_state(part[otc.STATE]) == want
        f = [p.view(np.float64) for p in part]
        K = f[otc.K_].reshape(s.n, s.m)
        K_ref = otc.kernel_matrix(i["X"], i["Y"], OT_REG)
        _bounded(worst, "ot K", K, K_ref, otc.kernel_matrix_bound(i["X"], i["Y"], OT_REG, K_ref))
        buf = otc.final_buffer(ref["break_iter"], ref["conv_iter"], OT_ITMAX)
        pref, bound = otc.projection(K, f[otc.U0 + buf], f[otc.V0 + buf], i["Y"])
        _bounded(worst, "ot projection", got["ybar"].reshape(s.n, 3), pref, bound)


def _bounded(worst, key, got, ref, bound):
    """|got - ref| <= bound elementwise, as test_gpu_ot_instances._worst."""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, LD), np.asarray(bound, LD)
    assert np.isfinite(got).all(), f"{key}: non-finite device value"
    assert np.isfinite(bound).all() and (bound >= 0).all(), f"{key}: the reference gives no bound here"
    diff = np.abs(got.astype(LD) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.where(diff == 0, LD(0), diff / bound)
    _note(worst, key + " (of the bound)", np.max(frac))
    assert np.max(frac) <= 1.0, f"{key}: {float(np.max(frac)):.3g} of the bound"


# =============================================================================================================================
# percentiles: the workspace (histograms, per-band state, compaction counters) that hsr_percentile_begin zeroes in-stream
# =============================================================================================================================
PctShape = namedtuple("PctShape", "npix nb")
PCT_PAIR = (50.0, 98.0)
TINY_MAX = 32768                                        # kTinyMaxPix of csrc/hsr_select.hip


class PctChain(Chain):
    def allocate(self, s):
        self.ins = dict(x=Buf(self.torch, s.nb * s.npix * 4), mask=Buf(self.torch, s.npix))
        self.outs = dict(lohi=(Buf(self.torch, s.nb * 16), np.float64))
        self.work = dict(work=Buf(self.torch, self.lib.hsr_percentile_work_bytes(s.nb)))

    def used(self, name):
        return self.shape.nb * 16

    def launch(self, st):
        s, lib = self.shape, self.lib
        x, mask, w, lohi = self.ins["x"].ptr, self.ins["mask"].ptr, self.work["work"].ptr, self.outs["lohi"][0].ptr
        if not self.row.staged:
            return [lib.hsr_percentile_limits(x, s.npix, 1, mask, s.npix, s.nb, PCT_PAIR[0], PCT_PAIR[1], w, lohi, st)]
        rcs = [lib.hsr_percentile_begin(w, s.nb, st)]
        for p in (1, 2, 3):
            rcs += [lib.hsr_percentile_hist(p, x, s.npix, 1, mask, s.npix, s.nb, w, st),
                    lib.hsr_percentile_scan(p, s.nb, PCT_PAIR[0], PCT_PAIR[1], w, lohi, st)]
        return rcs


class PctRow(Row):
    """Band-major planes and ONE mask for all bands.  Set 0: NaN samples - masked out in band 0, one inside the mask in band 1, whose
    limits are then NaN - and a random mask; set 1: every pixel masked out (no sample in any band: NaN limits); set 2: two values in
    different pass-1 bins, half the samples each, so that the two ranks of the 50th percentile straddle the bin edge, and rounded
    noise full of ties in the other bands.  Bar: equal to np.percentile of the masked float32 values, NaN in the same places
    (tests/test_gpu_aux_instances.py::_select_run)."""
    chain, log = PctChain, ("hsr_aux_last_launch", False)

    def __init__(self, name, covers, small, big, staged):
        super().__init__(name, covers, small, big)
        self.staged = staged

    def instances(self, s):
        return "select_scan_kernel<3>" if self.staged or s.npix > TINY_MAX else "select_tiny_kernel"

    def make_inputs(self, s, k):
        rng = np.random.default_rng(7 * s.npix + k)
        x = rng.normal(0.3, 0.2, (s.nb, s.npix)).astype(np.float32)
        if k == 0:
            mask = (rng.random(s.npix) < 0.6).astype(np.uint8)
            out_of, inside = np.flatnonzero(mask == 0), np.flatnonzero(mask)
            x[0, out_of[::7]] = np.nan
            x[1, inside[len(inside) // 2]] = np.nan
        elif k == 1:
            mask = np.zeros(s.npix, np.uint8)
        else:
            mask = np.ones(s.npix, np.uint8)
            mask[-1] = s.npix % 2 == 0                                    # an even count: the 50th percentile lies between two samples
            x[:] = np.round(x * 8) / 8
            x[0] = np.where(np.arange(s.npix) % 2 == 0, np.float32(0.25), np.float32(0.75))
        return dict(x=x, mask=mask)

    def make_reference(self, s, k):
        import warnings
        i = self.inputs(s, k)
        ref = np.empty((s.nb, 2))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for c in range(s.nb):
                vals = i["x"][c][i["mask"] != 0]
                ref[c] = np.percentile(vals, list(PCT_PAIR)) if len(vals) else np.nan
        return dict(lohi=ref)

    def check(self, got, s, k, worst):
        np.testing.assert_array_equal(got["lohi"].reshape(s.nb, 2), self.reference(s, k)["lohi"])


# =============================================================================================================================
# K2 on planes that exist already: moments -> slot reduction -> solve (-> K3): partial slots beyond the new slot count
# =============================================================================================================================
FitShape = namedtuple("FitShape", "npix nb deg")
FIT_MIN_COUNT, FIT_MIN_X, FIT_MIN_Y = 50, 0.05, -0.1


def fit_slots(npix):
    return min((npix + 63) // 64, 512)                   # include/hsr.h, hsr_partial_slots: the default geometry of hsr_poly_moments


def fit_valid(x, y, mask):
    """per band: mask && finite(x) && finite(y) && x > min_x && y > min_y (include/hsr.h, hsr_srf_integrate_moments)."""
    with np.errstate(invalid="ignore"):
        return (mask != 0)[None, :] & np.isfinite(x) & np.isfinite(y) & (x > np.float32(FIT_MIN_X)) & (y > np.float32(FIT_MIN_Y))


class FitChain(Chain):
    def allocate(self, s):
        M, item = 3 * s.deg + 2, 8 if self.row.f64 else 4
        self.ins = dict(x=Buf(self.torch, s.nb * s.npix * item), y=Buf(self.torch, s.nb * s.npix * item))
        self.outs = dict(moments=(Buf(self.torch, s.nb * M * 8), np.float64), coeffs=(Buf(self.torch, s.nb * (s.deg + 1) * 8), np.float64))
        if not self.row.f64:
            self.ins["mask"] = Buf(self.torch, s.npix)
            self.outs["matched"] = (Buf(self.torch, s.nb * s.npix * 4), np.float32)
        self.work = dict(partials=Buf(self.torch, self.lib.hsr_partials_bytes(s.nb, s.deg)))
        self.slots = C.c_int32(-1)

    def used(self, name):
        s = self.shape
        return dict(moments=s.nb * (3 * s.deg + 2) * 8, coeffs=s.nb * (s.deg + 1) * 8, matched=s.nb * s.npix * 4)[name]

    def launch(self, st):
        s, lib, i, o = self.shape, self.lib, self.ins, self.outs
        part, mom, co = self.work["partials"].ptr, o["moments"][0].ptr, o["coeffs"][0].ptr
        if self.row.f64:
            rcs = [lib.hsr_poly_moments_f64(i["x"].ptr, s.npix, i["y"].ptr, s.npix, s.npix, s.nb, s.deg, part, C.byref(self.slots), st)]
            assert self.slots.value == fit_slots(s.npix)
            return rcs + [lib.hsr_moments_reduce_solve(part, self.slots.value, s.nb, s.deg, FIT_MIN_COUNT, mom, co, st)]
        rcs = [lib.hsr_poly_moments(i["x"].ptr, s.npix, 1, i["y"].ptr, s.npix, 1, i["mask"].ptr, s.npix, s.nb, s.deg, FIT_MIN_X, FIT_MIN_Y,
                                    None, None, part, C.byref(self.slots), st)]
        assert self.slots.value == fit_slots(s.npix)
        return rcs + [lib.hsr_moments_reduce(part, self.slots.value, s.nb, s.deg, mom, st),
                      lib.hsr_poly_solve(mom, s.nb, s.deg, FIT_MIN_COUNT, co, st),
                      lib.hsr_poly_apply(i["x"].ptr, s.npix, 1, i["mask"].ptr, co, s.nb, s.deg, s.npix, None, 1,
                                         o["matched"][0].ptr, s.npix, 1, st)]


class FitRow(Row):
    """Set 0 plain (a random mask, a few non-finite samples); set 1: band 1 keeps fewer than min_count valid pixels - the identity
    fallback, fixture g9's rule - under another mask; set 2: a mask of ones (the pointer is fixed at capture) and every band fitted.
    Bars, of tests/test_gpu_poly_instances.py: moments - count exact, the other sums at rtol 1e-12 against float64
    (::_check_moments); coefficients - the bits of the host twin hsr_poly_solve_host on the device's moments, np.polyfit at rtol 1e-7 /
    atol 1e-9 on the fitted bands, exactly the identity on the fallback band
    (::test_solve_entry_points_identical_and_match_polyfit); matched - the bits of float64 Horner with the device's coefficients,
    mask select, clip (::_apply_ref)."""
    chain, log = FitChain, ("hsr_poly_last_launch", False)

    def __init__(self, name, covers, small, big, f64):
        super().__init__(name, covers, small, big)
        self.f64 = f64

    def instances(self, s):
        return "reduce_solve_kernel" if self.f64 else "apply_planar_kernel<%s>" % ("true" if s.npix % 4 == 0 else "false")

    def make_inputs(self, s, k):
        rng = np.random.default_rng(11 * s.npix + k + (100 if self.f64 else 0))
        dt = np.float64 if self.f64 else np.float32
        x = rng.uniform(0.06, 1.0, (s.nb, s.npix))
        y = 0.2 + (0.7 + 0.1 * k) * x - 0.3 * x * x + 0.02 * rng.standard_normal((s.nb, s.npix))
        x, y = x.astype(dt), y.astype(dt)
        mask = np.ones(s.npix, np.uint8) if k == 2 or self.f64 else (rng.random(s.npix) < (0.7, 0.8)[k]).astype(np.uint8)
        if k < 2:
            x[0, 5::97], y[2, 7::89] = np.nan, np.inf
        if k == 1:                                                        # band 1: 49 valid pixels, one fewer than min_count
            keep = np.flatnonzero(mask)[:FIT_MIN_COUNT - 1]
            gone = np.ones(s.npix, bool)
            gone[keep] = False
            (x if self.f64 else y)[1, gone] = np.nan
        out = dict(x=x, y=y)
        if not self.f64:
            out["mask"] = mask
        return out

    def valid(self, s, k):
        i = self.inputs(s, k)
        if self.f64:                                                      # hsr_poly_moments_f64: finite x and y only
            return np.isfinite(i["x"]) & np.isfinite(i["y"])
        return fit_valid(i["x"], i["y"], i["mask"])

    def make_reference(self, s, k):
        from test_gpu_poly_instances import _moments_ref, _polyfit
        i, ok = self.inputs(s, k), self.valid(s, k)
        ident = np.zeros(s.deg + 1)
        ident[-2] = 1.0
        mom = np.stack([_moments_ref(i["x"][b][ok[b]], i["y"][b][ok[b]], s.deg) for b in range(s.nb)])
        fitted = ok.sum(axis=1) >= FIT_MIN_COUNT
        co = np.stack([_polyfit(i["x"][b][ok[b]], i["y"][b][ok[b]], s.deg) if fitted[b] else ident for b in range(s.nb)])
        return dict(moments=mom, coeffs=co, fitted=fitted)

    def check(self, got, s, k, worst):
        from s2_emit import _engine as eng
        from test_gpu_poly_instances import _apply_ref, _check_moments
        i, ref = self.inputs(s, k), self.reference(s, k)
        mom, co = got["moments"].reshape(s.nb, -1), got["coeffs"].reshape(s.nb, -1)
        for b in range(s.nb):
            _check_moments(mom[b], ref["moments"][b], f"band {b}")
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.abs(mom[b] - ref["moments"][b]) / np.abs(ref["moments"][b])
            _note(worst, "fit moments / rtol 1e-12", np.nanmax(np.where(ref["moments"][b] == 0, 0.0, rel)) / 1e-12)
            if ref["fitted"][b]:
                np.testing.assert_allclose(co[b], ref["coeffs"][b], rtol=1e-7, atol=1e-9)
                _note(worst, "fit coefficients vs np.polyfit (rtol 1e-7 / atol 1e-9)",
                      np.max(np.abs(co[b] - ref["coeffs"][b]) / (1e-9 + 1e-7 * np.abs(ref["coeffs"][b]))))
            else:
                assert np.array_equal(co[b], ref["coeffs"][b]), (b, co[b])
        host = eng.poly_solve_host(np.ascontiguousarray(mom), s.deg, FIT_MIN_COUNT)
        assert np.array_equal(co.view(np.int64), host.view(np.int64)), "coefficients are not the host twin's bits"
        if not self.f64:
            want = _apply_ref(np.ascontiguousarray(i["x"].T), co, None, i["mask"], True).T
            a, b = got["matched"].reshape(s.nb, s.npix), np.ascontiguousarray(want)
            nan = np.isnan(b)
            assert np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]), "matched"


# =============================================================================================================================
# K1: SRF integration alone, the operator step (K1+K2 -> reduce + solve -> K3) and the fused fit with its tickets
# =============================================================================================================================
K1Shape = namedtuple("K1Shape", "H W")
K1_DEG, K1_MIN_COUNT, K1_NODATA = 2, 20, 65535
K1_SCALE = float(np.float32(1e-4))


class SrfLog:
    """hsr_srf_last_launch behind the interface of gpu_harness.LaunchLog: (deg, variant, lds bytes) of the last K1 launch."""

    def clear(self):
        _lib().hsr_srf_last_launch(None, None, None)

    def read(self):
        d, v, lds = C.c_int32(), C.c_int32(), C.c_int64()
        return (d.value, v.value, lds.value) if _lib().hsr_srf_last_launch(C.byref(d), C.byref(v), C.byref(lds)) == 1 else None


@functools.lru_cache(maxsize=None)
def k1_table():
    """(emit wavelengths, srf dict, good mask, SrfTable) of the 285-sample synthetic table: 12 supported bands."""
    from oracle import oracle_np as onp
    from s2_emit import _engine as eng
    w, good = onp.synthetic_wavelengths()
    srf = onp.synthetic_srf()
    return w, srf, good, eng.build_srf_table(w, srf, good)


class K1Chain(Chain):
    def allocate(self, s):
        from s2_emit import _native as nat
        t = k1_table()[3]
        self.nb, self.B, npix, M = t.nb, t.B, s.H * s.W, 3 * K1_DEG + 2
        self.k0, self.klen = (C.c_int32 * t.nb)(*t.k0.tolist()), (C.c_int32 * t.nb)(*t.klen.tolist())
        self.wn = Buf(self.torch, t.nb * t.B * 4, 0, t.weights.astype(np.float32))
        self.ins = dict(cube=Buf(self.torch, npix * t.B * (2 if self.row.u16 else 4)))
        self.outs = dict(pseudo=(Buf(self.torch, npix * t.nb * 4), np.float32))
        if self.row.mode != "k1":
            self.ins.update(real=Buf(self.torch, npix * t.nb * 4), mask=Buf(self.torch, npix))
            self.outs.update(moments=(Buf(self.torch, t.nb * M * 8), np.float64), coeffs=(Buf(self.torch, t.nb * (K1_DEG + 1) * 8), np.float64),
                             matched=(Buf(self.torch, npix * t.nb * 4), np.float32))
            self.work = dict(partials=Buf(self.torch, self.lib.hsr_partials_bytes(t.nb, K1_DEG)))
        if self.row.mode == "fit":
            # include/hsr.h, hsr_fused_fit: 64 * nb * (3 deg + 2) doubles of scratch; 65 tickets, ZERO before the first launch
            self.work["group_partials"] = Buf(self.torch, nat.HSR_FIT_GROUPS * t.nb * M * 8)
            self.work["tickets"] = Buf(self.torch, nat.HSR_FIT_TICKETS * 4, 0, np.zeros(nat.HSR_FIT_TICKETS, np.int32))
            self.fit = nat.FusedFit(self.work["group_partials"].ptr.value, self.work["tickets"].ptr.value,
                                    self.outs["moments"][0].ptr.value, self.outs["coeffs"][0].ptr.value, K1_MIN_COUNT)
        self.slots, self.plan = C.c_int32(-1), None
        if self.row.mode.startswith("plan"):                              # a plan is a host object bound to one npix: made here
            o = self.outs
            desc = nat.StepDesc(2 if self.row.u16 else 0, t.B, npix, K1_SCALE, K1_NODATA, self.wn.ptr, self.k0, self.klen, t.nb, K1_DEG,
                                o["pseudo"][0].ptr, 1, t.nb, 1, t.nb, 0.0, 0.0, self.work["partials"].ptr, o["moments"][0].ptr,
                                o["coeffs"][0].ptr, K1_MIN_COUNT, o["matched"][0].ptr, 1, t.nb, 1, 1, nat.SrfOptions(0, 0, 0, 0))
            self.plan = C.c_void_p()
            assert self.lib.hsr_step_plan_create(C.byref(desc), C.byref(self.plan)) == 0, self.lib.hsr_last_error()

    def __del__(self):
        if getattr(self, "plan", None):
            self.lib.hsr_step_plan_destroy(self.plan)

    def set_shape(self, shape):
        assert self.plan is None or shape == self.alloc, "a step plan is bound to its npix"
        self.shape = shape

    def buffers(self):
        return super().buffers() + [self.wn]

    def used(self, name):
        npix, nb = self.shape.H * self.shape.W, self.nb
        return dict(pseudo=npix * nb * 4, matched=npix * nb * 4, moments=nb * (3 * K1_DEG + 2) * 8, coeffs=nb * (K1_DEG + 1) * 8)[name]

    def launch(self, st):
        lib, i, o, nb, u16, mode = self.lib, self.ins, self.outs, self.nb, self.row.u16, self.row.mode
        npix = self.shape.H * self.shape.W
        head = (i["cube"].ptr, npix, self.B) + ((K1_SCALE, K1_NODATA) if u16 else ()) + (self.wn.ptr, self.k0, self.klen, nb, o["pseudo"][0].ptr, 1, nb)
        if mode == "k1":
            return [(lib.hsr_srf_integrate_u16 if u16 else lib.hsr_srf_integrate)(*head, None, st)]
        if mode == "plan":
            return [lib.hsr_step_run(self.plan, i["cube"].ptr, i["real"].ptr, i["mask"].ptr, st)]
        if mode == "plan-pieces":
            return [lib.hsr_step_run_k1(self.plan, i["cube"].ptr, i["real"].ptr, i["mask"].ptr, st), lib.hsr_step_run_reduce(self.plan, st),
                    lib.hsr_step_run_solve(self.plan, st), lib.hsr_step_run_apply(self.plan, i["mask"].ptr, st)]
        fitargs = head + (i["real"].ptr, 1, nb, i["mask"].ptr, 0.0, 0.0, K1_DEG, self.work["partials"].ptr, C.byref(self.slots))
        if mode == "fit":
            rcs = [(lib.hsr_srf_integrate_fit_u16 if u16 else lib.hsr_srf_integrate_fit)(*fitargs, C.byref(self.fit), None, st)]
        else:
            if mode == "step-apply":                                      # the _apply entries with job == NULL: the plain launch
                rcs = [(lib.hsr_srf_integrate_moments_u16_apply if u16 else lib.hsr_srf_integrate_moments_apply)(*fitargs, None, None, st)]
            else:
                rcs = [(lib.hsr_srf_integrate_moments_u16 if u16 else lib.hsr_srf_integrate_moments)(*fitargs, None, st)]
            assert self.slots.value == lib.hsr_partial_slots(npix, None)
            rcs.append(lib.hsr_moments_reduce_solve(self.work["partials"].ptr, self.slots.value, nb, K1_DEG, K1_MIN_COUNT, o["moments"][0].ptr,
                                                    o["coeffs"][0].ptr, st))
        return rcs + [lib.hsr_poly_apply(o["pseudo"][0].ptr, 1, nb, i["mask"].ptr, o["coeffs"][0].ptr, nb, K1_DEG, npix, None, 1,
                                         o["matched"][0].ptr, 1, nb, st)]


class K1Row(Row):
    """Pixel-major rows of 12 floats, degree 2.  Set 0 plain (a mask of ones); set 1: a random mask, a non-finite (uint16: nodata)
    sample in the cube, and band 1 with 19 valid pixels, one fewer than min_count - the identity fallback, fixture g9's rule; set 2: no
    pixel masked (the mask pointer is fixed at capture), every band fitted.  Bars, of tests/test_gpu_k1_instances.py: planes against
    oracle_np.pseudo_s2_srf_integral in float64 (uint16: of the decoded tile) at rel 2e-6, NaN placement exact (::_check_planes);
    moments over the kernel's own planes - count exact, sums rtol 1e-12 (::_check_moments); coefficients within 1e-7 of
    oracle_np.fit_per_band_poly relative to the band's largest (::_check_coeffs), the bits of the host twin of the solve, exactly the
    identity on the fallback band; matched rows bit-exact to oracle_np.apply_poly_planes with the device's coefficients."""
    chain, log = K1Chain, "srf"

    def __init__(self, name, covers, small, big, mode, u16, reuse):
        super().__init__(name, covers, small, big)
        self.mode, self.u16, self.reuse = mode, u16, reuse

    def make_inputs(self, s, k):
        from oracle import oracle_np as onp
        _, _, _, t = k1_table()
        npix = s.H * s.W
        rng = np.random.default_rng(31 * npix + k)
        R = (onp.synthetic_cube(s.H, s.W, seed=npix + k) * np.float32(0.6 + 0.2 * k)).astype(np.float32).reshape(npix, t.B)
        mask = np.ones(npix, np.uint8) if k != 1 else (rng.random(npix) < 0.7).astype(np.uint8)
        if k == 1:
            mask[:K1_MIN_COUNT] = 1
            R[npix // 3, 40] = np.nan
        cube = onp.tile_encode_u16(R) if self.u16 else R
        out = dict(cube=np.ascontiguousarray(cube))
        if self.mode != "k1":
            planes = self.planes(out["cube"])
            with np.errstate(invalid="ignore"):
                base = 0.9 * np.abs(np.nan_to_num(planes.T, nan=0.3)) ** 0.9 + 0.02           # test_gpu_k1_instances._targets
            real = (base + 0.01 * rng.standard_normal(base.shape)).astype(np.float32)
            real[npix // 5, 0] = np.nan
            if k == 1:
                real[K1_MIN_COUNT - 1:, 1] = -1.0                                             # not > min_y: 19 valid pixels are left
                real[npix // 3, 1] = -1.0
            out.update(real=real, mask=mask)
        return out

    def planes(self, cube):
        """The float64 oracle of the planes (nb, npix)."""
        from oracle import oracle_np as onp
        w, srf, good, _ = k1_table()
        R = onp.tile_decode_u16(cube, K1_SCALE, K1_NODATA) if self.u16 else cube
        ref = onp.pseudo_s2_srf_integral(R[None], w, srf, good)
        return np.stack([ref[b][0] for b in srf if ref[b] is not None]).astype(np.float64)

    def make_reference(self, s, k):
        i = self.inputs(s, k)
        ref = dict(planes=self.planes(i["cube"]))
        if self.mode != "k1":
            from oracle import oracle_np as onp
            with np.errstate(invalid="ignore"):
                ok = np.stack([onp.per_band_valid(ref["planes"][b], i["real"][:, b], i["mask"] != 0, 0.0) for b in range(ref["planes"].shape[0])])
            ref["fitted"] = ok.sum(axis=1) >= K1_MIN_COUNT
            ref["counts"] = ok.sum(axis=1)
        return ref

    def check(self, got, s, k, worst):
        from oracle import oracle_np as onp
        from s2_emit import _engine as eng
        from test_gpu_k1_instances import _check_coeffs, _check_moments, _check_planes, table_taps_global
        t = k1_table()[3]
        i, ref, npix, nb = self.inputs(s, k), self.reference(s, k), s.H * s.W, t.nb
        assert not table_taps_global(t.k0, t.klen, t.B)                   # the weights sit in LDS: the 2e-6 bar
        planes = got["pseudo"].reshape(npix, nb).T
        _check_planes(planes, ref["planes"], 2e-6, self.name)
        fin = np.isfinite(ref["planes"])
        scale = np.maximum(np.abs(ref["planes"]), 1e-3 * np.abs(np.where(fin, ref["planes"], 0)).max(axis=1, keepdims=True) + 1e-30)
        _note(worst, "k1 planes / rel 2e-6", np.max((np.abs(planes - ref["planes"]) / scale)[fin]) / 2e-6)
        if self.mode == "k1":
            return
        x, y, m = np.ascontiguousarray(planes, np.float32), np.ascontiguousarray(i["real"].T), i["mask"] != 0
        mom, co = got["moments"].reshape(nb, -1), got["coeffs"].reshape(nb, -1)
        _check_moments(mom, x, y, m, 0.0, K1_DEG, self.name)
        assert list(mom[:, 0] >= K1_MIN_COUNT) == list(ref["fitted"]) and (k != 1 or mom[1, 0] == K1_MIN_COUNT - 1), mom[:, 0]
        _check_coeffs(co, x, y, m, 0.0, K1_DEG, self.name, K1_MIN_COUNT, band1_empty=False)
        ident = np.zeros(K1_DEG + 1)
        ident[-2] = 1.0
        assert [np.array_equal(co[b], ident) for b in range(nb)] == [not f for f in ref["fitted"]], co
        host = eng.poly_solve_host(np.ascontiguousarray(mom), K1_DEG, K1_MIN_COUNT)
        assert np.array_equal(co.view(np.int64), host.view(np.int64)), "coefficients are not the host twin's bits"
        want = onp.apply_poly_planes(x, co, m, clip=True)
        matched = got["matched"].reshape(npix, nb).T
        np.testing.assert_array_equal(matched, want, err_msg="matched rows")
        f = np.isfinite(want)
        assert np.array_equal(matched[f].view(np.int32), np.ascontiguousarray(want, np.float32)[f].view(np.int32)), "matched rows: bits"


# =============================================================================================================================
# K4 fit: stats (partial -> finish) -> expand -> Gram (chunks -> reduce) -> assemble (clears the status) -> Cholesky -> finish
# =============================================================================================================================
RidgeShape = namedtuple("RidgeShape", "n")
RIDGE_IN, RIDGE_DEG, RIDGE_T, RIDGE_ALPHA = 4, 3, 5, 0.0       # alpha 0: a constant input (set 1) makes the first pivot exactly 0


@functools.lru_cache(maxsize=None)
def ridge_dims():
    from s2_emit.ridge import ridge_dims as dims
    return dims(RIDGE_IN, RIDGE_DEG, RIDGE_T)


class RidgeChain(Chain):
    in_place = ("Q",)                                   # the caller's [. | Y | 0] rows, whose first na columns hsr_polyfeat_expand_f64 fills

    def allocate(self, s):
        d, lib, t = ridge_dims(), self.lib, self.torch
        assert lib.hsr_polyfeat_prepare(RIDGE_IN, RIDGE_DEG) == 0, lib.hsr_last_error()      # not a launch-path call: here, not in launch
        self.ins = dict(X=Buf(t, s.n * RIDGE_IN * 4), Q=Buf(t, s.n * d.ldq * 8))
        f64, f32 = np.float64, np.float32
        sizes = dict(stats=(1 + 2 * RIDGE_IN, f64), mean=(RIDGE_IN, f64), scale=(RIDGE_IN, f64), G=(d.na * d.ldq, f64), A=(d.npad * d.npad, f64),
                     B=(d.npad * RIDGE_T, f64), info=(1, np.int32), b64=(RIDGE_T, f64), b32=(RIDGE_T, f32), W32=(d.kpad * RIDGE_T, f32),
                     mean32=(RIDGE_IN, f32), inv32=(RIDGE_IN, f32))
        self.outs = {k: (Buf(t, c * np.dtype(dt).itemsize), dt) for k, (c, dt) in sizes.items()}
        self.work = dict(stats_work=Buf(t, lib.hsr_ridge_stats_work_bytes(RIDGE_IN)), gram_work=Buf(t, lib.hsr_gram_work_bytes(d.na, d.ldq, s.n)),
                         chol_work=Buf(t, lib.hsr_chol_work_bytes(d.npad)))

    def used(self, name):
        return self.outs[name][0].nbytes                # no output depends on n

    def launch(self, st):
        d, lib, n, T = ridge_dims(), self.lib, self.shape.n, RIDGE_T
        o = {k: b.ptr for k, (b, _) in self.outs.items()}
        X, Q, w = self.ins["X"].ptr, self.ins["Q"].ptr, {k: b.ptr for k, b in self.work.items()}
        return [lib.hsr_ridge_stats(X, RIDGE_IN, 1, n, RIDGE_IN, w["stats_work"], o["stats"], o["mean"], o["scale"], st),
                lib.hsr_polyfeat_expand_f64(X, RIDGE_IN, 1, o["mean"], o["scale"], n, RIDGE_IN, RIDGE_DEG, Q, d.ldq, d.na, st),
                lib.hsr_gram_f64(Q, d.ldq, d.na, Q, d.ldq, d.ldq, n, w["gram_work"], o["G"], d.ldq, st),
                lib.hsr_ridge_assemble(o["G"], d.ldq, d.na, d.nf, T, RIDGE_ALPHA, o["A"], d.npad, o["B"], T, o["info"], st),
                lib.hsr_chol_solve_f64(o["A"], d.npad, d.npad, o["B"], T, T, w["chol_work"], o["info"], st),
                lib.hsr_ridge_finish(o["G"], d.na, d.nf, T, o["B"], T, o["mean"], o["scale"], RIDGE_IN, d.kpad, o["b64"], o["b32"], o["W32"],
                                     o["mean32"], o["inv32"], st)]

    def results(self):
        out = super().results()
        out["Q"] = self.ins["Q"].get(np.float64)[:self.shape.n * ridge_dims().ldq].copy()
        return out


class RidgeRow(Row):
    """4 inputs, degree 3 (34 monomials: a 64 x 64 system), 5 targets, alpha 0.  Sets 0 and 2: reflectance-like rows; set 1: one
    input vector on every row - every monomial of the centred data is 0, so the first pivot is exactly 0 and the status word is set
    (tests/test_gpu_k4_instances.py::test_single_fit_status); set 2 must read 0 again.  Bars, of tests/test_gpu_k4_instances.py,
    each stage against its reference from the device's own operands: mean and scale at rtol 1e-12 against long double
    (::test_stats_real_data); the monomial columns bit-equal to ((z_a z_b) z_c) (::test_expand); the Gram within 2 n 2^-53 |A|^T |B|
    of long double (::test_gram); the factor and the solution at LAPACK's two normwise ratios <= 1 against the system of
    ::_assemble_ref (::test_chol); the model read-out bit-equal to ::_finish_ref (::test_assemble_finish)."""
    chain, log = RidgeChain, ("hsr_k4_last_launch", True)

    def make_inputs(self, s, k):
        d = ridge_dims()
        rng = np.random.default_rng(13 * s.n + k)
        X = (600 + 4000 * rng.random((s.n, RIDGE_IN))).astype(np.float32)
        if k == 1:
            X[:] = X[0]
        Q = np.full((s.n, d.ldq), np.nan)               # the first na columns are the chain's to write
        Q[:, d.na:] = 0.0
        Q[:, d.na:d.na + RIDGE_T] = rng.standard_normal((s.n, RIDGE_T))
        return dict(X=X, Q=Q)

    def make_reference(self, s, k):
        xl = self.inputs(s, k)["X"].astype(LD)
        mu = xl.sum(axis=0) / s.n
        sc = np.sqrt(((xl - mu) ** 2).sum(axis=0) / s.n)
        sc[sc == 0] = 1
        return dict(mean=mu, scale=sc, info=1 if k == 1 else 0)

    def check(self, got, s, k, worst):
        from test_gpu_k4_instances import U53, _assemble_ref, _finish_ref, _monomials
        d, i, ref, T = ridge_dims(), self.inputs(s, k), self.reference(s, k), RIDGE_T
        mean, scale = got["mean"], got["scale"]
        np.testing.assert_allclose(mean, ref["mean"].astype(np.float64), rtol=1e-12, atol=0)
        np.testing.assert_allclose(scale, ref["scale"].astype(np.float64), rtol=1e-12, atol=0)
        _note(worst, "ridge stats mean (rtol 1e-12)", np.max(np.abs((mean - ref["mean"]) / ref["mean"])) / 1e-12)
        _note(worst, "ridge stats scale (rtol 1e-12)", np.max(np.abs((scale - ref["scale"]) / ref["scale"])) / 1e-12)
        assert got["stats"][0] == s.n and int(got["info"][0]) == ref["info"], (got["stats"][0], got["info"])
        Q = got["Q"].reshape(s.n, d.ldq)
        assert (Q[:, 0] == 1.0).all() and (Q[:, d.nf + 1:d.na].view(np.uint64) == 0).all()
        assert np.array_equal(Q[:, 1:d.nf + 1].view(np.uint64), _monomials(i["X"], mean, scale, RIDGE_IN, RIDGE_DEG).view(np.uint64)), "monomials"
        assert np.array_equal(Q[:, d.na:].view(np.uint64), i["Q"][:, d.na:].view(np.uint64)), "the targets were written to"
        G = got["G"].reshape(d.na, d.ldq)
        Ql = Q.astype(LD)
        err, bound = np.abs(G.astype(LD) - Ql[:, :d.na].T @ Ql), 2 * s.n * U53 * (np.abs(Q[:, :d.na]).T @ np.abs(Q))
        with np.errstate(invalid="ignore", divide="ignore"):
            _note(worst, "ridge gram (2 n 2^-53 |A|^T |B|)", np.max(np.where(err == 0, 0, err / bound)))
        assert (err <= bound).all()
        if ref["info"]:
            return
        A_ref, B_ref = _assemble_ref(G, d.na, d.nf, T, RIDGE_ALPHA, d.npad)
        L, W = np.tril(got["A"].reshape(d.npad, d.npad)).astype(LD), got["B"].reshape(d.npad, T)
        anorm = np.abs(A_ref).sum(axis=1).max()
        r1 = np.abs(L @ L.T - A_ref.astype(LD)).sum(axis=1).max() / (d.npad * anorm * U52)
        r2 = np.abs(A_ref.astype(LD) @ W.astype(LD) - B_ref.astype(LD)).sum(axis=0).max() / (d.npad * anorm * np.abs(W).sum(axis=0).max() * U52)
        _note(worst, "ridge chol factor ratio (<= 1)", r1)
        _note(worst, "ridge chol solve ratio (<= 1)", r2)
        assert r1 <= 1 and r2 <= 1, (float(r1), float(r2))
        want = _finish_ref(G, d.na, d.nf, T, W[:d.nf], mean, scale, d.kpad)
        for name, w in zip(("b64", "b32", "W32", "mean32", "inv32"), want):
            a, b = got[name].reshape(-1), np.ascontiguousarray(w).reshape(-1)
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), name


# =============================================================================================================================
# pairs, hold-out and score: the group codes are made on the device, the score is a partial -> finish pair over pixel chunks
# =============================================================================================================================
ScoreShape = namedtuple("ScoreShape", "T npix")
SCORE_P, SCORE_FACTOR = 2, 6


class ScoreChain(Chain):
    def allocate(self, s):
        t, P, T = self.torch, SCORE_P, s.T
        self.ins = dict(pred=Buf(t, P * T * s.npix * 4), y=Buf(t, P * T * s.npix * 4), valid=Buf(t, P * s.npix, 3), train=Buf(t, P * s.npix, 1))
        f64, i64 = np.float64, np.int64
        self.outs = dict(mask=(Buf(t, P * s.npix, 1), np.uint8), group=(Buf(t, P * s.npix), np.uint8), sam_map=(Buf(t, P * s.npix * 4), np.float32))
        self.outs.update({k: (Buf(t, P * 2 * T * 8, 8), dt) for k, dt in (("n", i64), ("rmse", f64), ("r2", f64), ("mean_ref", f64))})
        self.outs.update({k: (Buf(t, P * 2 * 8, 8), dt) for k, dt in (("sam", f64), ("n_sam", i64), ("ergas", f64))})
        self.work = dict(work=Buf(t, P * self.lib.hsr_pair_score_work_bytes(s.npix, T)))

    def used(self, name):
        s = self.shape
        if name in ("mask", "group", "sam_map"):
            return SCORE_P * s.npix * (4 if name == "sam_map" else 1)
        return self.outs[name][0].nbytes

    def launch(self, st):
        s, lib, i = self.shape, self.lib, self.ins
        o = {k: b.ptr for k, (b, _) in self.outs.items()}
        pair_work = lib.hsr_pair_score_work_bytes(s.npix, s.T) // 8
        return [lib.hsr_pair_holdout(i["valid"].ptr, i["train"].ptr, s.npix, s.npix, o["mask"], o["group"], SCORE_P, st),
                lib.hsr_pair_score_f64(i["pred"].ptr, s.T * s.npix, i["y"].ptr, s.T * s.npix, o["group"], s.npix, s.npix, s.T,
                                       100.0 / SCORE_FACTOR, self.work["work"].ptr, pair_work, o["n"], o["rmse"], o["r2"], o["mean_ref"],
                                       2 * s.T, o["sam"], o["n_sam"], o["ergas"], 2, o["sam_map"], s.npix, SCORE_P, st)]


class ScoreRow(Row):
    """Two pairs on the dyadic data of pair_cases.score_inputs, the group codes made by hsr_pair_holdout from a valid mask and a
    training mask that change with the set; in set 1 pair 1 has no training pixel (group 1 empty: n = 0, NaN statistics), in set 2
    pair 0 has no hold-out pixel.  Bars, of tests/test_gpu_pair_instances.py: mask and group codes exact (::test_holdout); n and
    n_sam exact, rmse / mean_ref / ergas at rtol 1e-12, r2 at rtol 1e-12 + atol 1e-6, sam at ANGLE_ATOL, sam_map at ANGLE_ATOL + 1 ulp
    of float32, NaN in the same places (::_check_score), against validation_reference of tests/test_tile_pairs_validate_host.py."""
    chain, log = ScoreChain, ("hsr_pairs_last_launch", True)

    def make_inputs(self, s, k):
        import pair_cases as pc
        pred, y, _ = pc.score_inputs(s.T, s.npix, ("mix", "ones", "twos"))
        rng = np.random.default_rng(s.npix + k)
        valid = rng.choice(np.array([0, 1, 1, 7], np.uint8), (SCORE_P, s.npix))
        train = rng.choice(np.array([0, 100, 200, 255], np.uint8), (SCORE_P, s.npix))
        if k == 1:
            train[1] = 0
        if k == 2:
            train[0] = 255
        roll = lambda a: np.ascontiguousarray(np.roll(a[:SCORE_P], 17 * k, axis=-1))
        return dict(pred=roll(pred), y=roll(y), valid=valid, train=train)

    def make_reference(self, s, k):
        import pair_cases as pc
        i = self.inputs(s, k)
        mask, group = pc.holdout_reference(i["valid"], i["train"])
        return dict(mask=mask, group=group, score=[pc.score_reference(i["pred"][p], i["y"][p], group[p], SCORE_FACTOR) for p in range(SCORE_P)])

    def check(self, got, s, k, worst):
        from test_gpu_pair_instances import ANGLE_ATOL
        ref, P, T = self.reference(s, k), SCORE_P, s.T
        np.testing.assert_array_equal(got["mask"].reshape(P, s.npix), ref["mask"])
        np.testing.assert_array_equal(got["group"].reshape(P, s.npix), ref["group"])
        g = {name: got[name].reshape(P, 2, T) for name in ("n", "rmse", "r2", "mean_ref")}
        g.update({name: got[name].reshape(P, 2) for name in ("sam", "n_sam", "ergas")})
        for p, r in enumerate(ref["score"]):
            np.testing.assert_array_equal(g["n"][p], r["n"])
            np.testing.assert_array_equal(g["n_sam"][p], r["n_sam"])
            for name in ("rmse", "mean_ref", "ergas"):
                _close(worst, "score rmse / mean_ref / ergas rtol 1e-12", g[name][p], r[name], 1e-12)
            _close(worst, "score r2 rtol 1e-12 atol 1e-6", g["r2"][p], r["r2"], 1e-12, 1e-6)
            const = r["m2"] == 0
            _close(worst, "score r2 (M2 == 0) rtol 1e-12", g["r2"][p][const], (1.0 - r["ss_res"] / 1e-8)[const], 1e-12)
            _close(worst, "score sam atol 5e-6 deg", g["sam"][p], r["sam"], 0.0, ANGLE_ATOL)
            m, ok = got["sam_map"].reshape(P, s.npix)[p], ~np.isnan(r["angle"])
            np.testing.assert_array_equal(np.isnan(m), ~ok)
            err = np.abs(m.astype(np.float64) - r["angle"])[ok]
            tol = (ANGLE_ATOL + np.spacing(np.abs(r["angle"].astype(np.float32))).astype(np.float64))[ok]
            if ok.any():
                _note(worst, "score sam_map atol 5e-6 deg + 1 ulp", (err / tol).max())
                assert (err <= tol).all(), (p, float(err.max()))


def _close(worst, key, got, ref, rtol, atol=0.0):
    """NaN in the same places, elsewhere |got - ref| <= atol + rtol |ref| (as test_gpu_pair_instances._close)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (key, got.shape, ref.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=f"{key}: NaN positions")
    ok = ~np.isnan(ref)
    if ok.any():
        err, bound = np.abs(got - ref)[ok], (atol + rtol * np.abs(ref))[ok]
        _note(worst, key, np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)).max())
        assert (err <= bound).all(), (key, float(err.max()))


# =============================================================================================================================
# the batch: T ragged tiles in one launch per stage, per-tile partial slots in one workspace
# =============================================================================================================================
BatchShape = namedtuple("BatchShape", "npix")           # the tiles' pixel counts


class BatchChain(Chain):
    def allocate(self, s):
        from s2_emit import _native as nat
        t, tb = self.torch, k1_table()[3]
        self.nb, self.B, total, T, M = tb.nb, tb.B, sum(s.npix), len(s.npix), 3 * K1_DEG + 2
        self.k0, self.klen = (C.c_int32 * tb.nb)(*tb.k0.tolist()), (C.c_int32 * tb.nb)(*tb.klen.tolist())
        self.wn = Buf(t, tb.nb * tb.B * 4, 0, tb.weights.astype(np.float32))
        self.ins = dict(cube=Buf(t, total * tb.B * 4), real=Buf(t, total * tb.nb * 4), mask=Buf(t, total))
        self.outs = dict(pseudo=(Buf(t, total * tb.nb * 4), np.float32), matched=(Buf(t, total * tb.nb * 4), np.float32),
                         moments=(Buf(t, T * tb.nb * M * 8), np.float64), coeffs=(Buf(t, T * tb.nb * (K1_DEG + 1) * 8), np.float64))
        self.nunits = sum(self.lib.hsr_partial_slots(n, None) for n in s.npix)
        self.work = dict(partials=Buf(t, self.lib.hsr_batch_partials_bytes(self.nunits, tb.nb, K1_DEG)))
        self.tables = dict(tiles=Buf(t, T * nat.BATCH_RECORD_BYTES), units=Buf(t, self.nunits * nat.BATCH_RECORD_BYTES))

    def buffers(self):
        return super().buffers() + [self.wn] + list(self.tables.values())

    def set_shape(self, s):
        """hsr_batch_plan: host work, done when the chain is bound to a shape - never in launch."""
        from s2_emit import _native as nat
        assert len(s.npix) == len(self.alloc.npix) and sum(s.npix) <= sum(self.alloc.npix)
        self.shape, T, nb = s, len(s.npix), self.nb
        tiles, at = (nat.BatchTile * T)(), 0
        base = {k: b.ptr.value for k, b in self.ins.items()}
        out = {k: b.ptr.value for k, (b, _) in self.outs.items()}
        for i, n in enumerate(s.npix):
            tl = tiles[i]
            tl.cube_dev, tl.real_dev, tl.mask_dev = base["cube"] + at * self.B * 4, base["real"] + at * nb * 4, base["mask"] + at
            tl.pseudo_dev, tl.matched_dev, tl.npix = out["pseudo"] + at * nb * 4, out["matched"] + at * nb * 4, n
            at += n
        self.info = nat.BatchInfo()
        assert self.lib.hsr_batch_plan(tiles, T, nb, K1_DEG, None, None, None, 0, C.byref(self.info)) == 0, self.lib.hsr_last_error()
        nunits = int(self.info.nunits)
        assert nunits <= self.nunits
        units = (C.c_uint8 * (nat.BATCH_RECORD_BYTES * nunits))()
        assert self.lib.hsr_batch_plan(tiles, T, nb, K1_DEG, self.work["partials"].ptr, None, units, nunits, C.byref(self.info)) == 0
        self.tables["tiles"].put(np.frombuffer(bytes(tiles), np.uint8))
        self.tables["units"].put(np.frombuffer(bytes(units), np.uint8))

    def used(self, name):
        total, T, nb = sum(self.shape.npix), len(self.shape.npix), self.nb
        return dict(pseudo=total * nb * 4, matched=total * nb * 4, moments=T * nb * (3 * K1_DEG + 2) * 8, coeffs=T * nb * (K1_DEG + 1) * 8)[name]

    def launch(self, st):
        lib, T, nb, o = self.lib, len(self.shape.npix), self.nb, self.outs
        tiles, units = self.tables["tiles"].ptr, self.tables["units"].ptr
        return [lib.hsr_srf_integrate_moments_batched(units, C.byref(self.info), 0, K1_SCALE, K1_NODATA, self.B, self.wn.ptr, self.k0, self.klen, nb,
                                                      nb, nb, 0.0, 0.0, K1_DEG, None, st),
                lib.hsr_moments_reduce_solve_batched(tiles, T, self.work["partials"].ptr, nb, K1_DEG, K1_MIN_COUNT, o["moments"][0].ptr,
                                                     o["coeffs"][0].ptr, st),
                lib.hsr_poly_apply_batched(tiles, T, int(self.info.max_npix), o["coeffs"][0].ptr, nb, K1_DEG, nb, 1, 1, st)]


class BatchRow(Row):
    """Three ragged tiles; tile t of set k holds set (k + t) % 3 of the single-tile operator step (K1Row), so every set has one tile
    with the fallback band, a mask and a non-finite sample, at another place of the batch.  Bars: those of K1Row, tile by tile
    (tests/test_gpu_k1_instances.py: 'a batch: each tile's rows and moments equal the references of that tile alone')."""
    chain, log = BatchChain, "srf"

    def __init__(self, name, covers, small, big):
        super().__init__(name, covers, small, big)
        self.tile = K1Row(name + "-tile", (), None, None, "step", False, False)

    def parts(self, s, k):
        return [(K1Shape(1, n), (k + t) % 3) for t, n in enumerate(s.npix)]

    def make_inputs(self, s, k):
        tiles = [self.tile.inputs(ts, tk) for ts, tk in self.parts(s, k)]
        return {key: np.concatenate([t[key] for t in tiles]) for key in ("cube", "real", "mask")}

    def make_reference(self, s, k):
        return [self.tile.reference(ts, tk) for ts, tk in self.parts(s, k)]

    def check(self, got, s, k, worst):
        nb, T, at = k1_table()[3].nb, len(s.npix), 0
        mom, co = got["moments"].reshape(T, -1), got["coeffs"].reshape(T, -1)
        for t, (ts, tk) in enumerate(self.parts(s, k)):
            n = ts.W
            one = dict(pseudo=got["pseudo"][at * nb:(at + n) * nb], matched=got["matched"][at * nb:(at + n) * nb], moments=mom[t], coeffs=co[t])
            self.tile.check(one, ts, tk, worst)
            at += n


# =============================================================================================================================
# the operators around K1 - K3: codec, ENVI transposer, resamplers, validity mask; the upsampling producer owns a histogram
# =============================================================================================================================
AuxShape = namedtuple("AuxShape", "nb Hc Wc f")         # coarse planes (nb, Hc, Wc) and a factor; codec / transposer: the element count
AUX_SCALE, AUX_PAIR = 0.37, (2.0, 98.0)


class AuxChain(Chain):
    def sizes(self, s):
        """(input name -> bytes, output name -> (bytes, dtype)) of the row's operator at shape s."""
        npc, npf, n = s.Hc * s.Wc, s.Hc * s.Wc * s.f * s.f, s.nb * s.Hc * s.Wc
        return {"codec": (dict(x=n * 4), dict(u16=(n * 2, np.uint16), dec=(n * 4, np.float32))),
                "interleave": (dict(x=n * 4), dict(out=(n * 4, np.float32))),
                "block-mean": (dict(x=s.nb * npf * 4), dict(out=(s.nb * npc * 4, np.float32))),
                "upsample": (dict(x=n * 4), dict(out=(s.nb * npf * 4, np.float32))),
                "upsample-hist": (dict(x=n * 4), dict(out=(npf * 16, np.float32), mask=(npf, np.uint8), lohi=(s.nb * 16, np.float64))),
                "valid-mask": (dict(x=n * 4, y=n * 4, mask_in=npc), dict(mask=(npc, np.uint8)))}[self.row.op]

    def allocate(self, s):
        ins, outs = self.sizes(s)
        self.ins = {k: Buf(self.torch, b) for k, b in ins.items()}
        self.outs = {k: (Buf(self.torch, b), dt) for k, (b, dt) in outs.items()}
        if self.row.op == "upsample-hist":
            self.work = dict(work=Buf(self.torch, self.lib.hsr_percentile_work_bytes(s.nb)))

    def used(self, name):
        return self.sizes(self.shape)[1][name][0]

    def launch(self, st):
        s, lib, op = self.shape, self.lib, self.row.op
        i, o = {k: b.ptr for k, b in self.ins.items()}, {k: b.ptr for k, (b, _) in self.outs.items()}
        npc, npf, n = s.Hc * s.Wc, s.Hc * s.Wc * s.f * s.f, s.nb * s.Hc * s.Wc
        if op == "codec":
            return [lib.hsr_tile_encode_u16(i["x"], n, 1e4, 1, -9999.0, 65535, o["u16"], st), lib.hsr_tile_decode_u16(o["u16"], n, 1e-4, 65535, o["dec"], st)]
        if op == "interleave":                                            # BIL (lines, bands, samples) float32 -> (lines, samples, bands)
            return [lib.hsr_interleave_to_bip(i["x"], 0, 1, s.Hc, s.Wc, s.nb, o["out"], 0, st)]
        if op == "block-mean":
            return [lib.hsr_block_mean(i["x"], 0, npf, 1, s.nb, s.Hc, s.Wc, s.f, AUX_SCALE, o["out"], npc, 1, st)]
        if op == "upsample":
            return [lib.hsr_bilinear_upsample(i["x"], npc, 1, s.nb, s.Hc, s.Wc, s.f, o["out"], npf, 1, st)]
        if op == "valid-mask":
            return [lib.hsr_valid_mask(i["x"], npc, 1, s.nb, 0, i["y"], npc, 1, s.nb, i["mask_in"], npc, o["mask"], st)]
        w = self.work["work"].ptr                                         # the producer and the select's scans and passes 2, 3 on its output
        rcs = [lib.hsr_percentile_begin(w, s.nb, st), lib.hsr_bilinear_upsample_mask_hist(i["x"], npc, 1, s.nb, s.Hc, s.Wc, s.f, o["out"], o["mask"], w, st),
               lib.hsr_percentile_scan(1, s.nb, AUX_PAIR[0], AUX_PAIR[1], w, o["lohi"], st)]
        for p in (2, 3):
            rcs += [lib.hsr_percentile_hist(p, o["out"], 1, 4, o["mask"], npf, s.nb, w, st),
                    lib.hsr_percentile_scan(p, s.nb, AUX_PAIR[0], AUX_PAIR[1], w, o["lohi"], st)]
        return rcs


class AuxRow(Row):
    """One operator a row, band-major planes.  Set 1 carries the non-finite samples (codec: also the source nodata value; producer: a
    band of NaN only, so that no pixel is valid and the limits are NaN), set 2 none.  Bars, of tests/test_gpu_aux_instances.py, all
    bit equality: oracle_np.tile_encode_u16 / tile_decode_u16 (::test_tile_encode_rows, ::test_tile_decode_rows), the transposition
    (::test_interleave_to_bip_rows), the ordered float64 sum ::_bm_ref_f32 (::test_block_mean_rows), oracle_np.bilinear_upsample
    (::test_bilinear_rows), and for the producer its rows of 4 with a zero pad, the mask of pixels finite in every band and
    np.percentile of them (::test_bilinear_producer_rows); the validity mask against the rule of include/hsr.h
    (tests/test_gpu_poly_instances.py)."""
    chain, log = AuxChain, ("hsr_aux_last_launch", False)

    def __init__(self, name, covers, small, big, op):
        super().__init__(name, covers, small, big)
        self.op, self.reuse = op, op == "upsample-hist"
        if op == "valid-mask":
            self.log = ("hsr_poly_last_launch", False)

    def make_inputs(self, s, k):
        rng = np.random.default_rng(1000 * s.Hc + 10 * s.Wc + s.f + k)
        npc, npf, n = s.Hc * s.Wc, s.Hc * s.Wc * s.f * s.f, s.nb * s.Hc * s.Wc
        special = np.array([np.nan, np.inf, -np.inf], np.float32)
        if self.op == "codec":
            x = rng.uniform(-0.1, 7.0, n).astype(np.float32)
            if k == 1:
                x[::13] = np.array([np.nan, -9999.0, np.inf, -np.inf, -0.0, 6.5535, 3e9], np.float32)[np.arange(len(x[::13])) % 7]
            return dict(x=x)
        if self.op == "block-mean":
            x = (rng.standard_normal((s.nb, s.Hc * s.f, s.Wc * s.f)) * 10.0 ** rng.integers(-6, 6, (s.nb, s.Hc * s.f, s.Wc * s.f))).astype(np.float32)
        else:
            x = rng.uniform(-0.3, 1.3, (s.nb, s.Hc, s.Wc)).astype(np.float32)
        if k < 2:
            flat = x.reshape(-1)
            flat[(7 + 3 * k)::(41 + 10 * k)] = special[np.arange(len(flat[(7 + 3 * k)::(41 + 10 * k)])) % 3]
        if k == 1 and self.op == "upsample-hist":
            x[1] = np.nan
        if self.op == "interleave":
            x = np.ascontiguousarray(x.reshape(s.nb, s.Hc, s.Wc).transpose(1, 0, 2))                  # (lines, bands, samples)
        out = dict(x=x)
        if self.op == "valid-mask":
            y = rng.uniform(0, 1, (s.nb, s.Hc, s.Wc)).astype(np.float32)
            y.reshape(-1)[5::(53 - 10 * k)] = np.nan
            x[0].reshape(-1)[3::17] = -0.25                                                            # band 0 must be > 0
            out.update(y=y, mask_in=(rng.random(npc) < (0.5, 0.9, 1.1)[k]).astype(np.uint8))
        return out

    def make_reference(self, s, k):
        from oracle import oracle_np as onp
        i = self.inputs(s, k)
        x = i["x"]
        if self.op == "codec":
            enc = onp.tile_encode_u16(x, -9999.0, 1e4, 65535)
            return dict(u16=enc, dec=onp.tile_decode_u16(enc, None, 65535))
        if self.op == "interleave":
            return dict(out=np.ascontiguousarray(x.transpose(0, 2, 1)))
        if self.op == "block-mean":
            from test_gpu_aux_instances import _bm_ref_f32
            with np.errstate(invalid="ignore"):
                return dict(out=_bm_ref_f32(x, s.f, AUX_SCALE))
        if self.op == "valid-mask":
            with np.errstate(invalid="ignore"):
                ok = np.isfinite(x).all(axis=0) & (x[0] > 0) & np.isfinite(i["y"]).all(axis=0)
            return dict(mask=(ok.reshape(-1) & (i["mask_in"] != 0)).astype(np.uint8))
        with np.errstate(invalid="ignore"):
            up = onp.bilinear_upsample(x, s.f).reshape(s.nb, -1)
        if self.op == "upsample":
            return dict(out=up)
        import warnings
        mask = np.isfinite(up).all(axis=0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            lohi = np.array([np.percentile(up[c][mask], list(AUX_PAIR)) if mask.any() else [np.nan, np.nan] for c in range(s.nb)])
        return dict(up=up, mask=mask.astype(np.uint8), lohi=lohi)

    def check(self, got, s, k, worst):
        from gpu_harness import bits_equal
        ref = self.reference(s, k)
        if self.op == "upsample-hist":
            rows = got["out"].reshape(-1, 4)
            bits_equal(np.ascontiguousarray(rows[:, :s.nb].T), ref["up"], "producer output")
            assert (rows[:, s.nb:].view(np.uint32) == 0).all(), "pad columns"
            np.testing.assert_array_equal(got["mask"], ref["mask"])
            np.testing.assert_array_equal(got["lohi"].reshape(s.nb, 2), ref["lohi"])
            return
        for name, want in ref.items():
            if want.dtype == np.float32:
                bits_equal(got[name].reshape(want.shape), want, f"{self.name}: {name}")
            else:
                np.testing.assert_array_equal(got[name].reshape(want.shape), want)


# =============================================================================================================================
# scene tiles: gather by a device-resident origin table, then the mosaic (slot table) or the feathered mosaic (start table)
# =============================================================================================================================
TileShape = namedtuple("TileShape", "bands H W th tw sy sx")          # sy, sx: the lattice pitch of the feathered mosaic (else th, tw)
TILE_ENCODE = sc.ENC_ND                                 # (scale, has source nodata, source nodata, nodata code)


def tile_grid(s):
    return (s.H - s.th) // s.sy + 1, (s.W - s.tw) // s.sx + 1


class TileChain(Chain):
    def allocate(self, s):
        ny, nx = tile_grid(s)
        P, t, mode = ny * nx, self.torch, self.row.mode
        self.ins = dict(scene=Buf(t, s.bands * s.H * s.W * 4), origins=Buf(t, P * 8))
        self.outs = dict(tiles=(Buf(t, P * s.bands * s.th * s.tw * (2 if mode == "encode" else 4)), np.uint16 if mode == "encode" else np.uint32))
        if mode != "encode":
            self.ins["table"] = Buf(t, P * 4)
            self.outs["image"] = (Buf(t, s.bands * s.H * s.W * 4), np.uint32)

    def used(self, name):
        s = self.shape
        ny, nx = tile_grid(s)
        return ny * nx * s.bands * s.th * s.tw * (2 if self.row.mode == "encode" else 4) if name == "tiles" else s.bands * s.H * s.W * 4

    def launch(self, st):
        s, lib, mode = self.shape, self.lib, self.row.mode
        ny, nx = tile_grid(s)
        P, tiles = ny * nx, self.outs["tiles"][0].ptr
        enc = TILE_ENCODE if mode == "encode" else (1.0, 0, 0.0, 65535)
        rcs = [lib.hsr_scene_gather_tiles(self.ins["scene"].ptr, 0, s.bands, s.H, s.W, self.ins["origins"].ptr, P, s.th, s.tw,
                                          int(mode == "encode"), *enc, tiles, st)]
        if mode == "mosaic":
            rcs.append(lib.hsr_scene_mosaic(tiles, P, s.bands, s.th, s.tw, self.outs["image"][0].ptr, s.H, s.W, self.ins["table"].ptr, ny, nx,
                                            float("nan"), 1, st))
        if mode == "blend":
            rcs.append(lib.hsr_scene_mosaic_blend(tiles, P, s.bands, s.th, s.tw, s.sy, s.sx, self.ins["table"].ptr, ny, nx,
                                                  self.outs["image"][0].ptr, s.H, s.W, float("nan"), st))
        return rcs


class TileRow(Row):
    """The windows of a regular grid (feathered: of a lattice of half-tile pitch) cut out of a scene in an order that changes with the
    set, and put back by the table that names them.  Set 1: one origin outside the scene (its slice keeps what it held) and table
    entries -1 (fill), -2 / an index past the stack (left alone); set 2: every window present.  Bars, of
    tests/test_gpu_scene_instances.py: tiles bit-equal to scene_cases.gather_ref (encoded: oracle_np.tile_encode_u16), the mosaic
    bit-equal to scene_cases.assemble (::test_gather_rows, ::test_mosaic_rows); the feathered mosaic under check_blend of
    tests/test_scene_blend_host.py - (K + 2) 2^-24 sum w |v| / sum w, copied bits where one value contributes (::test_blend_rows)."""
    chain, log, reuse = TileChain, ("hsr_scene_last_launch", False), False

    def __init__(self, name, covers, small, big, mode):
        super().__init__(name, covers, small, big)
        self.mode = mode

    def make_inputs(self, s, k):
        ny, nx = tile_grid(s)
        P = ny * nx
        rng = np.random.default_rng(100 * s.H + s.W + k)
        scene = np.roll(sc.gather_scene(np.float32, (s.bands, s.H, s.W)), 5 * k, axis=2).copy()
        if self.mode == "blend":                        # finite values and NaN only, as test_gpu_scene_blend.make_case
            scene = (rng.random((s.bands, s.H, s.W), dtype=np.float32) * 0.98 + 0.01).astype(np.float32)
            scene[rng.random(scene.shape) < 0.03] = np.nan
        order = rng.permutation(P)                      # cube order[c] holds the window of cell c
        cells = np.array([(j * s.sy, i * s.sx) for j in range(ny) for i in range(nx)], np.int32)
        origins = np.zeros((P, 2), np.int32)
        origins[order] = cells
        table = order.astype(np.int32).copy()
        if k == 1:
            origins[order[2]] = (s.H - s.th + 1, 0)     # leaves the scene: not gathered, and not placed
            table[2] = -1
            table[P // 2] = -2 if self.mode == "mosaic" else -1
            table[P - 2] = P + 3                        # past the stack
        elif k == 0:
            table[1] = -1
        out = dict(scene=scene, origins=origins)
        if self.mode != "encode":
            out["table"] = table.reshape(ny, nx)
        return out

    def make_reference(self, s, k):
        i = self.inputs(s, k)
        tiles, inside = sc.gather_ref(i["scene"], i["origins"], s.th, s.tw, TILE_ENCODE if self.mode == "encode" else None)
        ref = dict(tiles=tiles, inside=inside)
        if self.mode == "mosaic":
            pre = np.frombuffer(bytes([FILL]) * (s.bands * s.H * s.W * 4), np.float32).reshape(s.bands, s.H, s.W)
            ref["image"] = sc.assemble(tiles, i["table"], pre, s.th, s.tw, np.float32(np.nan), True)
        if self.mode == "blend":
            from test_scene_blend_host import blend_ref64
            ref["blend"] = blend_ref64(tiles, i["table"], s.sy, s.sx, s.H, s.W)
        return ref

    def check(self, got, s, k, worst):
        ref = self.reference(s, k)
        want = ref["tiles"]
        tiles = got["tiles"].reshape(want.shape)
        wbits = want if want.dtype == np.uint16 else np.ascontiguousarray(want).view(np.uint32)
        np.testing.assert_array_equal(tiles[ref["inside"]], wbits[ref["inside"]])
        assert (tiles[~ref["inside"]].view(np.uint8) == FILL).all(), "a window outside the scene was written"
        if self.mode == "mosaic":
            np.testing.assert_array_equal(got["image"].reshape(s.bands, s.H, s.W), np.ascontiguousarray(ref["image"]).view(np.uint32))
        if self.mode == "blend":
            from test_scene_blend_host import check_blend
            K = (s.th // s.sy) * (s.tw // s.sx)
            _note(worst, "scene blend ((K + 2) 2^-24 sum w |v| / sum w)",
                  check_blend(got["image"].view(np.float32).reshape(s.bands, s.H, s.W), ref["blend"], K, np.float32(np.nan)))


# =============================================================================================================================
# rows whose chain is a few calls on buffers of fixed roles: the row gives the layout and the calls, one chain class serves them
# =============================================================================================================================
class GenericChain(Chain):
    """row.layout(shape) -> (ins name -> bytes, outs name -> (bytes, dtype), work name -> bytes); row.calls(lib, shape, p, st) issues
    the chain with p = name -> device address (int); row.prepare(lib) does the host work that is no launch-path call."""

    def allocate(self, s):
        ins, outs, work = self.row.layout(s)
        self.ins = {k: Buf(self.torch, b) for k, b in ins.items()}
        self.outs = {k: (Buf(self.torch, b, self.row.out_off), dt) for k, (b, dt) in outs.items()}
        self.work = {k: Buf(self.torch, b) for k, b in work.items()}
        self.row.prepare(self.lib)

    def used(self, name):
        return self.row.layout(self.shape)[1][name][0]

    def launch(self, st):
        p = {k: b.ptr.value for k, b in self.ins.items()}
        p.update({k: b.ptr.value for k, (b, _) in self.outs.items()})
        p.update({k: b.ptr.value for k, b in self.work.items()})
        return self.row.calls(self.lib, self.shape, p, st)


class GenericRow(Row):
    chain, out_off = GenericChain, 8                     # outputs 8 bytes past a 256-byte boundary unless the row's entries need more

    def prepare(self, lib):
        pass


# ---- hsr_pair_report_f64: partial sums per chunk of 256 pixels, then the finish -----------------------------------------------
RepShape = namedtuple("RepShape", "na nf T npix")
REPORT_FLAGS = ((), ("status", "empty"), ("clip",))     # pair_cases.ReportRow.flags of set 0, 1, 2


class PairReportRow(GenericRow):
    """Three pairs on the exact-integer data of pair_cases.report_inputs.  Set 1: pair 1 carries status 2 and pair 2 has an all-zero
    mask and status 1 - NaN statistics; set 2: intercepts of +-80, which the sigmoid's clip decides; sets 0 and 2 report every pair.
    Bars, of tests/test_gpu_pair_instances.py::test_report: r2 at rtol 1e-12 + atol 1e-6, rmse at rtol 1e-6, NaN under a non-zero
    status, against report_reference of tests/test_tile_pairs_report_host.py."""
    log = ("hsr_pairs_last_launch", True)

    def pcrow(self, s, k):
        import pair_cases as pc
        return pc.ReportRow(s.na, s.nf, s.T, s.npix, False, REPORT_FLAGS[k])

    def layout(self, s):
        import pair_cases as pc
        st, P = self.pcrow(s, 0).strides(), pc.P
        ins = dict(Q=P * st["pair_q"] * 8, b64=P * st["pair_b"] * 8, Bp=P * st["pair_bp"] * 8, y=P * st["pair_y"] * 4, mask=P * st["pair_m"],
                   status=P * 4)
        outs = dict(r2=(P * s.T * 8, np.float64), rmse=(P * s.T * 8, np.float64))
        return ins, outs, dict(work=P * _lib().hsr_pair_report_work_bytes(s.npix, s.T))

    def calls(self, lib, s, p, st):
        import pair_cases as pc
        r = self.pcrow(s, 0)
        d = r.strides()
        return [lib.hsr_pair_report_f64(p["Q"], d["ldq"], d["pair_q"], s.na, s.npix, p["b64"], d["pair_b"], p["Bp"], d["ldbp"], d["pair_bp"], s.nf,
                                        p["y"], d["pair_y"], p["mask"], d["pair_m"], s.T, p["status"], p["work"],
                                        lib.hsr_pair_report_work_bytes(s.npix, s.T) // 8, p["r2"], p["rmse"], s.T, pc.P, st)]

    def make_inputs(self, s, k):
        import pair_cases as pc
        return {key: np.array(v) for key, v in pc.report_inputs(self.pcrow(s, k)).items()}

    def make_reference(self, s, k):
        import pair_cases as pc
        r = self.pcrow(s, k)
        return [pc.report_expected(r, pc.report_inputs(r), p) for p in range(pc.P)]

    def check(self, got, s, k, worst):
        for p, (r2, rmse) in enumerate(self.reference(s, k)):
            _close(worst, "report r2 rtol 1e-12 atol 1e-6", got["r2"].reshape(-1, s.T)[p], r2, 1e-12, 1e-6)
            _close(worst, "report rmse rtol 1e-6", got["rmse"].reshape(-1, s.T)[p], rmse, 1e-6)


# ---- pooling: hsr_pool_stats -> hsr_pool_gram -> hsr_pool_models over device-resident order / start / group tables ------------
PoolShape = namedtuple("PoolShape", "nb n_elems")
POOL_PERMS = ((0, 1, 2, 3, 4), (4, 2, 0, 3, 1), (1, 0, 4, 2, 3))      # the pairs of hsr_pool_models, reordered with the set


class PoolRow(GenericRow):
    """The 33 pairs and 7 groups of pair_cases (group sizes 1 .. 9, empty members, an all-empty group).  What changes with the set is
    the CONTENT of the tables the kernels walk: set 0 the layout of pair_cases.pool_ids; set 1 the same with order entries outside
    [0, P) (skipped; the pairs they named keep the sentinel); set 2 every group under the next id; the pairs of hsr_pool_models are
    reordered with the set.  Bars, of tests/test_gpu_pair_instances.py: group statistics at rtol 1e-12 against long double, every
    member's row the bits of its group's (::_check_pool_stats); the pooled Gram exact on integers (::test_pool_gram); the model
    copies bit-exact, zero rows nf .. npad, both status words, the sentinel for a pair outside [0, M) (::test_pool_models)."""
    log = ("hsr_pairs_last_launch", True)

    def tables(self, k):
        """-> order, start, the members every group walks, the pairs no group reaches."""
        import pair_cases as pc
        if k == 1:
            return pc.pool_skip_layout(pc.POOL_SKIPS[0][1])
        ids = tuple(int(g + (k == 2)) % pc.POOL_M for g in pc.pool_ids())
        return pc.pool_layout(ids) + (pc.pool_members(ids), [])

    def mrow(self):
        import pair_cases as pc
        return pc.MODELS_ROWS[0]

    def layout(self, s):
        import pair_cases as pc
        P, M, ls, r, Pm = pc.POOL_P, pc.POOL_M, 1 + 2 * s.nb, self.mrow(), pc.MODELS_P
        ins = dict(stats=(P + 4) * ls * 8, order=P * 4, start=(M + 1) * 4, src=(P + 2) * s.n_elems * 8, counts=(P + 4) * pc.GRAM_PAIR_COUNT * 8,
                   g_bp=pc.MODELS_M * r.group_bp * 8, g_b64=pc.MODELS_M * r.T * 8, g_w32=pc.MODELS_M * r.group_w32 * 4, g_b32=pc.MODELS_M * r.T * 4,
                   g_mean32=pc.MODELS_M * r.nb * 4, g_inv32=pc.MODELS_M * r.nb * 4, g_status=pc.MODELS_M * 4, n_train=Pm * 8, group_of=Pm * 4)
        f64, f32, i32 = np.float64, np.float32, np.int32
        outs = dict(gstats=(M * ls * 8, f64), n_pool=(M * 8, np.int64), gmean=(M * s.nb * 8, f64), gscale=(M * s.nb * 8, f64),
                    pmean=(P * s.nb * 8, f64), pscale=(P * s.nb * 8, f64), gram=(M * s.n_elems * 8, f64),
                    bp=(Pm * r.npad * r.T * 8, f64), b64=(Pm * r.T * 8, f64), w32=(Pm * r.kpad * r.T * 4, f32), b32=(Pm * r.T * 4, f32),
                    mean32=(Pm * r.nb * 4, f32), inv32=(Pm * r.nb * 4, f32), status=(Pm * 4, i32), report_status=(Pm * 4, i32))
        return ins, outs, {}

    def calls(self, lib, s, p, st):
        import pair_cases as pc
        P, M, ls, r = pc.POOL_P, pc.POOL_M, 1 + 2 * s.nb, self.mrow()
        return [lib.hsr_pool_stats(p["stats"] + 2 * ls * 8, s.nb, P, p["order"], p["start"], M, p["gstats"], p["n_pool"], p["gmean"], p["gscale"],
                                   p["pmean"], p["pscale"], st),
                lib.hsr_pool_gram(p["src"] + s.n_elems * 8, s.n_elems, s.n_elems, p["counts"] + 2 * pc.GRAM_PAIR_COUNT * 8, pc.GRAM_PAIR_COUNT, P,
                                  p["order"], p["start"], M, p["gram"], s.n_elems, st),
                lib.hsr_pool_models(p["g_bp"], r.group_bp, p["g_b64"], p["g_w32"], r.group_w32, p["g_b32"], p["g_mean32"], p["g_inv32"],
                                    p["g_status"], p["n_train"], p["group_of"], r.nf, r.npad, r.kpad, r.T, r.nb, p["bp"], p["b64"], p["w32"],
                                    p["b32"], p["mean32"], p["inv32"], p["status"], p["report_status"], pc.MODELS_P, pc.MODELS_M, st)]

    def make_inputs(self, s, k):
        import pair_cases as pc
        order, start, _, _ = self.tables(k)
        _, stats = pc.pool_stats_inputs(s.nb)
        src, cnt = pc.gram_inputs(s.n_elems)
        nan2 = lambda rows: np.concatenate([np.full((2, rows.shape[1]), np.nan), rows, np.full((2, rows.shape[1]), np.nan)])
        counts = np.full((pc.POOL_P, pc.GRAM_PAIR_COUNT), 9.0)
        counts[:, 0] = cnt
        g, perm = pc.models_inputs(self.mrow()), list(POOL_PERMS[k])
        out = dict(stats=nan2(np.array(stats)), order=np.array(order, np.int32), start=np.array(start, np.int32),
                   src=np.concatenate([np.full((1, s.n_elems), np.nan), src, np.full((1, s.n_elems), np.nan)]), counts=nan2(counts),
                   g_status=np.array(pc.MODELS_POOL_STATUS, np.int32), n_train=np.array(pc.MODELS_N_TRAIN, np.int64)[perm],
                   group_of=np.array(pc.MODELS_GROUP_OF, np.int32)[perm])
        out.update({"g_" + key: np.array(v) for key, v in g.items()})
        return out

    def make_reference(self, s, k):
        import pair_cases as pc
        _, _, members, untouched = self.tables(k)
        samples, _ = pc.pool_stats_inputs(s.nb)
        src, cnt = pc.gram_inputs(s.n_elems)
        return dict(members=members, untouched=untouched, stats=[pc.pool_stats_reference(samples, mem, s.nb) for mem in members],
                    gram=pc.gram_reference(src, cnt, members))

    def check(self, got, s, k, worst):
        import pair_cases as pc
        ref, P, M, nb, ls, r = self.reference(s, k), pc.POOL_P, pc.POOL_M, s.nb, 1 + 2 * s.nb, self.mrow()
        gstats, gmean, gscale = got["gstats"].reshape(M, ls), got["gmean"].reshape(M, nb), got["gscale"].reshape(M, nb)
        pmean, pscale = got["pmean"].reshape(P, nb), got["pscale"].reshape(P, nb)
        same = lambda a, b: np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
        for g, mem in enumerate(ref["members"]):
            n, mean, m2, scale = ref["stats"][g]
            assert got["n_pool"][g] == n == gstats[g, 0] and same(gstats[g, 1:1 + nb], gmean[g]), (g, n)
            if n == 0:
                assert (gstats[g] == 0).all() and (gmean[g] == 0).all() and (gscale[g] == 1).all(), g
            else:
                _close(worst, "pool stats mean rtol 1e-12", gmean[g], mean, 1e-12)
                _close(worst, "pool stats M2 rtol 1e-12", gstats[g, 1 + nb:], m2, 1e-12)
                _close(worst, "pool stats scale rtol 1e-12", gscale[g], scale, 1e-12)
            assert all(same(pmean[p], gmean[g]) and same(pscale[p], gscale[g]) for p in mem), g
        for p in ref["untouched"]:
            assert (pmean[p].view(np.uint8) == FILL).all() and (pscale[p].view(np.uint8) == FILL).all(), p
        np.testing.assert_array_equal(got["gram"].reshape(M, s.n_elems), ref["gram"])
        g, perm = pc.models_inputs(r), POOL_PERMS[k]
        sizes = dict(bp=r.npad * r.T, b64=r.T, w32=r.kpad * r.T, b32=r.T, mean32=r.nb, inv32=r.nb, status=1, report_status=1)
        m = {key: got[key].reshape(pc.MODELS_P, n) for key, n in sizes.items()}
        for pos, pair in enumerate(perm):
            grp = pc.MODELS_GROUP_OF[pair]
            if not 0 <= grp < pc.MODELS_M:
                assert all((m[key][pos].view(np.uint8) == FILL).all() for key in m), pos
                continue
            want = pc.models_expected(r, g, grp)
            assert all(same(m[key][pos], want[key]) for key in pc.MODELS_FIELDS), pos
            assert (int(m["status"][pos, 0]), int(m["report_status"][pos, 0])) == pc.models_status(grp, pc.MODELS_N_TRAIN[pair]), pos


# ---- K4 predict: hsr_polyfeat_predict (logit) and hsr_polyfeat_predict_cube (sigmoid, NaN rule) on one model ------------------
PredShape = namedtuple("PredShape", "n_in degree T npix")
PRED_BIAS = (0.0, 0.25, -0.5)                           # added to the intercepts in set 0, 1, 2


class PredictRow(GenericRow):
    """The oracle's fit of tests/test_gpu_k4_instances.py::_model; the intercepts move with the set; set 1 holds non-finite samples and
    samples at and next to the nodata value, set 2 one near but not close to it.  hsr_polyfeat_prepare runs at build.  Bars, of
    ::test_predict: the oracle's float64 prediction of the model at 2e-4 (logit) and 1e-4 (reflectance), NaN in the same places; the
    logit entry, which has no rule for unusable pixels, is compared where the pixel's inputs are finite."""
    log, reuse = ("hsr_k4_last_launch", True), False

    def prepare(self, lib):
        s = self.shapes["small"]
        assert lib.hsr_polyfeat_prepare(s.n_in, s.degree) == 0, lib.hsr_last_error()

    def dims(self, s):
        nf = _lib().hsr_polyfeat_count(s.n_in, s.degree)
        return nf, (nf + 1) // 2 * 2, s.n_in + (s.n_in & 1)

    def layout(self, s):
        nf, kpad, even = self.dims(s)
        ins = dict(X=s.npix * even * 4, W=kpad * s.T * 4, bias=s.T * 4, mean=s.n_in * 4, inv=s.n_in * 4)
        return ins, dict(logit=(s.T * s.npix * 4, np.float32), refl=(s.T * s.npix * 4, np.float32)), {}

    def calls(self, lib, s, p, st):
        from test_gpu_k4_instances import NODATA
        even = self.dims(s)[2]
        head = (p["X"], even, 1, p["mean"], p["inv"], s.npix, s.n_in, s.degree, p["W"], s.T, p["bias"], s.T)
        return [lib.hsr_polyfeat_predict(*head, 0, p["logit"], s.npix, st),
                lib.hsr_polyfeat_predict_cube(*head, 1, 1, NODATA, 1, p["refl"], s.npix, st)]

    def make_inputs(self, s, k):
        from test_gpu_k4_instances import NODATA, _inputs, _model
        nf, kpad, even = self.dims(s)
        model = _model(s.n_in, s.degree, s.T)
        X = np.full((s.npix, even), np.nan, np.float32)
        X[:, :s.n_in] = _inputs(np.random.default_rng(31 * s.T + s.npix + k), s.npix, s.n_in)
        if k == 1:
            for i, v in enumerate([np.nan, np.inf, -np.inf, NODATA, NODATA + 0.01, NODATA - 0.01]):
                X[(7 * i + 1) % s.npix, i % s.n_in] = v
        if k == 2:
            X[s.npix // 2, 0] = np.float32(NODATA + 0.06)
        W = np.zeros((kpad, s.T), np.float32)
        W[:nf] = model["coef"].T
        return dict(X=X, W=W, bias=(model["intercept"] + PRED_BIAS[k]).astype(np.float32), mean=model["mean"].astype(np.float32),
                    inv=(1.0 / model["scale"]).astype(np.float32))

    def make_reference(self, s, k):
        from test_gpu_k4_instances import _model, _predict_ref
        i = self.inputs(s, k)
        m = dict(_model(s.n_in, s.degree, s.T), intercept=i["bias"].astype(np.float64))
        X = i["X"][:, :s.n_in]
        return dict(logit=_predict_ref(m, X, 0, 0, 0), refl=_predict_ref(m, X, 1, 1, 1), finite=np.isfinite(X).all(axis=1))

    def check(self, got, s, k, worst):
        ref = self.reference(s, k)
        logit, refl = got["logit"].reshape(s.T, s.npix)[:, ref["finite"]], got["refl"].reshape(s.T, s.npix)
        err = np.max(np.abs(logit - ref["logit"][:, ref["finite"]]))
        _note(worst, "predict logit (2e-4)", err / 2e-4)
        assert np.isfinite(logit).all() and err <= 2e-4, err
        assert np.array_equal(np.isnan(refl), np.isnan(ref["refl"])), "NaN set"
        err = np.nanmax(np.abs(refl - ref["refl"]))
        _note(worst, "predict reflectance (1e-4)", err / 1e-4)
        assert err <= 1e-4, err


# ---- tile pairs, fit and predict: the per-pair flow of s2_emit.pairs for a batch of two pairs ---------------------------------
PairShape = namedtuple("PairShape", "H W")              # the EMIT grid; S2 lies PAIR_F times finer
PAIR_P, PAIR_F, PAIR_B, PAIR_BANDS, PAIR_EPS, PAIR_ALPHA = 2, 2, 20, (0, 19, 7, 7, 3), 1e-4, 1.0
PAIR_END, PAIR_SND = -9999.0, 1000.0                    # emit_nodata, s2_nodata


class PairFitRow(GenericRow):
    """Two pairs, 4 S2 bands (degree 3: the 64 x 64 system of the k4-fit row), the 5 EMIT bands of pair_cases.MIXED, float32 tiles on
    the dyadic data of pair_cases.prep_inputs.  Set 0: a few unusable samples; set 1: pair 1 has no usable pixel - no training
    pixel, status 1, the identity system, NaN intercepts and predictions; set 2: every pixel usable, status 0 again.  Bars, stage by
    stage from the device's own operands: x, y and mask the bits of pair_cases.prep_reference
    (tests/test_gpu_pair_instances.py::test_prep); counts exact, mean / M2 / scale at rtol 1e-12 of the long double two-pass
    statistics (::test_stats); the rows of Q as tests/test_gpu_k4_instances.py::test_pair_expand (monomials bit-equal, logit within 2
    ulp, zero rows for the other pixels); Gram, factor, solution and read-out as the k4-fit row (::test_gram, ::test_chol,
    ::test_assemble_finish); the prediction within 1e-4 of the float64 evaluation of the device's model, NaN in the same places
    (::test_predict)."""
    log, out_off = ("hsr_pairs_last_launch", True), 0     # hsr_gram_f64_batched: 16-byte aligned rows of Q

    def prepare(self, lib):
        assert lib.hsr_polyfeat_prepare(RIDGE_IN, RIDGE_DEG) == 0, lib.hsr_last_error()

    def pcrow(self, s):
        import pair_cases as pc
        return pc.PrepRow("capture %dx%d" % s, s.H, s.W, PAIR_F, RIDGE_IN, PAIR_B, PAIR_BANDS, "float32", "float32", end=PAIR_END, snd=PAIR_SND)

    def layout(self, s):
        d, lib, P, T, nb, npix = ridge_dims(), _lib(), PAIR_P, RIDGE_T, RIDGE_IN, s.H * s.W
        n10 = npix * PAIR_F * PAIR_F
        f64, f32, i32 = np.float64, np.float32, np.int32
        ins = dict(emit=P * PAIR_B * npix * 4, s2=P * nb * n10 * 4, bands=T * 4)
        sizes = dict(x=(P * nb * npix, f32), y=(P * T * npix, f32), mask=(P * npix, np.uint8), stats=(P * (1 + 2 * nb), f64), mean=(P * nb, f64),
                     scale=(P * nb, f64), n_train=(P, np.int64), Q=(P * npix * d.ldq, f64), G=(P * d.na * d.ldq, f64), A=(P * d.npad * d.npad, f64),
                     B=(P * d.npad * T, f64), info=(P, i32), b64=(P * T, f64), b32=(P * T, f32), W32=(P * d.kpad * T, f32), mean32=(P * nb, f32),
                     inv32=(P * nb, f32), status=(P, i32), pred=(P * T * n10, f32))
        outs = {k: (c * np.dtype(dt).itemsize, dt) for k, (c, dt) in sizes.items()}
        return ins, outs, dict(gram_work=P * lib.hsr_gram_work_bytes(d.na, d.ldq, npix), chol_work=P * lib.hsr_chol_work_bytes(d.npad))

    def calls(self, lib, s, p, st):
        d, P, T, nb, npix, f = ridge_dims(), PAIR_P, RIDGE_T, RIDGE_IN, s.H * s.W, PAIR_F
        n10, na, ldq, npad, nf, kpad = npix * f * f, d.na, d.ldq, d.npad, d.nf, d.kpad
        wq = lib.hsr_gram_work_bytes(na, ldq, npix) // 8
        return [
            lib.hsr_pair_prep(p["emit"], 0, PAIR_B * npix, PAIR_B, p["bands"], T, p["s2"], 0, nb * n10, nb, s.H, s.W, f, PAIR_END, 1, PAIR_SND, 1,
                              p["x"], p["y"], p["mask"], P, st),
            lib.hsr_pair_stats(p["x"], p["mask"], npix, nb, p["stats"], p["mean"], p["scale"], p["n_train"], P, st),
            lib.hsr_pair_expand_f64(p["x"], nb * npix, p["mean"], p["scale"], nb, p["y"], T * npix, p["mask"], npix, npix, nb, RIDGE_DEG, T,
                                    PAIR_EPS, p["Q"], ldq, npix * ldq, na, P, st),
            lib.hsr_gram_f64_batched(p["Q"], ldq, na, ldq, npix, npix * ldq, p["gram_work"], wq, p["G"], ldq, na * ldq, P, st),
            lib.hsr_ridge_assemble_batched(p["G"], ldq, na * ldq, na, nf, T, PAIR_ALPHA, p["A"], npad, npad * npad, p["B"], T, npad * T, p["info"],
                                           P, st),
            lib.hsr_chol_solve_f64_batched(p["A"], npad, npad, npad * npad, p["B"], T, T, npad * T, p["chol_work"], p["info"], P, st),
            lib.hsr_ridge_finish_batched(p["G"], na * ldq, na, nf, T, p["B"], T, npad * T, p["mean"], p["scale"], nb, nb, kpad, p["b64"], p["b32"],
                                         T, p["W32"], kpad * T, p["mean32"], p["inv32"], nb, p["info"], p["status"], P, st),
            lib.hsr_polyfeat_predict_cube_batched(p["s2"], 1, n10, nb * n10, p["mean32"], p["inv32"], nb, n10, nb, RIDGE_DEG, p["W32"], T, kpad * T,
                                                  p["b32"], T, T, 1, 1, PAIR_SND, 1, p["pred"], n10, T * n10, P, st)]

    def make_inputs(self, s, k):
        import pair_cases as pc
        emit, s2 = pc.prep_inputs(self.pcrow(s))
        emit, s2 = np.roll(emit[:PAIR_P], k, axis=3).copy(), np.roll(s2[:PAIR_P], 2 * k, axis=3).copy()
        if k == 0:
            s2[0, 1, 2, 3], emit[0, PAIR_BANDS[0], 1, 1] = np.inf, PAIR_END
        if k == 1:
            s2[1, 0] = np.nan
        if k == 2:                                      # prep_inputs plants nodata values in pair 1: none of them here
            emit[emit == np.float32(PAIR_END)] = np.float32(0.5)
            s2[s2 == np.float32(PAIR_SND)] = np.float32(7.0)
        return dict(emit=emit, s2=s2, bands=np.array(PAIR_BANDS, np.int32))

    def make_reference(self, s, k):
        import pair_cases as pc
        i, r = self.inputs(s, k), self.pcrow(s)
        prep = [pc.prep_reference(r, i["emit"][p], i["s2"][p]) for p in range(PAIR_P)]
        return dict(prep=prep, stats=[pc.stats_reference(x, m) for x, _, m in prep])

    def check(self, got, s, k, worst):
        from gpu_harness import bits_equal
        from oracle import oracle_np as onp
        from test_gpu_k4_instances import U53, _assemble_ref, _finish_ref, _monomials
        d, ref, i, P, T, nb, npix = ridge_dims(), self.reference(s, k), self.inputs(s, k), PAIR_P, RIDGE_T, RIDGE_IN, s.H * s.W
        n10, nf, na, ldq, npad, kpad = npix * PAIR_F * PAIR_F, d.nf, d.na, d.ldq, d.npad, d.kpad
        sh = lambda name, *dims: got[name].reshape(P, *dims)
        x, y, mask, stats, mean, scale = sh("x", nb, npix), sh("y", T, npix), sh("mask", npix), sh("stats", 1 + 2 * nb), sh("mean", nb), sh("scale", nb)
        Q, G, A, B, W32, pred = sh("Q", npix, ldq), sh("G", na, ldq), sh("A", npad, npad), sh("B", npad, T), sh("W32", kpad, T), sh("pred", T, n10)
        for p in range(P):
            xr, yr, mr = ref["prep"][p]
            bits_equal(x[p], xr, f"x of pair {p}")
            bits_equal(y[p], yr, f"y of pair {p}")
            np.testing.assert_array_equal(mask[p], mr)
            n, mu, m2, sc = ref["stats"][p]
            assert got["n_train"][p] == n == stats[p, 0] and np.array_equal(stats[p, 1:1 + nb], mean[p]), (p, n)
            assert int(got["status"][p]) == (0 if n else 1) and (n == 0) == (k == 1 and p == 1), (p, n, got["status"])
            ok = mask[p] != 0
            assert (Q[p][~ok].view(np.uint64) == 0).all(), "masked-out rows of Q"
            Xs = np.where(np.isfinite(i["s2"][p]), i["s2"][p], 0.0).reshape(nb, n10).T.astype(np.float64)
            unusable = ~np.isfinite(i["s2"][p]).all(axis=0).reshape(-1) | np.isclose(i["s2"][p], PAIR_SND).any(axis=0).reshape(-1)
            if n == 0:                                  # no training pixel: identity system, NaN intercepts, NaN predictions
                assert (stats[p] == 0).all() and (scale[p] == 1).all() and (A[p] == np.eye(npad)).all() and (B[p].view(np.uint64) == 0).all()
                assert np.isnan(got["b64"].reshape(P, T)[p]).all() and np.isnan(got["b32"].reshape(P, T)[p]).all() and np.isnan(pred[p]).all()
                continue
            _close(worst, "pair stats mean rtol 1e-12", mean[p], mu, 1e-12)
            _close(worst, "pair stats M2 rtol 1e-12", stats[p, 1 + nb:], m2, 1e-12)
            _close(worst, "pair stats scale rtol 1e-12", scale[p], sc, 1e-12)
            g = Q[p][ok]
            assert (g[:, 0] == 1.0).all() and (g[:, nf + 1:na].view(np.uint64) == 0).all() and (g[:, na + T:].view(np.uint64) == 0).all()
            assert np.array_equal(g[:, 1:nf + 1].view(np.uint64), _monomials(x[p].T[ok], mean[p], scale[p], nb, RIDGE_DEG).view(np.uint64)), "monomials"
            u = np.clip(y[p].T[ok].astype(np.float64), PAIR_EPS, 1 - PAIR_EPS)
            lg = np.log(u / (1 - u))
            ulp = np.abs(g[:, na:na + T] - lg) / np.spacing(np.abs(lg))
            _note(worst, "pair expand logit (2 ulp)", ulp.max() / 2)
            assert (ulp <= 2).all(), ulp.max()
            Ql = Q[p].astype(LD)
            err, bound = np.abs(G[p].astype(LD) - Ql[:, :na].T @ Ql), 2 * npix * U53 * (np.abs(Q[p][:, :na]).T @ np.abs(Q[p]))
            with np.errstate(invalid="ignore", divide="ignore"):
                _note(worst, "pair gram (2 n 2^-53 |A|^T |B|)", np.max(np.where(err == 0, 0, err / bound)))
            assert (err <= bound).all() and int(got["info"][p]) == 0
            A_ref, B_ref = _assemble_ref(G[p], na, nf, T, PAIR_ALPHA, npad)
            L, W = np.tril(A[p]).astype(LD), B[p]
            anorm = np.abs(A_ref).sum(axis=1).max()
            r1 = np.abs(L @ L.T - A_ref.astype(LD)).sum(axis=1).max() / (npad * anorm * U52)
            r2 = np.abs(A_ref.astype(LD) @ W.astype(LD) - B_ref.astype(LD)).sum(axis=0).max() / (npad * anorm * np.abs(W).sum(axis=0).max() * U52)
            _note(worst, "pair chol factor / solve ratio (<= 1)", max(r1, r2))
            assert r1 <= 1 and r2 <= 1, (float(r1), float(r2))
            want = _finish_ref(G[p], na, nf, T, W[:nf], mean[p], scale[p], kpad)
            have = (got["b64"].reshape(P, T)[p], got["b32"].reshape(P, T)[p], W32[p], got["mean32"].reshape(P, nb)[p], got["inv32"].reshape(P, nb)[p])
            for name, a, b in zip(("b64", "b32", "W32", "mean32", "inv32"), have, want):
                assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).reshape(a.shape).view(np.uint8)), name
            model = dict(mean=mean[p], scale=scale[p], coef=W[:nf].T, intercept=want[0], degree=RIDGE_DEG)
            pr = onp.sigmoid(onp.ridge_poly_predict(model, Xs)).T
            pr[:, unusable] = np.nan
            assert np.array_equal(np.isnan(pred[p]), np.isnan(pr)), "NaN set of the prediction"
            e = np.nanmax(np.abs(pred[p] - pr))
            _note(worst, "pair predict reflectance (1e-4)", e / 1e-4)
            assert e <= 1e-4, e


# =============================================================================================================================
# the table
# =============================================================================================================================
_ROWS = [
    # 3 x 65 output pixels are 6 workgroups, 5 x 150 are 15; quality mask + float4 path, band mask + LDS transposition
    OrthoRow("ortho-bip", ["hsr_ortho_glt"], OrthoShape(4, 6, 7, 3, 65, oc.BIP, True, False), OrthoShape(4, 6, 7, 5, 150, oc.BIP, True, False)),
    OrthoRow("ortho-bsq", ["hsr_ortho_glt"], OrthoShape(3, 6, 7, 3, 65, oc.BSQ, False, True), OrthoShape(3, 6, 7, 5, 150, oc.BSQ, False, True)),
    # 2 x 2 windows against 4 x 4; three waves a row as scene_cases.DECIDING_HW
    ScanRow("scene-black-counts", ["hsr_scene_black_counts"], SceneShape(2, 6, 150, 3, 64), SceneShape(2, 12, 300, 3, 64)),
    CholRow("chol", ["hsr_chol_solve_f64"], CholShape(96, 1, 3), CholShape(288, 1, 3)),
    CholRow("chol-batched", ["hsr_chol_solve_f64_batched"], CholShape(96, 2, 3), CholShape(288, 2, 3)),
    # two and three 64-row chunks, odd and even m
    OtRow("ot-staged", ["hsr_ot_begin", "hsr_ot_iterate", "hsr_ot_finish"], OtShape(97, 65), OtShape(130, 66), True),
    OtRow("ot-one-call", ["hsr_ot_sinkhorn_barycentric"], OtShape(97, 65), OtShape(130, 66), False),
    # one row on each side of kTinyMaxPix, and the tiny kernel after the three-pass select in a workspace sized for more bands
    PctRow("percentile-tiny", ["hsr_percentile_limits"], PctShape(999, 2), PctShape(TINY_MAX + 69, 3), False),
    PctRow("percentile-passes", ["hsr_percentile_limits"], PctShape(TINY_MAX + 69, 2), PctShape(70001, 3), False),
    PctRow("percentile-staged", ["hsr_percentile_begin", "hsr_percentile_hist", "hsr_percentile_scan"], PctShape(999, 2),
           PctShape(TINY_MAX + 69, 3), True),
    # 64 * 7 + 13 pixels are 8 partial slots, 64 * 40 are 40
    FitRow("k2-fit-apply", ["hsr_poly_moments", "hsr_moments_reduce", "hsr_poly_solve", "hsr_poly_apply"], FitShape(461, 3, 2),
           FitShape(2560, 3, 2), False),
    FitRow("k2-f64-fit", ["hsr_poly_moments_f64", "hsr_moments_reduce_solve"], FitShape(461, 3, 3), FitShape(2560, 3, 3), True),
    # K1: 8 partial slots against 40; the fused fit where 16 workgroups >= 12 bands (16 x 64 pixels) and where 5 < 12 (3 x 90), the
    # two tile geometries of tests/test_gpu_group_sizes.py
    K1Row("k1", ["hsr_srf_integrate"], K1Shape(1, 461), K1Shape(40, 64), "k1", False, False),
    K1Row("k1-u16", ["hsr_srf_integrate_u16"], K1Shape(1, 461), K1Shape(40, 64), "k1", True, False),
    K1Row("step", ["hsr_srf_integrate_moments", "hsr_moments_reduce_solve", "hsr_poly_apply"], K1Shape(1, 461), K1Shape(40, 64), "step", False, True),
    K1Row("step-u16", ["hsr_srf_integrate_moments_u16", "hsr_moments_reduce_solve", "hsr_poly_apply"], K1Shape(1, 461), K1Shape(40, 64), "step",
          True, True),
    # a plan stores the arguments of one npix: no reuse across shapes; the mask pointer is given at capture, its contents change
    K1Row("step-apply-null-job", ["hsr_srf_integrate_moments_apply", "hsr_moments_reduce_solve", "hsr_poly_apply"], K1Shape(1, 461), K1Shape(40, 64),
          "step-apply", False, True),
    K1Row("step-apply-null-job-u16", ["hsr_srf_integrate_moments_u16_apply", "hsr_moments_reduce_solve", "hsr_poly_apply"], K1Shape(1, 461),
          K1Shape(40, 64), "step-apply", True, True),
    K1Row("plan-step", ["hsr_step_run"], K1Shape(1, 461), K1Shape(40, 64), "plan", False, False),
    K1Row("plan-step-u16", ["hsr_step_run"], K1Shape(1, 461), K1Shape(40, 64), "plan", True, False),
    K1Row("plan-pieces", ["hsr_step_run_k1", "hsr_step_run_reduce", "hsr_step_run_solve", "hsr_step_run_apply"], K1Shape(1, 461),
          K1Shape(40, 64), "plan-pieces", False, False),
    K1Row("fused-fit-16x64", ["hsr_srf_integrate_fit", "hsr_poly_apply"], K1Shape(16, 64), K1Shape(40, 64), "fit", False, True),
    K1Row("fused-fit-3x90", ["hsr_srf_integrate_fit", "hsr_poly_apply"], K1Shape(3, 90), K1Shape(16, 64), "fit", False, True),
    K1Row("fused-fit-16x64-u16", ["hsr_srf_integrate_fit_u16", "hsr_poly_apply"], K1Shape(16, 64), K1Shape(40, 64), "fit", True, True),
    K1Row("fused-fit-3x90-u16", ["hsr_srf_integrate_fit_u16", "hsr_poly_apply"], K1Shape(3, 90), K1Shape(16, 64), "fit", True, True),
    # one row chunk of the Gram against three (gram_reg_chunks: 1024 rows a chunk)
    # two pixel chunks of the score against six (pair_cases.SCORE_PIX = 512 pixels a chunk)
    ScoreRow("pairs-holdout-score", ["hsr_pair_holdout", "hsr_pair_score_f64"], ScoreShape(5, 516), ScoreShape(5, 2564)),
    # a ragged three-tile batch: 8 + 5 + 16 partial slots against 40 + 8 + 18
    BatchRow("batch", ["hsr_srf_integrate_moments_batched", "hsr_moments_reduce_solve_batched", "hsr_poly_apply_batched"],
             BatchShape((461, 270, 1024)), BatchShape((2560, 461, 1100))),
    AuxRow("aux-codec", ["hsr_tile_encode_u16", "hsr_tile_decode_u16"], AuxShape(1, 13, 79, 1), AuxShape(1, 199, 201, 1), "codec"),
    AuxRow("aux-interleave", ["hsr_interleave_to_bip"], AuxShape(64, 3, 63, 1), AuxShape(65, 2, 130, 1), "interleave"),
    AuxRow("aux-block-mean", ["hsr_block_mean"], AuxShape(2, 5, 13, 6), AuxShape(2, 5, 64, 2), "block-mean"),
    AuxRow("aux-upsample", ["hsr_bilinear_upsample"], AuxShape(2, 1, 5, 7), AuxShape(1, 3, 85, 3), "upsample"),
    AuxRow("aux-upsample-hist", ["hsr_bilinear_upsample_mask_hist", "hsr_percentile_begin", "hsr_percentile_hist", "hsr_percentile_scan"],
           AuxShape(3, 6, 5, 6), AuxShape(3, 11, 85, 3), "upsample-hist"),
    AuxRow("aux-valid-mask", ["hsr_valid_mask"], AuxShape(3, 7, 67, 1), AuxShape(3, 40, 64, 1), "valid-mask"),
    TileRow("scene-gather-mosaic", ["hsr_scene_gather_tiles", "hsr_scene_mosaic"], TileShape(3, 23, 36, 6, 8, 6, 8), TileShape(3, 35, 52, 6, 8, 6, 8),
            "mosaic"),
    TileRow("scene-gather-encode", ["hsr_scene_gather_tiles"], TileShape(3, 21, 27, 5, 7, 5, 7), TileShape(3, 35, 52, 6, 8, 6, 8), "encode"),
    TileRow("scene-gather-blend", ["hsr_scene_gather_tiles", "hsr_scene_mosaic_blend"], TileShape(3, 19, 24, 6, 8, 3, 4),
            TileShape(3, 31, 36, 6, 8, 3, 4), "blend"),
    # one chunk of 256 pixels of the report against five
    PairReportRow("pairs-report", ["hsr_pair_report_f64"], RepShape(48, 47, 16, 255), RepShape(48, 47, 16, 1037)),
    # two blocks of 512 Gram elements against three; 4 bands against 16
    PoolRow("pairs-pool", ["hsr_pool_stats", "hsr_pool_gram", "hsr_pool_models"], PoolShape(4, 600), PoolShape(16, 1026)),
    # the generic predict kernel (4 inputs) and an orbit kernel (10 inputs, degree 3, T <= 16)
    PredictRow("k4-predict-generic", ["hsr_polyfeat_predict", "hsr_polyfeat_predict_cube"], PredShape(4, 3, 20, 33), PredShape(4, 3, 20, 1517)),
    PredictRow("k4-predict-orbit", ["hsr_polyfeat_predict", "hsr_polyfeat_predict_cube"], PredShape(10, 3, 16, 33), PredShape(10, 3, 16, 1517)),
    # 259 pixels a pair against 1050: one row chunk of the batched Gram against two
    PairFitRow("pairs-fit-predict", ["hsr_pair_prep", "hsr_pair_stats", "hsr_pair_expand_f64", "hsr_gram_f64_batched", "hsr_ridge_assemble_batched",
                                     "hsr_chol_solve_f64_batched", "hsr_ridge_finish_batched", "hsr_polyfeat_predict_cube_batched"],
               PairShape(7, 37), PairShape(15, 70)),
    RidgeRow("k4-fit", ["hsr_ridge_stats", "hsr_polyfeat_expand_f64", "hsr_gram_f64", "hsr_ridge_assemble", "hsr_chol_solve_f64",
                        "hsr_ridge_finish"], RidgeShape(1000), RidgeShape(2100)),
]
ROWS = {r.name: r for r in _ROWS}
assert len(ROWS) == len(_ROWS)

# =============================================================================================================================
# the entry points without a row
# =============================================================================================================================
NOT_LAUNCH_PATH = [
    # library, sizing and geometry queries (host only)
    "hsr_abi_version", "hsr_last_error", "hsr_moment_count", "hsr_partial_slots", "hsr_partials_bytes", "hsr_percentile_work_bytes",
    "hsr_percentile_hist_region", "hsr_batch_partials_bytes", "hsr_ot_work_bytes", "hsr_ot_work_region", "hsr_chol_work_bytes",
    "hsr_polyfeat_count", "hsr_gram_work_bytes", "hsr_ridge_stats_work_bytes", "hsr_pair_report_work_bytes", "hsr_pair_score_work_bytes",
    "hsr_srf_fused_launch_supported", "hsr_step_plan_slots", "hsr_pipeline_count",
    # host work done once, before a launch path exists
    "hsr_poly_solve_host", "hsr_batch_plan", "hsr_polyfeat_table", "hsr_polyfeat_prepare",
    # launch records and instance tables
    "hsr_srf_last_launch", "hsr_srf_kernel_instance", "hsr_poly_last_launch", "hsr_polyfeat_predict_kernel",
    "hsr_aux_last_launch", "hsr_aux_instance_count", "hsr_aux_instance_name", "hsr_scene_last_launch", "hsr_scene_instance_count",
    "hsr_scene_instance_name", "hsr_k4_last_launch", "hsr_k4_instance_count", "hsr_k4_instance_name", "hsr_pairs_last_launch",
    "hsr_pairs_instance_count", "hsr_pairs_instance_name", "hsr_ortho_last_launch", "hsr_ortho_instance_count", "hsr_ortho_instance_name",
    # objects: creation allocates (and synchronises, hsr_exec.hip), destruction frees, status synchronises both streams by contract
    "hsr_step_plan_create", "hsr_step_plan_destroy", "hsr_pipeline_create", "hsr_pipeline_create_fused", "hsr_pipeline_create_exchange",
    "hsr_pipeline_create_group", "hsr_pipeline_destroy", "hsr_pipeline_status",
    "hsr_comm_available", "hsr_comm_version", "hsr_comm_unique_id", "hsr_comm_init", "hsr_comm_destroy", "hsr_comm_rank", "hsr_comm_ranks",
]

_PIPELINE = ("csrc/hsr_exec.hip: a submit records and waits on events between the caller's stream and the pipeline's side stream (parallel "
             "branches in a graph), the exchange form polls device words and may run a host callback on the side stream, and the ticket base "
             "of the tail fit (fit_ticket_base = the pipeline's running count of workgroups) advances on the host per call: a replay would "
             "reuse the captured base")
_COLLECTIVE = ("csrc/hsr_comm.hip: a thin call into RCCL on a communicator; whether and how a collective can be captured is RCCL's "
               "contract, not this library's, and a replay needs every rank to replay")
EXCLUDED = {
    "hsr_pipeline_submit": _PIPELINE,
    "hsr_pipeline_flush": _PIPELINE,
    "hsr_pipeline_fit_done": _PIPELINE,
    "hsr_allreduce_f64": _COLLECTIVE,
    "hsr_reduce_f64": _COLLECTIVE,
    "hsr_allreduce_u32": _COLLECTIVE,
    "hsr_bcast": _COLLECTIVE,
    "hsr_probe_read": "csrc/hsr_lib.hip: a bandwidth probe for bench.py whose only output is a sink the kernels fold loads into; it has no "
                      "result a replay could be compared with",
}

# Forms of entries that HAVE a row which are nevertheless not capturable (not part of the partition by name).
EXCLUDED_FORMS = {
    "hsr_srf_integrate_moments_apply with job != NULL":
        "the launch takes hsr_apply_job.fit_ticket_base, which the host advances per launch by the workgroups of all earlier launches "
        "(csrc/hsr_srf.hip: a.lazy_base = job->fit_ticket_base, read only inside `if (job)`): frozen at capture, so a replay draws tickets "
        "against a stale base.  With job == NULL no field of the job is touched: rows step-apply-null-job[-u16]",
    "hsr_srf_integrate_moments_u16_apply with job != NULL":
        "the same launcher behind the uint16 ring kernel (csrc/hsr_srf.hip): fit_ticket_base is a host value frozen at capture",
}

def covered():
    return sorted({name for r in ROWS.values() for name in r.covers})
