"""Every stage and stop rule of the Sinkhorn kernels (csrc/hsr_ot.hip) on an MI355X, row by row of the table of tests/ot_cases.py,
against its long-double references.

The five entry points are called through ctypes.  X, Y, Ybar, info and the workspace lie in buffers filled with a sentinel byte
between two guard zones (Buf of gpu_harness.py); the workspace has exactly hsr_ot_work_bytes bytes and is never fresh.  What
the kernels leave in it - K, u, v and the 24-byte state - is read through hsr_ot_work_region after hsr_ot_begin and after every
single iteration, and compared with ONE reference step taken from the device's own previous (K, u, v): errors do not compound,
so every bound is the derived one of ot_cases.py, and a last-bit difference of exp cannot move a stop decision.  The int32 `pad`
of the state is never written by the library and is left out of every comparison.

The last test prints the largest observed error as a fraction of each bound."""
import ctypes as C

import numpy as np
import pytest

import ot_cases as oc
from gpu_harness import Buf, same_bits, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from gpu_harness import lib as _lib, stream as _stream

pytestmark = pytest.mark.gpu

LD = oc.LD
WORST = {"K": 0.0, "step": 0.0, "err": 0.0, "projection": 0.0, "exp ulp": 0.0}


def _worst(key, got, ref, bound):
    """|got - ref| <= bound elementwise (got float64, ref and bound long double); keeps the largest fraction of the bound."""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, LD), np.asarray(bound, LD)
    assert np.isfinite(got).all(), f"{key}: non-finite device value"
    assert np.isfinite(bound).all() and (bound >= 0).all(), f"{key}: the reference gives no bound here"
    diff = np.abs(got.astype(LD) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.where(diff == 0, LD(0), diff / bound)                   # an exact value needs no bound
    worst = float(np.max(frac))
    WORST[key] = max(WORST[key], worst)
    assert worst <= 1.0, f"{key}: {worst:.3g} of the bound at {np.unravel_index(np.argmax(frac), frac.shape)}"


def _state(raw):
    """(break_iter, conv_iter, checks, err) of 24 state bytes; None for 'never'."""
    i = raw[:12].view(np.int32)
    return (None if i[0] == oc.NEVER else int(i[0]), None if i[1] == oc.NEVER else int(i[1]), int(i[2]), raw[16:24].view(np.float64)[0])


def _same_state(a, b, what):
    assert a[:3] == b[:3], (what, a, b)
    same_bits(np.array([a[3]]), np.array([b[3]]), what + ": err")


class Run:
    """The device buffers of one solve of the row's inputs."""

    def __init__(self, torch, X, Y, off, work_bytes=None):
        self.torch, self.lib, self.st = torch, _lib(), _stream(torch)
        self.X, self.Y, self.n, self.m = X, Y, len(X), len(Y)
        self.xb, self.yb = Buf(torch, X.nbytes, off, X), Buf(torch, Y.nbytes, off, Y)
        self.ob, self.ib = Buf(torch, self.n * 24, 0), Buf(torch, 24, 0)
        self.wb = Buf(torch, self.lib.hsr_ot_work_bytes(self.n, self.m), 0)
        if work_bytes is not None:
            self.wb.put(work_bytes)
        off_, cnt = C.c_int64(), C.c_int64()
        self.regions = []
        for which in range(8):
            assert self.lib.hsr_ot_work_region(self.n, self.m, which, C.byref(off_), C.byref(cnt)) == 0
            self.regions.append((off_.value, cnt.value))

    def ok(self, rc):
        assert rc == 0, (rc, self.lib.hsr_last_error())

    def begin(self, reg):
        self.ok(self.lib.hsr_ot_begin(self.xb.ptr, self.n, self.yb.ptr, self.m, reg, self.wb.ptr, self.st))

    def iterate(self, first, count, thr):
        self.ok(self.lib.hsr_ot_iterate(self.n, self.m, first, count, thr, self.wb.ptr, self.ib.ptr, self.st))

    def finish(self, iters):
        self.ok(self.lib.hsr_ot_finish(self.yb.ptr, self.n, self.m, iters, self.wb.ptr, self.ob.ptr, self.ib.ptr, self.st))

    def whole(self, reg, itmax, thr):
        self.ok(self.lib.hsr_ot_sinkhorn_barycentric(self.xb.ptr, self.n, self.yb.ptr, self.m, reg, itmax, thr, self.wb.ptr, self.ob.ptr,
                                                     self.ib.ptr, self.st))
        return self.result()

    def work(self):
        """The workspace as the kernels left it (guard zones checked): raw bytes, state, K, u[2], v[2]."""
        raw = self.wb.get(np.uint8)
        part = [raw[o: o + 8 * c] for o, c in self.regions]
        f = [p.view(np.float64) for p in part]
        return dict(raw=raw, state=_state(part[oc.STATE]), K=f[oc.K_].reshape(self.n, self.m), u=[f[oc.U0], f[oc.U1]], v=[f[oc.V0], f[oc.V1]])

    def result(self):
        """(Ybar, state from info) after checking every guard zone and that the inputs are as they were."""
        same_bits(self.xb.get(np.float64), self.X.reshape(-1), "X")
        same_bits(self.yb.get(np.float64), self.Y.reshape(-1), "Y")
        self.wb.get(np.uint8)
        return self.ob.get(np.float64).reshape(self.n, 3), _state(self.ib.get(np.uint8))


def _exp_ulp(X, Y, reg, K):
    """Largest distance, in spacings of K, between the device's K and the correctly rounded exp of the argument the kernel forms."""
    t = np.maximum(oc.device_sqdist(X, Y), 0.0) / (-reg)
    ref = np.exp(t.astype(LD))
    return float(np.max(np.abs(K.astype(LD) - ref) / np.spacing(oc.f64(ref)).astype(LD)))


def _expected_state(e, ii):
    """(break_iter, conv_iter, checks) after iteration ii of a row with expectations e."""
    brk = e["break_iter"] if e["break_iter"] is not None and ii >= e["break_iter"] else None
    conv = e["conv_iter"] if e["conv_iter"] is not None and ii >= e["conv_iter"] else None
    last = min([ii] + [s for s in (e["break_iter"], e["conv_iter"]) if s is not None])
    checks = len(range(0, last + 1, 10)) - (1 if brk is not None and brk % 10 == 0 else 0)
    return brk, conv, checks


def _check_step(r, ii, prev, cur):
    """Iteration ii took `prev` to `cur`: one reference step from the device's own operands."""
    n, m, e = r["n"], r["m"], r["expect"]
    K, src, dst = prev["K"], ii & 1, (ii + 1) & 1
    same_bits(cur["K"], K, "K after an iteration")
    same_bits(cur["u"][src], prev["u"][src], "u read by the iteration")
    same_bits(cur["v"][src], prev["v"][src], "v read by the iteration")
    KtU, vn = oc.col_update(K, prev["u"][src], m)
    Kv, un = oc.row_update(K, cur["v"][dst], n)                           # from the device's new v: the operand its row pass had
    hit = oc.breakdown(KtU, vn, un)
    if e["break_iter"] is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            q = float(np.log(np.nanmax(np.concatenate([vn, un])) / oc.DBL_MAX))
        assert abs(q) > oc.MARGIN and (q > 0) == (ii == e["break_iter"]), f"case lost its margin: ln(q / DBL_MAX) = {q:.3g} at iteration {ii}"
    brk, conv, checks = cur["state"][:3]
    assert (brk, conv, checks) == _expected_state(e, ii), (ii, cur["state"])
    if any(hit.values()):
        assert brk == ii and e["through"] == ("zero" if hit["zero"] else "v" if hit["v"] else "u"), (ii, hit)
        same_bits(np.array([cur["state"][3]]), np.array([prev["state"][3]]), "err after a breakdown")
        return
    assert brk is None
    _worst("step", cur["v"][dst], vn, oc.matvec_bound(n, KtU) * vn)
    _worst("step", cur["u"][dst], un, oc.matvec_bound(m, Kv) * un)
    if ii % 10 == 0:
        err, bound = oc.marginal_error(K, cur["u"][dst], cur["v"][dst])   # the updated pair
        _worst("err", cur["state"][3], err, bound)
        assert conv == (ii if cur["state"][3] < r["thr"] else None)
    else:
        same_bits(np.array([cur["state"][3]]), np.array([prev["state"][3]]), "err without a check")


def _staged(torch, name, off):
    """Steps 1-4: the row through begin, single iterations, the rest, finish.  -> (Ybar, state)"""
    r = oc.ROWS[name]
    X, Y = oc.inputs(name)
    n, m, e, itmax = r["n"], r["m"], r["expect"], r["itmax"]
    run = Run(torch, X, Y, off)
    # 1. begin
    run.begin(r["reg"])
    cur = run.work()
    K_ref = oc.kernel_matrix(X, Y, r["reg"])
    _worst("K", cur["K"], K_ref, oc.kernel_matrix_bound(X, Y, r["reg"], K_ref))
    assert (cur["K"] <= 1.0).all(), "K above 1: a negative squared distance reached exp"      # d is clamped at 0
    WORST["exp ulp"] = max(WORST["exp ulp"], _exp_ulp(X, Y, r["reg"], cur["K"]))
    same_bits(cur["u"][0], np.full(n, 1.0 / n), "u0 after begin")
    same_bits(cur["v"][0], np.full(m, 1.0 / m), "v0 after begin")
    assert cur["state"] == (None, None, 0, np.inf), cur["state"]
    K0 = cur["K"]
    # 2. one iteration at a time
    stop = e["break_iter"] if e["break_iter"] is not None else e["conv_iter"]
    done = 0
    for k in range(min(r["stepwise"], itmax)):
        prev = cur
        run.iterate(k, 1, r["thr"])
        cur, done = run.work(), k + 1
        _same_state(_state(run.ib.get(np.uint8)), cur["state"], "info of iterate")
        if stop is not None and k > stop:                                 # one more call after the stop: nothing moves
            assert np.array_equal(cur["raw"], prev["raw"]), "an iteration after the stop wrote to the workspace"
            break
        _check_step(r, k, prev, cur)
    # 3. the rest in one call
    if done < itmax:
        run.iterate(done, itmax - done, r["thr"])
        cur = run.work()
        same_bits(cur["K"], K0, "K after the rest of the iterations")
    assert cur["state"][:3] == (e["break_iter"], e["conv_iter"], e["checks"]), cur["state"]
    buf = oc.final_buffer(e["break_iter"], e["conv_iter"], itmax)
    last = e["break_iter"] - 1 if e["break_iter"] is not None else (e["conv_iter"] if e["conv_iter"] is not None else itmax - 1)
    if last >= 0 and last % 10 == 0:                                      # the pair the loop ended on is the pair of the last check
        err, bound = oc.marginal_error(cur["K"], cur["u"][buf], cur["v"][buf])
        _worst("err", cur["state"][3], err, bound)
    # 4. finish
    run.finish(itmax)
    ybar, info = run.result()
    _same_state(info, cur["state"], "info of finish")
    assert np.array_equal(run.work()["raw"], cur["raw"]), "finish wrote to the workspace"
    ref, bound = oc.projection(cur["K"], cur["u"][buf], cur["v"][buf], Y)
    _worst("projection", ybar, ref, bound)
    with np.errstate(all="ignore"):
        other, obound = oc.projection(cur["K"], cur["u"][buf ^ 1], cur["v"][buf ^ 1], Y)
        apart = ~(np.abs(other - ref) <= bound + obound)                  # also where the other pair gives no number at all
        assert not (np.abs(ybar.astype(LD) - other) <= obound)[apart].any(), "Ybar is the projection of the other (u, v) buffer"
    if n > 1:
        assert apart.any(), "the two buffers give the same projection: the row cannot tell them apart"
    return ybar, info


@pytest.mark.parametrize("off", [0, 8])
@pytest.mark.parametrize("name", list(oc.ROWS))
def test_rows(torch_gpu, name, off):
    torch = torch_gpu
    r = oc.ROWS[name]
    X, Y = oc.inputs(name)
    ybar, info = _staged(torch, name, off)
    # 5. the same row in one call, in a sentinel-filled workspace, in one full of NaN and in one a larger problem has used
    args = (r["reg"], r["itmax"], r["thr"])
    first = Run(torch, X, Y, off)
    big = Run(torch, *oc.clouds(r["n"] + 9, r["m"] + 7, 3), 0)
    big.whole(0.05, 3, 0.0)
    nbytes = first.wb.nbytes
    for what, run in (("sentinel", first), ("0xFF", Run(torch, X, Y, off, np.full(nbytes, 0xFF, np.uint8))),
                      ("after a larger problem", Run(torch, X, Y, off, big.wb.get(np.uint8)[:nbytes]))):
        got, ginfo = run.whole(*args)
        same_bits(got, ybar, "Ybar of the one-call solve, workspace " + what)
        _same_state(ginfo, info, "info of the one-call solve, workspace " + what)
    # 6. again in the workspace that has just been used
    got, ginfo = first.whole(*args)
    same_bits(got, ybar, "Ybar of a second run")
    _same_state(ginfo, info, "info of a second run")


def test_public_path_non_contiguous_on_a_side_stream(torch_gpu):
    """barycentric_targets_device with X[::2] and Y[::2] views on a non-default stream: the bits of the contiguous call."""
    torch = torch_gpu
    from s2_emit import _ot
    X, Y = oc.clouds(140, 132, 7)
    Xd, Yd = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    xv, yv = Xd[::2], Yd[::2]
    assert not xv.is_contiguous() and not yv.is_contiguous()
    want, winfo = _ot.barycentric_targets_device(xv.contiguous(), yv.contiguous(), 0.05, 25, 1e-3, return_info=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    with torch.cuda.stream(side):
        got, ginfo = _ot.barycentric_targets_device(xv, yv, 0.05, 25, 1e-3, return_info=True)
        polled = _ot.barycentric_targets_device(xv, yv, 0.05, 25, 1e-3, poll_every=4)
    side.synchronize()
    same_bits(got.cpu().numpy(), want.cpu().numpy(), "Ybar from the views")
    same_bits(polled.cpu().numpy(), want.cpu().numpy(), "Ybar from the views, polled")
    assert ginfo == winfo and winfo["conv_iter"] in (10, 20) and winfo["checks"] >= 2
    ref = oc.solve(X[::2], Y[::2], 0.05, 25, 1e-3)
    assert (ginfo["break_iter"], ginfo["conv_iter"], ginfo["checks"]) == (ref["break_iter"], ref["conv_iter"], ref["checks"])


def test_report_worst_fractions(torch_gpu):
    """Not a check of its own: what the rows above measured, for the profile note (each figure was asserted <= 1 where it arose;
    the exp distance against EXP_ULP here)."""
    print("ot rows: %d x 2 alignments" % len(oc.ROWS))
    for key, val in WORST.items():
        print("ot worst %s: %.4g%s" % (key, val, "" if key == "exp ulp" else " of the bound"))
    assert WORST["exp ulp"] <= oc.EXP_ULP
