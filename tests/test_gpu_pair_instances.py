"""Every kernel instance of csrc/hsr_pairs.hip - pair prep, pair stats, the fit report, the hold-out codes, the validation score and
the three pooling kernels - on an MI355X, row by row of the tables of tests/pair_cases.py, against the references stated there.

The entry points are called through ctypes.  Inputs and outputs lie in buffers filled with a sentinel byte between two guard
zones (Buf of gpu_harness.py), pairs `stride` elements apart with sentinel gaps: what a call does not own must come
back untouched.  After every call the library's launch record (hsr_pairs_last_launch) is read and compared with the sequence the
row names; a second launch must give identical bits; and a pair's outputs must carry the same bits alone and at every position of
a batch of 3 (_positions).  The last test checks that the rows reached every name hsr_pairs_instance_name enumerates and prints
the largest error seen under every bar.  What the rows claim about themselves is checked without a GPU in
test_pair_instances_host.py."""
import ctypes as C

import numpy as np
import pytest

import pair_cases as pc
from gpu_harness import FILL, Buf, LaunchLog, bits_equal, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from gpu_harness import lib as _lib, stream as _stream
from test_gpu_tile_pairs_pool import SMALL, small  # noqa: F401  (the fixture of the driver test)
from test_gpu_tile_pairs_validate import ANGLE_ATOL

pytestmark = pytest.mark.gpu

LOG = LaunchLog("hsr_pairs_last_launch", joined=True)
_call, _record = LOG.call, LOG.read
WORST = {}                       # bar -> largest error seen under it
ORDERS = ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0,), (1,), (2,))
F32, F64, I64, I32, U8 = np.float32, np.float64, np.int64, np.int32, np.uint8


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


def _close(got, ref, what, key, rtol, atol=0.0):
    """NaN in the same places, elsewhere |got - ref| <= atol + rtol |ref|; the largest error / bound goes to WORST[key]."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=f"{what}: NaN positions")
    ok = ~np.isnan(ref)
    if ok.any():
        err, bound = np.abs(got - ref)[ok], (atol + rtol * np.abs(ref))[ok]
        ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
        _note(key, ratio.max())
        assert (err <= bound).all(), (what, float(err.max()), float(ratio.max()))


def _positions(run):
    """run(order) -> dict of (len(order), ...) arrays.  The batch twice (identical bits), then every pair at every position of
    a batch of 3 and alone.  -> the batch's outputs."""
    base = run((0, 1, 2))
    again = run((0, 1, 2))
    for k in base:
        assert _same(base[k], again[k]), f"{k}: a second launch gave other bits"
    for order in ORDERS[1:]:
        got = run(order)
        for pos, i in enumerate(order):
            for k in base:
                assert _same(got[k][pos], base[k][i]), f"{k}: pair {i} at position {pos} of {order}"
    return base


def _in(torch, parts, stride, off=0):
    """The parts `stride` elements apart (sentinel gaps) in a Buf `off` bytes past a 256-byte boundary -> (Buf, host image)."""
    img = pc.pack(parts, stride)
    return Buf(torch, img.nbytes, off, img), img


def _unchanged(buf, img):
    assert _same(buf.get(img.dtype), img), "an input was written"


def _out(torch, count, stride, n, dtype, off):
    return Buf(torch, pc.span(count, stride, n) * np.dtype(dtype).itemsize, off)


def _take(buf, count, stride, n, dtype):
    return pc.unpack(buf.get(dtype), count, stride, n)


# =============================================================================================================================
# the record itself
# =============================================================================================================================
def test_record_lists_launches_in_order_and_keeps_the_last_32(torch_gpu):
    lib = _lib()
    row = pc.StatsRow(63, 1, "dyadic")
    npix = 255
    valid, train = pc.holdout_inputs(npix)
    vb, tb = Buf(torch_gpu, npix, 0, valid[0]), Buf(torch_gpu, npix, 0, train[0])
    mb, gb = Buf(torch_gpu, npix), Buf(torch_gpu, npix)
    lib.hsr_pairs_last_launch(None, 0)
    _stats_call(torch_gpu, row, (0,), check=False)
    for _ in range(3):
        assert lib.hsr_pair_holdout(vb.ptr, tb.ptr, npix, npix, mb.ptr, gb.ptr, 1, _stream(torch_gpu)) == 0
    assert lib.hsr_pair_holdout(vb.ptr, tb.ptr, npix, 0, mb.ptr, gb.ptr, 1, _stream(torch_gpu)) != 0      # refused: adds nothing
    buf = C.create_string_buffer(b"\x7f" * 64, 64)
    assert lib.hsr_pairs_last_launch(buf, 25) == 1                         # truncated to the capacity, NUL-terminated
    assert buf.raw[:25] == b"pair_stats_kernel; pair_holdout_kernel"[:24] + b"\0" and buf.raw[25] == 0x7f
    assert _record() is None
    _stats_call(torch_gpu, row, (0,), check=False)
    for _ in range(32):
        assert lib.hsr_pair_holdout(vb.ptr, tb.ptr, npix, npix, mb.ptr, gb.ptr, 1, _stream(torch_gpu)) == 0
    assert _record() == ["pair_holdout_kernel"] * 32                       # the oldest entry was dropped
    torch_gpu.cuda.synchronize()


# =============================================================================================================================
# prep
# =============================================================================================================================
def _prep_call(torch, row, order, refused=False, **over):
    r, n, o = row, len(order), list(order)
    emit, s2 = pc.prep_inputs(r)
    eb, eimg = _in(torch, [emit[i] for i in o], r.pair_emit)
    sb, simg = _in(torch, [s2[i] for i in o], r.pair_s2)
    bands = np.array(r.bands, I32)
    bb = Buf(torch, bands.nbytes, 0, bands)
    xb, yb, mb = Buf(torch, n * r.nb * r.npix * 4, 4), Buf(torch, n * r.T * r.npix * 4, 12), Buf(torch, n * r.npix, 1)
    a = dict(edt=r.edt, pair_emit=r.pair_emit, T=r.T, sdt=r.sdt, pair_s2=r.pair_s2, nb=r.nb, f=r.f, P=n)
    a.update(over)
    check = LOG.refused if refused else lambda *call: _call(pc.PREP_SEQ, *call)
    check(_lib().hsr_pair_prep, eb.ptr, pc.DT_CODE[a["edt"]], a["pair_emit"], r.B, bb.ptr, a["T"], sb.ptr, pc.DT_CODE[a["sdt"]],
          a["pair_s2"], a["nb"], r.H, r.W, a["f"], 0.0 if r.end is None else r.end, int(r.end is not None),
          0.0 if r.snd is None else r.snd, int(r.snd is not None), xb.ptr, yb.ptr, mb.ptr, a["P"], _stream(torch))
    out = dict(x=xb.get(F32).reshape(n, r.nb, r.npix), y=yb.get(F32).reshape(n, r.T, r.npix), mask=mb.get(U8).reshape(n, r.npix))
    _unchanged(eb, eimg)
    _unchanged(sb, simg)
    return out


@pytest.mark.parametrize("row", pc.PREP_ROWS, ids=lambda r: r.name)
def test_prep(torch_gpu, row):
    """x bit-equal to oracle_np.block_mean and NaN exactly on the blocks with a non-finite or nodata sample; y bit-equal to the
    decoded selection; the mask exact under the float32 closeness rule."""
    base = _positions(lambda order: _prep_call(torch_gpu, row, order))
    emit, s2 = pc.prep_inputs(row)
    for p in range(pc.P):
        x, y, mask = pc.prep_reference(row, emit[p], s2[p])
        bits_equal(base["x"][p], x, f"x of pair {p}")
        bits_equal(base["y"][p], y, f"y of pair {p}")
        np.testing.assert_array_equal(base["mask"][p], mask, err_msg=f"mask of pair {p}")


@pytest.mark.parametrize("case", pc.PREP_REFUSED, ids=lambda c: c[0])
def test_prep_refusals_launch_nothing(torch_gpu, case):
    out = _prep_call(torch_gpu, pc.PREP_REFUSED_BASE, (0, 1, 2), refused=True, **case[1])
    for k, v in out.items():
        assert (v.view(U8) == FILL).all(), k


# =============================================================================================================================
# stats
# =============================================================================================================================
def _stats_call(torch, row, order, check=True):
    n, o, nb, npix = len(order), list(order), row.nb, row.npix
    x, mask = pc.stats_inputs(row)
    xb, ximg = _in(torch, [x[o]], 1, 4)
    mb, mimg = _in(torch, [mask[o]], 1, 1)
    sb, meb, scb, ntb = (Buf(torch, n * k * 8, 8) for k in (1 + 2 * nb, nb, nb, 1))
    args = (xb.ptr, mb.ptr, npix, nb, sb.ptr, meb.ptr, scb.ptr, ntb.ptr, n, _stream(torch))
    if not check:
        assert _lib().hsr_pair_stats(*args) == 0
        return None
    _call(pc.STATS_SEQ, _lib().hsr_pair_stats, *args)
    out = dict(stats=sb.get(F64).reshape(n, -1), mean=meb.get(F64).reshape(n, nb), scale=scb.get(F64).reshape(n, nb), n_train=ntb.get(I64))
    _unchanged(xb, ximg)
    _unchanged(mb, mimg)
    return out


@pytest.mark.parametrize("row", pc.STATS_ROWS, ids=lambda r: r.name)
def test_stats(torch_gpu, row):
    """Counts exact; dyadic rows: mean == float64(exact sum) / n bit for bit, M2 within rtol 1e-12 of the longdouble two-pass
    value (a one-pass M2 is off by 1e-7 there, test_pair_instances_host.py) and == 0 exactly for one pixel or a constant band;
    random rows: mean / scale / M2 rtol 1e-12 (M2: n 2^-53 = 4.5e-13 at n = 4097 bounds a two-pass sum of squares)."""
    base = _positions(lambda order: _stats_call(torch_gpu, row, order))
    x, mask = pc.stats_inputs(row)
    nb = row.nb
    for p in range(pc.P):
        n, mean, m2, scale = pc.stats_reference(x[p], mask[p])
        st = base["stats"][p]
        assert base["n_train"][p] == n == st[0], (p, base["n_train"][p], n, st[0])
        assert _same(st[1:1 + nb], base["mean"][p])
        if n == 0:
            assert (st == 0).all() and (base["scale"][p] == 1).all()
            continue
        if row.kind == "dyadic":
            assert _same(base["mean"][p], pc.dyadic_mean(x[p], mask[p])), (p, base["mean"][p])
        else:
            _close(base["mean"][p], mean, "mean", "stats mean rtol 1e-12", 1e-12)
        zero = m2 == 0
        assert n > 1 or zero.all()
        assert (st[1 + nb:][zero] == 0).all() and (base["scale"][p][zero] == 1).all(), "M2 of one pixel / a constant band is not 0"
        _close(st[1 + nb:], m2, "M2", f"stats M2 {row.kind} rtol 1e-12", 1e-12)
        _close(base["scale"][p], scale, "scale", "stats scale rtol 1e-12", 1e-12)


# =============================================================================================================================
# report
# =============================================================================================================================
def _report_call(torch, row, order):
    r, n, o, s = row, len(order), list(order), row.strides()
    d = pc.report_inputs(r)
    ins = [_in(torch, [d[k][i] for i in o], st) for k, st in (("Q", s["pair_q"]), ("b64", s["pair_b"]), ("Bp", s["pair_bp"]),
                                                             ("y", s["pair_y"]), ("mask", s["pair_m"]), ("status", 1))]
    (qb, _), (bb, _), (pb, _), (yb, _), (mb, _), (sb, _) = ins
    wb = _out(torch, n, s["pair_work"], r.work, F64, 0)
    r2b, rmb = _out(torch, n, s["pair_out"], r.T, F64, 8), _out(torch, n, s["pair_out"], r.T, F64, 24)
    lib = _lib()
    assert lib.hsr_pair_report_work_bytes(r.npix, r.T) == r.work * 8
    _call(pc.REPORT_SEQ, lib.hsr_pair_report_f64, qb.ptr, s["ldq"], s["pair_q"], r.na, r.npix, bb.ptr, s["pair_b"], pb.ptr, s["ldbp"],
          s["pair_bp"], r.nf, yb.ptr, s["pair_y"], mb.ptr, s["pair_m"], r.T, sb.ptr, wb.ptr, s["pair_work"], r2b.ptr, rmb.ptr,
          s["pair_out"], n, _stream(torch))
    out = dict(r2=_take(r2b, n, s["pair_out"], r.T, F64), rmse=_take(rmb, n, s["pair_out"], r.T, F64))
    _take(wb, n, s["pair_work"], r.work, F64)                # the gaps of the workspace
    for b, img in ins:
        _unchanged(b, img)
    return out


@pytest.mark.parametrize("row", pc.REPORT_ROWS, ids=lambda r: r.name)
def test_report(torch_gpu, row):
    """The bars of test_report_kernel_on_exact_integer_data: r2 rtol 1e-12 atol 1e-6, rmse rtol 1e-6; NaN under a non-zero status."""
    base = _positions(lambda order: _report_call(torch_gpu, row, order))
    d = pc.report_inputs(row)
    for p in range(pc.P):
        r2, rmse = pc.report_expected(row, d, p)
        _close(base["r2"][p], r2, f"r2 of pair {p}", "report r2 rtol 1e-12 atol 1e-6", 1e-12, 1e-6)
        _close(base["rmse"][p], rmse, f"rmse of pair {p}", "report rmse rtol 1e-6", 1e-6)


# =============================================================================================================================
# holdout
# =============================================================================================================================
def _holdout_call(torch, npix, pad, order):
    n, o = len(order), list(order)
    valid, train = pc.holdout_inputs(npix)
    vb, vimg = _in(torch, [valid[o]], 1, 3)
    tb, timg = _in(torch, [train[i] for i in o], npix + pad, 1)
    mb, gb = Buf(torch, n * npix, 1), Buf(torch, n * npix, 2)
    _call(pc.HOLDOUT_SEQ, _lib().hsr_pair_holdout, vb.ptr, tb.ptr, npix + pad, npix, mb.ptr, gb.ptr, n, _stream(torch))
    out = dict(mask=mb.get(U8).reshape(n, npix), group=gb.get(U8).reshape(n, npix))
    _unchanged(vb, vimg)
    _unchanged(tb, timg)
    return out


@pytest.mark.parametrize("npix,pad", pc.HOLDOUT_ROWS)
def test_holdout(torch_gpu, npix, pad):
    base = _positions(lambda order: _holdout_call(torch_gpu, npix, pad, order))
    mask, group = pc.holdout_reference(*pc.holdout_inputs(npix))
    np.testing.assert_array_equal(base["mask"], mask)
    np.testing.assert_array_equal(base["group"], group)


# =============================================================================================================================
# score
# =============================================================================================================================
SCORE_FIELDS = (("n", I64), ("rmse", F64), ("r2", F64), ("mean_ref", F64))
SAM_FIELDS = (("sam", F64), ("n_sam", I64), ("ergas", F64))


def _score_call(torch, row, order, factor=6):
    r, n, o, lay = row, len(order), list(order), row.layout()
    T, npix = r.T, r.npix
    pred, y, group = pc.score_inputs(T, npix, r.groups)
    pb, pimg = _in(torch, [pred[i] for i in o], lay["pair_pred"], lay["off_pred"])
    yb, yimg = _in(torch, [y[i] for i in o], lay["pair_y"], lay["off_y"])
    gb, gimg = _in(torch, [group[i] for i in o], lay["pair_group"], lay["off_group"])
    pair_work, pair_out, pair_sam = r.work + 2, 2 * T + 3, 3
    lib = _lib()
    assert lib.hsr_pair_score_work_bytes(npix, T) == r.work * 8
    wb = _out(torch, n, pair_work, r.work, F64, 0)
    ob = {k: _out(torch, n, pair_out, 2 * T, dt, 8) for k, dt in SCORE_FIELDS}
    sb = {k: _out(torch, n, pair_sam, 2, dt, 8) for k, dt in SAM_FIELDS}
    mb = _out(torch, n, lay["pair_map"], npix, F32, lay["off_map"])
    _call(r.expect, lib.hsr_pair_score_f64, pb.ptr, lay["pair_pred"], yb.ptr, lay["pair_y"], gb.ptr, lay["pair_group"], npix, T,
          100.0 / factor, wb.ptr, pair_work, ob["n"].ptr, ob["rmse"].ptr, ob["r2"].ptr, ob["mean_ref"].ptr, pair_out, sb["sam"].ptr,
          sb["n_sam"].ptr, sb["ergas"].ptr, pair_sam, mb.ptr, lay["pair_map"], n, _stream(torch))
    out = {k: _take(ob[k], n, pair_out, 2 * T, dt).reshape(n, 2, T) for k, dt in SCORE_FIELDS}
    out.update({k: _take(sb[k], n, pair_sam, 2, dt) for k, dt in SAM_FIELDS})
    out["sam_map"] = _take(mb, n, lay["pair_map"], npix, F32)
    _take(wb, n, pair_work, r.work, F64)
    for b, img in ((pb, pimg), (yb, yimg), (gb, gimg)):
        _unchanged(b, img)
    return out


def _check_score(row, got):
    """The bars of test_score_kernel_on_exact_data, NaN-aware (an empty group has n = 0 and NaN statistics)."""
    pred, y, group = pc.score_inputs(row.T, row.npix, row.groups)
    for p in range(pc.P):
        ref = pc.score_reference(pred[p], y[p], group[p])
        np.testing.assert_array_equal(got["n"][p], ref["n"], err_msg=f"n of pair {p}")
        np.testing.assert_array_equal(got["n_sam"][p], ref["n_sam"], err_msg=f"n_sam of pair {p}")
        for k in ("rmse", "mean_ref", "ergas"):
            _close(got[k][p], ref[k], f"{k} of pair {p}", "score rmse / mean_ref / ergas rtol 1e-12", 1e-12)
        _close(got["r2"][p], ref["r2"], f"r2 of pair {p}", "score r2 rtol 1e-12 atol 1e-6", 1e-12, 1e-6)
        const = ref["m2"] == 0                               # M2 == 0 on the device too
        _close(got["r2"][p][const], (1.0 - ref["ss_res"] / 1e-8)[const], "r2 with M2 == 0", "score r2 (M2 == 0) rtol 1e-12", 1e-12)
        _close(got["sam"][p], ref["sam"], f"sam of pair {p}", "score sam atol 5e-6 deg", 0.0, ANGLE_ATOL)
        a32 = ref["angle"].astype(F32)
        np.testing.assert_array_equal(np.isnan(got["sam_map"][p]), np.isnan(ref["angle"]), err_msg=f"sam_map NaNs of pair {p}")
        ok = ~np.isnan(ref["angle"])
        err = np.abs(got["sam_map"][p].astype(F64) - ref["angle"])[ok]
        tol = (ANGLE_ATOL + np.spacing(np.abs(a32)).astype(F64))[ok]
        if ok.any():
            _note("score sam_map atol 5e-6 deg + 1 ulp", (err / tol).max())
            assert (err <= tol).all(), (p, float(err.max()))
        kind = row.groups[p]
        if kind == "zeros":
            assert not got["n"][p].any() and not got["n_sam"][p].any() and np.isnan(got["sam_map"][p]).all()
            assert all(np.isnan(got[k][p]).all() for k in ("rmse", "r2", "mean_ref", "sam", "ergas"))
        if kind == "lastlane":                               # the two-group walk ran: group 2 holds the chunks' last pixels
            held = np.arange(pc.LASTLANE_PIXEL, row.npix, pc.SCORE_PIX)
            np.testing.assert_array_equal(got["n"][p][1], np.isfinite(pred[p][:, held]).sum(axis=1))
            assert got["n"][p][1].max() == len(held) > 0 and np.isfinite(got["rmse"][p][1][got["n"][p][1] > 0]).all()


@pytest.mark.parametrize("row", pc.SCORE_ROWS, ids=lambda r: r.name)
def test_score(torch_gpu, row):
    _check_score(row, _positions(lambda order: _score_call(torch_gpu, row, order)))


def test_score_predicate_terms_one_by_one(torch_gpu):
    """Every term of hsr_pair_score_f64's predicate flipped alone records the plain instance and gives the bits of the 16-byte one."""
    assert pc.SCORE_BASE.vec
    base = _positions(lambda order: _score_call(torch_gpu, pc.SCORE_BASE, order))
    _check_score(pc.SCORE_BASE, base)
    for row in pc.SCORE_FLIP_ROWS:
        assert not row.vec
        got = _positions(lambda order: _score_call(torch_gpu, row, order))
        for k in base:
            assert _same(got[k], base[k]), (row.flip, k)


# =============================================================================================================================
# pool stats
# =============================================================================================================================
def _poisoned(torch, rows, off=0):
    """rows (n, k) float64 between two NaN rows (the rows -1 and n that a missing index guard would read) -> Buf, pointer to row 0."""
    k = rows.shape[1]
    img = np.concatenate([np.full((2, k), np.nan), rows, np.full((2, k), np.nan)]).reshape(-1)
    buf = Buf(torch, img.nbytes, off, img)
    return buf, C.c_void_p(buf.ptr.value + 2 * k * 8), img


def _pool_stats_call(torch, nb, stats, order, start, M):
    Pn, ls = len(stats), 1 + 2 * nb
    sb, sptr, simg = _poisoned(torch, np.asarray(stats))
    ob, tb = Buf(torch, order.nbytes, 0, order), Buf(torch, start.nbytes, 0, start)
    gs, npool, gm, gsc = (Buf(torch, M * k * 8, 8) for k in (ls, 1, nb, nb))
    pm, psc = Buf(torch, Pn * nb * 8, 8), Buf(torch, Pn * nb * 8, 24)
    _call(pc.POOL_STATS_SEQ, _lib().hsr_pool_stats, sptr, nb, Pn, ob.ptr, tb.ptr, M, gs.ptr, npool.ptr, gm.ptr, gsc.ptr, pm.ptr, psc.ptr,
          _stream(torch))
    out = dict(gstats=gs.get(F64).reshape(M, ls), n_pool=npool.get(I64), gmean=gm.get(F64).reshape(M, nb), gscale=gsc.get(F64).reshape(M, nb),
               pmean=pm.get(F64).reshape(Pn, nb), pscale=psc.get(F64).reshape(Pn, nb))
    _unchanged(sb, simg)
    return out


GROUP_KEYS = ("gstats", "n_pool", "gmean", "gscale")


def _check_pool_stats(nb, got, samples, members, untouched=()):
    for g, mem in enumerate(members):
        n, mean, m2, scale = pc.pool_stats_reference(samples, mem, nb)
        assert got["n_pool"][g] == n == got["gstats"][g, 0], (g, n)
        assert _same(got["gstats"][g, 1:1 + nb], got["gmean"][g])
        if n == 0:
            assert (got["gstats"][g] == 0).all() and (got["gmean"][g] == 0).all() and (got["gscale"][g] == 1).all(), g
        else:
            _close(got["gmean"][g], mean, f"mean of group {g}", "pool stats mean rtol 1e-12", 1e-12)
            _close(got["gstats"][g, 1 + nb:], m2, f"M2 of group {g}", "pool stats M2 rtol 1e-12", 1e-12)
            _close(got["gscale"][g], scale, f"scale of group {g}", "pool stats scale rtol 1e-12", 1e-12)
        for p in mem:                                        # every member's row, an empty member's too
            assert _same(got["pmean"][p], got["gmean"][g]) and _same(got["pscale"][p], got["gscale"][g]), (g, p)
    for p in untouched:
        assert (got["pmean"][p].view(U8) == FILL).all() and (got["pscale"][p].view(U8) == FILL).all(), p


@pytest.mark.parametrize("nb", [1, 16])
def test_pool_stats(torch_gpu, nb):
    """Group sizes 1, 3, 4, 5, 8, 9 and an all-empty group, empty members first / in the middle / last, against the longdouble
    statistics of the concatenation at rtol 1e-12; the singleton bit-equal to its member; a group alone and under other ids."""
    from s2_emit.pairs import pool_layout
    torch = torch_gpu
    ids = np.array(pc.pool_ids(), I32)
    order, start = pool_layout(ids)
    ro, rs = pc.pool_layout(ids)
    assert _same(order, ro) and _same(start, rs) and order.dtype == np.int32 and start.dtype == np.int32
    samples, stats = pc.pool_stats_inputs(nb)
    members = pc.pool_members()
    got = _pool_stats_call(torch, nb, stats, order, start, pc.POOL_M)
    again = _pool_stats_call(torch, nb, stats, order, start, pc.POOL_M)
    for k in got:
        assert _same(got[k], again[k]), k
    _check_pool_stats(nb, got, samples, members)
    one = members[0][0]
    m2_one = stats[one, 1 + nb:]
    assert _same(got["gstats"][0], stats[one]) and _same(got["gscale"][0], np.where(m2_one == 0, 1.0, np.sqrt(m2_one / stats[one, 0])))
    for g, mem in enumerate(members):                        # the group alone: the same bits
        alone = _pool_stats_call(torch, nb, stats[mem], np.arange(len(mem), dtype=I32), np.array([0, len(mem)], I32), 1)
        for k in GROUP_KEYS:
            assert _same(alone[k][0], got[k][g]), (g, k)
    shifted = (ids + 1) % pc.POOL_M                          # every group under the next id
    moved = _pool_stats_call(torch, nb, stats, *pool_layout(shifted), pc.POOL_M)
    for g in range(pc.POOL_M):
        for k in GROUP_KEYS:
            assert _same(moved[k][(g + 1) % pc.POOL_M], got[k][g]), (g, k)
    assert _same(moved["pmean"], got["pmean"]) and _same(moved["pscale"], got["pscale"])


@pytest.mark.parametrize("skip", pc.POOL_SKIPS, ids=lambda s: s[0])
def test_pool_stats_skips_bad_entries(torch_gpu, skip):
    """Indices outside [0, P) and slices outside [0, P] are skipped (the guards of pool_slice and of the member loops): the rows
    -1 and P of the statistics hold NaN, and the groups carry the bits of a clean layout in which the skipped pairs are empty."""
    nb = 16
    samples, stats = pc.pool_stats_inputs(nb)
    order, start, members, untouched = pc.pool_skip_layout(skip[1])
    got = _pool_stats_call(torch_gpu, nb, stats, order, start, pc.POOL_M)
    _check_pool_stats(nb, got, samples, members, untouched)
    emptied = np.array(stats)
    emptied[untouched] = 0.0
    clean = _pool_stats_call(torch_gpu, nb, emptied, *pc.pool_layout(pc.pool_ids()), pc.POOL_M)
    for k in GROUP_KEYS:
        assert _same(got[k], clean[k]), k


# =============================================================================================================================
# pool gram
# =============================================================================================================================
def _gram_call(torch, row, src, cnt, order, start, M):
    lay, n, Pn = row.layout(), row.n_elems, len(src)
    pair_g, group_out = lay["pair_g"], lay["group_out"]
    lead = 2 * pair_g                                        # an even count: the offset of pair 0 keeps the base's alignment
    img = np.concatenate([np.full(lead, np.nan), pc.pack(list(src), pair_g), np.full(lead, np.nan)])
    gb = Buf(torch, img.nbytes, lay["off_g"], img)
    counts = np.full((Pn, pc.GRAM_PAIR_COUNT), 9.0)
    counts[:, 0] = cnt
    cb, cptr, _ = _poisoned(torch, counts)
    ob, tb = Buf(torch, order.nbytes, 0, order), Buf(torch, start.nbytes, 0, start)
    out = _out(torch, M, group_out, n, F64, lay["off_out"])
    _call(row.expect, _lib().hsr_pool_gram, C.c_void_p(gb.ptr.value + lead * 8), pair_g, n, cptr, pc.GRAM_PAIR_COUNT, Pn, ob.ptr, tb.ptr,
          M, out.ptr, group_out, _stream(torch))
    got = _take(out, M, group_out, n, F64)
    _unchanged(gb, img)
    return got


def _gram_row(torch, row):
    src, cnt = pc.gram_inputs(row.n_elems)
    order, start = pc.pool_layout(pc.pool_ids())
    members = pc.pool_members()
    got = _gram_call(torch, row, src, cnt, order, start, pc.POOL_M)
    assert _same(got, _gram_call(torch, row, src, cnt, order, start, pc.POOL_M)), "a second launch gave other bits"
    np.testing.assert_array_equal(got, pc.gram_reference(src, cnt, members))
    assert _same(got[0], src[members[0][0]]), "the singleton group is not a copy of its member"     # -0.0 included
    assert (got[pc.POOL_M - 1] == 0).all()
    return got


@pytest.mark.parametrize("row", pc.GRAM_ROWS, ids=lambda r: r.name)
def test_pool_gram(torch_gpu, row):
    """Exact on integers for group sizes 1, 3, 4, 5, 8, 9 (the four-ahead member loop: one trip, a trip and one member, two trips,
    two trips and one member) with empty members first / in the middle / last; a group alone carries the same bits."""
    got = _gram_row(torch_gpu, row)
    src, cnt = pc.gram_inputs(row.n_elems)
    for g, mem in enumerate(pc.pool_members()):
        alone = _gram_call(torch_gpu, row, src[mem], cnt[mem], np.arange(len(mem), dtype=I32), np.array([0, len(mem)], I32), 1)
        assert _same(alone[0], got[g]), g


def test_pool_gram_predicate_terms_one_by_one(torch_gpu):
    """Every term of hsr_pool_gram's predicate flipped alone records the plain instance; the four that leave the problem as it is
    give the bits of the 16-byte instance."""
    assert pc.GRAM_BASE.expect == ["pool_gram_kernel<true>"]
    base = _gram_row(torch_gpu, pc.GRAM_BASE)
    for row in pc.GRAM_FLIP_ROWS:
        assert row.expect == ["pool_gram_kernel<false>"]
        got = _gram_row(torch_gpu, row)
        if row.n_elems == pc.GRAM_BASE.n_elems:
            assert _same(got, base), row.flip


@pytest.mark.parametrize("skip", pc.POOL_SKIPS, ids=lambda s: s[0])
@pytest.mark.parametrize("row", [pc.GRAM_BASE, pc.GRAM_FLIP_ROWS[2]], ids=lambda r: r.name)
def test_pool_gram_skips_bad_entries(torch_gpu, row, skip):
    """As for the statistics: the pairs -1 and P of the Grams and of the counts hold NaN and are never read."""
    src, cnt = pc.gram_inputs(row.n_elems)
    order, start, members, untouched = pc.pool_skip_layout(skip[1])
    got = _gram_call(torch_gpu, row, src, cnt, order, start, pc.POOL_M)
    np.testing.assert_array_equal(got, pc.gram_reference(src, cnt, members))


# =============================================================================================================================
# pool models
# =============================================================================================================================
def _models_call(torch, row, perm):
    r, M, Pn = row, pc.MODELS_M, len(perm)
    g = pc.models_inputs(r)
    ins = dict(bp=_in(torch, list(g["bp"]), r.group_bp), b64=_in(torch, [g["b64"]], 1), w32=_in(torch, list(g["w32"]), r.group_w32, 4),
               b32=_in(torch, [g["b32"]], 1, 4), mean32=_in(torch, [g["mean32"]], 1, 4), inv32=_in(torch, [g["inv32"]], 1, 4),
               status=_in(torch, [np.array(pc.MODELS_POOL_STATUS, I32)], 1), n_train=_in(torch, [np.array(pc.MODELS_N_TRAIN, I64)[list(perm)]], 1),
               group_of=_in(torch, [np.array(pc.MODELS_GROUP_OF, I32)[list(perm)]], 1))
    sizes = dict(bp=(r.npad * r.T, F64), b64=(r.T, F64), w32=(r.kpad * r.T, F32), b32=(r.T, F32), mean32=(r.nb, F32), inv32=(r.nb, F32),
                 status=(1, I32), report_status=(1, I32))
    outs = {k: Buf(torch, Pn * n * np.dtype(dt).itemsize, 8) for k, (n, dt) in sizes.items()}
    i, o = {k: v[0].ptr for k, v in ins.items()}, {k: v.ptr for k, v in outs.items()}
    _call(pc.POOL_MODELS_SEQ, _lib().hsr_pool_models, i["bp"], r.group_bp, i["b64"], i["w32"], r.group_w32, i["b32"], i["mean32"], i["inv32"],
          i["status"], i["n_train"], i["group_of"], r.nf, r.npad, r.kpad, r.T, r.nb, o["bp"], o["b64"], o["w32"], o["b32"], o["mean32"],
          o["inv32"], o["status"], o["report_status"], Pn, M, _stream(torch))
    got = {k: outs[k].get(dt).reshape(Pn, n) for k, (n, dt) in sizes.items()}
    for b, img in ins.values():
        _unchanged(b, img)
    return got


@pytest.mark.parametrize("row", pc.MODELS_ROWS, ids=lambda r: r.name)
def test_pool_models(torch_gpu, row):
    """Every copy bit-exact, rows nf .. npad of Bp zero, the two status words; a pair whose group is outside [0, M) keeps the
    sentinel in all its outputs.  One block (total < 1024), two, and the 64-block cap with its stride loop (npad 288, T 285)."""
    assert pc.pool_models_blocks(row.npad, row.kpad, row.T, row.nb) in (1, 2, 64)
    g = pc.models_inputs(row)
    ident = tuple(range(pc.MODELS_P))
    got = _models_call(torch_gpu, row, ident)
    again = _models_call(torch_gpu, row, ident)
    perm = (4, 2, 0, 3, 1)
    moved = _models_call(torch_gpu, row, perm)
    for k in got:
        assert _same(got[k], again[k]), k
        assert _same(moved[k], got[k][list(perm)]), k
    for p, grp in enumerate(pc.MODELS_GROUP_OF):
        if not 0 <= grp < pc.MODELS_M:
            assert all((got[k][p].view(U8) == FILL).all() for k in got), p
            continue
        want = pc.models_expected(row, g, grp)
        for k in pc.MODELS_FIELDS:
            assert _same(got[k][p], want[k]), (p, k)
        assert (got["bp"][p].reshape(row.npad, row.T)[row.nf:] == 0).all()
        assert (int(got["status"][p, 0]), int(got["report_status"][p, 0])) == pc.models_status(grp, pc.MODELS_N_TRAIN[p]), p


# =============================================================================================================================
# the driver
# =============================================================================================================================
def _driver_calls(emit, s2):
    from oracle import oracle_np as onp
    coarse = np.stack([onp.block_mean(s, SMALL["factor"]) for s in s2])
    tm = np.ones((len(emit),) + emit.shape[2:], bool)
    tm[:, ::2, 1::2] = False
    return {"plain": {}, "report": dict(report=True), "train_mask+validate": dict(train_mask=tm, validate=True),
            "pool": dict(pool=[0, 1, 0, 1, 2]), "s2_coarse": dict(s2_coarse=coarse)}


@pytest.mark.parametrize("side", [False, True], ids=["default stream", "side stream"])
def test_driver_records_what_pairs_py_launches(torch_gpu, small, side):
    """fuse_tile_pairs on the small geometry: the record after the call is the list read off s2_emit/pairs.py - no pool kernel
    without pool=, no hold-out kernel without train_mask=, two score launches per view - on the default and on a side stream."""
    import s2_emit
    torch = torch_gpu
    emit, s2 = small
    calls = _driver_calls(emit, s2)
    assert set(calls) == set(pc.DRIVER_RECORDS)
    stream = torch.cuda.Stream() if side else torch.cuda.current_stream()
    stream.wait_stream(torch.cuda.current_stream())
    for name, kw in calls.items():
        _lib().hsr_pairs_last_launch(None, 0)
        with torch.cuda.stream(stream):
            out = s2_emit.fuse_tile_pairs(emit, s2, **kw, **SMALL)
        stream.synchronize()
        got = _record()
        assert got == pc.DRIVER_RECORDS[name], (name, got)
        assert (out.status.cpu().numpy() == 0).all(), name
        LOG.seen.update(got)


# =============================================================================================================================
# closing
# =============================================================================================================================
def test_rows_reached_every_instance():
    lib = _lib()
    table = [lib.hsr_pairs_instance_name(i).decode() for i in range(lib.hsr_pairs_instance_count())]
    assert table == list(pc.NAMES) and len(set(table)) == pc.INSTANCE_COUNT
    assert LOG.seen == set(table), sorted(set(table) - LOG.seen)
    for key in sorted(WORST):
        print(f"largest error / bound under [{key}]: {WORST[key]:.3e}")
