"""Every kernel instance of the histogram-matching family (include/hsr_hist.h) on an MI355X, each stage on its own so that a sort bug
and a lookup bug cannot hide each other:

    keys     against hist_cases.key_of and the counts, both layouts, strides of their own;
    sort     against np.sort of the keys: every npix at which the code takes another path, every key pattern and sentinel share, 2, 6
             and 32 planes in one call, a plane stride that is no multiple of anything;
    lookup   on planes that NumPy sorted, against the statement of hist_cases by value and against the host twin bit for bit: ties on
             either side, constants, the clamps, n round the pivot, runs across pivots, both layouts.

Every buffer is a gpu_harness.Buf (guard zones checked, inputs compared after the call); every call goes through LaunchLog, and the
last test checks that every name of the instance table was recorded."""
import ctypes as C

import numpy as np
import pytest

import hist_cases as hc
from gpu_harness import FILL, SENT32, Buf, LaunchLog, lib, stream, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from test_hist_host import host_match

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
LOG = LaunchLog("hsr_hist_last_launch", joined=True)


def _unchanged(buf, arr, what):
    raw = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
    assert np.array_equal(buf.get(np.uint8)[:raw.size], raw), f"{what} was written to"


# ---- keys ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planar", (False, True))
@pytest.mark.parametrize("npix, Cn", [(1, 1), (255, 3), (257, 16), (1000, 5)])
def test_keys(torch_gpu, planar, npix, Cn):
    torch, L = torch_gpu, lib()
    rng = np.random.default_rng(npix + Cn)
    src = (rng.random((Cn, npix)) * 4 - 2).astype(np.float32)
    ref = rng.random((Cn, npix)).astype(np.float32)
    src[0, ::7], ref[Cn - 1, 3::11] = np.nan, np.inf
    src[Cn // 2, 1::13] = -0.0
    mask = (rng.random(npix) < 0.7).astype(np.uint8) * np.uint8(1 + npix % 3)          # any nonzero byte is inside
    pad = 3
    if planar:
        cs, ps, shape = npix + pad, 1, (Cn, npix + pad)
        lay = lambda a: np.concatenate([a, np.full((Cn, pad), -7, np.float32)], axis=1)  # noqa: E731
    else:
        cs, ps, shape = 1, Cn + pad, (npix, Cn + pad)
        lay = lambda a: np.concatenate([a.T, np.full((npix, pad), -7, np.float32)], axis=1)  # noqa: E731
    s, r = lay(src), lay(ref)
    assert s.shape == shape
    bs, br, bm = Buf(torch, s.nbytes, 4, s), Buf(torch, r.nbytes, 0, r), Buf(torch, npix, 1, mask)
    stride = npix + 9
    bk, bn = Buf(torch, ((2 * Cn - 1) * stride + npix) * 4, 4), Buf(torch, 8 * Cn, 8)
    LOG.call([f"hist_keys_kernel<{hc.layout_name(planar)}>"], L.hsr_hist_keys, bs.ptr, cs, ps, br.ptr, cs, ps, bm.ptr, npix, Cn, bk.ptr, stride,
             bn.ptr, stream(torch))
    valid = (mask != 0)[None] & np.isfinite(src) & np.isfinite(ref)
    got = np.concatenate([bk.get(np.uint32), np.full(stride - npix, SENT32, np.uint32)]).reshape(2 * Cn, stride)
    assert (got[:, npix:] == SENT32).all(), "write between two key planes"
    want = np.concatenate([np.where(valid, hc.key_of(src), hc.SENTINEL), np.where(valid, hc.key_of(ref), hc.SENTINEL)])
    assert np.array_equal(got[:, :npix], want)
    assert np.array_equal(bn.get(np.int64), valid.sum(axis=1))
    _unchanged(bs, s, "src"), _unchanged(br, r, "ref"), _unchanged(bm, mask, "mask")


# ---- sort ---------------------------------------------------------------------------------------------------------------------------------
COMBOS = [(p, s) for p in hc.SORT_PATTERNS for s in hc.SENTINEL_SHARES]
assert len(COMBOS) == 40


@pytest.mark.parametrize("npix", hc.SORT_NPIX)
def test_sort_equals_np_sort(torch_gpu, npix):
    """40 (pattern, sentinel share) planes per npix, as calls of 32, 6 and 2 planes (C = 16, 3, 1)."""
    torch, L = torch_gpu, lib()
    stride = npix + 5
    at = 0
    for P in (32, 6, 2):
        planes = np.stack([hc.sort_keys(pat, npix, j, share) for j, (pat, share) in enumerate(COMBOS[at: at + P])])
        at += P
        laid = np.full((P, stride), SENT32, np.uint32)
        laid[:, :npix] = planes
        nbytes = ((P - 1) * stride + npix) * 4
        bk, bt = Buf(torch, nbytes, 0, laid.reshape(-1)[: nbytes // 4]), Buf(torch, nbytes, 4)
        cbytes = L.hsr_hist_sort_bytes(npix, P)
        assert cbytes == P * 256 * -(-npix // hc.TILE) * 4
        bc = Buf(torch, cbytes)
        LOG.call(hc.sort_record(), L.hsr_hist_sort, bk.ptr, bt.ptr, stride, npix, P, bc.ptr, cbytes, stream(torch))
        got = np.concatenate([bk.get(np.uint32), np.full(stride - npix, SENT32, np.uint32)]).reshape(P, stride)
        bt.get(np.uint32), bc.get(np.uint32)                # guard zones
        assert (got[:, npix:] == SENT32).all(), "write between two planes"
        want = np.sort(planes, axis=1)
        bad = np.flatnonzero((got[:, :npix] != want).any(axis=1))
        assert not len(bad), f"npix={npix} P={P}: planes {[COMBOS[at - P + b] for b in bad]} are not sorted"
    assert at == len(COMBOS)


@pytest.mark.parametrize("which", (0, 1, 2, 3))
def test_sort_pass_is_stable(torch_gpu, which):
    """One pass alone: ascending in its digit, keys of equal digit in their order of arrival (a stable argsort of the digit)."""
    torch, L = torch_gpu, lib()
    npix, P = 2 * hc.TILE + 3, 3
    rng = np.random.default_rng(which)
    planes = np.stack([rng.integers(0, 1 << 32, npix, dtype=np.uint64).astype(np.uint32),
                       (rng.integers(0, 3, npix).astype(np.uint32) << np.uint32(8 * which)) | rng.integers(0, 1 << 8, npix).astype(np.uint32) << np.uint32(8 * ((which + 1) % 4)),
                       hc.sort_keys("specials", npix, 0, "half")]).astype(np.uint32)
    bi, bo = Buf(torch, planes.nbytes, 0, planes), Buf(torch, planes.nbytes, 4)
    cbytes = L.hsr_hist_sort_bytes(npix, P)
    bc = Buf(torch, cbytes)
    LOG.call([f"hist_count_kernel<{which}>", "hist_scan_kernel", f"hist_scatter_kernel<{which}>"], L.hsr_hist_sort_pass, bi.ptr, bo.ptr, npix, npix,
             P, which, bc.ptr, cbytes, stream(torch))
    got = bo.get(np.uint32).reshape(P, npix)
    _unchanged(bi, planes, "the input planes")
    for p in range(P):
        order = np.argsort((planes[p] >> np.uint32(8 * which)) & np.uint32(255), kind="stable")
        assert np.array_equal(got[p], planes[p][order]), f"plane {p}"


# ---- lookup -------------------------------------------------------------------------------------------------------------------------------
def _lookup_inputs(rows, extra, seed):
    """rows: [(src, ref)] of n valid pixels each (one n for all) -> (src, ref (C, npix), mask (npix,)): the valid pixels at common
    places among `extra` others that are masked out or hold a non-finite sample in some channels."""
    rng = np.random.default_rng(seed)
    n, Cn = len(rows[0][0]), len(rows)
    npix = n + extra
    at = np.sort(rng.permutation(npix)[:n])
    rest = np.setdiff1d(np.arange(npix), at)
    src = (rng.random((Cn, npix)) * 3 - 1).astype(np.float32)
    ref = rng.random((Cn, npix)).astype(np.float32)
    mask = np.zeros(npix, np.uint8)
    mask[at] = 1
    for c, (s, r) in enumerate(rows):
        src[c, at], ref[c, at] = s, r
    for j, i in enumerate(rest):
        if j % 3 == 0:
            mask[i] = 1
            src[:, i] = (np.nan, np.inf, -np.inf)[j % 9 // 3]
        elif j % 3 == 1:
            mask[i] = 1
            ref[:, i] = (np.nan, -np.inf, np.inf)[j % 9 // 3]
    return src, ref, mask


def _sorted_planes(src, ref, mask, stride):
    """What keys + sort leave, made by NumPy: per plane the valid keys ascending, then sentinels; the counts."""
    valid = (mask != 0)[None] & np.isfinite(src) & np.isfinite(ref)
    planes = np.full((2 * len(src), stride), SENT32, np.uint32)          # the stride's padding: never read, never written
    for c in range(len(src)):
        for p, img in ((c, src), (len(src) + c, ref)):
            k = np.where(valid[c], hc.key_of(img[c]), hc.SENTINEL)
            planes[p, : src.shape[1]] = np.sort(k)
    return planes, valid.sum(axis=1).astype(np.int64)


def _run_lookup(torch, src, ref, mask, planar, what):
    L = lib()
    Cn, npix = src.shape
    stride = npix + 3
    planes, counts = _sorted_planes(src, ref, mask, stride)
    nbytes = ((2 * Cn - 1) * stride + npix) * 4
    bk, bn = Buf(torch, nbytes, 0, planes.reshape(-1)[: nbytes // 4]), Buf(torch, 8 * Cn, 8, counts)
    pbytes = L.hsr_hist_pivot_bytes(npix, Cn)
    bp = Buf(torch, pbytes, 4)
    pad = 2
    if planar:
        cs, ps = npix + pad, 1
        lay = lambda a: np.concatenate([a, np.full((Cn, pad), -7, np.float32)], axis=1)  # noqa: E731
        unlay = lambda o: o.reshape(Cn, npix + pad)[:, :npix]  # noqa: E731
        gap = lambda o: o.reshape(Cn, npix + pad)[:, npix:]  # noqa: E731
    else:
        cs, ps = 1, Cn + pad
        lay = lambda a: np.concatenate([a.T, np.full((npix, pad), -7, np.float32)], axis=1)  # noqa: E731
        unlay = lambda o: o.reshape(npix, Cn + pad)[:, :Cn].T  # noqa: E731
        gap = lambda o: o.reshape(npix, Cn + pad)[:, Cn:]  # noqa: E731
    s, r = lay(src), lay(ref)
    bs, br, bm, bo = Buf(torch, s.nbytes, 0, s), Buf(torch, r.nbytes, 4, r), Buf(torch, npix, 3, mask), Buf(torch, s.nbytes, 4)
    LOG.call(["hist_pivots_kernel", f"hist_lookup_kernel<{hc.layout_name(planar)}>"], L.hsr_hist_lookup, bk.ptr, stride, bn.ptr, bp.ptr,
             pbytes, bs.ptr, cs, ps, br.ptr, cs, ps, bm.ptr, npix, Cn, bo.ptr, cs, ps, stream(torch))
    o = bo.get(np.uint32)
    assert (gap(o) == SENT32).all(), f"{what}: write into the stride's padding"
    got = np.ascontiguousarray(unlay(o)).view(np.float32)
    bp.get(np.uint32)
    _unchanged(bk, planes.reshape(-1)[: nbytes // 4], "sorted planes"), _unchanged(bn, counts, "counts")
    _unchanged(bs, s, "src"), _unchanged(br, r, "ref"), _unchanged(bm, mask, "mask")
    want, n = hc.match_planes(src, ref, mask != 0)
    assert np.array_equal(n, counts)
    hc.equal_by_value(got, want, what)
    twin, _ = host_match(src, ref, mask, True)
    gn = np.isnan(got)
    assert np.array_equal(gn, np.isnan(twin)) and np.array_equal(got.view(np.uint32)[~gn], twin.view(np.uint32)[~gn]), f"{what}: not the host twin's bits"
    return got


@pytest.mark.parametrize("planar", (False, True))
@pytest.mark.parametrize("n", hc.LOOKUP_N)
def test_lookup_rows(torch_gpu, planar, n):
    """The ten lookup rows as ten channels of one call, n valid pixels each among 13 that are not."""
    rows = [hc.lookup_case(name, n) for name in hc.LOOKUP_CASES]
    src, ref, mask = _lookup_inputs(rows, 13, n)
    _run_lookup(torch_gpu, src, ref, mask, planar, f"n={n}")


@pytest.mark.parametrize("planar", (False, True))
@pytest.mark.parametrize("n, runs", [(3 * hc.PIVOT + 9, ((hc.PIVOT - 3, 7), (2 * hc.PIVOT - 40, 300))),
                                     (hc.PIVOT ** 2 + 500, ((hc.PIVOT - 1, 2), (1000, 5 * hc.PIVOT + 3), (hc.PIVOT ** 2 - 5, 400)))])
def test_lookup_runs_across_pivots(torch_gpu, planar, n, runs):
    """A run that crosses one pivot and runs that span several; one table level, and two with a top level of 2 entries.  The second
    channel swaps the roles: ties in S."""
    s, r = hc.pivot_run_case(n, runs)
    src, ref, mask = _lookup_inputs([(s, r), (r, s)], 1500, n)            # more than one workgroup of 1024 pixels
    _run_lookup(torch_gpu, src, ref, mask, planar, f"n={n}")


def test_lookup_counts_out_of_range_are_read_as_npix(torch_gpu):
    """A count the caller corrupted cannot index outside a plane: it is read as npix."""
    torch, L = torch_gpu, lib()
    npix = 300
    rng = np.random.default_rng(5)
    src, ref = rng.random((1, npix)).astype(np.float32), rng.random((1, npix)).astype(np.float32)
    mask = np.ones(npix, np.uint8)
    planes, _ = _sorted_planes(src, ref, mask, npix)
    want, _ = hc.match_planes(src, ref, mask != 0)
    for bad in (-1, npix + 1, 2 ** 40):
        bk, bn = Buf(torch, planes.nbytes, 0, planes), Buf(torch, 8, 0, np.array([bad], np.int64))
        pbytes = L.hsr_hist_pivot_bytes(npix, 1)
        bp, bs, br, bm, bo = Buf(torch, pbytes), Buf(torch, 4 * npix, 0, src), Buf(torch, 4 * npix, 0, ref), Buf(torch, npix, 0, mask), Buf(torch, 4 * npix)
        LOG.call(["hist_pivots_kernel", "hist_lookup_kernel<PLANAR>"], L.hsr_hist_lookup, bk.ptr, npix, bn.ptr, bp.ptr, pbytes, bs.ptr, npix, 1,
                 br.ptr, npix, 1, bm.ptr, npix, 1, bo.ptr, npix, 1, stream(torch))
        hc.equal_by_value(bo.get(np.float32).reshape(1, npix), want, f"count {bad}")
        bp.get(np.uint32)


def test_lookup_three_table_levels(torch_gpu):
    """n just above 256^3 - the least size at which the pivot tables have three levels, as at 6144 x 6144 - on planes whose ranks are
    known in closed form: S is a ramp of consecutive float32 keys from 0.25 on, so the pixel that holds S[i] has cs = i + 1; R is a
    ramp in runs of seven equal keys, so a = R[i] has lo = 7 (i // 7) and hi = min(lo + 7, n).  Every pixel is checked."""
    import math
    torch, L = torch_gpu, lib()
    n = hc.PIVOT ** 3 + 300
    step = 7919
    assert math.gcd(step, n) == 1 and L.hsr_hist_pivot_bytes(n, 1) > 2 * 4 * (n // hc.PIVOT + n // hc.PIVOT ** 2 + 1)
    i = (np.arange(n, dtype=np.int64) * step) % n                        # the rank of pixel j in S: a bijection
    s_keys = (np.uint32(hc.key_of(np.float32(0.25))[0]) + np.arange(n, dtype=np.uint32)).astype(np.uint32)
    r_keys = (np.uint32(hc.key_of(np.float32(0.125))[0]) + (np.arange(n, dtype=np.uint32) // np.uint32(7)) * np.uint32(3)).astype(np.uint32)
    Sv, Rv = hc.value_of(s_keys), hc.value_of(r_keys)
    assert Sv[-1] > 1.0 and np.isfinite(Sv).all() and np.isfinite(Rv).all()
    src = Sv[i]
    ref = np.full(n, 0.5, np.float32)                                    # read for its finiteness alone
    mask = np.ones(n, np.uint8)
    planes = np.stack([s_keys, r_keys])
    bk, bn = Buf(torch, planes.nbytes, 0, planes), Buf(torch, 8, 0, np.array([n], np.int64))
    pbytes = L.hsr_hist_pivot_bytes(n, 1)
    bp, bs, br, bm, bo = Buf(torch, pbytes), Buf(torch, 4 * n, 0, src), Buf(torch, 4 * n, 0, ref), Buf(torch, n, 0, mask), Buf(torch, 4 * n)
    LOG.call(["hist_pivots_kernel", "hist_lookup_kernel<PLANAR>"], L.hsr_hist_lookup, bk.ptr, n, bn.ptr, bp.ptr, pbytes, bs.ptr, n, 1,
             br.ptr, n, 1, bm.ptr, n, 1, bo.ptr, n, 1, stream(torch))
    got = bo.get(np.float32)
    bp.get(np.uint32)
    cs, lo = i + 1, 7 * (i // 7)
    hi = np.minimum(lo + 7, n)
    a, b, nn = Rv[i].astype(np.float64), Rv[np.maximum(lo, 1) - 1].astype(np.float64), np.float64(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        res = ((a - b) / (hi / nn - lo / nn)) * (cs / nn - lo / nn) + b
    want = np.clip(np.where((hi == cs) | (lo == 0), a, res).astype(np.float32), 0, 1)
    assert ((hi != cs) & (lo != 0)).mean() > 0.8                          # most pixels interpolate
    hc.equal_by_value(got, want, "three levels")


def test_refusals_leave_no_record(torch_gpu):
    torch, L = torch_gpu, lib()
    b = Buf(torch, 4096)
    LOG.refused(L.hsr_hist_sort, b.ptr, b.ptr, 16, 16, 1, b.ptr, 4096, stream(torch))
    LOG.refused(L.hsr_hist_keys, b.ptr, 1, 3, None, 1, 3, b.ptr, 16, 3, b.ptr, 16, b.ptr, stream(torch))
    assert (b.get(np.uint8) == FILL).all()


def test_every_instance_was_launched():
    assert LOG.seen == set(hc.all_instances()), sorted(set(hc.all_instances()) ^ LOG.seen)
    L = lib()
    assert [L.hsr_hist_instance_name(i).decode() for i in range(L.hsr_hist_instance_count())] == hc.all_instances()
