"""The fixed-order sums of csrc/hsr_tree_dev.h, pinned bit for bit against the documented tree written out in NumPy
(slot_tree, thread_sums and wave_tree of gpu_harness.py) - never against another kernel of the library:
  * the workgroup join (block_join4) behind hsr_poly_moments, hsr_poly_moments_f64, hsr_affine_moments, hsr_affine_moments_f64
    and hsr_ridge_stats: every partial slot (for the ridge statistics the [n, mean.., M2..] that the finish kernel derives from
    the blocks' partial sums) equals the per-thread sums in pixel order, the xor butterfly over each wave, then
    ((w0 + w1) + w2) + w3;
  * the slot reduction of hsr_affine_reduce_solve (lane_slot_sum + butterfly_tree64) on hand-made partials.
The per-thread sums can be restated exactly because the library is built without contraction: every product and every add is
rounded on its own.  Inputs carry mixed exponents (values times 2^k, k in -20..20), so that any other order of the adds changes
bits; some pixels are masked and some are not finite.  (The slot reductions of hsr_poly.hip are pinned the same way in
test_gpu_poly_instances.py.)"""
import ctypes as C

import numpy as np
import pytest

import affine_cases as ac
from gpu_harness import Buf, butterfly64, same_bits, slot_tree, thread_sums, torch_gpu, wave_tree  # noqa: F401  (torch_gpu: the fixture)
from gpu_harness import lib as _lib, stream as _stream

pytestmark = pytest.mark.gpu


def _mixed(rng, shape, lo=0.1, hi=1.0, kmax=20):
    """float64 values in +-[lo, hi) times 2^k, k in -kmax..kmax."""
    return rng.uniform(lo, hi, shape) * rng.choice([-1.0, 1.0], shape) * np.exp2(rng.integers(-kmax, kmax + 1, shape))


def _strided(first, count, step=256):
    """owned[pass][t] of a thread that takes the items first[t], first[t] + step, ... below count."""
    passes = max(1, -(-count // step))
    own = first[None, :] + step * np.arange(passes)[:, None]
    return np.where(own < count, own, -1)


# ---- 1. workgroup join, poly -------------------------------------------------------------------------------------------------------------
def _poly_terms(xd, yd, deg):
    """moment_add's terms per pixel, in the order of the accumulators: 1, pw_1 .. pw_2deg, y, pw_1 y .. pw_deg y (pw *= x step by step)."""
    t = np.empty((len(xd), 3 * deg + 2))
    t[:, 0] = 1.0
    t[:, 2 * deg + 1] = yd
    pw = np.ones_like(xd)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(1, 2 * deg + 1):
            pw = pw * xd
            t[:, k] = pw
            if k <= deg:
                t[:, 2 * deg + 1 + k] = pw * yd
    return t


def _poly_slots_ref(x, y, ok, deg, slots):
    """x, y (npix,) float64, ok (npix,) -> (slots, M): contiguous ranges of ceil(npix / slots) pixels, thread t takes t, t + 256, ..."""
    npix = len(x)
    per = -(-npix // slots)
    terms = _poly_terms(x, y, deg)
    ref = np.zeros((slots, terms.shape[1]))
    for s in range(slots):
        beg, end = min(s * per, npix), min(s * per + per, npix)
        ref[s] = wave_tree(thread_sums(terms[beg:end], ok[beg:end], _strided(np.arange(256), end - beg)))
    return ref


# 512 slots (the cap) of more than 256 pixels: all four waves hold data and a thread owns more than one pixel.  131 073 is the
# smallest such npix (257 per slot: thread 0 alone owns two, the last slots are ragged or empty); 153 523 gives slots of 300.
POLY_NPIX = (512 * 256 + 1, 512 * 300 - 77)


@pytest.mark.parametrize("npix", POLY_NPIX)
@pytest.mark.parametrize("deg", [1, 4])
def test_poly_moments_slots_follow_the_tree(torch_gpu, deg, npix):
    torch = torch_gpu
    rng = np.random.default_rng(100 * deg + npix % 89)
    nb, M = 2, 3 * deg + 2
    kmax = 20 if deg == 1 else 12                                     # x^8: keep every power far inside float64's range
    x = _mixed(rng, (nb, npix), kmax=kmax).astype(np.float32)
    y = _mixed(rng, (nb, npix)).astype(np.float32)
    x[0, ::97], y[1, 5::211], x[1, 7::1009] = np.nan, np.inf, -np.inf
    mask = (rng.random(npix) < 0.8).astype(np.uint8)
    min_x, min_y = np.float32(-0.25), np.float32(-1.0)                # values at or below are excluded
    xd, yd, md = (torch.from_numpy(a.reshape(-1)).cuda() for a in (x, y, mask))
    part = torch.full((512 * nb * M,), np.nan, dtype=torch.float64, device="cuda")
    slots = C.c_int32(-1)
    rc = _lib().hsr_poly_moments(xd.data_ptr(), npix, 1, yd.data_ptr(), npix, 1, md.data_ptr(), npix, nb, deg, C.c_float(min_x),
                                 C.c_float(min_y), None, None, part.data_ptr(), C.byref(slots), _stream(torch))
    assert rc == 0 and slots.value == 512, (rc, _lib().hsr_last_error())
    torch.cuda.synchronize()
    got = part.cpu().numpy().reshape(512, nb, M)
    for b in range(nb):
        ok = (mask != 0) & np.isfinite(x[b]) & np.isfinite(y[b]) & (x[b] > min_x) & (y[b] > min_y)
        assert 0.3 * npix < ok.sum() < 0.6 * npix
        same_bits(got[:, b], _poly_slots_ref(x[b].astype(np.float64), y[b].astype(np.float64), ok, deg, 512), f"deg {deg} band {b}")


@pytest.mark.parametrize("npix", POLY_NPIX)
@pytest.mark.parametrize("deg", [1, 4])
def test_poly_moments_f64_slots_follow_the_tree(torch_gpu, deg, npix):
    torch = torch_gpu
    rng = np.random.default_rng(200 * deg + npix % 89)
    nb, M, stride = 2, 3 * deg + 2, npix + 3
    x, y = _mixed(rng, (nb, stride), kmax=20 if deg == 1 else 12), _mixed(rng, (nb, stride))
    x[0, ::97], y[1, 5::211], x[1, 7::1009] = np.nan, np.inf, -np.inf
    xd, yd = torch.from_numpy(x.reshape(-1)).cuda(), torch.from_numpy(y.reshape(-1)).cuda()
    part = torch.full((512 * nb * M,), np.nan, dtype=torch.float64, device="cuda")
    slots = C.c_int32(-1)
    rc = _lib().hsr_poly_moments_f64(xd.data_ptr(), stride, yd.data_ptr(), stride, npix, nb, deg, part.data_ptr(), C.byref(slots),
                                     _stream(torch))
    assert rc == 0 and slots.value == 512, (rc, _lib().hsr_last_error())
    torch.cuda.synchronize()
    got = part.cpu().numpy().reshape(512, nb, M)
    for b in range(nb):
        xb, yb = x[b, :npix], y[b, :npix]
        same_bits(got[:, b], _poly_slots_ref(xb, yb, np.isfinite(xb) & np.isfinite(yb), deg, 512), f"f64 deg {deg} band {b}")


# ---- 2. workgroup join, affine -----------------------------------------------------------------------------------------------------------
AFFINE_NPIX = 3077                                                    # two slots of 1540 rows: two passes per thread, a ragged end


def _affine_terms(xs, ys):
    """affine_add's 22 terms per row, the order of hsr_color.h; xs, ys (n, 3) float64."""
    z = np.concatenate([xs, np.ones((len(xs), 1))], axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([z[:, i] * z[:, j] for i, j in ac.TRI] + [z[:, i] * ys[:, c] for i in range(3) for c in range(3)]
                        + [ys[:, c] for c in range(3)], axis=1)


def _affine_slots_ref(xs, ys, ok, owned):
    """owned(count): which of a slot's `count` rows a thread takes, in its order (see thread_sums)."""
    npix = len(xs)
    nslots = ac.slots(npix)
    per = ac.slot_rows(npix, nslots)
    terms = _affine_terms(xs, ys)
    ref = np.zeros((nslots, ac.NMOM))
    for s in range(nslots):
        beg, end = min(s * per, npix), min(s * per + per, npix)
        ref[s] = wave_tree(thread_sums(terms[beg:end], ok[beg:end], owned(end - beg)))
    return ref


def _groups_of_four(count):
    """Thread t takes the groups t, t + 256, ... of four rows, each group in row order: rows 4t .. 4t + 3, then those 1024 on."""
    passes = max(1, -(-count // 1024))
    own = np.stack([1024 * k + 4 * np.arange(256) + j for k in range(passes) for j in range(4)])
    return np.where(own < count, own, -1)


def _affine_rows(seed):
    rng = np.random.default_rng(seed)
    x, y = _mixed(rng, (AFFINE_NPIX, 3)), _mixed(rng, (AFFINE_NPIX, 3))
    x[11::197, 0], y[3::301, 2], x[1500, 1] = np.nan, np.inf, -np.inf
    return x, y


@pytest.mark.parametrize("layout", [ac.PLANAR, ac.PADDED, ac.PACKED])
def test_affine_moments_slots_follow_the_tree(torch_gpu, layout):
    """Whatever the load mode, a thread takes its slot's pixels as _groups_of_four says."""
    torch = torch_gpu
    x, y = (a.astype(np.float32) for a in _affine_rows(7))
    mask = ac.make_mask(AFFINE_NPIX, "part", 5)
    xb, yb = (Buf(torch, f.nbytes, 0, f) for f in (ac.pack(x, layout), ac.pack(y, layout)))
    mb = Buf(torch, AFFINE_NPIX, 1, mask)
    nslots = ac.slots(AFFINE_NPIX)
    assert nslots == 2 and ac.slot_rows(AFFINE_NPIX, nslots) == 1540
    pb = Buf(torch, nslots * ac.NMOM * 8, 0)
    bs, ps, _ = ac.strides(layout, AFFINE_NPIX)
    rc = _lib().hsr_affine_moments(xb.ptr, bs, ps, yb.ptr, bs, ps, mb.ptr, AFFINE_NPIX, None, None, pb.ptr, None, _stream(torch))
    assert rc == 0, _lib().hsr_last_error()
    got = pb.get(np.float64).reshape(nslots, ac.NMOM)
    ok = ac.usable(x, y, mask)
    ref = _affine_slots_ref(x.astype(np.float64), y.astype(np.float64), ok, _groups_of_four)
    assert ref[:, 9].sum() == ok.sum() and 0.7 * AFFINE_NPIX < ok.sum() < AFFINE_NPIX
    same_bits(got, ref, f"affine moments, {layout}")


def test_affine_moments_f64_slots_follow_the_tree(torch_gpu):
    """Thread t takes the rows t, t + 256, ... of its slot."""
    torch = torch_gpu
    x, y = _affine_rows(8)
    xb, yb = Buf(torch, x.nbytes, 0, x), Buf(torch, y.nbytes, 8, y)
    nslots = ac.slots(AFFINE_NPIX)
    pb = Buf(torch, nslots * ac.NMOM * 8, 0)
    rc = _lib().hsr_affine_moments_f64(xb.ptr, 3, yb.ptr, 3, AFFINE_NPIX, pb.ptr, None, _stream(torch))
    assert rc == 0, _lib().hsr_last_error()
    ok = ac.usable(x, y, None)
    ref = _affine_slots_ref(x, y, ok, lambda count: _strided(np.arange(256), count))
    assert ref[:, 9].sum() == ok.sum() < AFFINE_NPIX
    same_bits(pb.get(np.float64).reshape(nslots, ac.NMOM), ref, "affine moments, float64 rows")


# ---- 3. workgroup join, ridge statistics -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in", [1, 16])
def test_ridge_stats_follow_the_tree(torch_gpu, n_in):
    """64 blocks of ceil(n / 64) = 1094 rows: a thread walks rows t, t + 256, ... of its block (a second pass of the four-row
    loop for t < 70); sums of d = x - x[0] and of d * d per column; the finish kernel's butterfly over the blocks (a lane per
    block, the other lanes 0.0), then mean = K + s1 / n and M2 = max(s2 - s1 * s1 / n, 0)."""
    torch = torch_gpu
    lib = _lib()
    n, nblocks = 70001, 64
    rows = -(-n // nblocks)
    assert rows > 1024
    rng = np.random.default_rng(n_in)
    X = _mixed(rng, (n, n_in)).astype(np.float32)
    xb = Buf(torch, X.nbytes, 0, X)
    work = Buf(torch, lib.hsr_ridge_stats_work_bytes(n_in), 0)
    stats, mean, scale = (Buf(torch, 8 * k, 0) for k in (1 + 2 * n_in, n_in, n_in))
    rc = lib.hsr_ridge_stats(xb.ptr, n_in, 1, n, n_in, work.ptr, stats.ptr, mean.ptr, scale.ptr, _stream(torch))
    assert rc == 0, lib.hsr_last_error()
    K = X[0].astype(np.float64)
    d = X.astype(np.float64) - K
    terms = np.stack([d, d * d], axis=2).reshape(n, 2 * n_in)         # acc[2c] = sum d, acc[2c + 1] = sum d^2
    part = np.zeros((64, 2 * n_in))
    for blk in range(nblocks):
        r0, r1 = min(blk * rows, n), min(blk * rows + rows, n)
        part[blk] = wave_tree(thread_sums(terms[r0:r1], np.ones(r1 - r0, bool), _strided(np.arange(256), r1 - r0)))
    same_bits(work.get(np.float64).reshape(nblocks, 2 * n_in), part, "partial sums of the blocks")
    tot = butterfly64(part)
    s1, s2, nn = tot[0::2], tot[1::2], np.float64(n)
    m2 = np.maximum(s2 - s1 * s1 / nn, 0.0)
    same_bits(stats.get(np.float64), np.concatenate([[nn], K + s1 / nn, m2]), f"stats n_in={n_in}")
    same_bits(mean.get(np.float64), K + s1 / nn, "mean")
    sc = np.sqrt(m2 / nn)
    same_bits(scale.get(np.float64), np.where(sc == 0.0, 1.0, sc), "scale")


# ---- 4. the affine slot reduction ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [1, 63, 64, 65, 512])
def test_affine_reduce_solve_follows_the_tree(torch_gpu, slots):
    """Hand-made partials: slot i holds the 22 terms of one row (x_i, y_i) with mixed exponents, so the reduced moments are the
    Gram of real rows.  moments = slot_tree per column; At = the host twin of the solve on exactly those moments."""
    torch = torch_gpu
    lib = _lib()
    rng = np.random.default_rng(slots)
    part = _affine_terms(_mixed(rng, (slots, 3)), _mixed(rng, (slots, 3)))
    pb, mo, at = Buf(torch, part.nbytes, 0, part), Buf(torch, ac.NMOM * 8, 0), Buf(torch, 96, 0)
    rc = lib.hsr_affine_reduce_solve(pb.ptr, slots, 0, mo.ptr, at.ptr, _stream(torch))
    assert rc == 0, lib.hsr_last_error()
    ref = slot_tree(part)
    assert ref[9] == slots
    same_bits(mo.get(np.float64), ref, f"moments, {slots} slots")
    host = (C.c_double * 12)()
    assert lib.hsr_affine_solve_host((C.c_double * ac.NMOM)(*ref), 0, host) == 0
    same_bits(at.get(np.float64), np.array(host[:]), f"At, {slots} slots")
