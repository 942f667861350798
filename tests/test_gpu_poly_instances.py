"""Every kernel instance of csrc/hsr_poly.hip (K2 moments, the slot reduction, the solve, K3 apply, the validity mask) against
float64 NumPy references.

One case table.  Each row names a geometry, the entry point it calls and the instance the library's launch record
(hsr_poly_last_launch) must show.  References:
  * apply: bit-exact float32 against Horner in float64 (np.polyval's order, separately rounded) after the stretch
    float32(clip((x - lo) / (hi - lo + 1e-12), 0, 1)) restated in NumPy; inputs hold NaN, +-Inf, -0.0 and values outside [0, 1];
    pad columns of rows pass through; batch tiles are checked one by one and rows past a tile's npix stay untouched;
  * moments: float64 sums of the per_band_valid rule (count exact, other sums rtol 1e-12), slot count and bits of a relaunch;
  * reduction: the documented tree written out (lane l adds slots l, l + 64, ... from 0.0, then the xor butterfly over the 64
    lane sums), bit for bit, on partials with mixed exponents;
  * solve: the four solve entry points give identical bits on identical moments, Cholesky and Jacobi branch alike, the
    identity fallback holds, and fits match np.polyfit; rank-deficient bands match np.polyfit's minimum-norm coefficients;
  * valid mask: both load paths, pos_band -1 / 0 / last, y absent / rows / planar, mask_in absent / present, NaN in pad columns.
The last test checks that the rows reach all 62 instances.
"""
import ctypes as C
import warnings

import numpy as np
import pytest

from gpu_harness import LaunchLog, bits_equal, slot_tree, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from gpu_harness import lib as _lib
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu

LOG = LaunchLog("hsr_poly_last_launch")
_call = LOG.call
ALL_INSTANCES = (
    {f"apply_rows_kernel<{q}, {n}, {b}>" for q in range(1, 5) for n in range(1, 6) for b in ("false", "true")}
    | {f"apply_rows_lds_kernel<{q}>" for q in range(1, 5)}
    | {"apply_pixmajor_scalar_kernel", "apply_planar_kernel<true>", "apply_planar_kernel<false>"}
    | {f"moments_kernel<{d}>" for d in range(1, 5)} | {f"moments_f64_kernel<{d}>" for d in range(1, 5)}
    | {"reduce_kernel", "solve_kernel", "reduce_solve_kernel"}
    | {f"reduce_solve_batched_kernel<{u}, {t}>" for u, t in ((8, "true"), (12, "true"), (16, "false"))}
    | {"valid_mask_kernel"})
assert len(ALL_INSTANCES) == 62


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---- float64 references ------------------------------------------------------------------------------------------------------
def _stretch(v, lo, hi):
    r = (v.astype(np.float64) - lo) / (hi - lo + 1e-12)
    r = np.where(r < 0.0, 0.0, np.where(r > 1.0, 1.0, r))          # NaN falls through both compares
    return r.astype(np.float32)


def _horner(v, c):
    xd = v.astype(np.float64)
    y = np.zeros_like(xd)
    for ck in c:
        y = y * xd + ck                                              # NumPy: separate multiply and add
    return y.astype(np.float32)


def _apply_ref(x, coeffs, lohi, mask, clip):
    """x (npix, nb) float32 -> (npix, nb) float32."""
    out = x.copy()
    for b in range(x.shape[1]):
        v = x[:, b]
        if lohi is not None:
            v = _stretch(v, lohi[b, 0], lohi[b, 1])
        if coeffs is not None:
            p = _horner(v, coeffs[b])
            v = p if mask is None else np.where(mask != 0, p, v)
        if clip:
            v = np.where(v < 0, np.float32(0), np.where(v > 1, np.float32(1), v)).astype(np.float32)
        out[:, b] = v
    return out


def _values(rng, n):
    """float32 samples with NaN, +-Inf, -0.0 and values outside [0, 1]."""
    v = rng.uniform(-0.3, 1.3, n).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 2.5, -7.0], np.float32)
    k = min(n, len(special))
    idx = rng.choice(n, k, replace=False)
    v[idx] = special[:k]
    return v


def _coeffs(rng, nb, deg):
    return rng.uniform(-1.5, 1.5, (nb, deg + 1))


def _lohi(rng, nb):
    lo = rng.uniform(-0.1, 0.3, nb)
    return np.stack([lo, lo + rng.uniform(0.2, 1.0, nb)], 1)


# ---- apply ------------------------------------------------------------------------------------------------------------------
def _apply_rows_case(torch, rng, nb, row, deg, npix, expect, *, use_coeffs=True, stretch=False, use_mask=False, clip=True,
                     offset=0, out_row=None):
    """Pixel-major in (npix, row) and out (npix, out_row): the rows / lds / scalar paths (and planar<false> for out_row != row)."""
    out_row = row if out_row is None else out_row
    x = _values(rng, npix * row).reshape(npix, row)
    c = _coeffs(rng, nb, deg) if use_coeffs else None
    lohi = _lohi(rng, nb) if stretch else None
    mask = (rng.random(npix) < 0.6).astype(np.uint8) if use_mask else None
    xb = torch.zeros(npix * row + 8, dtype=torch.float32, device="cuda")
    xd = xb[offset:offset + npix * row]
    xd.copy_(torch.from_numpy(x.reshape(-1)))
    sentinel = np.float32(-123.0)
    ob = torch.full((npix * out_row + 8,), float(sentinel), dtype=torch.float32, device="cuda")
    od = ob[offset:offset + npix * out_row]
    cd = torch.from_numpy(np.ascontiguousarray(c)).cuda() if c is not None else None
    ld = torch.from_numpy(lohi).cuda() if lohi is not None else None
    md = torch.from_numpy(mask).cuda() if mask is not None else None
    lib = _lib()
    _call(expect, lib.hsr_poly_apply, _p(xd), 1, row, _p(md), _p(cd), nb, deg, npix, _p(ld), int(clip), _p(od), 1, out_row, None)
    torch.cuda.synchronize()
    got = od.cpu().numpy().reshape(npix, out_row)
    ref = _apply_ref(x[:, :nb], c, lohi, mask, clip)
    bits_equal(got[:, :nb], ref, f"{expect} nb={nb} deg={deg} npix={npix}")
    if out_row == row and expect.startswith("apply_rows"):
        bits_equal(got[:, nb:], x[:, nb:], f"{expect}: pad columns pass through")
    else:                                                            # scalar / planar paths write the band columns only
        assert (got[:, nb:] == sentinel).all(), f"{expect}: pad columns written"
    rest = ob.cpu().numpy()
    assert (rest[:offset] == sentinel).all() and (rest[offset + npix * out_row:] == sentinel).all(), "write outside the image"


def _apply_planar_case(torch, rng, nb, deg, npix, plane, expect, *, mask_offset=0, use_mask=True, stretch=True, clip=True):
    x = _values(rng, nb * plane).reshape(nb, plane)
    c = _coeffs(rng, nb, deg)
    lohi = _lohi(rng, nb) if stretch else None
    mask = (rng.random(npix) < 0.5).astype(np.uint8)
    xd = torch.from_numpy(x.reshape(-1)).cuda()
    od = torch.full((nb * plane,), -5.0, dtype=torch.float32, device="cuda")
    cd, ld = torch.from_numpy(c).cuda(), (torch.from_numpy(lohi).cuda() if lohi is not None else None)
    mb = torch.zeros(npix + 8, dtype=torch.uint8, device="cuda")
    md = mb[mask_offset:mask_offset + npix]
    md.copy_(torch.from_numpy(mask))
    _call(expect, _lib().hsr_poly_apply, _p(xd), plane, 1, _p(md) if use_mask else None, _p(cd), nb, deg, npix, _p(ld),
          int(clip), _p(od), plane, 1, None)
    torch.cuda.synchronize()
    got = od.cpu().numpy().reshape(nb, plane)
    ref = _apply_ref(np.ascontiguousarray(x[:, :npix].T), c, lohi, mask if use_mask else None, clip).T
    bits_equal(got[:, :npix], ref, f"{expect} nb={nb} npix={npix} plane={plane}")
    assert (got[:, npix:] == -5.0).all()


def _apply_batch_case(torch, rng, nb, deg, sizes, use_mask, expect, clip=True):
    from s2_emit import _native as nat
    row = (nb + 3) // 4 * 4
    T = len(sizes)
    xs = [_values(rng, n * row).reshape(n, row) for n in sizes]
    masks = [(rng.random(n) < 0.5).astype(np.uint8) for n in sizes]
    shared = bool(use_mask & 2)
    c = rng.uniform(-1.5, 1.5, ((1 if shared else T), nb, deg + 1))
    slack = 64                                                       # rows past npix: must stay untouched
    xds = [torch.from_numpy(x.reshape(-1)).cuda() for x in xs]
    ods = [torch.full(((n + slack) * row,), -9.0, dtype=torch.float32, device="cuda") for n in sizes]
    mds = [torch.from_numpy(m).cuda() for m in masks]
    tiles = (nat.BatchTile * T)()
    for i, n in enumerate(sizes):
        tiles[i].pseudo_dev, tiles[i].matched_dev = xds[i].data_ptr(), ods[i].data_ptr()
        tiles[i].mask_dev, tiles[i].npix = mds[i].data_ptr(), n
    td = torch.frombuffer(bytearray(bytes(tiles)), dtype=torch.uint8).cuda()
    cd = torch.from_numpy(np.ascontiguousarray(c)).cuda()
    _call(expect, _lib().hsr_poly_apply_batched, _p(td), T, max(sizes), _p(cd), nb, deg, row, use_mask, int(clip), None)
    torch.cuda.synchronize()
    for i, n in enumerate(sizes):
        got = ods[i].cpu().numpy().reshape(n + slack, row)
        ref = _apply_ref(xs[i][:, :nb], c[0 if shared else i], None, masks[i] if use_mask & 1 else None, clip)
        bits_equal(got[:n, :nb], ref, f"{expect} tile {i} npix={n} use_mask={use_mask}")
        bits_equal(got[:n, nb:], xs[i][:, nb:], f"{expect} tile {i}: pad columns")
        assert (got[n:] == -9.0).all(), f"{expect} tile {i}: rows past npix written"


def _apply_cases():
    cases = []
    nbs = {q: [nb for nb in range(4 * q - 3, 4 * q + 1)] for q in range(1, 5)}
    pix = [1, 3, 1001, 4099, 20000]
    k = 0
    for q in range(1, 5):
        for n in range(1, 6):
            for j in range(2):                                       # two geometries per instance: every nb of the class
                nb = nbs[q][(2 * n + j) % 4]
                kw = dict(use_coeffs=(k % 5 != 4), stretch=(k % 3 == 1), use_mask=(k % 2 == 0), clip=(k % 4 != 3))
                cases.append(("rows", dict(nb=nb, row=4 * q, deg=n - 1, npix=pix[k % len(pix)],
                                           expect=f"apply_rows_kernel<{q}, {n}, false>", **kw)))
                k += 1
    for q in range(1, 5):
        for deg in (5, 6, 7, 8):
            nb = nbs[q][deg % 4]
            cases.append(("rows", dict(nb=nb, row=4 * q, deg=deg, npix=pix[(q + deg) % len(pix)], use_mask=deg % 2 == 0,
                                       stretch=deg == 6, expect=f"apply_rows_lds_kernel<{q}>")))
    # routing: rows of 3 / 5 floats, a misaligned pointer, different in / out strides, single-band rows of 1
    cases.append(("rows", dict(nb=3, row=3, deg=3, npix=1001, use_mask=True, expect="apply_pixmajor_scalar_kernel")))
    cases.append(("rows", dict(nb=5, row=5, deg=7, npix=333, stretch=True, expect="apply_pixmajor_scalar_kernel")))
    cases.append(("rows", dict(nb=4, row=4, deg=2, npix=999, offset=1, use_mask=True, expect="apply_pixmajor_scalar_kernel")))
    cases.append(("rows", dict(nb=1, row=1, deg=1, npix=77, expect="apply_pixmajor_scalar_kernel")))
    cases.append(("rows", dict(nb=6, row=8, out_row=12, deg=3, npix=500, use_mask=True, expect="apply_planar_kernel<false>")))
    cases.append(("planar", dict(nb=3, deg=3, npix=4099, plane=4100, expect="apply_planar_kernel<true>")))
    cases.append(("planar", dict(nb=2, deg=8, npix=3, plane=4, use_mask=False, expect="apply_planar_kernel<true>")))
    cases.append(("planar", dict(nb=3, deg=2, npix=1001, plane=1001, expect="apply_planar_kernel<false>")))
    cases.append(("planar", dict(nb=2, deg=3, npix=1000, plane=1000, mask_offset=1, expect="apply_planar_kernel<false>")))
    # batch: every (Q, N), tiles of 1 .. 1e4 pixels, use_mask 0..3
    sizes = [[1, 10000, 37], [4099, 3], [64, 65, 1], [2500]]
    k = 0
    for q in range(1, 5):
        for n in range(1, 6):
            nb = nbs[q][(n + 1) % 4]
            cases.append(("batch", dict(nb=nb, deg=n - 1, sizes=sizes[k % 4], use_mask=k % 4, clip=k % 3 != 2,
                                        expect=f"apply_rows_kernel<{q}, {n}, true>")))
            k += 1
    return cases


APPLY = _apply_cases()


@pytest.mark.parametrize("i", range(len(APPLY)), ids=[f"{i}-{k}-{kw['expect']}-nb{kw['nb']}-deg{kw['deg']}" for i, (k, kw) in enumerate(APPLY)])
def test_apply_instance_bit_exact(torch_gpu, i):
    kind, kw = APPLY[i]
    rng = np.random.default_rng(1000 + i)
    if kind == "rows":
        _apply_rows_case(torch_gpu, rng, **kw)
    elif kind == "planar":
        _apply_planar_case(torch_gpu, rng, **kw)
    else:
        _apply_batch_case(torch_gpu, rng, **kw)


def test_apply_rows_grid_stride_branch(torch_gpu):
    """Past ~33.5 M float4 the rows kernel runs 2046 workgroups that stride over the image (the 6144^2 apply of match_pair)."""
    torch = torch_gpu
    npix = 8190 * 256 * 16 + 4097                                    # gb > 8190 -> grid-stride
    rng = np.random.default_rng(7)
    x = rng.uniform(-0.2, 1.2, (npix, 4)).astype(np.float32)
    x[::1000003, 0] = np.nan
    c = np.array([[0.31, -0.7, 1.1]])
    xd = torch.from_numpy(x.reshape(-1)).cuda()
    od = torch.empty_like(xd)
    cd = torch.from_numpy(c).cuda()
    _call("apply_rows_kernel<1, 3, false>", _lib().hsr_poly_apply, _p(xd), 1, 4, None, _p(cd), 1, 2, npix, None, 1, _p(od), 1, 4, None)
    torch.cuda.synchronize()
    got = od.cpu().numpy().reshape(npix, 4)
    bits_equal(got[:, 0], _apply_ref(x[:, :1], c, None, None, True)[:, 0], "grid-stride apply")
    bits_equal(got[:, 1:], x[:, 1:], "grid-stride pad columns")


def _tie_probe(rng):
    """(x, c0, c1) with float32(c0 * x + c1) different when the multiply and add are fused: the separately rounded sum lands
    exactly on a float32 rounding tie, the fused one a double ulp off it.  Bit-exact float32 outputs hide a contraction
    otherwise (the double results differ in the last bit, the float32 store rounds that away)."""
    from fractions import Fraction
    while True:
        x = np.float32(rng.uniform(0.1, 1.0))
        c0 = float(rng.uniform(1.0, 4.0))
        pd = c0 * float(x)
        f = np.float32(pd / 4)
        m = (float(f) + float(np.nextafter(f, np.float32(np.inf)))) / 2      # a float32 tie, exact in double
        c1 = m - pd
        if pd + c1 != m:
            continue
        fused = float(Fraction(c0) * Fraction(float(x)) + Fraction(c1))
        if np.float32(fused) != np.float32(m):
            return x, c0, c1


TIE_CASES = ([("rows", q, n) for q in range(1, 5) for n in range(2, 6)] + [("batch", q, n) for q in range(1, 5) for n in range(2, 6)]
             + [("rows", q, n) for q in range(1, 5) for n in (6, 9)] + [("scalar", 1, 4), ("planar", 1, 3), ("planar_nv", 1, 7)])


@pytest.mark.parametrize("kind,q,n", TIE_CASES)
def test_apply_horner_is_not_contracted(torch_gpu, kind, q, n):
    """Every Horner of K3 multiplies and adds separately (np.polyval's rounding), checked where a fused multiply-add shows."""
    torch = torch_gpu
    rng = np.random.default_rng(q * 10 + n)
    nb = 4 * q - 1 if kind in ("rows", "batch") else 3
    npix = 37
    probes = [_tie_probe(rng) for _ in range(nb)]
    c = np.zeros((nb, n))
    c[:, -2] = [p[1] for p in probes]
    c[:, -1] = [p[2] for p in probes]
    x = np.tile(np.array([p[0] for p in probes], np.float32), (npix, 1))
    ref = _apply_ref(x, c, None, None, False)
    if kind in ("rows", "batch", "scalar"):
        row = 4 * q if kind != "scalar" else nb
        xs = np.zeros((npix, row), np.float32)
        xs[:, :nb] = x
        xd = torch.from_numpy(xs.reshape(-1)).cuda()
        od = torch.zeros_like(xd)
        cd = torch.from_numpy(c).cuda()
        if kind == "batch":
            from s2_emit import _native as nat
            tiles = (nat.BatchTile * 1)()
            tiles[0].pseudo_dev, tiles[0].matched_dev, tiles[0].npix = xd.data_ptr(), od.data_ptr(), npix
            td = torch.frombuffer(bytearray(bytes(tiles)), dtype=torch.uint8).cuda()
            _call(f"apply_rows_kernel<{q}, {n}, true>", _lib().hsr_poly_apply_batched, _p(td), 1, npix, _p(cd), nb, n - 1, row, 0, 0, None)
        else:
            expect = ("apply_pixmajor_scalar_kernel" if kind == "scalar" else
                      f"apply_rows_kernel<{q}, {n}, false>" if n <= 5 else f"apply_rows_lds_kernel<{q}>")
            _call(expect, _lib().hsr_poly_apply, _p(xd), 1, row, None, _p(cd), nb, n - 1, npix, None, 0, _p(od), 1, row, None)
        torch.cuda.synchronize()
        got = od.cpu().numpy().reshape(npix, row)[:, :nb]
    else:
        plane = npix + (3 if kind == "planar" else 0)                # 37 + 3: whole float4 rows; 37: the unaligned form
        xp = np.zeros((nb, plane), np.float32)
        xp[:, :npix] = x.T
        xd = torch.from_numpy(xp.reshape(-1)).cuda()
        od = torch.zeros_like(xd)
        cd = torch.from_numpy(c).cuda()
        _call(f"apply_planar_kernel<{'true' if kind == 'planar' else 'false'}>", _lib().hsr_poly_apply, _p(xd), plane, 1, None,
              _p(cd), nb, n - 1, npix, None, 0, _p(od), plane, 1, None)
        torch.cuda.synchronize()
        got = od.cpu().numpy().reshape(nb, plane)[:, :npix].T
    bits_equal(got, ref, f"{kind} Q={q} N={n}: Horner contracted")


# ---- moments ----------------------------------------------------------------------------------------------------------------
def _moments_ref(x, y, deg):
    x, y = x.astype(np.float64), y.astype(np.float64)
    return np.array([np.sum(x ** k) for k in range(2 * deg + 1)] + [np.sum(x ** j * y) for j in range(deg + 1)])


def _check_moments(got, ref, what):
    assert got[0] == ref[0], f"{what}: count {got[0]} != {ref[0]}"
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0, err_msg=what)


def _reduce(torch, part, slots, nb, deg):
    M = 3 * deg + 2
    mom = torch.zeros(nb * M, dtype=torch.float64, device="cuda")
    _call("reduce_kernel", _lib().hsr_moments_reduce, _p(part), slots, nb, deg, _p(mom), None)
    return mom.cpu().numpy().reshape(nb, M)


MOMENT_CASES = [(deg, layout, npix) for deg, layout, npix in
                [(1, "planar", 64), (2, "rows4", 65), (3, "rows8", 32768), (4, "rows12", 32769), (1, "rows16", 1000000),
                 (2, "planar", 32769), (3, "rows4", 1), (4, "planar", 1000000), (4, "rows16", 65), (3, "planar", 64)]]


@pytest.mark.parametrize("deg,layout,npix", MOMENT_CASES)
def test_moments_kernel_vs_float64(torch_gpu, deg, layout, npix):
    torch = torch_gpu
    rng = np.random.default_rng(deg * 1000 + npix % 997)
    nb = 3 if layout == "planar" else min(int(layout[4:]), 13) - (deg % 2)
    row = nb if layout == "planar" else int(layout[4:])
    x = _values(rng, npix * nb).reshape(npix, nb)
    y = _values(rng, npix * nb).reshape(npix, nb)
    mask = (rng.random(npix) < 0.8).astype(np.uint8)
    stretch = deg % 2 == 0
    lx, ly = _lohi(rng, nb), _lohi(rng, nb)
    min_x, min_y = np.float32(0.05), np.float32(-0.1)
    if layout == "planar":
        xd, yd = torch.from_numpy(np.ascontiguousarray(x.T).reshape(-1)).cuda(), torch.from_numpy(np.ascontiguousarray(y.T).reshape(-1)).cuda()
        bs, ps = npix, 1
    else:
        xp, yp = np.zeros((npix, row), np.float32), np.zeros((npix, row), np.float32)
        xp[:, :nb], yp[:, :nb] = x, y
        xp[:, nb:] = np.nan                                           # pad columns are never read
        xd, yd = torch.from_numpy(xp.reshape(-1)).cuda(), torch.from_numpy(yp.reshape(-1)).cuda()
        bs, ps = 1, row
    md = torch.from_numpy(mask).cuda()
    lxd, lyd = torch.from_numpy(lx).cuda(), torch.from_numpy(ly).cuda()
    M = 3 * deg + 2
    part = torch.zeros(512 * nb * M, dtype=torch.float64, device="cuda")
    slots = C.c_int32(-1)
    args = (_p(xd), bs, ps, _p(yd), bs, ps, _p(md), npix, nb, deg, C.c_float(min_x), C.c_float(min_y),
            _p(lxd) if stretch else None, _p(lyd) if stretch else None, _p(part), C.byref(slots), None)
    _call(f"moments_kernel<{deg}>", _lib().hsr_poly_moments, *args)
    assert slots.value == min((npix + 63) // 64, 512)
    first = part.clone()
    _call(f"moments_kernel<{deg}>", _lib().hsr_poly_moments, *args)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int64), part.view(torch.int64)), "relaunch changed bits"
    got = _reduce(torch, part, slots.value, nb, deg)
    for b in range(nb):
        ok = (mask != 0) & np.isfinite(x[:, b]) & np.isfinite(y[:, b]) & (x[:, b] > min_x) & (y[:, b] > min_y)
        xv, yv = x[ok, b], y[ok, b]
        if stretch:
            xv, yv = _stretch(xv, lx[b, 0], lx[b, 1]), _stretch(yv, ly[b, 0], ly[b, 1])
        _check_moments(got[b], _moments_ref(xv, yv, deg), f"moments_kernel<{deg}> {layout} npix={npix} band {b}")


@pytest.mark.parametrize("deg,npix", [(1, 65), (2, 32769), (3, 1000000), (4, 64)])
def test_moments_f64_kernel_vs_float64(torch_gpu, deg, npix):
    torch = torch_gpu
    rng = np.random.default_rng(deg)
    nb, stride = 3, npix + 5
    x, y = rng.uniform(0, 1, (nb, stride)), rng.uniform(0, 1, (nb, stride))
    x[0, :: 97] = np.nan
    y[1, 5] = np.inf
    xd, yd = torch.from_numpy(x.reshape(-1)).cuda(), torch.from_numpy(y.reshape(-1)).cuda()
    M = 3 * deg + 2
    part = torch.zeros(512 * nb * M, dtype=torch.float64, device="cuda")
    slots = C.c_int32(-1)
    _call(f"moments_f64_kernel<{deg}>", _lib().hsr_poly_moments_f64, _p(xd), stride, _p(yd), stride, npix, nb, deg, _p(part),
          C.byref(slots), None)
    assert slots.value == min((npix + 63) // 64, 512)
    got = _reduce(torch, part, slots.value, nb, deg)
    for b in range(nb):
        ok = np.isfinite(x[b, :npix]) & np.isfinite(y[b, :npix])
        _check_moments(got[b], _moments_ref(x[b, :npix][ok], y[b, :npix][ok], deg), f"moments_f64_kernel<{deg}> band {b}")


# ---- reduction: the documented tree (slot_tree of gpu_harness), bit for bit -------------------------------------------------
def _partials(rng, slots, nb, M):
    return rng.standard_normal((slots, nb, M)) * np.exp2(rng.integers(-40, 40, (slots, nb, M)))


SLOTS = [1, 63, 64, 65, 128, 129, 512, 4096]


@pytest.mark.parametrize("slots", SLOTS)
def test_reduce_kernels_follow_the_documented_tree(torch_gpu, slots):
    torch = torch_gpu
    lib = _lib()
    rng = np.random.default_rng(slots)
    deg, nb = 1 + slots % 4, 1 + slots % 16
    M = 3 * deg + 2
    p = _partials(rng, slots, nb, M)
    p[..., 0] = np.abs(p[..., 0])                                    # a count-like column: keeps the solve in business
    ref = slot_tree(p)
    pd = torch.from_numpy(p.reshape(-1)).cuda()
    got = _reduce(torch, pd, slots, nb, deg)
    assert np.array_equal(got.view(np.int64), ref.view(np.int64)), "reduce_kernel"
    mom = torch.zeros(nb * M, dtype=torch.float64, device="cuda")
    co = torch.zeros(nb * (deg + 1), dtype=torch.float64, device="cuda")
    _call("reduce_solve_kernel", lib.hsr_moments_reduce_solve, _p(pd), slots, nb, deg, 0, _p(mom), _p(co), None)
    torch.cuda.synchronize()
    assert np.array_equal(mom.cpu().numpy().reshape(nb, M).view(np.int64), ref.view(np.int64)), "reduce_solve_kernel"


def _batched(torch, parts, nb, deg, min_count=0):
    """parts: list of (slots, nb, M) arrays, one per tile -> (moments, coeffs, instance)."""
    from s2_emit import _native as nat
    M = 3 * deg + 2
    T = len(parts)
    tiles = (nat.BatchTile * T)()
    off = 0
    for i, p in enumerate(parts):
        tiles[i].slot0, tiles[i].slots, tiles[i].npix = off, p.shape[0], 1
        off += p.shape[0]
    td = torch.frombuffer(bytearray(bytes(tiles)), dtype=torch.uint8).cuda()
    pd = torch.from_numpy(np.concatenate([p.reshape(-1) for p in parts])).cuda()
    mom = torch.zeros(T * nb * M, dtype=torch.float64, device="cuda")
    co = torch.zeros(T * nb * (deg + 1), dtype=torch.float64, device="cuda")
    u = 8 if nb <= 8 else 12 if nb <= 12 else 16
    _call(f"reduce_solve_batched_kernel<{u}, {'true' if u <= 12 else 'false'}>", _lib().hsr_moments_reduce_solve_batched,
          _p(td), T, _p(pd), nb, deg, min_count, _p(mom), _p(co), None)
    torch.cuda.synchronize()
    return mom.cpu().numpy().reshape(T, nb, M), co.cpu().numpy().reshape(T, nb, deg + 1)


@pytest.mark.parametrize("nb", [1, 8, 9, 12, 13, 16])
def test_reduce_solve_batched_follows_the_documented_tree(torch_gpu, nb):
    rng = np.random.default_rng(nb)
    deg = 1 + nb % 4
    M = 3 * deg + 2
    parts = [_partials(rng, s, nb, M) for s in SLOTS]
    mom, _ = _batched(torch_gpu, parts, nb, deg)
    for t, p in enumerate(parts):
        ref = slot_tree(p)
        assert np.array_equal(mom[t].view(np.int64), ref.view(np.int64)), f"tile {t} ({p.shape[0]} slots)"


# ---- solve --------------------------------------------------------------------------------------------------------------------
def _polyfit(x, y, deg):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.polyfit(x.astype(np.float64), y.astype(np.float64), deg)


RANK = {1: [0.3], 2: [0.2, 0.7], 3: [0.2, 0.5, 0.9], 4: [0.1, 0.4, 0.7, 0.95]}


def _solve_sets(deg):
    """Moment sets of one degree: well-conditioned fits, exactly rank-deficient bands, the identity fallbacks."""
    rng = np.random.default_rng(100 + deg)
    sets = []
    for n in (200, 5000):                                            # well conditioned: Cholesky
        x = rng.uniform(0, 1, n).astype(np.float32)
        y = (0.2 + 0.7 * x - 0.3 * x * x + 0.02 * rng.standard_normal(n)).astype(np.float32)
        sets.append(("fit", x, y))
    for nd in range(1, deg + 1):                                     # rank-deficient: Jacobi
        for n, scale in ((333, 1e-3), (10000, 1.0), (100000, 1e3)):
            x = np.repeat(np.float32(np.array(RANK[nd]) * scale), (n + nd - 1) // nd)[:n]
            sets.append(("rank", x, rng.uniform(0, 1, n).astype(np.float32)))
    mom = np.stack([_moments_ref(x, y, deg) for _, x, y in sets] + [np.zeros(3 * deg + 2), _moments_ref(x[:40], y[:40], deg)])
    return sets, mom


@pytest.mark.parametrize("deg", [1, 2, 3, 4])
def test_solve_entry_points_identical_and_match_polyfit(torch_gpu, deg):
    torch = torch_gpu
    from s2_emit import _engine as eng
    lib = _lib()
    sets, mom = _solve_sets(deg)
    nb_all, M = mom.shape[0], 3 * deg + 2
    min_count = 50
    host = eng.poly_solve_host(mom, deg, min_count)
    for lo in range(0, nb_all, 16):                                  # the device entry points take <= 16 bands
        m = mom[lo:lo + 16]
        nb = m.shape[0]
        md = torch.from_numpy(np.ascontiguousarray(m).reshape(-1)).cuda()
        co = torch.zeros(nb * (deg + 1), dtype=torch.float64, device="cuda")
        _call("solve_kernel", lib.hsr_poly_solve, _p(md), nb, deg, min_count, _p(co), None)
        torch.cuda.synchronize()
        assert np.array_equal(co.cpu().numpy().reshape(nb, -1).view(np.int64), host[lo:lo + nb].view(np.int64)), "solve_kernel"
        mo2 = torch.zeros_like(md)
        co2 = torch.zeros_like(co)
        _call("reduce_solve_kernel", lib.hsr_moments_reduce_solve, _p(md), 1, nb, deg, min_count, _p(mo2), _p(co2), None)
        torch.cuda.synchronize()
        assert np.array_equal(co2.cpu().numpy().reshape(nb, -1).view(np.int64), host[lo:lo + nb].view(np.int64)), "reduce_solve"
        _, cb = _batched(torch, [m[None]], nb, deg, min_count)
        assert np.array_equal(cb[0].view(np.int64), host[lo:lo + nb].view(np.int64)), "batched"
    ident = np.zeros(deg + 1)
    ident[-2] = 1.0
    assert np.array_equal(host[-2], ident) and np.array_equal(host[-1], ident)   # count 0, count 40 < 50
    for i, (kind, x, y) in enumerate(sets):
        ref = _polyfit(x, y, deg)
        if kind == "fit":
            np.testing.assert_allclose(host[i], ref, rtol=1e-6 if deg == 4 else 1e-7, atol=1e-9)
        else:
            scale = float(np.max(x))
            assert np.max(np.abs(host[i] - ref)) <= 1e-9 * np.max(np.abs(ref)), (kind, len(x), scale, host[i], ref)
            grid = np.linspace(0, 1.5 * scale, 64)
            pr = np.polyval(ref, grid)
            assert np.max(np.abs(np.polyval(host[i], grid) - pr)) <= 1e-9 * np.max(np.abs(pr))


def test_rank_deficient_fit_through_fused_step(torch_gpu):
    """A constant cube gives every pseudo band one value: the fused K1 tail must return np.polyfit's minimum-norm coefficients."""
    torch = torch_gpu
    from s2_emit import SpectralFusion
    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths()
    rng = np.random.default_rng(3)
    for deg, val in ((2, 0.3), (3, 0.7), (4, 0.1)):
        Rc = torch.full((64, 64, 285), val, dtype=torch.float32, device="cuda")
        plan = SpectralFusion(w, srf, good, deg=deg, min_count=10)
        real = rng.uniform(0, 1, (len(plan.names), 64, 64)).astype(np.float32)
        out = plan.step(Rc, torch.from_numpy(real).cuda(), reuse_buffers=False)
        torch.cuda.synchronize()
        pseudo = out.planes("pseudo").cpu().numpy().reshape(len(plan.names), -1)
        co = out.coeffs.cpu().numpy()
        for b in range(len(plan.names)):
            ref = _polyfit(pseudo[b], real[b].reshape(-1), deg)
            assert np.max(np.abs(co[b] - ref)) <= 1e-9 * np.max(np.abs(ref)), (deg, b, co[b], ref)


# ---- valid mask -------------------------------------------------------------------------------------------------------------
VALID = [(nbx, row, pos, ylay, min_in, npix) for nbx, row, pos, ylay, min_in, npix in [
    (13, 16, 0, "rows", True, 1001), (12, 12, 11, "planar", False, 4099), (3, 4, -1, None, True, 65), (1, 4, 0, "rows", False, 3),
    (5, 5, 4, "rows", True, 777), (7, 8, -1, "planar", True, 1), (16, 16, 15, None, False, 20000), (2, 2, 1, "planar", False, 300),
    (4, 0, 3, "rows", True, 513)]]


@pytest.mark.parametrize("nbx,row,pos,ylay,min_in,npix", VALID)
def test_valid_mask_kernel(torch_gpu, nbx, row, pos, ylay, min_in, npix):
    torch = torch_gpu
    rng = np.random.default_rng(nbx * 31 + npix)
    x = rng.uniform(-0.2, 1.0, (npix, nbx)).astype(np.float32)
    x[rng.random((npix, nbx)) < 0.02] = np.nan
    x[rng.random((npix, nbx)) < 0.01] = np.inf
    nby = 3
    y = rng.uniform(0, 1, (npix, nby)).astype(np.float32)
    y[rng.random((npix, nby)) < 0.02] = -np.inf
    if row:                                                          # pixel-major rows; NaN in the pad columns
        xs = np.full((npix, row), np.nan, np.float32)
        xs[:, :nbx] = x
        xd, xbs, xps = torch.from_numpy(xs.reshape(-1)).cuda(), 1, row
    else:                                                            # planar
        xd, xbs, xps = torch.from_numpy(np.ascontiguousarray(x.T).reshape(-1)).cuda(), npix, 1
    if ylay == "rows":
        ys = np.full((npix, 4), np.nan, np.float32)
        ys[:, :nby] = y
        yd, ybs, yps = torch.from_numpy(ys.reshape(-1)).cuda(), 1, 4
    elif ylay == "planar":
        yd, ybs, yps = torch.from_numpy(np.ascontiguousarray(y.T).reshape(-1)).cuda(), npix, 1
    else:
        yd, ybs, yps = None, 0, 0
    mi = (rng.random(npix) < 0.9).astype(np.uint8)
    mid = torch.from_numpy(mi).cuda() if min_in else None
    out = torch.full((npix,), 7, dtype=torch.uint8, device="cuda")
    _call("valid_mask_kernel", _lib().hsr_valid_mask, _p(xd), xbs, xps, nbx, pos, _p(yd), ybs, yps, nby, _p(mid), npix, _p(out), None)
    torch.cuda.synchronize()
    ok = np.isfinite(x).all(1)
    if pos >= 0:
        ok &= x[:, pos] > 0
    if ylay:
        ok &= np.isfinite(y).all(1)
    if min_in:
        ok &= mi != 0
    np.testing.assert_array_equal(out.cpu().numpy(), ok.astype(np.uint8))


def test_poly_case_table_reaches_every_instance(torch_gpu):
    """Runs last in this module: the rows above reached all 62 instances."""
    missing = ALL_INSTANCES - LOG.seen
    assert not missing, sorted(missing)
    assert LOG.seen <= ALL_INSTANCES, sorted(LOG.seen - ALL_INSTANCES)
