"""Parity tests proper: the HIP path (through the C ABI) against the oracle and the golden fixtures.

Run on an MI355X with ``pytest -m gpu``.  Tolerances (stated where used):
  * K1 planes: float32 accumulation of <= ~40 taps vs the float64 reference: rel 2e-6 (target 1e-4)
  * Inf/NaN classification: exact
  * polynomial apply / percentile stretch: bit-exact float32 (float64 arithmetic inside)
  * coefficients from moments vs np.polyfit: rel 1e-7 (deg <= 3), 1e-6 (deg 4)
  * end-to-end matched planes: 1e-4 relative (the north-star tolerance), observed ~1e-6
"""
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import load_golden, unpack_srf
from gpu_harness import torch_gpu  # noqa: F401
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu

warnings.simplefilter("ignore")


def _rel_err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref))
    if not fin.any():
        return 0.0
    scale = np.maximum(np.abs(ref[fin]), 1e-3 * np.max(np.abs(ref[fin])) + 1e-30)
    return float(np.max(np.abs(got[fin] - ref[fin]) / scale))


# ---------------------------------------------------------------------------------------------
# K1
# ---------------------------------------------------------------------------------------------
def test_k1_srf_golden_g1(torch_gpu):
    import s2_emit
    g = load_golden("g1_srf")
    srf = unpack_srf(g)
    for tag, gm in (("masked", g["good_mask"]), ("nomask", None)):
        out = s2_emit.pseudo_s2_srf_integral(g["R"], g["emit_w"], srf, gm)
        assert list(out) == list(srf)
        none = {str(n) for n in g[f"{tag}_none"]}
        for k, v in out.items():
            if k in none:
                assert v is None
            else:
                assert v.dtype == np.float64 and v.shape == (10, 10)
                assert _rel_err(v, g[f"{tag}_{k}"]) < 2e-6
    rgb = s2_emit.pseudo_s2_rgb(s2_emit.pseudo_s2_srf_integral(g["R"], g["emit_w"], srf, g["good_mask"]))
    assert _rel_err(rgb, g["rgb_masked"]) < 2e-6


def test_k1_edge_semantics_golden_g2(torch_gpu):
    """NaN / +-Inf / nodata rows: same classification as the reference, per band."""
    import s2_emit
    g = load_golden("g2_srf_edge")
    srf = unpack_srf(g)
    out = s2_emit.pseudo_s2_srf_integral(g["R"], g["emit_w"], srf, g["good_mask"])
    for k, v in out.items():
        if k in {str(n) for n in g["none"]}:
            assert v is None
            continue
        ref = g[f"out_{k}"]
        assert _rel_err(v, ref) < 2e-6, k
    assert np.isposinf(out["B1"][0, 2]) and np.isneginf(out["B1"][0, 3]) and np.isnan(out["B1"][0, 4])
    assert np.isnan(out["B12"][0, 2]) and np.isnan(out["B1"][0, 5])
    np.testing.assert_allclose(out["B2"][1, 0], -9999.0, rtol=1e-6)


@pytest.mark.parametrize("H,W,B,offset", [(64, 64, 285, 0),      # config C1
                                          (37, 53, 285, 0),      # ragged last tile
                                          (1, 1, 285, 0),        # single pixel
                                          (3, 21, 285, 0),       # less than one tile
                                          (40, 40, 285, 1),      # cube base only 4-byte aligned -> generic loader
                                          (33, 17, 224, 0),      # even B (AVIRIS-like) -> padded LDS rows
                                          (20, 30, 31, 0)])      # short spectra
def test_k1_vs_oracle_shapes(torch_gpu, H, W, B, offset):
    torch = torch_gpu
    from s2_emit import _engine as eng
    from s2_emit import _native as nat
    rng = np.random.default_rng(H * 1000 + W + B)
    w = np.linspace(381.0, 2493.0, B).astype(np.float32)
    good = np.ones(B, bool)
    good[B // 2: B // 2 + 3] = False
    srf = onp.synthetic_srf()
    R = (rng.random((H, W, B)) * 0.6).astype(np.float32)
    R[H // 2, W // 2, B // 3] = np.nan
    R[0, 0, B // 2 + 1] = np.inf                     # zero-weight band
    ref = onp.pseudo_s2_srf_integral(R, w, srf, good)
    table = eng.build_srf_table(w, srf, good)
    flat = torch.empty(H * W * B + 4, dtype=torch.float32, device="cuda")
    cube = flat[offset: offset + H * W * B].view(H, W, B)
    cube.copy_(torch.from_numpy(R))
    planes = eng.srf_integrate(cube, table).cpu().numpy().reshape(table.nb, H, W)
    assert [k for k, v in ref.items() if v is not None] == table.supported
    for i, k in enumerate(table.supported):
        assert _rel_err(planes[i], ref[k]) < 2e-6, (k, H, W, B)
    # pixel-major (band-last) output: the LDS-staged slab path must give the same bits as the planes
    pm = eng.srf_integrate(cube, table, layout=nat.PIXMAJOR)
    assert pm.shape == (H * W, eng.padded_row(table.nb))
    assert torch.equal(pm[:, :table.nb].t().contiguous().view(torch.int32),
                       torch.from_numpy(planes.reshape(table.nb, -1)).cuda().view(torch.int32))
    # launch options travel with the call (no process-wide state to restore): reserved CUs change the grid, not the planes
    p2 = eng.srf_integrate(cube, table, opts=eng.srf_options(tile_pixels=64, reserved_cus=8)).cpu().numpy().reshape(table.nb, H, W)
    assert np.array_equal(p2.view(np.int32), planes.view(np.int32))


def test_k1_torch_input_zero_copy_and_many_bands(torch_gpu):
    """torch cube in -> torch planes out; 20 bands exercise the >16-band chunking."""
    torch = torch_gpu
    import s2_emit
    w, good = onp.synthetic_wavelengths()
    lam = np.arange(380.0, 2500.0)
    srf = {f"N{i}": (lam, np.exp(-0.5 * ((lam - (450 + 90 * i)) / 25.0) ** 2) + 1e-9) for i in range(20)}
    for k in srf:
        m = srf[k][1] > 1e-3
        srf[k] = (lam[m], srf[k][1][m])
    R = onp.synthetic_cube(24, 24, seed=5)
    ref = onp.pseudo_s2_srf_integral(R, w, srf, good)
    out = s2_emit.pseudo_s2_srf_integral(torch.from_numpy(R).cuda(), w, srf, good)
    assert list(out) == list(srf)
    for k, v in ref.items():
        if v is None:
            assert out[k] is None
        else:
            assert out[k].is_cuda and out[k].dtype == torch.float32
            assert _rel_err(out[k].cpu().numpy(), v) < 2e-6
    assert s2_emit.pseudo_s2_srf_integral(np.zeros((0, 5, 285), np.float32), w, srf, good)["N0"].shape == (0, 5)


# ---------------------------------------------------------------------------------------------
# K2 + solve
# ---------------------------------------------------------------------------------------------
def _np_moments(x, y, ok, deg):
    xd, yd = x[ok].astype(np.float64), y[ok].astype(np.float64)
    return np.array([np.sum(xd ** k) for k in range(2 * deg + 1)] + [np.sum(xd ** j * yd) for j in range(deg + 1)])


@pytest.mark.parametrize("deg", [1, 2, 3, 4])
def test_k2_moments_and_solve_vs_polyfit(torch_gpu, deg):
    torch = torch_gpu
    from s2_emit import _engine as eng
    rng = np.random.default_rng(deg)
    nb, npix = 5, 40000 + 13
    x = (rng.random((nb, npix)) * 0.6).astype(np.float32)
    y = np.clip(0.9 * x.astype(np.float64) ** 0.9 + 0.02 + 0.01 * rng.standard_normal(x.shape), 0, 1).astype(np.float32)
    x[0, 5] = np.nan
    y[1, 7] = np.inf
    x[2, :100] = -0.01
    mask = rng.random(npix) > 0.2
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    md = torch.from_numpy(mask.view(np.uint8)).cuda()
    ws = eng.MomentWorkspace("cuda", nb, deg)
    mom = eng.poly_moments(xd, yd, deg, ws, md, 0.0, 0.0).cpu().numpy()
    co = eng.poly_solve(ws.moments, deg, 50).cpu().numpy()
    ref_c, counts = onp.fit_per_band_poly(x.reshape(nb, 1, npix), y.reshape(nb, 1, npix), mask.reshape(1, npix), deg, 0.0, 50)
    for b in range(nb):
        ok = onp.per_band_valid(x[b], y[b], mask, 0.0)
        np.testing.assert_allclose(mom[b], _np_moments(x[b], y[b], ok, deg), rtol=1e-12)
        assert mom[b, 0] == counts[b]
    np.testing.assert_allclose(co, ref_c, rtol=1e-6 if deg == 4 else 1e-7, atol=1e-9)
    # determinism: same launch twice -> identical bits
    mom2 = eng.poly_moments(xd, yd, deg, ws, md, 0.0, 0.0).cpu().numpy()
    np.testing.assert_array_equal(mom, mom2)


def test_polyfit_columns_f64_golden_g3(torch_gpu):
    from s2_emit.poly_regression import polyfit_columns
    g = load_golden("g3_polyfit")
    for N in (200, 5000):
        for deg in (1, 2, 3, 4):
            c = polyfit_columns(g[f"x_{N}"][:, None], g[f"y_{N}"][:, None], deg)[0]
            np.testing.assert_allclose(c, g[f"coef_{N}_{deg}"], rtol=2e-8, atol=1e-10)


def test_calibrate_linear_golden_g6(torch_gpu):
    import s2_emit
    g = load_golden("g6_lsq")
    for tag, mask, mv in (("", g["mask"], 0.0), ("_few", g["mask_few"], 0.0), ("_mv", g["mask"], 0.1)):
        corr, params = s2_emit.calibrate_pseudo_to_real_linear(g["pseudo"], g["real"], mask, mv)
        np.testing.assert_allclose(np.array(params), g[f"params{tag}"], rtol=1e-9, atol=1e-12)
        assert _rel_err(corr, g[f"corrected{tag}"]) < 1e-6


# ---------------------------------------------------------------------------------------------
# K3 + stretch
# ---------------------------------------------------------------------------------------------
def test_k3_apply_poly_golden_g4_bitexact(torch_gpu):
    import s2_emit
    g = load_golden("g4_apply")
    for deg in (1, 2, 3, 4):
        co = g[f"coeffs_{deg}"]
        a = s2_emit.apply_poly_rgb(g["rgb"], co, None)
        b = s2_emit.apply_poly_rgb(g["rgb"], co, g["mask"])
        assert a.dtype == np.float32 and b.dtype == np.float32
        np.testing.assert_array_equal(a, g[f"out_nomask_{deg}"])
        np.testing.assert_array_equal(b, g[f"out_mask_{deg}"])
    rgb0 = g["rgb"].copy()
    s2_emit.apply_poly_rgb(g["rgb"], g["coeffs_3"], g["mask"])
    np.testing.assert_array_equal(g["rgb"], rgb0)                       # input not mutated


def test_k3_planar_vec_and_scalar_paths(torch_gpu):
    torch = torch_gpu
    from s2_emit import _engine as eng
    rng = np.random.default_rng(11)
    for npix in (4096, 4099, 7):
        x = (rng.random((3, npix)) * 1.3 - 0.1).astype(np.float32)
        m = rng.random(npix) > 0.4
        co = rng.standard_normal((3, 4)) * 0.4
        ref = onp.apply_poly_planes(x.reshape(3, 1, npix), co, m.reshape(1, npix)).reshape(3, npix)
        got = eng.poly_apply(torch.from_numpy(x).cuda(), torch.from_numpy(co).cuda(),
                             torch.from_numpy(m.view(np.uint8)).cuda()).cpu().numpy()
        np.testing.assert_array_equal(got, ref)
        ref2 = onp.apply_poly_planes(x.reshape(3, 1, npix), co, None, clip=False).reshape(3, npix)
        got2 = eng.poly_apply(torch.from_numpy(x).cuda(), torch.from_numpy(co).cuda(), None, clip=False).cpu().numpy()
        np.testing.assert_array_equal(got2, ref2)


def test_pixel_major_paths_match_planar_bits(torch_gpu):
    """K2 / K3 / mask / percentiles on band-last rows (incl. 13 bands padded to 16) == band-major results."""
    torch = torch_gpu
    from s2_emit import _engine as eng
    from s2_emit import _native as nat
    rng = np.random.default_rng(31)
    for nb, npix in ((13, 5000), (12, 4099), (3, 777), (1, 100)):
        row = eng.padded_row(nb)
        x = (rng.random((nb, npix)) * 1.2 - 0.1).astype(np.float32)
        y = np.clip(x * 0.9 + 0.05 + 0.01 * rng.standard_normal(x.shape), 0, 1).astype(np.float32)
        x[0, 3] = np.nan
        m = rng.random(npix) > 0.3
        xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        md = torch.from_numpy(m.view(np.uint8)).cuda()
        xr = torch.full((npix, row), 7.0, dtype=torch.float32, device="cuda")
        yr = torch.full((npix, row), 7.0, dtype=torch.float32, device="cuda")
        xr[:, :nb], yr[:, :nb] = xd.t(), yd.t()
        co = torch.from_numpy(rng.standard_normal((nb, 4)) * 0.3).cuda()
        a = eng.poly_apply(xd, co, md, None, True, nat.PLANAR)
        b = eng.poly_apply(xr, co, md, None, True, nat.PIXMAJOR, nb=nb)
        assert torch.equal(a.view(torch.int32), b[:, :nb].t().contiguous().view(torch.int32))
        assert bool((b[:, nb:] == 7.0).all())                       # padding passes through
        ws = eng.MomentWorkspace("cuda", nb, 3)
        m1 = eng.poly_moments(xd, yd, 3, ws, md, 0.0, 0.0, layout=nat.PLANAR).clone()
        m2 = eng.poly_moments(xr, yr, 3, ws, md, 0.0, 0.0, layout=nat.PIXMAJOR, nb=nb).clone()
        assert torch.equal(m1, m2)
        l1 = eng.percentile_limits(xd[1:], md, 2, 98, nat.PLANAR) if nb > 1 else None
        l2 = eng.percentile_limits(xr[:, 1:], md, 2, 98, nat.PIXMAJOR, nb=nb - 1) if nb > 1 else None
        if nb > 1:
            assert torch.equal(l1, l2)
        v1 = eng.valid_mask(xd, 0, yd, md, nat.PLANAR)
        v2 = eng.valid_mask(xr, 0, yr, md, nat.PIXMAJOR, nbx=nb, nby=nb)
        ref = m & np.isfinite(x).all(0) & (x[0] > 0) & np.isfinite(y).all(0)
        assert torch.equal(v1, v2) and np.array_equal(v1.cpu().numpy().astype(bool), ref)


def test_fused_13_bands_padded_rows(torch_gpu):
    """No good_mask -> all 13 S2 bands supported -> band-last rows of 16 floats (3 padding columns)."""
    torch = torch_gpu
    from s2_emit import SpectralFusion
    srf = onp.synthetic_srf()
    w, _ = onp.synthetic_wavelengths()
    R = onp.synthetic_cube(48, 40, seed=4)
    ps_ref = onp.pseudo_s2_srf_integral(R, w, srf, None)
    names = list(ps_ref)
    assert len(names) == 13 and all(v is not None for v in ps_ref.values())
    real = onp.synthetic_real_planes(np.stack([ps_ref[k] for k in names]).astype(np.float32), seed=8)
    pseudo_o, coeffs_o, matched_o, _ = onp.fuse_lsq_reference(R, w, srf, None, real, 2)
    plan = SpectralFusion(w, srf, None, deg=2)
    out = plan.step(torch.from_numpy(R).cuda(), torch.from_numpy(real).cuda())
    assert out.pseudo.shape == (48 * 40, 16)
    assert _rel_err(out.planes("pseudo").cpu().numpy().reshape(pseudo_o.shape), pseudo_o) < 2e-6
    assert _rel_err(out.planes("matched").cpu().numpy().reshape(matched_o.shape), matched_o) < 1e-4
    assert _rel_err(out.band("B8A").cpu().numpy().reshape(48, 40), matched_o[names.index("B8A")]) < 1e-4


def test_percentile_stretch_golden_g5(torch_gpu):
    torch = torch_gpu
    import s2_emit
    from s2_emit import _engine as eng
    from s2_emit import _native as nat
    g = load_golden("g5_stretch")
    x = torch.from_numpy(g["img"]).cuda().reshape(-1, 3)
    m = torch.from_numpy(g["mask"].view(np.uint8)).cuda().reshape(-1)
    lohi = eng.percentile_limits(x, m, 2, 98, nat.PIXMAJOR).cpu().numpy()
    np.testing.assert_array_equal(lohi, g["lohi"])                      # exact order statistics + NumPy lerp
    np.testing.assert_array_equal(s2_emit.apply_shared_percentile_stretch(g["img"], g["mask"]), g["out_f32"])
    np.testing.assert_array_equal(s2_emit.apply_shared_percentile_stretch(g["img"], g["mask"], 5, 95), g["out_5_95"])
    # float64 image input is computed in float32 on the device: limits differ by <= 1 ulp(f32)
    np.testing.assert_allclose(s2_emit.apply_shared_percentile_stretch(g["img"].astype(np.float64), g["mask"]),
                               g["out_f64"], atol=2e-6)
    # a larger image regenerated from its seed: limits exact, stretched image checksum equal
    rng = np.random.default_rng(5)
    rng.random((20, 17, 3)); rng.random((20, 17))          # advance the stream as gen_golden.py did
    big = (rng.random((300, 257, 3)) ** 2).astype(np.float32)
    mb = rng.random((300, 257)) > 0.5
    xb = torch.from_numpy(big).cuda().reshape(-1, 3)
    lohi_b = eng.percentile_limits(xb, torch.from_numpy(mb.view(np.uint8)).cuda().reshape(-1), 2, 98,
                                   nat.PIXMAJOR).cpu().numpy()
    np.testing.assert_array_equal(lohi_b, g["big_lohi"])
    assert s2_emit.apply_shared_percentile_stretch(big, mb).astype(np.float64).sum() == float(g["big_out_checksum"])


def test_percentile_limits_random_planes(torch_gpu):
    """Exact np.percentile for several distributions, planar layout, incl. ties, negatives, tiny n."""
    torch = torch_gpu
    from s2_emit import _engine as eng
    rng = np.random.default_rng(21)
    npix = 70001
    planes = np.stack([rng.random(npix), rng.standard_normal(npix) * 50, np.round(rng.random(npix) * 8) / 8,
                       -rng.random(npix) ** 3, np.full(npix, 0.25)]).astype(np.float32)
    for frac in (0.7, 0.001, 1.0):
        mask = rng.random(npix) < frac
        mask[:3] = True
        for pmin, pmax in ((2, 98), (0, 100), (50, 50.5)):
            got = eng.percentile_limits(torch.from_numpy(planes).cuda(), torch.from_numpy(mask.view(np.uint8)).cuda(),
                                        pmin, pmax).cpu().numpy()
            ref = np.array([np.percentile(p[mask], [pmin, pmax]) for p in planes])
            np.testing.assert_array_equal(got, ref)
    got = eng.percentile_limits(torch.from_numpy(planes).cuda(), None, 2, 98).cpu().numpy()
    np.testing.assert_array_equal(got, np.array([np.percentile(p, [2, 98]) for p in planes]))
    # band-last rows of 4 floats (select_hist_rows4_kernel), three channels; sparse masks put the four ranks of a channel into
    # different radix bins (r03: only two of them are histogrammed in LDS, the others count into global memory)
    rows = np.zeros((npix, 4), np.float32)
    rows[:, :3] = planes[[1, 0, 3]].T
    for frac in (0.6, 0.0007, 1.0):
        mask = rng.random(npix) < frac
        mask[:2] = True
        for pmin, pmax in ((2, 98), (0, 100), (33.3, 66.6)):
            got = eng.percentile_limits(torch.from_numpy(rows).cuda(), torch.from_numpy(mask.view(np.uint8)).cuda(), pmin, pmax,
                                        "pixmajor", nb=3).cpu().numpy()
            ref = np.array([np.percentile(rows[mask, c], [pmin, pmax]) for c in range(3)])
            np.testing.assert_array_equal(got, ref)
    pn = planes.copy()
    pn[0, 10] = np.nan
    got = eng.percentile_limits(torch.from_numpy(pn).cuda(), None, 2, 98).cpu().numpy()
    assert np.isnan(got[0]).all() and not np.isnan(got[1:]).any()
    # tiny images (r04): up to 32 768 pixels a channel is selected inside one workgroup's registers (select_tiny_kernel) - the sizes of
    # the reference's own tiles; 32 769 takes the multi-launch path again.  Same checks: planes and rows of 4, masks, ties, NaN, no sample
    for n in (1, 2, 63, 10000, 32768, 32769):
        pl = planes[:, :n].copy()
        for frac in (0.6, 1.0):
            mask = rng.random(n) < frac
            mask[0] = True
            for pmin, pmax in ((2, 98), (0, 100), (37.5, 62.5)):
                got = eng.percentile_limits(torch.from_numpy(pl).cuda(), torch.from_numpy(mask.view(np.uint8)).cuda(), pmin, pmax).cpu().numpy()
                np.testing.assert_array_equal(got, np.array([np.percentile(p[mask], [pmin, pmax]) for p in pl]), err_msg=f"n={n}")
                rw = np.ascontiguousarray(rows[:n])
                got = eng.percentile_limits(torch.from_numpy(rw).cuda(), torch.from_numpy(mask.view(np.uint8)).cuda(), pmin, pmax, "pixmajor", nb=3).cpu().numpy()
                np.testing.assert_array_equal(got, np.array([np.percentile(rw[mask, c], [pmin, pmax]) for c in range(3)]), err_msg=f"rows n={n}")
        if n > 2:
            pl[1, n // 2] = np.nan
            got = eng.percentile_limits(torch.from_numpy(pl).cuda(), None, 2, 98).cpu().numpy()
            assert np.isnan(got[1]).all() and not np.isnan(got[[0, 2, 3, 4]]).any(), n
            none = torch.zeros(n, dtype=torch.uint8, device="cuda")
            assert np.isnan(eng.percentile_limits(torch.from_numpy(pl).cuda(), none, 2, 98).cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------
# the fused pipeline (configs C1 / reduced C2) against the reference-ordered oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,deg", [(64, 64, 2), (128, 96, 3), (50, 33, 1), (64, 64, 4)])
def test_fused_pipeline_vs_oracle(torch_gpu, H, W, deg):
    torch = torch_gpu
    from s2_emit import SpectralFusion
    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths()
    R = onp.synthetic_cube(H, W, seed=deg)
    ps_ref = onp.pseudo_s2_srf_integral(R, w, srf, good)
    names = [k for k, v in ps_ref.items() if v is not None]
    pseudo_ref = np.stack([ps_ref[k] for k in names]).astype(np.float32)
    real = onp.synthetic_real_planes(pseudo_ref, seed=3)
    real[0, 0, 0] = np.nan
    pseudo_o, coeffs_o, matched_o, names_o = onp.fuse_lsq_reference(R, w, srf, good, real, deg, 0.0, 50, True)
    plan = SpectralFusion(w, srf, good, deg=deg, min_valid=0.0, min_count=50, clip=True)
    assert plan.names == names_o
    out = plan.step(torch.from_numpy(R).cuda(), torch.from_numpy(real).cuda())     # band-major target
    assert out.layout == "pixmajor" and out.pseudo.shape == (H * W, 12)
    # band-last target + planar internal layout must give the same bits
    real_bl = torch.from_numpy(np.ascontiguousarray(np.moveaxis(real, 0, -1))).cuda()
    out_b = plan.step(torch.from_numpy(R).cuda(), real_bl, reuse_buffers=False)
    assert torch.equal(out_b.coeffs, out.coeffs) and torch.equal(out_b.matched.view(torch.int32), out.matched.view(torch.int32))
    plan_p = SpectralFusion(w, srf, good, deg=deg, min_valid=0.0, min_count=50, clip=True, layout="planar")
    out_p = plan_p.step(torch.from_numpy(R).cuda(), torch.from_numpy(real).cuda())
    assert torch.equal(out_p.coeffs, out.coeffs)
    assert torch.equal(out_p.matched.view(torch.int32), out.planes("matched").view(torch.int32))
    assert _rel_err(out.planes("pseudo").cpu().numpy().reshape(pseudo_o.shape), pseudo_o) < 2e-6
    # the fit sees float32 planes that differ by <= 1 ulp from the reference's: coefficients move by
    # cond * 6e-8; compare the fitted CURVES (what the 1e-4 target is about) and the coefficients loosely
    co = out.coeffs.cpu().numpy()
    xs = np.linspace(pseudo_o.min(), pseudo_o.max(), 50)
    for b in range(len(names)):
        np.testing.assert_allclose(np.polyval(co[b], xs), np.polyval(coeffs_o[b], xs), rtol=1e-5, atol=1e-6)
    assert _rel_err(out.planes("matched").cpu().numpy().reshape(matched_o.shape), matched_o) < 1e-4
    ok0 = onp.per_band_valid(pseudo_o[0], real[0], np.ones((H, W), bool), 0.0)
    assert out.moments.cpu().numpy()[0, 0] == ok0.sum() == H * W - 1


def test_config_c2_512_tile_vs_oracle(torch_gpu):
    """BASELINE.json configs[1]: a single 512 x 512 x 285 tile, SRF synthesis + deg-3 fit + apply on one GPU,
    against the reference-ordered float64 oracle on the same inputs; the north-star tolerance (1e-4 relative)
    is asserted on the matched planes, the pseudo planes are held to 2e-6."""
    torch = torch_gpu
    from s2_emit import SpectralFusion
    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths()
    H = W = 512
    R = onp.synthetic_cube(H, W, seed=2)
    ps_ref = onp.pseudo_s2_srf_integral(R[:8], w, srf, good)
    names = [k for k, v in ps_ref.items() if v is not None]
    rng = np.random.default_rng(2)
    real = np.clip(rng.random((len(names), H, W)) * 0.5 + 0.01, 0.01, 1).astype(np.float32)
    pseudo_o, coeffs_o, matched_o, names_o = onp.fuse_lsq_reference(R, w, srf, good, real, 3, 0.0, 50, True)
    plan = SpectralFusion(w, srf, good, deg=3, min_valid=0.0, min_count=50, clip=True)
    assert plan.names == names_o
    out = plan.step(torch.from_numpy(R).cuda(), torch.from_numpy(real).cuda())
    assert _rel_err(out.planes("pseudo").cpu().numpy().reshape(pseudo_o.shape), pseudo_o) < 2e-6
    assert _rel_err(out.planes("matched").cpu().numpy().reshape(matched_o.shape), matched_o) < 1e-4
    co = out.coeffs.cpu().numpy()
    xs = np.linspace(float(pseudo_o.min()), float(pseudo_o.max()), 64)
    for b in range(len(names)):
        np.testing.assert_allclose(np.polyval(co[b], xs), np.polyval(coeffs_o[b], xs), rtol=1e-4, atol=1e-6)


def test_fuse_pair_numpy_wrapper(torch_gpu):
    import s2_emit
    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths()
    R = onp.synthetic_cube(32, 32, seed=9)
    ps_ref = onp.pseudo_s2_srf_integral(R, w, srf, good)
    names = [k for k, v in ps_ref.items() if v is not None]
    real = onp.synthetic_real_planes(np.stack([ps_ref[k] for k in names]).astype(np.float32))
    pseudo, coeffs, matched = s2_emit.fuse_pair(R, w, srf, good, {k: real[i] for i, k in enumerate(names)}, deg=2)
    assert pseudo["B10"] is None and matched["B10"] is None and coeffs["B10"] is None
    _, co, ma, _ = onp.fuse_lsq_reference(R, w, srf, good, real, 2)
    for i, k in enumerate(names):
        assert _rel_err(matched[k], ma[i]) < 1e-4


# ---------------------------------------------------------------------------------------------
# full-size properties (BASELINE config C3: 1024 x 1024 x 285): size-independent checks
# ---------------------------------------------------------------------------------------------
def test_full_size_properties_c3(torch_gpu):
    torch = torch_gpu
    from s2_emit import SpectralFusion
    from s2_emit import _engine as eng
    from s2_emit.synthetic import device_problem
    prob = device_problem(1024, 1024, deg=3, seed=0)
    plan = SpectralFusion(prob.emit_w, prob.srf, prob.good_mask, deg=3, min_valid=0.0)
    out = plan.step(prob.cube, prob.real)
    torch.cuda.synchronize()
    assert out.layout == "pixmajor"
    pseudo = out.planes("pseudo")
    matched = out.planes("matched")
    real_pl = prob.real_planes.reshape(plan.table.nb, -1)
    # (1) a sampled sub-block equals the oracle on the same data
    rows = slice(300, 316)
    sub = prob.cube[rows, :64].cpu().numpy()
    ref = onp.pseudo_s2_srf_integral(sub, prob.emit_w, prob.srf, prob.good_mask)
    got = pseudo.reshape(plan.table.nb, 1024, 1024)[:, rows, :64].cpu().numpy()
    for i, k in enumerate(plan.names):
        assert _rel_err(got[i], ref[k]) < 2e-6
    # (2) linearity: SRF(2*R) == 2*SRF(R) exactly in float32 (power-of-two scaling)
    p2 = eng.srf_integrate(prob.cube * 2.0, plan.table)
    assert torch.equal(p2, pseudo * 2.0)
    # (3) a constant spectrum integrates to the constant (weights sum to 1) within float32 rounding
    const = torch.full((4096, 285), 0.37, dtype=torch.float32, device="cuda")
    pc = eng.srf_integrate(const, plan.table)
    assert float((pc - 0.37).abs().max()) < 1e-6
    # (4) moments: the count equals the number of valid pixels; device moments == float64 torch sums
    mom = out.moments.cpu().numpy()
    x, y = pseudo.double(), real_pl.double()
    ok = torch.isfinite(x) & torch.isfinite(y) & (x > 0) & (y > 0)
    assert np.array_equal(mom[:, 0], ok.sum(dim=1).cpu().numpy().astype(np.float64))
    s2 = torch.where(ok, x * x, torch.zeros_like(x)).sum(dim=1).cpu().numpy()
    t1 = torch.where(ok, x * y, torch.zeros_like(x)).sum(dim=1).cpu().numpy()
    np.testing.assert_allclose(mom[:, 2], s2, rtol=1e-11)
    np.testing.assert_allclose(mom[:, 3 * 2 + 1 + 1], t1, rtol=1e-11)
    # (5) coefficients == np.polyfit on the device planes (host float64), one band checked in full
    b = 2
    xb = pseudo[b].cpu().numpy().astype(np.float64)
    yb = real_pl[b].cpu().numpy().astype(np.float64)
    okb = ok[b].cpu().numpy()
    ref_c = np.polyfit(xb[okb], yb[okb], 3)
    xs = np.linspace(xb[okb].min(), xb[okb].max(), 64)
    np.testing.assert_allclose(np.polyval(out.coeffs[b].cpu().numpy(), xs), np.polyval(ref_c, xs), rtol=1e-7, atol=1e-9)
    # (6) apply is idempotent w.r.t. clipping and bit-exact vs the oracle on a slab
    slab = slice(0, 65536)
    ref_m = onp.apply_poly_planes(pseudo[:, slab].cpu().numpy().reshape(plan.table.nb, 1, -1), out.coeffs.cpu().numpy(), None)
    assert np.array_equal(matched[:, slab].cpu().numpy(), ref_m.reshape(plan.table.nb, -1))
    # (7) run-to-run determinism of the whole step (fixed summation tree, no float atomics)
    c1 = out.coeffs.clone()
    out2 = plan.step(prob.cube, prob.real)
    assert torch.equal(out2.coeffs, c1)


def test_rccl_exchange_path_single_rank(torch_gpu):
    """One-rank RCCL group on the GPU: the multi-GPU step (reduce -> all-reduce / reduce+broadcast -> solve ->
    apply) must give bit-identical coefficients and output to the fused single-GPU launch."""
    torch = torch_gpu
    import os
    import torch.distributed as dist
    from s2_emit import SpectralFusion
    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths()
    R = torch.from_numpy(onp.synthetic_cube(96, 80, seed=12)).cuda()
    ps = onp.pseudo_s2_srf_integral(R.cpu().numpy(), w, srf, good)
    names = [k for k, v in ps.items() if v is not None]
    real = torch.from_numpy(onp.synthetic_real_planes(np.stack([ps[k] for k in names]).astype(np.float32))).cuda()
    base = SpectralFusion(w, srf, good, deg=3, coeff_sync="local").step(R, real, reuse_buffers=False)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29517", rank=0, world_size=1,
                                device_id=torch.device("cuda", 0))
        created = True
    try:
        for mode in ("allreduce", "broadcast"):
            plan = SpectralFusion(w, srf, good, deg=3, coeff_sync=mode, force_exchange=True)
            out = plan.step(R, real, reuse_buffers=False)
            torch.cuda.synchronize()
            assert torch.equal(out.coeffs, base.coeffs), mode
            assert torch.equal(out.moments, base.moments), mode
            assert torch.equal(out.matched.view(torch.int32), base.matched.view(torch.int32)), mode
            # the pipelined path issues the RCCL collective from the side stream
            plan = SpectralFusion(w, srf, good, deg=3, coeff_sync=mode, force_exchange=True)
            assert plan.submit(R, real) is None
            o1 = plan.submit(R, real)
            o2 = plan.flush()
            torch.cuda.synchronize()
            for o in (o1, o2):
                assert torch.equal(o.coeffs, base.coeffs) and torch.equal(o.matched.view(torch.int32), base.matched.view(torch.int32)), mode
        # the other collectives of the path over RCCL: global percentile limits (integer histograms) and the
        # distributed polynomial-ridge fit (all-gather of scaler statistics, all-reduce of the Gram)
        from s2_emit import PolyRidge, _engine as eng
        x3 = torch.rand(3, 5000, device="cuda")
        assert torch.equal(eng.percentile_limits(x3, None, 2, 98, distributed=True), eng.percentile_limits(x3, None, 2, 98))
        g = load_golden("g7_ridge")
        Xr, Yr = g["X"].astype(np.float32), g["Ylogit"]
        m0 = PolyRidge(3, 1.0).fit(Xr, Yr)
        m1 = PolyRidge(3, 1.0).fit(Xr, Yr, distributed=True)
        np.testing.assert_array_equal(m0.coef_, m1.coef_)
        np.testing.assert_array_equal(m0.intercept_, m1.intercept_)
    finally:
        if created:
            dist.destroy_process_group()


def test_pipeline_fallback_and_shape_change_lose_no_tile(torch_gpu):
    """ADVICE r3 (both medium).  (1) fuse_apply=True on a geometry the fused launch cannot carry - uint16 tiles with B = 300, 13
    bands in rows of 16: the two ring buffers do not fit next to the rows - must fall back to the two-slot pipeline AT CREATION
    (hsr_srf_fused_launch_supported inside hsr_pipeline_create_fused), not fail at the first carrying launch with tiles in flight.
    (2) a tile of another shape in mid-stream rebuilds the pipeline: the tiles still in flight are finished and come back from the
    following submit() / drain() calls in order - none is dropped.  (3) plans that share a work buffer are refused."""
    torch = torch_gpu
    import ctypes as C
    from s2_emit import SpectralFusion, _engine as eng, _native as nat
    g = torch.Generator(device="cuda")
    g.manual_seed(41)
    # (1)
    B = 300
    w300 = np.linspace(381.0, 2493.0, B).astype(np.float32)
    srf13 = onp.synthetic_srf()
    nb = eng.build_srf_table(w300, srf13, None).nb
    assert nb == 13
    H, W = 24, 64
    cubes = [eng.tile_encode_u16(torch.rand((H, W, B), generator=g, device="cuda") * 0.6) for _ in range(2)]
    reals = [torch.rand((H, W, 16), generator=g, device="cuda") for _ in range(2)]
    kw = dict(deg=3, min_valid=0.0, min_count=5)
    pipe = SpectralFusion(w300, srf13, None, fuse_apply=True, **kw)
    ref = SpectralFusion(w300, srf13, None, **kw)
    got = []
    for i in range(5):
        o = pipe.submit(cubes[i % 2], reals[i % 2])
        if o is not None:
            got.append((o.matched.clone(), o.coeffs.clone()))
    got += [(o.matched.clone(), o.coeffs.clone()) for o in pipe.drain()]
    assert not pipe._pipe["fused"] and pipe._pipe["S"] == 2 and "80 KB" in pipe.fused_fallback and len(got) == 5
    for i, (mt, co) in enumerate(got):
        want = ref.step(cubes[i % 2], reals[i % 2], reuse_buffers=False)
        assert torch.equal(mt.view(torch.int32), want.matched.view(torch.int32)) and torch.equal(co.view(torch.int64), want.coeffs.view(torch.int64)), i
    pipe.close()
    # (2)
    w, good = onp.synthetic_wavelengths()
    shapes = [(40, 64), (40, 64), (40, 64), (17, 50), (17, 50), (40, 64), (40, 64), (40, 64)]      # a ragged tile in the middle
    tiles = [(torch.rand((h, ww, 285), generator=g, device="cuda") * 0.6, torch.rand((h, ww, 12), generator=g, device="cuda")) for h, ww in shapes]
    for fuse in (False, True):
        pipe = SpectralFusion(w, srf13, good, fuse_apply=fuse, **kw)
        ref = SpectralFusion(w, srf13, good, **kw)
        got = []
        for c, r in tiles:
            o = pipe.submit(c, r)
            if o is not None:
                got.append((o.matched.clone(), o.coeffs.clone()))
        got += [(o.matched.clone(), o.coeffs.clone()) for o in pipe.drain()]
        assert len(got) == len(tiles), (fuse, len(got))
        for i, ((c, r), (mt, co)) in enumerate(zip(tiles, got)):
            want = ref.step(c, r, reuse_buffers=False)
            assert mt.shape == want.matched.shape, (fuse, i)
            assert torch.equal(mt.view(torch.int32), want.matched.view(torch.int32)) and torch.equal(co.view(torch.int64), want.coeffs.view(torch.int64)), (fuse, i)
        assert len(pipe._native_handles) <= 5          # the replaced pipelines and their plans were destroyed, not kept until close()
        pipe.close()
    # (3)
    lib = nat.load()
    plan = SpectralFusion(w, srf13, good, **kw)
    c, r = tiles[0]
    npix = c.shape[0] * c.shape[1]
    r2, rl = plan._real_image(r, npix)
    imgs = [eng.alloc_image(torch, 12, npix, nat.PIXMAJOR, c.device) for _ in range(6)]
    wss = [eng.MomentWorkspace(c.device, 12, 3) for _ in range(3)]
    h0, k0_ = plan._native_plan(c, r2, rl, imgs[0], imgs[1], wss[0])
    h1, k1_ = plan._native_plan(c, r2, rl, imgs[2], imgs[3], wss[1])
    h2, k2_ = plan._native_plan(c, r2, rl, imgs[4], imgs[5], wss[1])          # shares slot 1's workspace
    side = torch.cuda.Stream()
    ph = C.c_void_p()
    assert lib.hsr_pipeline_create_fused(h0, h1, h2, C.c_void_p(side.cuda_stream), 0, C.byref(ph)) == 1 and b"share a work buffer" in lib.hsr_last_error()
    assert lib.hsr_pipeline_create_fused(h0, h1, h1, C.c_void_p(side.cuda_stream), 0, C.byref(ph)) == 1
    assert lib.hsr_pipeline_create_fused(h0, h1, h2, C.c_void_p(side.cuda_stream), 1, C.byref(ph)) == 2       # no exchange in the three-slot form
    plan.close()


def test_group_pipeline_one_fit_per_mosaic_step_bit_identical(torch_gpu):
    """SpectralFusion(fuse_apply=True, group_tiles=T): one kernel per tile on the caller's stream, ONE polynomial per group of T
    tiles (hsr_pipeline_create_group; VERDICT r3 #3: the resident mosaic through the fused per-tile launch with a deferred global
    fit).  Every tile - T + 1 submits late, the rest through drain() - carries the bits of fuse_mosaic() over its own group:
    images, the group's moments and its coefficients; groups with different data, masks that come and go, uint16 tiles, tiles of
    fewer 64-pixel groups than bands (reduction and group fit as launches of their own); a drain needs whole groups."""
    torch = torch_gpu
    from s2_emit import SpectralFusion, _engine as eng, _native as nat
    w, good = onp.synthetic_wavelengths()
    srf = onp.synthetic_srf()
    g = torch.Generator(device="cuda")
    g.manual_seed(77)
    for (H, W), T, u16 in (((40, 64), 3, False), ((3, 90), 2, False), ((24, 64), 4, True)):
        npix = H * W
        steps = 3
        tiles = []
        for k in range(steps * T):
            c = torch.rand((H, W, 285), generator=g, device="cuda") * (0.3 + 0.1 * (k % 4))
            r = torch.rand((H, W, 12), generator=g, device="cuda")
            m = (torch.rand(npix, generator=g, device="cuda") > 0.4).to(torch.uint8) if k % 3 == 1 else None
            tiles.append((eng.tile_encode_u16(c) if u16 else c, r, m))
        for deg in (1, 3):
            kw = dict(deg=deg, min_valid=0.0, min_count=5, apply_mask=True)
            pipe = SpectralFusion(w, srf, good, fuse_apply=True, group_tiles=T, **kw)
            ref = SpectralFusion(w, srf, good, **kw)
            got = []

            def keep(o):
                got.append(tuple(t.clone() for t in (o.pseudo, o.matched, o.moments, o.coeffs)))
            for k, (c, r, m) in enumerate(tiles):
                o = pipe.submit(c, r, m)
                assert (o is None) == (k < T + 1), (k, T)
                if o is not None:
                    keep(o)
                if k == T:                                  # one tile into the second group: a drain must refuse
                    with pytest.raises(nat.HsrError, match="whole number of groups"):
                        pipe.drain()
            st = pipe._pipe
            assert st["fused"] and st["S"] == T + 2 and st["group"] is not None
            for o in pipe.drain():
                keep(o)
            assert len(got) == len(tiles) and pipe.drain() == []
            for s_ in range(steps):
                grp = tiles[s_ * T:(s_ + 1) * T]
                co, tot, outs = ref.fuse_mosaic([(c, r) for c, r, _ in grp], [m for _, _, m in grp])
                for i, o in enumerate(outs):
                    gt = got[s_ * T + i]
                    tag = (H, W, T, u16, deg, s_, i)
                    assert torch.equal(gt[0].view(torch.int32), o.pseudo.view(torch.int32)), tag + ("pseudo",)
                    assert torch.equal(gt[2].view(torch.int64), tot.view(torch.int64)), tag + ("moments",)
                    assert torch.equal(gt[3].view(torch.int64), co.view(torch.int64)), tag + ("coeffs",)
                    assert torch.equal(gt[1].view(torch.int32), o.matched.view(torch.int32)), tag + ("matched",)
            pipe.close()


def _one_rank_rccl_group(torch):
    """(created?, dist): a one-rank RCCL group on cuda:0 unless the process already has a group."""
    import os
    import torch.distributed as dist
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if dist.is_initialized():
        return False, dist
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29519", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    return True, dist


def test_comm_c_abi_single_rank(torch_gpu):
    """include/hsr.h hsr_comm_*: RCCL's C API behind the C ABI.  One rank on the box: the id round trip, init,
    every collective stream-ordered and value-preserving, ranks / rank, destroy; argument errors come back as codes."""
    torch = torch_gpu
    import ctypes as C
    from s2_emit import _engine as eng, _native as nat
    lib = nat.load()
    assert lib.hsr_comm_available() == 1 and lib.hsr_comm_version() >= 20000
    c = eng.Comm(rank=0, world=1)
    assert lib.hsr_comm_ranks(c.handle) == 1 and lib.hsr_comm_rank(c.handle) == 0
    x = torch.arange(132, dtype=torch.float64, device="cuda") * 0.37
    x0 = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c.allreduce_f64(x)
        c.reduce_f64(x, 0)
        c.bcast(x, 0)
    side.synchronize()
    assert torch.equal(x, x0)
    h = torch.arange(4096, dtype=torch.int32, device="cuda")
    c.allreduce_u32(h)
    torch.cuda.synchronize()
    assert torch.equal(h, torch.arange(4096, dtype=torch.int32, device="cuda"))
    assert lib.hsr_allreduce_f64(c.handle, None, 4, None) == 1 and b"hsr_allreduce_f64" in lib.hsr_last_error()
    assert lib.hsr_bcast(c.handle, C.c_void_p(x.data_ptr()), 8, 3, None) == 1
    hh = C.c_void_p()
    assert lib.hsr_comm_init(2, 2, (C.c_ubyte * 128)(), C.byref(hh)) == 1
    c.close()


def test_exchange_pipeline_from_c_single_rank(torch_gpu):
    """The fused pipeline WITH an exchange (hsr_pipeline_create_exchange): one kernel per tile on the caller's
    stream - K3 of tile i-3 as a pre-phase, K1+K2 of tile i, the slot reduction of tile i-1 in the tail - and gate -> RCCL
    collective -> solve on the side stream, all issued from C.  One-rank RCCL communicator through the C ABI; every tile (three
    submits late, the rest through drain()) carries the bits of its own step(): both sync modes, masks that come and go,
    float32 and uint16 tiles, a tile of fewer 64-pixel groups than bands (its reduction runs as a launch of its own), a drain
    in the middle of the stream, and the host transport (a gloo group: pinned round trip + callback).  No poll may time out."""
    torch = torch_gpu
    from s2_emit import SpectralFusion, _engine as eng
    created, dist = _one_rank_rccl_group(torch)
    try:
        w, good = onp.synthetic_wavelengths()
        srf = onp.synthetic_srf()
        g = torch.Generator(device="cuda")
        g.manual_seed(23)
        gloo = dist.new_group(backend="gloo")
        for (H, W), u16 in (((70, 61), False), ((40, 64), True), ((3, 90), False)):
            npix = H * W
            cubes = [torch.rand((H, W, 285), generator=g, device="cuda") * 0.6 for _ in range(3)]
            if u16:
                cubes = [eng.tile_encode_u16(c) for c in cubes]
                cubes[1].view(torch.int16)[3, 5, 100] = -1                      # nodata
            reals = [torch.rand((H, W, 12), generator=g, device="cuda") for _ in range(3)]
            masks = [None, (torch.rand(npix, generator=g, device="cuda") > 0.3).to(torch.uint8), None,
                     (torch.rand(npix, generator=g, device="cuda") > 0.6).to(torch.uint8), None]
            for mode, group in (("allreduce", None), ("broadcast", None), ("allreduce", gloo)):
                for deg in (1, 3):
                    kw = dict(deg=deg, min_valid=0.0, min_count=5, apply_mask=True)
                    ref = SpectralFusion(w, srf, good, coeff_sync="local", **kw)
                    pipe = SpectralFusion(w, srf, good, coeff_sync=mode, force_exchange=True, fuse_apply=True, group=group, **kw)
                    assert pipe.opts.reserved_cus == 8
                    seq = [(cubes[i % 3], reals[i % 3], masks[i % 5]) for i in range(9)]
                    got = []

                    def keep(o):
                        got.append(tuple(t.clone() for t in (o.pseudo, o.matched, o.moments, o.coeffs)))
                    for i, (c, r, m) in enumerate(seq):
                        o = pipe.submit(c, r, m)
                        if i == 5:                                                 # a drain in mid-stream, then on
                            assert o is not None
                            keep(o)
                            for o in pipe.drain():
                                keep(o)
                            assert len(got) == 6
                            continue
                        assert (o is None) == (i < 3 or 6 <= i < 9), (i, o is None)
                        if o is not None:
                            keep(o)
                    st = pipe._pipe
                    assert st["fused"] and st["S"] == 4 and st["c_exchange"] and st["transport"] == ("host" if group is not None else "rccl")
                    for o in pipe.drain():
                        keep(o)
                    assert len(got) == len(seq) and pipe.drain() == []
                    assert pipe.pipeline_status() == 0
                    for i, ((c, r, m), gt) in enumerate(zip(seq, got)):
                        want = ref.step(c, r, m, reuse_buffers=False)
                        tag = (H, W, u16, mode, deg, i)
                        assert torch.equal(gt[0].view(torch.int32), want.pseudo.view(torch.int32)), tag + ("pseudo",)
                        assert torch.equal(gt[2].view(torch.int64), want.moments.view(torch.int64)), tag + ("moments",)
                        assert torch.equal(gt[3].view(torch.int64), want.coeffs.view(torch.int64)), tag + ("coeffs",)
                        assert torch.equal(gt[1].view(torch.int32), want.matched.view(torch.int32)), tag + ("matched",)
                    pipe.close()
    finally:
        if created:
            dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------
# variant a9: multivariate polynomial ridge on the matrix cores
# ---------------------------------------------------------------------------------------------
def test_gram_f64_mfma_layout_exact(torch_gpu):
    """A^T B with small-integer data is exact in float64: catches any row/col or k-order slip of the
    v_mfma_f64_16x16x4_f64 lane maps (asymmetric B on purpose)."""
    torch = torch_gpu
    import ctypes as C
    from s2_emit import _native as nat
    from s2_emit._engine import _ptr, _stream
    lib = nat.load()
    rng = np.random.default_rng(3)
    for n in (4, 37, 1024, 5003):
        A = rng.integers(-4, 5, (n, 32)).astype(np.float64)
        B = rng.integers(-4, 5, (n, 48)).astype(np.float64)
        Ad, Bd = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
        work = torch.empty(max(1, lib.hsr_gram_work_bytes(32, 48, n) // 8), dtype=torch.float64, device="cuda")
        Cd = torch.full((32, 48), -1.0, dtype=torch.float64, device="cuda")
        nat.check(lib.hsr_gram_f64(_ptr(Ad), 32, 32, _ptr(Bd), 48, 48, n, _ptr(work), _ptr(Cd), 48, _stream(torch)))
        np.testing.assert_array_equal(Cd.cpu().numpy(), A.T @ B)
    for n, na, nb_ in ((777, 48, 128), (50, 96, 32), (3000, 112, 16)):       # two different matrices, B ending in a narrow strip
        A = rng.integers(-4, 5, (n, na)).astype(np.float64)
        B = rng.integers(-4, 5, (n, nb_)).astype(np.float64)
        Ad, Bd = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
        work = torch.empty(max(1, lib.hsr_gram_work_bytes(na, nb_, n) // 8), dtype=torch.float64, device="cuda")
        Cd = torch.full((na, nb_), -1.0, dtype=torch.float64, device="cuda")
        nat.check(lib.hsr_gram_f64(_ptr(Ad), na, na, _ptr(Bd), nb_, nb_, n, _ptr(work), _ptr(Cd), nb_, _stream(torch)))
        np.testing.assert_array_equal(Cd.cpu().numpy(), A.T @ B)
    # odd leading dimensions cannot be moved by 16-byte LDS-DMA: the register-operand kernel (and the tile-level mirror of the
    # shared reduction) takes over, for two matrices and for one matrix with itself
    for n, na, nb_, lda, ldb in ((300, 32, 48, 33, 49), (1029, 48, 80, 81, 81)):
        A = rng.integers(-4, 5, (n, lda)).astype(np.float64)
        B = A if lda == ldb and nb_ >= na else rng.integers(-4, 5, (n, ldb)).astype(np.float64)
        Ad = torch.from_numpy(A).cuda()
        Bd = Ad if B is A else torch.from_numpy(B).cuda()
        work = torch.empty(max(1, lib.hsr_gram_work_bytes(na, nb_, n) // 8), dtype=torch.float64, device="cuda")
        Cd = torch.full((na, nb_), -1.0, dtype=torch.float64, device="cuda")
        nat.check(lib.hsr_gram_f64(_ptr(Ad), lda, na, _ptr(Bd), ldb, nb_, n, _ptr(work), _ptr(Cd), nb_, _stream(torch)))
        np.testing.assert_array_equal(Cd.cpu().numpy(), A[:, :na].T @ B[:, :nb_])
    # the Gram of one matrix with itself takes the symmetric path (blocks below the diagonal mirrored):
    # [first na columns]^T [all columns], shapes that leave ragged 3 x 3 tile blocks on both axes
    # r03: a last strip of <= 32 columns becomes narrow blocks (96 x 32, chunks 5/2 as long), every workgroup splits its
    # chunk's batches of 8 rows over three 4-wave groups: shapes with and without a strip (16 / 32 wide), strip only,
    # fewer batches than groups, ragged last batches, one and many chunks, the fit's own (288 | 32) and (288 | 288)
    for n, na, nb_ in ((501, 112, 160), (64, 16, 16), (2000, 288, 320), (333, 64, 64), (7, 16, 32), (25, 32, 32),
                       (1237, 96, 112), (4099, 96, 128), (9001, 192, 208), (29127, 288, 320), (6151, 288, 576),
                       (8, 288, 304), (70001, 48, 80)):
        Q = rng.integers(-3, 4, (n, nb_)).astype(np.float64)
        Qd = torch.from_numpy(Q).cuda()
        work = torch.empty(max(1, lib.hsr_gram_work_bytes(na, nb_, n) // 8), dtype=torch.float64, device="cuda")
        Cd = torch.full((na, nb_), -1.0, dtype=torch.float64, device="cuda")
        nat.check(lib.hsr_gram_f64(_ptr(Qd), nb_, na, _ptr(Qd), nb_, nb_, n, _ptr(work), _ptr(Cd), nb_, _stream(torch)))
        np.testing.assert_array_equal(Cd.cpu().numpy(), Q[:, :na].T @ Q)


def test_poly_ridge_golden_g7(torch_gpu):
    """Fit + predict vs the scikit-learn float64 pipeline frozen in g7 (the notebook's own composition)."""
    import s2_emit
    g = load_golden("g7_ridge")
    X = g["X"].astype(np.float32)
    model = s2_emit.PolyRidge(degree=3, alpha=1.0).fit(X, g["Ylogit"])
    assert model.n_feat == 285 and model.coef_.shape == (6, 285)
    np.testing.assert_allclose(model.mean_, g["mean"], rtol=1e-12)
    np.testing.assert_allclose(model.scale_, g["scale"], rtol=1e-12)
    np.testing.assert_allclose(model.intercept_, g["intercept"], rtol=1e-6, atol=1e-7)
    # coefficients of an alpha-regularised ill-conditioned system: compare through their effect
    Xte = g["Xtest"].reshape(-1, 10).astype(np.float32)
    pl = model.predict(Xte)
    assert pl.dtype == np.float32 and pl.shape == (256, 6)
    np.testing.assert_allclose(pl, g["pred_logit"], rtol=0, atol=2e-4)          # float32 features + f32 MFMA
    cube = np.ascontiguousarray(np.moveaxis(g["Xtest"].astype(np.float32), -1, 0))   # (10, 16, 16)
    pc = s2_emit.predict_cube_logit(model, cube)
    assert pc.shape == (6, 16, 16) and pc.dtype == np.float32
    np.testing.assert_allclose(pc.reshape(6, -1).T, g["pred"], rtol=0, atol=1e-4)   # the 1e-4 reflectance target
    cube[3, 2, 5] = np.nan
    cube[0, 7, 7] = 600.0
    pn = s2_emit.predict_cube_logit(model, cube, nodata=600.0)
    assert np.isnan(pn[:, 2, 5]).all() and np.isnan(pn[:, 7, 7]).all() and np.isfinite(pn[:, 0, 0]).all()
    np.testing.assert_array_equal(s2_emit.subsample_bands_evenly(285, 32), g["subsample_285_32"])


def test_poly_ridge_many_targets_vs_oracle(torch_gpu):
    """T = 70 targets (3 MFMA target tiles), degree 2, odd pixel count: the generalised a9 configuration."""
    import s2_emit
    rng = np.random.default_rng(17)
    N, Cin, T = 3001, 10, 70
    base = rng.random((N, 4))
    X = (600 + 4000 * np.clip(base @ rng.random((4, Cin)) / 2, 0, 1)).astype(np.float32)
    Y = onp.logit(np.clip(base @ rng.random((4, T)) / 3 + 0.01 * rng.standard_normal((N, T)), 0, 0.6))
    ref = onp.ridge_poly_fit(X.astype(np.float64), Y, 2, 1.0)
    model = s2_emit.PolyRidge(degree=2, alpha=1.0).fit(X, Y)
    Xt = (600 + 4000 * rng.random((777, Cin))).astype(np.float32)
    np.testing.assert_allclose(model.predict(Xt), onp.ridge_poly_predict(ref, Xt.astype(np.float64)), rtol=0, atol=3e-4)
    pc = model.predict_cube(np.ascontiguousarray(Xt[:770].T.reshape(Cin, 22, 35)))
    np.testing.assert_allclose(pc.reshape(T, -1).T, onp.sigmoid(onp.ridge_poly_predict(ref, Xt[:770].astype(np.float64))),
                               rtol=0, atol=1e-4)


def _a9_problem(rng, N, Cin, T):
    base = rng.random((N, 4))
    X = (600 + 4000 * np.clip(base @ rng.random((4, Cin)) / 2 + 0.02 * rng.standard_normal((N, Cin)), 0, 1)).astype(np.float32)
    Y = onp.logit(np.clip(base @ rng.random((4, T)) / 3 + 0.01 * rng.standard_normal((N, T)), 0.001, 0.6))
    return X, Y


@pytest.mark.parametrize("T", [5, 16, 33, 41, 48, 64, 96, 97, 128, 130, 192, 285])
def test_predict103_kernel_families_vs_oracle(torch_gpu, T):
    """Every many-target predict kernel of the notebook's shape (10 inputs, degree 3; Spectral_matching.ipynb raw :192-213,
    :475-490 generalised to T targets) against the float64 oracle, NOT against itself: T <= 16 runs the 16-target tiles of
    predict103_x16_kernel (v_mfma_f32_16x16x4_f32, r04), T 33-64 one 64-target slice of
    predict103_slice_kernel<2>, 65-96 one 96-target slice of <3>, above that as few and as narrow slices as T allows (97 and
    128: two of 64; 130, 192: two of 96; 285: three of 96) (hsr_ridge.hip).  Two views:
      (a) the kernels alone - the ORACLE'S model loaded with from_params, so a wrong W-slice offset or target-tile epilogue
          cannot hide behind a consistent fit;
      (b) fit + predict end to end.
    Odd pixel counts (ragged last 128-pixel tile), pixel-major rows and the band-major cube.  Bars: logit 2e-4, reflectance
    1e-4 (float32 features and f32 MFMA accumulation against float64)."""
    import s2_emit
    rng = np.random.default_rng(100 + T)
    X, Y = _a9_problem(rng, 2501, 10, T)
    ref = onp.ridge_poly_fit(X.astype(np.float64), Y, 3, 1.0)
    loaded = s2_emit.PolyRidge.from_params(ref["mean"], ref["scale"], ref["coef"], ref["intercept"], degree=3)
    fitted = s2_emit.PolyRidge(degree=3, alpha=1.0).fit(X, Y)
    assert fitted.n_feat == 285 and fitted.coef_.shape == (T, 285)
    for npx in (1, 127, 777, 1517):
        Xt = (600 + 4000 * np.clip(rng.random((npx, 4)) @ rng.random((4, 10)) / 2, 0, 1)).astype(np.float32)
        want = onp.ridge_poly_predict(ref, Xt.astype(np.float64))
        for tag, model in (("loaded", loaded), ("fitted", fitted)):
            got = model.predict(Xt)
            assert got.shape == (npx, T) and got.dtype == np.float32
            np.testing.assert_allclose(got, want, rtol=0, atol=2e-4, err_msg=f"{tag} T={T} npx={npx}")
    H, W = 37, 41
    cube = (600 + 4000 * np.clip(rng.random((H * W, 4)) @ rng.random((4, 10)) / 2, 0, 1)).astype(np.float32).T.reshape(10, H, W).copy()
    cube[2, 5, 6] = np.nan
    cube[7, 36, 40] = -9999.0
    want = onp.predict_cube_logit(ref, cube, nodata=-9999.0)
    for tag, model in (("loaded", loaded), ("fitted", fitted)):
        got = s2_emit.predict_cube_logit(model, cube, nodata=-9999.0)
        assert got.shape == (T, H, W)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-4, equal_nan=True, err_msg=f"{tag} T={T}")
    # every target really is its own row of W: permuting the targets of the model permutes the outputs, bit for bit
    perm = rng.permutation(T)
    shuffled = s2_emit.PolyRidge.from_params(ref["mean"], ref["scale"], ref["coef"][perm], ref["intercept"][perm], degree=3)
    Xt = (600 + 4000 * rng.random((300, 10))).astype(np.float32)
    np.testing.assert_array_equal(shuffled.predict(Xt), loaded.predict(Xt)[:, perm])


def test_poly_ridge_golden_g11_notebook_shapes(torch_gpu):
    """a9 at the notebook's own shapes, against scikit-learn and the notebook's predict_cube_logit frozen in g11:
    train (10000, 10) -> 32 targets (raw :426), predict_cube_logit on (10, 600, 600) -> (32, 600, 600) (raw :634) checked on
    the stored strided sample, one full row, the NaN count and per-band checksums; and the 97-target sklearn model (the
    sliced predict kernel against scikit-learn itself) on 257 pixels."""
    import s2_emit
    from conftest import g11_cube
    g = load_golden("g11_ridge_notebook_shapes")
    X = g["X"].astype(np.float32)
    Yl = onp.logit((g["Yu16"].astype(np.float32) * np.float32(1e-4)).astype(np.float64))
    model = s2_emit.PolyRidge(degree=3, alpha=1.0).fit(X, Yl)
    assert model.n_feat == 285 and model.coef_.shape == (32, 285)
    np.testing.assert_allclose(model.mean_, g["mean"], rtol=1e-12)
    np.testing.assert_allclose(model.scale_, g["scale"], rtol=1e-12)
    np.testing.assert_allclose(model.intercept_, g["intercept"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(model.predict(X[:512]), g["train_pred_logit"], rtol=0, atol=2e-4)
    cube = g11_cube(g)
    nodata = float(g["nodata"])
    for tag, m in (("fitted", model),
                   ("sklearn's parameters", s2_emit.PolyRidge.from_params(g["mean"], g["scale"], g["coef"], g["intercept"]))):
        pred = s2_emit.predict_cube_logit(m, cube, nodata=nodata)
        assert pred.shape == (32, 600, 600) and pred.dtype == np.float32
        fin = np.isfinite(pred)
        assert int((~fin).sum()) == int(g["pred_nan_count"]) == 32 * 7, tag
        for c_, i_, j_ in list(g["cube_nan"]) + list(g["cube_nd"]):
            assert np.isnan(pred[:, i_, j_]).all(), tag
        np.testing.assert_allclose(pred[:, ::7, ::11], g["pred_sample"], rtol=0, atol=1e-4, equal_nan=True, err_msg=tag)
        np.testing.assert_allclose(pred[:, 299, :], g["pred_rows_299"], rtol=0, atol=1e-4, equal_nan=True, err_msg=tag)
        zs = np.where(fin, pred, 0).astype(np.float64)
        np.testing.assert_allclose(zs.sum(axis=(1, 2)), g["pred_band_sum"], rtol=2e-6, err_msg=tag)        # 360 000 pixels per band
        np.testing.assert_allclose((zs ** 2).sum(axis=(1, 2)), g["pred_band_sumsq"], rtol=4e-6, err_msg=tag)
    # 97 targets: fit on 2000 pixels, predict 257
    Yl2 = onp.logit((g["Y2u16"].astype(np.float32) * np.float32(1e-4)).astype(np.float64))
    m2 = s2_emit.PolyRidge(degree=3, alpha=1.0).fit(X[:2000], Yl2)
    np.testing.assert_allclose(m2.intercept_, g["intercept2"], rtol=1e-6, atol=1e-7)
    Xt2 = g["Xtest2"].astype(np.float32)
    np.testing.assert_allclose(m2.predict(Xt2), g["pred2_logit"], rtol=0, atol=2e-4)
    m2s = s2_emit.PolyRidge.from_params(m2.mean_, m2.scale_, g["coef2"], g["intercept2"])
    np.testing.assert_allclose(m2s.predict(Xt2), g["pred2_logit"], rtol=0, atol=2e-4)


# ---------------------------------------------------------------------------------------------
# f1 resamplers and the reference-ordered driver (a7)
# ---------------------------------------------------------------------------------------------
def test_upsample_mask_limits_in_one_chain_bit_identical(torch_gpu):
    """hsr_bilinear_upsample_mask_hist (r03): the upsampler also writes the finite mask and counts the first radix pass of the
    percentile select.  Fine image, mask and limits must carry the bits of bilinear_upsample + valid_mask + percentile_limits:
    ragged sizes (a last column block and a last row block that are not full), 1-4 bands, NaN / Inf pixels in the coarse image
    (they spread to their fine neighbours), a coarse image that is all NaN (empty mask -> NaN limits), 16-byte rows or not."""
    torch = torch_gpu
    from s2_emit import _engine as eng, _native as nat
    rng = np.random.default_rng(77)
    for Hc, Wc, f, nb in ((37, 45, 6, 3), (64, 64, 6, 3), (9, 130, 3, 4), (50, 7, 10, 1), (33, 33, 2, 2)):
        row = eng.padded_row(nb)
        c = np.zeros((Hc * Wc, row), np.float32)
        c[:, :nb] = (rng.random((Hc * Wc, nb)) ** 2).astype(np.float32)
        c[5, 0] = np.nan
        c[Hc * Wc // 2, nb - 1] = np.inf
        c[-1, 0] = -np.inf
        for variant in ("data", "allnan"):
            cd = torch.from_numpy(c if variant == "data" else np.full_like(c, np.nan)).cuda()
            fine, mask, lohi = eng.bilinear_upsample_mask_limits(cd, Hc, Wc, f, 2, 98, nb=nb)
            ref_f = eng.bilinear_upsample(cd, Hc, Wc, f, layout=nat.PIXMAJOR, nb=nb)
            ref_m = eng.valid_mask(ref_f, -1, None, None, nat.PIXMAJOR, nbx=nb)
            ref_l = eng.percentile_limits(ref_f, ref_m, 2, 98, nat.PIXMAJOR, nb=nb)
            assert torch.equal(fine.view(torch.int32)[:, :nb], ref_f.view(torch.int32)[:, :nb]), (Hc, Wc, f, nb, variant)
            assert torch.equal(mask, ref_m), (Hc, Wc, f, nb, variant)
            assert torch.equal(lohi.view(torch.int64), ref_l.view(torch.int64)), (Hc, Wc, f, nb, variant, lohi, ref_l)
            if variant == "data":
                assert 0 < int(mask.sum()) < mask.numel()


def test_resamplers_vs_oracle(torch_gpu):
    torch = torch_gpu
    from s2_emit import _engine as eng
    from s2_emit import _native as nat
    rng = np.random.default_rng(41)
    fine8 = rng.integers(0, 256, (3, 30, 42), dtype=np.uint8)
    ref = onp.block_mean(fine8, 6)
    ref = ref * np.float32(1.0 / 255.0)
    got = eng.block_mean(torch.from_numpy(fine8).cuda().reshape(3, -1), 5, 7, 6, 1.0 / 255.0).cpu().numpy()
    np.testing.assert_array_equal(got.reshape(3, 5, 7), ref)
    fine32 = rng.random((2, 24, 16)).astype(np.float32)
    got = eng.block_mean(torch.from_numpy(fine32).cuda().reshape(2, -1), 6, 4, 4).cpu().numpy()
    np.testing.assert_allclose(got.reshape(2, 6, 4), onp.block_mean(fine32, 4), rtol=1e-7)
    pm = torch.from_numpy(np.ascontiguousarray(np.moveaxis(fine8, 0, -1))).cuda().reshape(-1, 3)   # (npix, 3) uint8
    got_pm = eng.block_mean(pm, 5, 7, 6, 1.0 / 255.0, layout=nat.PIXMAJOR, nb=3)
    np.testing.assert_array_equal(got_pm[:, :3].t().cpu().numpy().reshape(3, 5, 7), ref)
    # shapes whose fine rows are 16-byte multiples take the LDS-staged kernel (one full 64-pixel segment + a
    # ragged one): same (dy, dx) summation order -> same bits as the restatement, all dtypes and both layouts
    for f_, Wc_ in ((6, 80), (4, 72), (2, 200)):
        Hc_ = 5
        a8 = rng.integers(0, 256, (3, Hc_ * f_, Wc_ * f_), dtype=np.uint8)
        want8 = onp.block_mean(a8, f_) * np.float32(1.0 / 255.0)
        got = eng.block_mean(torch.from_numpy(a8).cuda().reshape(3, -1), Hc_, Wc_, f_, 1.0 / 255.0)
        np.testing.assert_array_equal(got.cpu().numpy().reshape(3, Hc_, Wc_), want8)
        pm8 = torch.from_numpy(np.ascontiguousarray(np.moveaxis(a8, 0, -1))).cuda().reshape(-1, 3)
        got = eng.block_mean(pm8, Hc_, Wc_, f_, 1.0 / 255.0, layout=nat.PIXMAJOR, nb=3)
        np.testing.assert_array_equal(got[:, :3].t().cpu().numpy().reshape(3, Hc_, Wc_), want8)
        got = eng.block_mean(pm8, Hc_, Wc_, f_, 1.0 / 255.0, layout=nat.PIXMAJOR, out_layout=nat.PLANAR, nb=3)
        np.testing.assert_array_equal(got.cpu().numpy().reshape(3, Hc_, Wc_), want8)
        a32 = rng.random((2, Hc_ * f_, Wc_ * f_)).astype(np.float32)
        got = eng.block_mean(torch.from_numpy(a32).cuda().reshape(2, -1), Hc_, Wc_, f_)
        np.testing.assert_array_equal(got.cpu().numpy().reshape(2, Hc_, Wc_), onp.block_mean(a32, f_))
        a16 = rng.integers(0, 65536, (2, Hc_ * f_, Wc_ * f_), dtype=np.uint16)
        got = eng.block_mean(torch.from_numpy(a16).cuda().reshape(2, -1), Hc_, Wc_, f_, 1e-4)
        np.testing.assert_array_equal(got.cpu().numpy().reshape(2, Hc_, Wc_), onp.block_mean(a16, f_) * np.float32(1e-4))
    coarse = rng.random((3, 9, 11)).astype(np.float32)
    coarse[1, 4, 4] = np.nan
    up = eng.bilinear_upsample(torch.from_numpy(coarse).cuda().reshape(3, -1), 9, 11, 6).cpu().numpy().reshape(3, 54, 66)
    refu = onp.bilinear_upsample(coarse, 6)
    assert np.array_equal(np.isnan(up), np.isnan(refu))
    np.testing.assert_allclose(up[~np.isnan(refu)], refu[~np.isnan(refu)], rtol=2e-7, atol=1e-7)
    # same float64 expressions in the same order, no contraction: the bits agree too; all output layouts and the
    # 16-byte store path for band-last rows of 4, on a grid that is not a multiple of the 256 x 8 workgroup block
    big = rng.random((3, 37, 50)).astype(np.float32)
    refb = onp.bilinear_upsample(big, 6)
    bd = torch.from_numpy(big).cuda().reshape(3, -1)
    up_pl = eng.bilinear_upsample(bd, 37, 50, 6).cpu().numpy().reshape(3, 222, 300)
    np.testing.assert_array_equal(up_pl, refb)
    up_pm = eng.bilinear_upsample(bd, 37, 50, 6, "planar", "pixmajor")            # (npix, 4): vector store path
    assert up_pm.shape == (222 * 300, 4)
    np.testing.assert_array_equal(up_pm[:, :3].t().cpu().numpy().reshape(3, 222, 300), refb)
    pm_in = torch.from_numpy(np.ascontiguousarray(np.moveaxis(big, 0, -1))).cuda().reshape(-1, 3)
    up_pp = eng.bilinear_upsample(pm_in, 37, 50, 6, "pixmajor", "planar", nb=3)
    np.testing.assert_array_equal(up_pp.cpu().numpy().reshape(3, 222, 300), refb)
    five = rng.random((5, 8, 9)).astype(np.float32)
    up5 = eng.bilinear_upsample(torch.from_numpy(five).cuda().reshape(5, -1), 8, 9, 3, "planar", "pixmajor")   # rows of 8: scalar stores
    np.testing.assert_array_equal(up5[:, :5].t().cpu().numpy().reshape(5, 24, 27), onp.bilinear_upsample(five, 3))


@pytest.mark.parametrize("use_ot", [False, True])
def test_match_pair_reference_driver(torch_gpu, use_ot):
    """The whole reference driver (poly_regression.py:96-172) on a synthetic aligned pair vs the oracle."""
    import s2_emit
    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths()
    H, W, f = 40, 36, 6
    R = onp.synthetic_cube(H, W, seed=21)
    R[3, 4, :] = -0.01                       # B2 <= 0 -> invalid at 60 m
    R[10, 10, 50] = np.nan                   # non-finite spectrum
    rng = np.random.default_rng(5)
    ps = onp.pseudo_s2_srf_integral(R, w, srf, good)
    rgb60 = np.stack([ps["B4"], ps["B3"], ps["B2"]], -1)
    hi = np.repeat(np.repeat(np.nan_to_num(rgb60, nan=0.1), f, 0), f, 1)
    # (clip before the power: a negative base gave NaN, and NaN -> uint8 is platform-defined)
    s2_hi = np.clip((np.clip(hi, 0, None) / 0.45) ** 0.8 * 255 + rng.normal(0, 6, hi.shape), 0, 255).astype(np.uint8)
    ref = onp.match_pair_reference(R, w, srf, good, s2_hi, f, deg=4 if use_ot else 3, use_ot=use_ot, n_samples=600)
    got = s2_emit.match_pair(R, w, srf, good, s2_hi, f, deg=4 if use_ot else 3, use_ot=use_ot, n_samples=600)
    assert np.array_equal(got["valid60"], ref["valid60"]) and not ref["valid60"][3, 4] and not ref["valid60"][10, 10]
    assert np.array_equal(got["mask10"], ref["mask10"])
    np.testing.assert_array_equal(got["s2_rgb_60m_n"], ref["s2_rgb_60m_n"])          # integer-exact path: bit-identical
    # Error budget in stretched units (measured stage by stage, tools/dbg/match_pair_budget.py): the float32 K1 planes
    # move the percentile limits by 4e-8 over a range of 0.15 -> stretched x off by <= 3e-7 (+ 6e-8 float32 rounding);
    # the fitted curves have slope <= 1.1 and themselves differ by 2e-7 -> matched images off by 5e-7 (60 m) / 8e-7
    # (10 m, bilinear weights in between).  1e-5 leaves a factor 10; the north-star target is 1e-4.
    xs = np.linspace(0, 1, 33)
    for c in range(3):
        np.testing.assert_allclose(np.polyval(got["coeffs"][c], xs), np.polyval(ref["coeffs"][c], xs), rtol=0, atol=2e-6)
    m = ref["valid60"]
    np.testing.assert_allclose(got["emit_rgb_matched_60m"][m], ref["emit_rgb_matched_60m"][m], rtol=0, atol=1e-5)
    m10 = ref["mask10"]
    np.testing.assert_allclose(got["emit_rgb_10m_matched"][m10], ref["emit_rgb_10m_matched"][m10], rtol=0, atol=1e-5)
    assert np.array_equal(np.isnan(got["emit_rgb_10m_matched"]), np.isnan(ref["emit_rgb_10m_matched"]))


def test_match_pair_two_streams_same_bits_from_any_stream(torch_gpu):
    """r04: match_pair runs its 10 m producer chain and one of the 60 m selects on side streams.  Called repeatedly, and from inside a
    non-default current stream with work queued in front of it, it returns the bits of the first call (the event / wait_stream
    bracket follows the CURRENT stream; nothing waits on the host)."""
    torch = torch_gpu
    import s2_emit
    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths()
    H, W, f = 64, 48, 6
    R = onp.synthetic_cube(H, W, seed=77)
    rng = np.random.default_rng(9)
    ps = onp.pseudo_s2_srf_integral(R, w, srf, good)
    rgb60 = np.stack([ps["B4"], ps["B3"], ps["B2"]], -1)
    hi = np.repeat(np.repeat(rgb60, f, 0), f, 1)
    s2_hi = np.clip((np.clip(hi, 0, None) / 0.45) ** 0.8 * 255 + rng.normal(0, 5, hi.shape), 0, 255).astype(np.uint8)
    first = s2_emit.match_pair(R, w, srf, good, s2_hi, f, deg=3, use_ot=False)
    keys = ("coeffs", "emit_rgb_matched_60m", "emit_rgb_10m_matched", "mask10", "valid60")
    for rep in range(3):
        again = s2_emit.match_pair(R, w, srf, good, s2_hi, f, deg=3, use_ot=False)
        for k in keys:
            np.testing.assert_array_equal(np.asarray(again[k]), np.asarray(first[k]), err_msg=f"default stream, call {rep}: {k}")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        junk = torch.rand((4096, 4096), device="cuda")
        for _ in range(20):                              # work in front of the call on this stream
            junk = junk * 1.0001 + 0.5
        other = s2_emit.match_pair(R, w, srf, good, s2_hi, f, deg=3, use_ot=False)
    st.synchronize()
    for k in keys:
        np.testing.assert_array_equal(np.asarray(other[k]), np.asarray(first[k]), err_msg=f"side stream: {k}")


def test_pipelined_submit_flush_matches_step(torch_gpu):
    """submit()/flush() (one tile in flight on a side stream) must reproduce step() bit for bit, tile by tile."""
    torch = torch_gpu
    from s2_emit import SpectralFusion
    from s2_emit import _native as nat
    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths()
    tiles = []
    for seed in range(4):
        R = torch.from_numpy(onp.synthetic_cube(64, 48, seed=30 + seed)).cuda()
        ps = onp.pseudo_s2_srf_integral(R.cpu().numpy(), w, srf, good)
        names = [k for k, v in ps.items() if v is not None]
        real = torch.from_numpy(onp.synthetic_real_planes(np.stack([ps[k] for k in names]).astype(np.float32), seed=seed)).cuda()
        tiles.append((R, real))
    for reserve in (0, 1, 8):     # the reserved CUs belong to the plan: step() and submit() of one plan always agree
        ref_plan = SpectralFusion(w, srf, good, deg=3, reserved_cus=reserve)
        refs = []
        for R, real in tiles:
            o = ref_plan.step(R, real, reuse_buffers=False)
            refs.append((o.coeffs.clone(), o.matched.clone()))
        plan = SpectralFusion(w, srf, good, deg=3, reserved_cus=reserve)
        outs = []
        for R, real in tiles:
            o = plan.submit(R, real)
            if o is not None:
                outs.append((o.coeffs.clone(), o.matched.clone()))
        o = plan.flush()
        outs.append((o.coeffs.clone(), o.matched.clone()))
        assert plan.flush() is None
        torch.cuda.synchronize()
        assert len(outs) == len(refs) == 4
        for (c, m), (rc, rm) in zip(outs, refs):
            assert torch.equal(c, rc) and torch.equal(m.view(torch.int32), rm.view(torch.int32))


# ---------------------------------------------------------------------------------------------
# edge cases: degenerate fits, limits, error paths
# ---------------------------------------------------------------------------------------------
def test_fused_degenerate_fits(torch_gpu):
    """All-masked / too-few / constant inputs: the reference's soft fallbacks, no NaNs, no crashes."""
    torch = torch_gpu
    from s2_emit import SpectralFusion
    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths()
    R = onp.synthetic_cube(16, 16, seed=2)
    ps = onp.pseudo_s2_srf_integral(R, w, srf, good)
    names = [k for k, v in ps.items() if v is not None]
    pseudo = np.stack([ps[k] for k in names]).astype(np.float32)
    real = onp.synthetic_real_planes(pseudo)
    Rd, reald = torch.from_numpy(R).cuda(), torch.from_numpy(real).cuda()
    ident = np.array([0.0, 0.0, 1.0, 0.0])
    # (1) mask of zeros -> count 0 -> identity polynomial for every band (min_count = 50)
    plan = SpectralFusion(w, srf, good, deg=3, min_count=50)
    out = plan.step(Rd, reald, mask=torch.zeros(256, dtype=torch.uint8, device="cuda"), reuse_buffers=False)
    assert np.array_equal(out.coeffs.cpu().numpy(), np.tile(ident, (12, 1))) and (out.moments.cpu().numpy() == 0).all()
    np.testing.assert_array_equal(out.planes("matched").cpu().numpy(), np.clip(out.planes("pseudo").cpu().numpy(), 0, 1))
    # (2) 49 valid pixels < 50 -> identity; 50 -> a fit
    m = np.zeros(256, np.uint8)
    m[:49] = 1
    out = plan.step(Rd, reald, mask=torch.from_numpy(m).cuda(), reuse_buffers=False)
    assert np.array_equal(out.coeffs.cpu().numpy(), np.tile(ident, (12, 1))) and (out.moments.cpu().numpy()[:, 0] == 49).all()
    m[49] = 1
    out = plan.step(Rd, reald, mask=torch.from_numpy(m).cuda(), reuse_buffers=False)
    assert not np.array_equal(out.coeffs.cpu().numpy()[0], ident) and np.isfinite(out.coeffs.cpu().numpy()).all()
    # (3) constant cube -> rank-1 Vandermonde -> minimum-norm fit like np.polyfit, finite everywhere
    Rc = torch.full((16, 16, 285), 0.25, dtype=torch.float32, device="cuda")
    out = SpectralFusion(w, srf, good, deg=2, min_count=10).step(Rc, reald, reuse_buffers=False)
    assert torch.isfinite(out.coeffs).all() and torch.isfinite(out.matched[:, :12]).all()
    x0 = float(out.planes("pseudo")[0, 0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = np.polyfit(np.full(256, np.float64(np.float32(x0))), real[0].reshape(-1).astype(np.float64), 2)
    np.testing.assert_allclose(np.polyval(out.coeffs[0].cpu().numpy(), x0), np.polyval(ref, x0), rtol=1e-6)
    # ... and the coefficients themselves, which K3 evaluates at every pixel: the minimum-norm solution is unique
    c0 = out.coeffs[0].cpu().numpy()
    assert np.max(np.abs(c0 - ref)) <= 1e-9 * np.max(np.abs(ref)), (c0, ref)
    # (4) a single band and deg 4
    one = {"B4": srf["B4"]}
    r1 = torch.from_numpy(real[names.index("B4")][None]).cuda()
    out = SpectralFusion(w, one, good, deg=4, min_count=50).step(Rd, r1, reuse_buffers=False)
    xs = pseudo[names.index("B4")].reshape(-1).astype(np.float64)
    ref = np.polyfit(xs, real[names.index("B4")].reshape(-1).astype(np.float64), 4)
    np.testing.assert_allclose(np.polyval(out.coeffs[0].cpu().numpy(), xs), np.polyval(ref, xs), rtol=0, atol=2e-5)


def test_limits_and_error_paths(torch_gpu):
    torch = torch_gpu
    import s2_emit
    from s2_emit import _engine as eng
    from s2_emit import _native as nat
    lam = np.arange(300.0, 2600.0)
    srf = {"A": (lam, np.exp(-0.5 * ((lam - 900) / 60) ** 2)), "Z": (lam, np.exp(-0.5 * ((lam - 2300) / 200) ** 2))}
    # the largest supported spectrum (B = 560, even -> padded LDS rows, generic loader, 1 workgroup per CU)
    B = nat.HSR_MAX_SPECTRAL
    w = np.linspace(400, 2500, B).astype(np.float32)
    R = (np.random.default_rng(1).random((9, 13, B)) * 0.5).astype(np.float32)
    ref = onp.pseudo_s2_srf_integral(R, w, srf, None)
    got = s2_emit.pseudo_s2_srf_integral(R, w, srf, None)
    for k in srf:
        assert _rel_err(got[k], ref[k]) < 3e-6
    # wide supports: more taps than the LDS weight area holds -> weights read from global memory
    wide = {f"W{i}": (lam, np.ones_like(lam)) for i in range(8)}
    w285, _ = onp.synthetic_wavelengths()
    R2 = onp.synthetic_cube(8, 8, seed=6)
    ref = onp.pseudo_s2_srf_integral(R2, w285, wide, None)
    got = s2_emit.pseudo_s2_srf_integral(R2, w285, wide, None)
    for k in wide:
        assert _rel_err(got[k], ref[k]) < 3e-6
    # B beyond the limit is refused with a message, not silently mis-computed
    big = torch.zeros((4, B + 1), dtype=torch.float32, device="cuda")
    table = eng.build_srf_table(np.linspace(400, 2500, B + 1), srf, None)
    with pytest.raises(nat.HsrError) as ei:
        eng.srf_integrate(big, table)
    assert "outside [1,560]" in str(ei.value)
    with pytest.raises(ValueError):
        eng.srf_integrate(torch.zeros((4, 285), dtype=torch.float64, device="cuda"), table)
    with pytest.raises(ValueError):
        s2_emit.SpectralFusion(w285, onp.synthetic_srf(), None, deg=5)
    with pytest.raises(ValueError) as ei:
        s2_emit.match_pair(R2, w285, {"B4": srf["A"]}, None, np.zeros((48, 48, 3), np.uint8))
    assert "Band B3 is None/missing in pseudo_s2." in str(ei.value)
    # apply_poly_rgb keeps channels beyond len(coeffs) untouched except for the clip, like the reference
    rgb = (np.random.default_rng(2).random((5, 7, 4)) * 1.4 - 0.2).astype(np.float32)
    co = np.array([[0.5, 0.2], [1.0, 0.0], [2.0, -0.1]])
    np.testing.assert_array_equal(s2_emit.apply_poly_rgb(rgb, co), np.concatenate(
        [onp.apply_poly_rgb(rgb[..., :3].copy(), co), np.clip(rgb[..., 3:], 0, 1)], axis=-1))


@pytest.mark.parametrize("B", [1, 2, 3, 7, 15, 16, 17, 33, 64, 129, 286, 559])
def test_k1_spectral_size_sweep(torch_gpu, B):
    """Every loader / weight-staging branch: tiny B (weights from global memory: the 16-tap chunks do not fit
    the row), even B (padded LDS rows, generic loader), odd B (LDS-DMA path), both tile geometries, both layouts."""
    torch = torch_gpu
    from s2_emit import _engine as eng
    from s2_emit import _native as nat
    rng = np.random.default_rng(B)
    w = np.linspace(400.0, 2400.0, B).astype(np.float32) if B > 1 else np.array([900.0], np.float32)
    lam = np.arange(300.0, 2600.0)
    srf = {f"S{i}": (lam, np.exp(-0.5 * ((lam - c) / s) ** 2) + 1e-12)
           for i, (c, s) in enumerate(((450, 40), (900, 150), (1600, 90), (2200, 300), (1250, 700)))}
    H, W = 5, 29                      # 145 pixels: two full 64-pixel tiles + a ragged one
    R = (rng.random((H, W, B)) * 0.7 - 0.05).astype(np.float32)
    if B > 2:
        R[2, 3, B // 2] = np.nan
        R[4, 28, B - 1] = -np.inf
    ref = onp.pseudo_s2_srf_integral(R, w, srf, None)
    table = eng.build_srf_table(w, srf, None)
    names = [k for k, v in ref.items() if v is not None]
    assert table.supported == names
    if not names:
        return
    cube = torch.from_numpy(R).cuda()
    base = None
    for tile in (64, 0):
        o = eng.srf_options(tile_pixels=tile)
        pl = eng.srf_integrate(cube, table, layout=nat.PLANAR, opts=o)
        pm = eng.srf_integrate(cube, table, layout=nat.PIXMAJOR, opts=o)
        got = pl.cpu().numpy().reshape(len(names), H, W)
        for i, k in enumerate(names):
            assert _rel_err(got[i], ref[k]) < 3e-6, (B, tile, k)
        assert torch.equal(pm[:, :len(names)].t().contiguous().view(torch.int32), pl.view(torch.int32))
        if base is None:
            base = pl.clone()
        assert torch.equal(base.view(torch.int32), pl.view(torch.int32))      # tile geometry does not change bits


def test_envi_loader_device_path(torch_gpu, tmp_path):
    """BSQ / BIL / BIP files -> pixel-major (H, W, B) float32 GPU tensor == the host loader, then K1 on it."""
    torch = torch_gpu
    import s2_emit
    rng = np.random.default_rng(0)
    cube = (rng.random((11, 13, 285)) * 0.5).astype(np.float32)
    for inter, arr in (("bip", cube), ("bil", cube.transpose(0, 2, 1)), ("bsq", cube.transpose(2, 0, 1))):
        np.ascontiguousarray(arr).tofile(tmp_path / f"c_{inter}.bin")
        (tmp_path / f"c_{inter}.hdr").write_text(
            f"ENVI\nsamples = 13\nlines = 11\nbands = 285\nheader offset = 0\ndata type = 4\n"
            f"interleave = {inter}\nbyte order = 0\n")
        Rh = s2_emit.load_emit_envi_rfl(str(tmp_path / f"c_{inter}.hdr"), str(tmp_path / f"c_{inter}.bin"))
        Rd = s2_emit.load_emit_envi_rfl(str(tmp_path / f"c_{inter}.hdr"), str(tmp_path / f"c_{inter}.bin"), device="cuda")
        assert Rd.is_cuda and Rd.dtype == torch.float32 and Rd.is_contiguous() and tuple(Rd.shape) == (11, 13, 285)
        np.testing.assert_array_equal(Rd.cpu().numpy(), Rh)
        np.testing.assert_array_equal(Rh, cube)
    w, good = onp.synthetic_wavelengths()
    srf = onp.synthetic_srf()
    out = s2_emit.pseudo_s2_srf_integral(Rd, w, srf, good)
    ref = onp.pseudo_s2_srf_integral(cube, w, srf, good)
    assert _rel_err(out["B4"].cpu().numpy(), ref["B4"]) < 2e-6


def test_ot_color_transfer_and_ot_fit_vs_oracle(torch_gpu):
    """ot_match_rgb_sinkhorn_pot (color.py:65-116) and fit_ot_poly_rgb (poly_regression.py:16-62): device
    Sinkhorn vs the oracle's restatement of POT's documented algorithm (parity with POT itself unpinned)."""
    import s2_emit
    rng = np.random.default_rng(77)
    H, W = 48, 40
    src = rng.random((H, W, 3)) ** 1.5
    ref = np.clip(0.8 * src[..., ::-1] + 0.1 + 0.03 * rng.standard_normal((H, W, 3)), 0, 1)
    mask = rng.random((H, W)) > 0.15
    src[2, 3, 1] = np.nan
    got = s2_emit.ot_match_rgb_sinkhorn_pot(src, ref, mask, n_samples=700, seed=3)
    want = onp.ot_match_rgb_sinkhorn_pot(src, ref, mask, n_samples=700, seed=3)
    assert got.dtype == np.float32 and got.shape == src.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got[~np.isnan(want)], want[~np.isnan(want)], rtol=0, atol=5e-5)
    c_got = s2_emit.fit_ot_poly_rgb(src, ref, mask, deg=3, n_samples=700, seed=3)
    c_want = onp.fit_ot_poly_rgb(src, ref, mask, deg=3, n_samples=700, seed=3)
    xs = np.linspace(0, 1, 41)
    for c in range(3):
        np.testing.assert_allclose(np.polyval(c_got[c], xs), np.polyval(c_want[c], xs), rtol=0, atol=5e-5)
    # too few rows -> source returned unchanged (color.py:88-89)
    tiny = np.zeros((H, W), bool)
    tiny[0, 0] = True
    np.testing.assert_array_equal(s2_emit.ot_match_rgb_sinkhorn_pot(src, ref, tiny), src)


def test_global_percentiles_across_simulated_ranks(torch_gpu):
    """Distributed order statistic: three 'ranks' (three pixel shards on one GPU) exchange only the integer
    histogram of each radix-select pass (summed here by hand, by RCCL all-reduce in a real job) and must all
    arrive at np.percentile of the union - exactly."""
    torch = torch_gpu
    from s2_emit import _engine as eng
    rng = np.random.default_rng(99)
    nb = 3
    shards = [rng.standard_normal((nb, n)).astype(np.float32) * s + o for n, s, o in ((30011, 1.0, 0.0), (777, 5.0, 2.0), (12000, 0.1, -3.0))]
    masks = [rng.random(x.shape[1]) > 0.3 for x in shards]
    xs = [torch.from_numpy(x).cuda() for x in shards]
    ms = [torch.from_numpy(m.view(np.uint8)).cuda() for m in masks]
    R = len(xs)
    # lock-step emulation: a per-pass buffer collects every rank's histogram; each rank's turn k contributes
    # its region, and a second sweep overwrites every rank's region with the sum (what all-reduce does)
    import threading
    results = [None] * R
    barrier = threading.Barrier(R)
    shared = {}
    lock = threading.Lock()

    def worker(r):
        torch.cuda.set_device(0)

        def red(p, region):
            torch.cuda.synchronize()
            with lock:
                shared.setdefault(p, torch.zeros_like(region))
                shared[p] += region
            barrier.wait()
            region.copy_(shared[p])
            torch.cuda.synchronize()
            barrier.wait()
        results[r] = eng.percentile_limits(xs[r], ms[r], 2, 98, _reduce=red).cpu().numpy()

    ts = [threading.Thread(target=worker, args=(r,)) for r in range(R)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    allx = np.concatenate([x[:, m] for x, m in zip(shards, masks)], axis=1)
    ref = np.array([np.percentile(allx[c], [2, 98]) for c in range(nb)])
    for r in range(R):
        np.testing.assert_array_equal(results[r], ref)
    # and the single-rank pass-by-pass path equals the one-call path
    a = eng.percentile_limits(xs[0], ms[0], 5, 95).cpu().numpy()
    b = eng.percentile_limits(xs[0], ms[0], 5, 95, _reduce=lambda p, region: None).cpu().numpy()
    np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------------------------
# uint16 tiles: writer quantisation bit-exact, K1 on the 2-byte cube
# ---------------------------------------------------------------------------------------------
def test_tile_u16_codec_bitexact(torch_gpu):
    torch = torch_gpu
    from s2_emit import _engine as eng
    g = load_golden("g10_tile_u16")
    t = torch.from_numpy(g["tile"]).cuda()
    np.testing.assert_array_equal(eng.tile_encode_u16(t).cpu().numpy(), g["u16_plain"])
    np.testing.assert_array_equal(eng.tile_encode_u16(t, src_nodata=-9999.0).cpu().numpy(), g["u16_srcnodata"])
    np.testing.assert_array_equal(eng.tile_encode_u16(t, 2000.0, None, 4095).cpu().numpy(), g["u16_scale2000_nd4095"])
    # a big random array with every float32 exponent, the specials sprinkled in, odd length and an odd offset
    rng = np.random.default_rng(77)
    x = (rng.standard_normal(1_000_003) * np.exp(rng.uniform(-12, 25, 1_000_003))).astype(np.float32)
    x[::1013] = np.nan
    x[5::4099] = -9999.0
    x[7::5003] = np.inf
    ties = (rng.integers(0, 70000, 50000) + 0.5) / 10000.0
    x[100:100 + ties.size] = ties.astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    with np.errstate(all="ignore"):
        ref = onp.tile_encode_u16(x, src_nodata=-9999.0)
    np.testing.assert_array_equal(eng.tile_encode_u16(xd, src_nodata=-9999.0).cpu().numpy(), ref)
    np.testing.assert_array_equal(eng.tile_encode_u16(xd[1:].clone()[2:], src_nodata=-9999.0).cpu().numpy(), ref[3:])   # 8-byte offset: scalar path
    np.testing.assert_array_equal(eng.tile_encode_u16(xd[1:1000].contiguous()).cpu().numpy(), onp.tile_encode_u16(x[1:1000]))
    # decode: all 65536 codes, bit-exact against float32(u) * float32(1e-4), NaN at nodata
    codes = np.arange(65536, dtype=np.uint16)
    dec = eng.tile_decode_u16(torch.from_numpy(codes).cuda()).cpu().numpy()
    np.testing.assert_array_equal(dec.view(np.uint32)[:-1], onp.tile_decode_u16(codes).view(np.uint32)[:-1])
    assert np.isnan(dec[-1])
    dec2 = eng.tile_decode_u16(torch.from_numpy(codes[3:60001]).cuda().clone(), scale=0.5e-3, nodata=None).cpu().numpy()
    np.testing.assert_array_equal(dec2, onp.tile_decode_u16(codes[3:60001], 0.5e-3, None))
    assert eng.tile_encode_u16(torch.empty(0, device="cuda")).numel() == 0


@pytest.mark.parametrize("npix,B,offset,nodata_mode", [(64 * 40, 285, 0, "some"), (64 * 7 + 13, 285, 0, "some"),
                                                       (1000, 285, 1, "some"), (640, 284, 0, "none"),
                                                       (64 * 9, 285, 0, "off"), (5, 285, 0, "some"), (4096, 64, 0, "some")])
def test_k1_on_u16_tiles_matches_decode_then_k1_bits(torch_gpu, npix, B, offset, nodata_mode):
    """K1(+K2) on the uint16 cube == hsr_tile_decode_u16 followed by the float32 K1, bit for bit, on the
    DMA path, the ragged last tile, a 2-byte-misaligned cube, an even band count and without nodata."""
    torch = torch_gpu
    from s2_emit import _engine as eng
    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths(B) if B == 285 else (np.linspace(400, 2400, B).astype(np.float32), None)
    table = eng.build_srf_table(w, srf, good)
    nb = table.nb
    rng = np.random.default_rng(npix + B)
    u = rng.integers(0, 6000, (npix, B)).astype(np.uint16)
    nodata = 65535
    if nodata_mode == "some":
        u[rng.integers(0, npix, max(1, npix // 50)), rng.integers(0, B, max(1, npix // 50))] = 65535
        u[npix - 1, B - 1] = 65535
        u[0, 0] = 65535
    elif nodata_mode == "off":
        u[3, 7] = 65535           # just a large sample when no nodata value is set
        nodata = None
    flat = torch.from_numpy(np.concatenate([np.zeros(offset, np.uint16), u.reshape(-1)])).cuda()
    ud = flat[offset:].view(npix, B) if offset == 0 else torch.as_strided(flat, (npix, B), (B, 1), offset)
    assert ud.is_contiguous() and ud.data_ptr() % 16 == (2 * offset) % 16
    f = eng.tile_decode_u16(ud.clone(), nodata=nodata)
    np.testing.assert_array_equal(f.cpu().numpy(), onp.tile_decode_u16(u, None, nodata))
    for layout in ("planar", "pixmajor"):
        a = eng.srf_integrate(ud, table, layout=layout, nodata=nodata)
        b = eng.srf_integrate(f, table, layout=layout)
        if layout == "pixmajor":          # rows are padded to a multiple of 4 floats; the padding is not written
            a, b = a[:, :nb], b[:, :nb]
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())       # NaN == NaN here
        fin = torch.isfinite(b)
        assert torch.equal(a[fin].view(torch.int32), b[fin].view(torch.int32))
    planes = eng.srf_integrate(f, table, layout="planar")
    if nodata_mode == "some":
        bad = (u == 65535).any(axis=1)
        assert bool(torch.isnan(planes[:, torch.from_numpy(bad).cuda()]).all())
        assert bool(torch.isfinite(planes[:, torch.from_numpy(~bad).cuda()]).all())
    # fused moments: same partial sums, same coefficients
    real = (torch.nan_to_num(planes, nan=0.1) * 1.1 + 0.01 + 0.01 * torch.randn_like(planes)).contiguous()
    mask = torch.from_numpy((rng.random(npix) > 0.2).astype(np.uint8)).cuda()
    for deg in (1, 3):
        ws_a, ws_b = eng.MomentWorkspace("cuda", nb, deg), eng.MomentWorkspace("cuda", nb, deg)
        pa, ma = eng.srf_integrate_moments(ud, table, real, deg, ws_a, mask, 0.0, 0.0, layout="pixmajor",
                                           real_layout="planar", nodata=nodata)
        pb, mb = eng.srf_integrate_moments(f, table, real, deg, ws_b, mask, 0.0, 0.0, layout="pixmajor", real_layout="planar")
        np.testing.assert_array_equal(pa[:, :nb].cpu().numpy(), pb[:, :nb].cpu().numpy())
        if (npix + 63) // 64 <= 512:          # same tile -> slot assignment in both kernels
            assert torch.equal(ma, mb)
        else:
            np.testing.assert_allclose(ma.cpu().numpy(), mb.cpu().numpy(), rtol=1e-12)
        assert ma[0, 0].item() > 0 or npix < 10


def test_fused_step_on_u16_cube(torch_gpu):
    """The whole hot path fed with the reference's on-disk tile format: encode (writer semantics) on the
    device, then SpectralFusion.step on the uint16 cube == step on the decoded float32 cube."""
    torch = torch_gpu
    from s2_emit import SpectralFusion, _engine as eng
    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths()
    H, W = 96, 80
    R = onp.synthetic_cube(H, W, seed=21)
    R[5, 6, 100] = np.nan                       # -> nodata code -> pixel NaN in every band
    R[9, 9, :] = -0.01                          # EMIT's masked-band fill clips to 0
    cube_f = torch.from_numpy(R).cuda()
    u = eng.tile_encode_u16(cube_f)
    np.testing.assert_array_equal(u.cpu().numpy(), onp.tile_encode_u16(R))
    dec = eng.tile_decode_u16(u)
    ps = onp.pseudo_s2_srf_integral(onp.tile_decode_u16(onp.tile_encode_u16(R)), w, srf, good)
    names = [k for k, v in ps.items() if v is not None]
    pseudo_ref = np.stack([ps[k] for k in names]).astype(np.float32)
    real = onp.synthetic_real_planes(np.nan_to_num(pseudo_ref, nan=0.1), seed=3)
    real_d = torch.from_numpy(real).cuda()
    plan = SpectralFusion(w, srf, good, deg=3, min_valid=0.0, min_count=50, clip=True)
    a = plan.step(u, real_d, reuse_buffers=False)
    b = plan.step(dec, real_d, reuse_buffers=False)
    assert torch.equal(a.coeffs, b.coeffs) and torch.equal(a.moments, b.moments)
    np.testing.assert_array_equal(a.matched.cpu().numpy(), b.matched.cpu().numpy())
    got = a.planes("pseudo").cpu().numpy().reshape(pseudo_ref.shape)
    assert np.isnan(got[:, 5, 6]).all() and np.isnan(pseudo_ref[:, 5, 6]).all()
    assert _rel_err(got, pseudo_ref) < 2e-6
    assert a.moments[0, 0].item() == onp.per_band_valid(pseudo_ref[0], real[0], np.ones((H, W), bool), 0.0).sum()
    # pipelined submit/flush takes the same dtype
    plan.submit(u, real_d)
    c = plan.flush()
    assert torch.equal(c.coeffs, a.coeffs)


# ---------------------------------------------------------------------------------------------
# device Sinkhorn (parity unpinned: POT absent - oracle restatement + invariants)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,nt,reg,itmax,thr", [(700, 640, 0.05, 300, 1e-6), (333, 401, 0.05, 300, 1e-6),
                                                 (512, 512, 0.02, 35, 0.0), (257, 129, 0.5, 300, 1e-9),
                                                 (64, 50, 0.05, 0, 1e-6)])
def test_device_sinkhorn_vs_oracle(torch_gpu, ns, nt, reg, itmax, thr):
    torch = torch_gpu
    from s2_emit import _ot
    rng = np.random.default_rng(ns + nt)
    X = rng.random((ns, 3))
    Y = np.clip(X[rng.integers(0, ns, nt)] ** 0.8 * 0.9 + 0.05 + 0.02 * rng.standard_normal((nt, 3)), 0, 1)
    want = onp.ot_barycentric_targets(X, Y, reg, itmax, thr)
    got, info = _ot.barycentric_targets_device(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), reg, itmax, thr,
                                               return_info=True)
    got = got.cpu().numpy()
    # same schedule as the restatement: replay it on the host to know where it stopped
    a, b = np.full(ns, 1 / ns), np.full(nt, 1 / nt)
    K = np.exp(onp.sqeuclidean_cost(X, Y) / -reg)
    u, v, stop, checks = a.copy(), b.copy(), None, 0
    for ii in range(itmax):
        v = b / (K.T @ u)
        u = a / (K @ v)
        if ii % 10 == 0:
            checks += 1
            if np.linalg.norm(v * (K.T @ u) - b) < thr:
                stop = ii
                break
    assert info["break_iter"] is None and info["conv_iter"] == stop and info["checks"] == checks
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)
    # invariants of the plan behind the targets: rows of P sum to a (after the u update), targets are convex
    # combinations of Y
    assert (got.min(0) >= Y.min(0) - 1e-12).all() and (got.max(0) <= Y.max(0) + 1e-12).all()
    # run-to-run bitwise reproducible (fixed summation trees, no float atomics)
    again = _ot.barycentric_targets_device(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), reg, itmax, thr)
    assert np.array_equal(again.cpu().numpy().view(np.int64), got.view(np.int64))
    # enqueueing in blocks with a look at the device state in between stops early and changes nothing
    for k in (7, 50):
        polled, pinfo = _ot.barycentric_targets_device(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), reg, itmax, thr,
                                                       return_info=True, poll_every=k)
        assert np.array_equal(polled.cpu().numpy().view(np.int64), got.view(np.int64))
        assert pinfo["conv_iter"] == info["conv_iter"] and pinfo["checks"] == info["checks"]


def test_device_sinkhorn_breakdown_keeps_previous_iterate(torch_gpu):
    """reg so small that K underflows to 0 for a far-away target: K^T u == 0 -> POT keeps the previous (u, v)."""
    torch = torch_gpu
    from s2_emit import _ot
    rng = np.random.default_rng(5)
    X = rng.random((200, 3)) * 0.1
    Y = rng.random((180, 3)) * 0.1
    Y[7] = 50.0                                   # exp(-~7500/0.01) == 0 in float64
    with np.errstate(all="ignore"):
        want = onp.ot_barycentric_targets(X, Y, 0.01, 50, 1e-9)
    got, info = _ot.barycentric_targets_device(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), 0.01, 50, 1e-9,
                                               return_info=True)
    assert info["break_iter"] == 0 and info["conv_iter"] is None and info["checks"] == 0
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-9, atol=1e-12)


# ---------------------------------------------------------------------------------------------
# host -> device tile feed: double-buffered H2D under compute == tile-by-tile step()
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,kind", [(2, "f32"), (1, "f32"), (3, "u16")])
def test_stream_host_tiles_matches_step(torch_gpu, depth, kind):
    torch = torch_gpu
    from s2_emit import SpectralFusion
    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths()
    H, W = 48, 40
    plan = SpectralFusion(w, srf, good, deg=2, min_valid=0.0, min_count=50, clip=True)
    tiles, expect = [], []
    for i in range(5):
        R = onp.synthetic_cube(H, W, seed=100 + i)
        if kind == "u16":
            R = onp.tile_encode_u16(R)
        ps = onp.pseudo_s2_srf_integral(onp.tile_decode_u16(R) if kind == "u16" else R, w, srf, good)
        real = onp.synthetic_real_planes(np.stack([ps[k] for k in plan.names]).astype(np.float32), seed=i)
        mask = (np.random.default_rng(i).random((H, W)) > 0.1) if i % 2 else None
        # pinned tensors and plain NumPy arrays are both accepted
        cube_in = SpectralFusion.pinned_like(R) if i % 2 == 0 else R
        tiles.append((cube_in, real, mask))
        o = plan.step(torch.from_numpy(R).cuda(), torch.from_numpy(real).cuda(),
                      None if mask is None else torch.from_numpy(mask.view(np.uint8).reshape(-1)).cuda(), reuse_buffers=False)
        expect.append((o.coeffs.cpu().numpy(), o.matched.cpu().numpy()))
    seen = []
    for i, coeffs, matched, out in plan.stream(iter(tiles), depth=depth):
        seen.append(i)
        np.testing.assert_array_equal(coeffs, expect[i][0])
        np.testing.assert_array_equal(matched[:, :len(plan.names)], expect[i][1][:, :len(plan.names)])
        assert out.layout == "pixmajor"
    assert seen == [0, 1, 2, 3, 4]
    dev = [(i, c.clone(), m.clone()) for i, c, m, _ in plan.stream(tiles[:2], depth=depth, to_host=False)]
    assert [d[0] for d in dev] == [0, 1] and dev[1][1].is_cuda
    np.testing.assert_array_equal(dev[1][1].cpu().numpy(), expect[1][0])
    assert list(plan.stream([], depth=depth)) == []


def test_poly_ridge_fit_over_pixel_shards(torch_gpu):
    """Distributed a9 fit emulated on one GPU: three 'ranks' hold disjoint pixel shards; exchanging only the
    scaler statistics (all-gather) and the Gram matrices (all-reduce = sum) reproduces the fit on the union."""
    torch = torch_gpu
    from s2_emit import PolyRidge
    g = load_golden("g7_ridge")
    X, Y = g["X"].astype(np.float32), g["Ylogit"]
    n = X.shape[0]
    cuts = [0, n // 5, n // 5 + 1, n]               # very unequal shards, one of a single pixel
    ref = PolyRidge(3, 1.0).fit(X, Y)
    shards = [PolyRidge._to_dev(X[a:b], Y[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    stats = torch.stack([PolyRidge.local_stats(xd) for xd, _ in shards])
    mean, scale = PolyRidge.combine_stats(stats)
    np.testing.assert_allclose(mean.cpu().numpy(), g["mean"], rtol=1e-12)
    np.testing.assert_allclose(scale.cpu().numpy(), g["scale"], rtol=1e-12)
    model = PolyRidge(3, 1.0)
    G = sum(model.local_gram(xd, yd, mean, scale) for xd, yd in shards)
    model.solve_gram(G, mean, scale, X.shape[1], Y.shape[1])
    np.testing.assert_allclose(model.intercept_, g["intercept"], rtol=1e-6, atol=1e-7)
    Xte = g["Xtest"].reshape(-1, 10).astype(np.float32)
    np.testing.assert_allclose(model.predict(Xte), ref.predict(Xte), rtol=0, atol=2e-5)
    np.testing.assert_allclose(model.predict(Xte), g["pred_logit"], rtol=0, atol=2e-4)
    # an empty shard contributes nothing
    e = PolyRidge._to_dev(X[:0], Y[:0])
    st2 = torch.stack([stats[0], PolyRidge.local_stats(e[0]), stats[1], stats[2]])
    m2, s2 = PolyRidge.combine_stats(st2)
    assert torch.equal(m2, mean) and torch.equal(s2, scale)
    assert float(model.local_gram(e[0], e[1], mean, scale).abs().max()) == 0.0



def test_ot_sampling_on_device_matches_host_rows(torch_gpu):
    """The row selection of fit_ot_poly_rgb done on the GPU (nonzero of mask & finite rows, the reference's PCG64
    draw on the two counts, gather) returns exactly the rows the host code of poly_regression.py:31-47 picks."""
    torch = torch_gpu
    from s2_emit import _ot
    rng = np.random.default_rng(17)
    src = rng.random((61, 47, 3)).astype(np.float32)
    ref = rng.random((61, 47, 3))
    src[5, 5, 1] = np.nan
    src[40, 2, 0] = np.inf
    ref[7, 7, 2] = np.nan
    mask = rng.random((61, 47)) > 0.3
    for ns in (500, 100000):
        X, Y = _ot.sample_pairs(src, ref, mask, ns, 4, 200)
        Xd, Yd = _ot.sample_pairs_device(torch.from_numpy(src).cuda(), torch.from_numpy(ref).cuda(),
                                         torch.from_numpy(mask).cuda(), ns, 4, 200)
        np.testing.assert_array_equal(Xd.cpu().numpy(), X)
        np.testing.assert_array_equal(Yd.cpu().numpy(), Y)
    few = np.zeros((61, 47), bool)
    few[0, :50] = True
    assert _ot.sample_pairs_device(torch.from_numpy(src).cuda(), torch.from_numpy(ref).cuda(), torch.from_numpy(few).cuda(), 500, 0, 200) is None


def test_chol_solve_vs_numpy(torch_gpu):
    """hsr_chol_solve_f64 (single-workgroup blocked Cholesky + per-column substitution) against numpy.linalg.solve
    on random SPD systems of the supported sizes, and LAPACK's info convention on an indefinite matrix."""
    torch = torch_gpu
    from s2_emit import _native as nat
    from s2_emit._engine import _ptr, _stream
    lib = nat.load()
    rng = np.random.default_rng(23)
    for n, T in ((32, 1), (96, 5), (288, 32), (288, 285), (512, 7), (64, 4)):
        M = rng.standard_normal((n, n + 40))
        A = M @ M.T / n + 0.5 * np.eye(n)
        Bm = rng.standard_normal((n, T))
        Ad, Bd = torch.from_numpy(A.copy()).cuda(), torch.from_numpy(Bm.copy()).cuda()
        info = torch.full((1,), -5, dtype=torch.int32, device="cuda")
        cw = torch.empty(lib.hsr_chol_work_bytes(n) // 8, dtype=torch.float64, device="cuda")
        nat.check(lib.hsr_chol_solve_f64(_ptr(Ad), n, n, _ptr(Bd), T, T, _ptr(cw), _ptr(info), _stream(torch)))
        assert int(info.item()) == 0
        X = np.linalg.solve(A, Bm)
        np.testing.assert_allclose(Bd.cpu().numpy(), X, rtol=1e-9, atol=1e-11)
        Lg = np.tril(Ad.cpu().numpy())
        np.testing.assert_allclose(Lg, np.linalg.cholesky(A), rtol=1e-10, atol=1e-12)
    # leading dimensions larger than the matrix / the right-hand sides
    n, T = 64, 3
    M = rng.standard_normal((n, 2 * n))
    A = M @ M.T / n + np.eye(n)
    Bm = rng.standard_normal((n, T))
    Abig = torch.zeros((n, n + 7), dtype=torch.float64, device="cuda")
    Abig[:, :n] = torch.from_numpy(A).cuda()
    Bbig = torch.zeros((n, T + 2), dtype=torch.float64, device="cuda")
    Bbig[:, :T] = torch.from_numpy(Bm).cuda()
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    cw = torch.empty(lib.hsr_chol_work_bytes(512) // 8, dtype=torch.float64, device="cuda")
    nat.check(lib.hsr_chol_solve_f64(_ptr(Abig), n + 7, n, _ptr(Bbig), T + 2, T, _ptr(cw), _ptr(info), _stream(torch)))
    np.testing.assert_allclose(Bbig[:, :T].cpu().numpy(), np.linalg.solve(A, Bm), rtol=1e-9, atol=1e-11)
    assert float(Bbig[:, T:].abs().max()) == 0.0
    # not positive definite: first bad pivot reported (1-based), nothing raised on the device
    Ai = np.eye(64)
    Ai[40, 40] = -1.0
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    Aid, Bid = torch.from_numpy(Ai).cuda(), torch.zeros((64, 1), dtype=torch.float64, device="cuda")   # keep them alive
    nat.check(lib.hsr_chol_solve_f64(_ptr(Aid), 64, 64, _ptr(Bid), 1, 1, _ptr(cw), _ptr(info), _stream(torch)))
    assert int(info.item()) == 41
    assert lib.hsr_chol_solve_f64(_ptr(Abig), n + 7, 40, _ptr(Bbig), T + 2, T, _ptr(cw), _ptr(info), _stream(torch)) == 2   # n % 32 != 0


def test_round4_select_runs_upsampler_rows_and_cholesky_sizes(torch_gpu):
    """Round-4 kernels against independent references.
    (a) percentile select on SMOOTH images (pass 1 counts runs of equal bins per thread; above a megapixel a workgroup takes two
        iterations): planes on the 16-byte path and band-last rows, masked stripes, a NaN - np.percentile, bit for bit;
    (b) the upsamplers that keep their horizontal interpolations while the rows share a coarse pair: factors 1, 2, 3, 6, planes vs the
        NumPy restatement, and the band-last form / the producer form (mask + pass-1 histogram) carry the planes' bits;
    (c) the register-resident Cholesky (n <= 288) at every block count, padded leading dimensions, a bad pivot in a late block."""
    torch = torch_gpu
    from s2_emit import _engine as eng
    from s2_emit import _native as nat
    from s2_emit._engine import _ptr, _stream
    lib = nat.load()
    rng = np.random.default_rng(404)
    # (a)
    for side in (1100, 640):
        c = rng.random((3, side // 6 + 2, side // 6 + 2)).astype(np.float32) ** 2
        up = eng.bilinear_upsample(torch.from_numpy(c).cuda().reshape(3, -1), c.shape[1], c.shape[2], 6).reshape(3, c.shape[1] * 6, c.shape[2] * 6)
        img = up[:, :side, :side].contiguous().reshape(3, -1)
        n = side * side
        mask = np.ones(n, np.uint8)
        mask.reshape(side, side)[side // 3: side // 3 + 40] = 0          # a masked stripe
        mask[rng.integers(0, n, n // 50)] = 0
        md = torch.from_numpy(mask).cuda()
        x = img.cpu().numpy()
        for pmin, pmax in ((2, 98), (0.01, 99.99)):
            got = eng.percentile_limits(img, md, pmin, pmax).cpu().numpy()
            np.testing.assert_array_equal(got, np.array([np.percentile(p[mask != 0], [pmin, pmax]) for p in x]), err_msg=f"planes {side}")
            rows = torch.zeros((n, 4), device="cuda")
            rows[:, :3] = img.t()
            got = eng.percentile_limits(rows, md, pmin, pmax, "pixmajor", nb=3).cpu().numpy()
            np.testing.assert_array_equal(got, np.array([np.percentile(p[mask != 0], [pmin, pmax]) for p in x]), err_msg=f"rows {side}")
        xn = img.clone()
        xn[1, 12345] = float("nan")
        got = eng.percentile_limits(xn, md if mask[12345] else None, 2, 98).cpu().numpy()
        assert np.isnan(got[1]).all() and not np.isnan(got[[0, 2]]).any()
    # (b)
    for f_, Hc, Wc in ((6, 9, 11), (1, 7, 5), (2, 33, 40), (3, 12, 70), (6, 37, 50)):
        coarse = rng.random((3, Hc, Wc)).astype(np.float32)
        coarse[2, Hc // 2, Wc // 3] = np.nan
        cd = torch.from_numpy(coarse).cuda()
        up = eng.bilinear_upsample(cd.reshape(3, -1), Hc, Wc, f_).cpu().numpy().reshape(3, Hc * f_, Wc * f_)
        refu = onp.bilinear_upsample(coarse, f_)
        assert np.array_equal(np.isnan(up), np.isnan(refu))
        np.testing.assert_allclose(up[~np.isnan(refu)], refu[~np.isnan(refu)], rtol=2e-7, atol=1e-7)
        pm = torch.zeros((Hc * Wc, 4), device="cuda")
        pm[:, :3] = cd.reshape(3, -1).t()
        up_pm = eng.bilinear_upsample(pm, Hc, Wc, f_, layout=nat.PIXMAJOR, nb=3)
        np.testing.assert_array_equal(up_pm[:, :3].t().cpu().numpy().reshape(3, Hc * f_, Wc * f_), up)
        out, msk, lohi = eng.bilinear_upsample_mask_limits(pm, Hc, Wc, f_, 2.0, 98.0, nb=3)
        np.testing.assert_array_equal(out[:, :3].t().cpu().numpy().reshape(3, Hc * f_, Wc * f_), up)
        fin = np.isfinite(up).all(axis=0).reshape(-1)
        np.testing.assert_array_equal(msk.cpu().numpy() != 0, fin)
        np.testing.assert_array_equal(lohi.cpu().numpy(), np.array([np.percentile(p.reshape(-1)[fin], [2.0, 98.0]) for p in up]))
    # (c)
    for n, T, lda, ldb in ((32, 3, 32, 3), (64, 17, 70, 20), (128, 16, 128, 16), (160, 33, 161, 40), (192, 5, 200, 5), (224, 48, 224, 48),
                           (256, 32, 300, 32), (288, 285, 288, 285)):
        M = rng.standard_normal((n, n + 30))
        A = M @ M.T / n + 0.3 * np.eye(n)
        Bm = rng.standard_normal((n, T))
        Ad = torch.zeros((n, lda), dtype=torch.float64, device="cuda")
        Ad[:, :n] = torch.from_numpy(A).cuda()
        Bd = torch.zeros((n, ldb), dtype=torch.float64, device="cuda")
        Bd[:, :T] = torch.from_numpy(Bm).cuda()
        info = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        cw = torch.empty(lib.hsr_chol_work_bytes(n) // 8, dtype=torch.float64, device="cuda")
        nat.check(lib.hsr_chol_solve_f64(_ptr(Ad), lda, n, _ptr(Bd), ldb, T, _ptr(cw), _ptr(info), _stream(torch)))
        assert int(info.item()) == 0
        np.testing.assert_allclose(Bd[:, :T].cpu().numpy(), np.linalg.solve(A, Bm), rtol=1e-9, atol=1e-11, err_msg=f"n={n}")
        np.testing.assert_allclose(np.tril(Ad[:, :n].cpu().numpy()), np.linalg.cholesky(A), rtol=1e-10, atol=1e-12, err_msg=f"n={n}")
        if ldb > T:
            assert float(Bd[:, T:].abs().max()) == 0.0
    Ai = np.eye(288) * 2.0
    Ai[203, 203] = -1.0                                                    # first non-positive pivot in block 6 (1-based index 204)
    Aid, Bid = torch.from_numpy(Ai).cuda(), torch.zeros((288, 2), dtype=torch.float64, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    cw = torch.empty(lib.hsr_chol_work_bytes(288) // 8, dtype=torch.float64, device="cuda")
    nat.check(lib.hsr_chol_solve_f64(_ptr(Aid), 288, 288, _ptr(Bid), 2, 2, _ptr(cw), _ptr(info), _stream(torch)))
    assert int(info.item()) == 204


def test_fuse_mosaic_equals_one_big_tile(torch_gpu):
    """A global fit over several tiles of different sizes on one GPU (moments added in tile order, one solve, K3 per
    tile) is the fit of the tiles laid end to end."""
    torch = torch_gpu
    from s2_emit import SpectralFusion
    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths()
    plan = SpectralFusion(w, srf, good, deg=3, coeff_sync="local")
    tiles, cubes, reals = [], [], []
    for i, (H, W) in enumerate(((40, 36), (64, 20), (17, 90))):
        R = onp.synthetic_cube(H, W, seed=300 + i)
        ps = onp.pseudo_s2_srf_integral(R, w, srf, good)
        real = onp.synthetic_real_planes(np.stack([ps[k] for k in plan.names]).astype(np.float32), seed=i)
        real = np.clip(real + 0.02 * i, 0, 1).astype(np.float32)
        tiles.append((torch.from_numpy(R).cuda(), torch.from_numpy(real).cuda()))
        cubes.append(R.reshape(-1, R.shape[-1]))
        reals.append(real.reshape(real.shape[0], -1))
    coeffs, moments, outs = plan.fuse_mosaic(tiles)
    big = plan.step(torch.from_numpy(np.concatenate(cubes, 0)).cuda(), torch.from_numpy(np.concatenate(reals, 1)).cuda(),
                    reuse_buffers=False)
    np.testing.assert_allclose(moments.cpu().numpy(), big.moments.cpu().numpy(), rtol=1e-12)
    xs = np.linspace(0.0, 0.6, 40)
    for b in range(coeffs.shape[0]):
        np.testing.assert_allclose(np.polyval(coeffs[b].cpu().numpy(), xs), np.polyval(big.coeffs[b].cpu().numpy(), xs),
                                   rtol=1e-6, atol=1e-9)
    got = np.concatenate([o.matched.cpu().numpy() for o in outs], 0)
    np.testing.assert_allclose(got[:, :len(plan.names)], big.matched.cpu().numpy()[:, :len(plan.names)], rtol=0, atol=1e-6)
    # resident mosaic: the same through the batch machinery (five launches), twice (buffers reused)
    for _ in range(2):
        c2, m2, outs2 = plan.fuse_mosaic(tiles, resident=True)
        # both forms add the tiles' moments with the same fixed-order reduction (r03; a sequential sum in the per-tile form
        # used to differ from it in the last bit): same bits throughout
        assert torch.equal(m2.view(torch.int64), moments.view(torch.int64)) and torch.equal(c2.view(torch.int64), coeffs.view(torch.int64))
        for o, o2 in zip(outs, outs2):
            assert torch.equal(o.pseudo.view(torch.int32), o2.pseudo.view(torch.int32))
            assert torch.equal(o.matched.view(torch.int32), o2.matched.view(torch.int32))
    # and differs from per-tile fits (the tiles do not share one polynomial)
    solo = plan.step(*tiles[2], reuse_buffers=False)
    assert not torch.allclose(solo.coeffs, coeffs)
    with pytest.raises(ValueError):
        plan.fuse_mosaic([])


def test_u16_single_buffer_kernel_matches_ring(torch_gpu):
    """The single-buffer uint16 K1 (taken when two tile buffers do not fit, or with the ring switched off) gives the
    same bits as the double-buffered one; B = 400 does not fit the ring at all and must still be right."""
    torch = torch_gpu
    from s2_emit import _engine as eng, _native as nat
    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths()
    table = eng.build_srf_table(w, srf, good)
    rng = np.random.default_rng(8)
    u = rng.integers(0, 6000, (64 * 30 + 17, 285)).astype(np.uint16)
    u[5, 5] = 65535
    ud = torch.from_numpy(u).cuda()
    real = torch.rand((table.nb, u.shape[0]), device="cuda")
    res = []
    for single in (False, True):
        ws = eng.MomentWorkspace("cuda", table.nb, 3)
        p, m = eng.srf_integrate_moments(ud, table, real, 3, ws, None, 0.0, 0.0, layout="pixmajor", real_layout="planar",
                                         opts=eng.srf_options(u16_single_buffer=single))
        res.append((p[:, :table.nb].cpu().numpy(), m.cpu().numpy().copy()))
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    B = 400
    w4 = np.linspace(400, 2400, B).astype(np.float32)
    t4 = eng.build_srf_table(w4, srf, None)
    u4 = rng.integers(0, 6000, (64 * 5, B)).astype(np.uint16)
    a = eng.srf_integrate(torch.from_numpy(u4).cuda(), t4, layout="planar")
    b = eng.srf_integrate(eng.tile_decode_u16(torch.from_numpy(u4).cuda()), t4, layout="planar")
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())


# ---------------------------------------------------------------------------------------------
# batched small tiles: the reference's own workload (100 x 100 EMIT tiles, one fit per tile,
# tiles_helpers/utils.py:223-305; Spectral_matching.ipynb "EMIT: (285, 100, 100)")
# ---------------------------------------------------------------------------------------------
def _small_tiles(torch, T, H, W, seed0=100):
    """T synthetic (cube, real band-last) tile pairs on the GPU, plus what the oracle needs for the first ones."""
    from s2_emit import _engine as eng
    from s2_emit.synthetic import device_problem
    probs = [device_problem(H, W, 285, deg=3, seed=seed0 + i) for i in range(T)]
    return probs


@pytest.mark.parametrize("kind", ["f32", "u16"])
def test_step_batch_64_tiles_100x100_bit_identical_to_step(torch_gpu, kind):
    """T = 64 tiles of 100 x 100 x 285 in three launches: coefficients, moments and both images are bit-identical to
    64 step() calls, and tiles 0 and 37 agree with the oracle (pseudo 2e-6, matched 1e-4)."""
    torch = torch_gpu
    from s2_emit import SpectralFusion, _engine as eng
    T, H, W = 64, 100, 100
    probs = _small_tiles(torch, T, H, W)
    p0 = probs[0]
    plan = SpectralFusion(p0.emit_w, p0.srf, p0.good_mask, deg=3, min_valid=0.0, min_count=50)
    cubes = [p.cube for p in probs]
    if kind == "u16":
        cubes = [eng.tile_encode_u16(c) for c in cubes]
        for c in cubes[:3]:
            c.view(-1)[12345] = 65535                     # a nodata sample: that pixel is NaN in every band
    reals = [p.real for p in probs]
    masks = [None] * T
    masks[5] = (torch.rand(H * W, device="cuda") > 0.3).to(torch.uint8)
    out = plan.step_batch(cubes, reals, masks)
    torch.cuda.synchronize()
    assert len(out) == T and out.coeffs.shape == (T, 12, 4) and out.pseudo.shape == (T * H * W, 12)
    nb = len(plan.names)
    for i in range(T):
        o = plan.step(cubes[i], reals[i], masks[i], reuse_buffers=False)
        ti = out.tile(i)
        assert torch.equal(o.coeffs.view(torch.int64), ti.coeffs.view(torch.int64)), i
        assert torch.equal(o.moments.view(torch.int64), ti.moments.view(torch.int64)), i
        assert torch.equal(o.pseudo.view(torch.int32), ti.pseudo.view(torch.int32)), i
        assert torch.equal(o.matched.view(torch.int32), ti.matched.view(torch.int32)), i
    # the same call again reuses the batch plan and gives the same bits (no state left behind by the flushes)
    c1, m1 = out.coeffs.clone(), out.matched.clone()
    out2 = plan.step_batch(cubes, reals, masks)
    torch.cuda.synchronize()
    assert torch.equal(out2.coeffs.view(torch.int64), c1.view(torch.int64)) and torch.equal(out2.matched.view(torch.int32), m1.view(torch.int32))
    for i in (0, 37):
        R = (eng.tile_decode_u16(cubes[i]) if kind == "u16" else cubes[i]).cpu().numpy()
        real = probs[i].real_planes.cpu().numpy()
        pseudo_o, coeffs_o, matched_o, names = onp.fuse_lsq_reference(R, p0.emit_w, p0.srf, p0.good_mask, real, deg=3)
        ti = out.tile(i)
        assert names == plan.names
        assert _rel_err(ti.planes("pseudo").cpu().numpy().reshape(nb, H, W), pseudo_o) < 2e-6
        got_m = ti.planes("matched").cpu().numpy().reshape(nb, H, W)
        if kind == "u16" and i == 0:
            assert np.isnan(got_m).sum() == nb              # the nodata pixel
        ok = np.isfinite(matched_o)
        assert np.max(np.abs(got_m[ok] - matched_o[ok])) < 1e-4
        # coefficients: the oracle fits ITS float32 planes, the kernel its own (1e-7 apart); with cond(V) ~ 1e4 for a
        # cubic on [0, 0.6] that moves the coefficients by ~1e-5 while the polynomial (matched, above) moves by 1e-7
        np.testing.assert_allclose(ti.coeffs.cpu().numpy(), coeffs_o, rtol=1e-4, atol=1e-5)


def test_step_batch_ragged_tile_sizes_and_masks(torch_gpu):
    """Arbitrary npix per tile in one batch: 1 pixel, just under / at / over one group, a 100 x 100 tile, and a tile
    with more groups than resident workgroups (its units run several groups each) - every tile bit-identical to
    its own step(), with and without masks, for every fit degree, float32 and uint16."""
    torch = torch_gpu
    from s2_emit import SpectralFusion, _engine as eng
    w, good = onp.synthetic_wavelengths()
    srf = onp.synthetic_srf()
    shapes = [(1, 1), (1, 63), (8, 8), (5, 13), (100, 100), (130, 300), (3, 50)]      # 130 x 300 = 610 groups > 512
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    cubes, reals, masks = [], [], []
    for i, (H, W) in enumerate(shapes):
        c = torch.rand((H, W, 285), generator=g, device="cuda") * 0.6
        if i == 4:
            c[3, 7, 100] = float("nan")
            c[50, 50, 150] = float("inf")             # zero-weight band
        cubes.append(c)
        reals.append(torch.rand((H, W, 12), generator=g, device="cuda"))
        masks.append((torch.rand(H * W, generator=g, device="cuda") > 0.2).to(torch.uint8) if i % 2 else None)
    for deg in (1, 2, 3, 4):
        for kind in ("f32", "u16"):
            cs = cubes if kind == "f32" else [eng.tile_encode_u16(torch.nan_to_num(c, nan=0.1, posinf=0.2)) for c in cubes]
            plan = SpectralFusion(w, srf, good, deg=deg, min_valid=0.0, min_count=5, apply_mask=True)
            out = plan.step_batch(cs, reals, masks)
            torch.cuda.synchronize()
            for i in range(len(shapes)):
                o = plan.step(cs[i], reals[i], masks[i], reuse_buffers=False)
                ti = out.tile(i)
                assert torch.equal(o.coeffs.view(torch.int64), ti.coeffs.view(torch.int64)), (deg, kind, i)
                assert torch.equal(o.moments.view(torch.int64), ti.moments.view(torch.int64)), (deg, kind, i)
                assert torch.equal(o.pseudo.view(torch.int32), ti.pseudo.view(torch.int32)), (deg, kind, i)
                assert torch.equal(o.matched.view(torch.int32), ti.matched.view(torch.int32)), (deg, kind, i)
    # one stacked tensor in, same thing
    st_c = torch.stack([cubes[4], cubes[4].flip(0)])
    st_r = torch.stack([reals[4], reals[4].flip(0)])
    plan = SpectralFusion(w, srf, good, deg=2, min_valid=0.0)
    out = plan.step_batch(st_c, st_r)
    o = plan.step(st_c[1], st_r[1], reuse_buffers=False)
    assert torch.equal(o.matched.view(torch.int32), out.tile(1).matched.view(torch.int32))


def test_fit_targets_and_mask_reach_every_kernel_variant_repeatably(torch_gpu):
    """The fit's operands (two target values and the mask byte per thread) are staged through LDS by per-lane LDS-DMA in
    srf_kernel / srf_u16_kernel and by ordinary prefetch loads in srf_u16_ring_kernel (rounds 1-2 used inline-asm loads
    whose results the compiler could copy before they had landed: a masked tile's moments changed from launch to launch).
    For every degree x {float32 fast loader, float32 generic loader (unaligned cube), uint16 ring, uint16 single buffer}
    x {mask, no mask} x {single launch, batch launch}: two launches give identical bits, and the moments are the ones an
    independent torch evaluation of the same pixels gives (count exact, sums to 1e-12) - so a target or mask value that
    arrived late, or in the wrong lane, cannot pass."""
    torch = torch_gpu
    from s2_emit import _engine as eng, _native as nat
    w, good = onp.synthetic_wavelengths()
    table = eng.build_srf_table(w, onp.synthetic_srf(), good)
    nb = table.nb
    g = torch.Generator(device="cuda")
    g.manual_seed(77)
    npix = 64 * 37 + 29                                  # ragged last group
    base = torch.rand((npix * 285 + 4,), generator=g, device="cuda") * 0.6
    cube_al = base[:npix * 285].view(npix, 285)
    cube_un = base[1:npix * 285 + 1].view(npix, 285)     # 4-byte aligned only: the generic loader
    real = torch.rand((npix, eng.padded_row(nb)), generator=g, device="cuda")
    real[5, 2] = float("nan")
    mask = (torch.rand(npix, generator=g, device="cuda") > 0.3).to(torch.uint8)
    variants = [("f32 fast", cube_al, None), ("f32 generic", cube_un, None),
                ("u16 ring", eng.tile_encode_u16(cube_al.contiguous()), eng.srf_options()),
                ("u16 single", eng.tile_encode_u16(cube_al.contiguous()), eng.srf_options(u16_single_buffer=True))]
    for deg in (1, 2, 3, 4):
        M = 3 * deg + 2
        for tag, cube, opts in variants:
            cube = cube if cube.is_contiguous() else cube
            for m in (None, mask):
                ws = eng.MomentWorkspace(cube.device, nb, deg)
                runs = []
                for _ in range(2):
                    img, mom = eng.srf_integrate_moments(cube, table, real, deg, ws, m, 0.0625, 0.0625, layout=nat.PIXMAJOR, opts=opts)
                    runs.append((img.clone(), mom.clone()))
                assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)), (deg, tag, m is not None)
                assert torch.equal(runs[0][1].view(torch.int64), runs[1][1].view(torch.int64)), (deg, tag, m is not None)
                x = runs[0][0][:, :nb].double()
                y = real[:, :nb].double()
                ok = torch.isfinite(x) & torch.isfinite(y) & (x > 0.0625) & (y > 0.0625)
                if m is not None:
                    ok &= m.bool()[:, None]
                xs, ys = torch.where(ok, x, torch.zeros_like(x)), torch.where(ok, y, torch.zeros_like(y))
                want = torch.stack([(xs ** k * ok).sum(0) for k in range(2 * deg + 1)] +
                                   [(xs ** k * ys).sum(0) for k in range(deg + 1)], dim=1)          # (nb, 3 deg + 2)
                got = runs[0][1]
                assert got.shape == (nb, M)
                assert torch.equal(got[:, 0], ok.sum(0).double()), (deg, tag, m is not None)       # the count is exact
                assert torch.allclose(got, want, rtol=1e-12, atol=0), (deg, tag, m is not None)
                # the same tile as a batch of two (second tile: the first 640 pixels, mask only on one of them)
                tb = eng.TileBatch([cube, cube[:640]], [real, real[:640]], [m, None if m is not None else mask[:640]], table, deg, opts)
                for rep in range(2):
                    eng.batch_srf_integrate_moments(tb, 0.0625, 0.0625)
                    eng.batch_reduce_solve(tb, 5)
                    if rep == 0:
                        first = (tb.pseudo.clone(), tb.moments.clone())
                assert torch.equal(first[0].view(torch.int32), tb.pseudo.view(torch.int32)), (deg, tag, "batch")
                assert torch.equal(first[1].view(torch.int64), tb.moments.view(torch.int64)), (deg, tag, "batch")
                assert torch.equal(tb.moments[0].view(torch.int64), got.view(torch.int64)), (deg, tag, "batch tile 0 == single launch")


def test_prepared_launches_match_the_operator_path_bit_for_bit(torch_gpu):
    """The step executor (include/hsr.h ABI 4, csrc/hsr_exec.hip): step() builds an hsr_step_plan on the first call for a
    shape and runs later calls as ONE hsr_step_run; submit() / flush() run on the native pipeline (K1 and K3 on the caller's
    stream, the fit on a side stream, events and stream waits issued from C).  Same launches -> identical bits to the
    operator-by-operator path (reuse_buffers=False never takes the prepared path), for float32 and uint16 cubes, masks that
    come and go from tile to tile, a changing tile shape, and through the C ABI directly."""
    torch = torch_gpu
    import ctypes as C
    from s2_emit import SpectralFusion, _engine as eng, _native as nat
    from s2_emit.synthetic import device_problem
    p = device_problem(96, 80, 285, deg=3, seed=21)
    q = device_problem(64, 100, 285, deg=3, seed=22)
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    mask = (torch.rand(96 * 80, generator=g, device="cuda") > 0.25).to(torch.uint8)
    for kind in ("f32", "u16"):
        cube_p = p.cube if kind == "f32" else eng.tile_encode_u16(p.cube)
        cube_q = q.cube if kind == "f32" else eng.tile_encode_u16(q.cube)
        plan = SpectralFusion(p.emit_w, p.srf, p.good_mask, deg=3, min_valid=0.0, min_count=5, apply_mask=True)
        ref = SpectralFusion(p.emit_w, p.srf, p.good_mask, deg=3, min_valid=0.0, min_count=5, apply_mask=True)

        def same(a, b, tag):
            for f in ("pseudo", "matched"):
                assert torch.equal(getattr(a, f).view(torch.int32), getattr(b, f).view(torch.int32)), (kind, tag, f)
            for f in ("moments", "coeffs"):
                assert torch.equal(getattr(a, f).view(torch.int64), getattr(b, f).view(torch.int64)), (kind, tag, f)
        for rep in range(3):                                   # call 0 builds the plan, calls 1-2 run it
            for tag, (c, r, m) in {"p": (cube_p, p.real, None), "p+mask": (cube_p, p.real, mask), "q": (cube_q, q.real, None)}.items():
                got = plan.step(c, r, m)
                want = ref.step(c, r, m, reuse_buffers=False)
                same(got, want, (tag, rep))
        assert len(plan._native) == 3 and len(ref._native) == 0
        # pipeline: tiles alternate shape-compatible inputs and masks; every finished tile equals its own step()
        pipe = SpectralFusion(p.emit_w, p.srf, p.good_mask, deg=3, min_valid=0.0, min_count=5, apply_mask=True)
        seq = [(cube_p, p.real, None), (cube_p, p.real, mask), (cube_p.clone(), p.real.clone(), None), (cube_p, p.real, mask)]
        outs = []
        for c, r, m in seq:
            o = pipe.submit(c, r, m)
            if o is not None:
                outs.append((o.pseudo.clone(), o.matched.clone(), o.moments.clone(), o.coeffs.clone()))
        o = pipe.flush()
        outs.append((o.pseudo.clone(), o.matched.clone(), o.moments.clone(), o.coeffs.clone()))
        assert pipe.flush() is None and len(outs) == len(seq)
        for (c, r, m), got in zip(seq, outs):
            want = ref.step(c, r, m, reuse_buffers=False)
            assert torch.equal(got[0].view(torch.int32), want.pseudo.view(torch.int32)), kind
            assert torch.equal(got[1].view(torch.int32), want.matched.view(torch.int32)), kind
            assert torch.equal(got[2].view(torch.int64), want.moments.view(torch.int64)), kind
            assert torch.equal(got[3].view(torch.int64), want.coeffs.view(torch.int64)), kind
        # a new tile shape rebuilds the pipeline (the tile in flight is finished first)
        assert pipe.submit(cube_q, q.real) is None
        same(pipe.flush(), ref.step(cube_q, q.real, reuse_buffers=False), "pipeline, new shape")
        plan.close(); pipe.close()
        assert plan._native == {} and plan._native_handles == []
    # the C ABI's own argument checks
    lib = nat.load()
    h = C.c_void_p()
    d = nat.StepDesc()
    assert lib.hsr_step_plan_create(C.byref(d), C.byref(h)) == 1 and b"hsr_step_plan_create" in lib.hsr_last_error()
    assert lib.hsr_step_run(None, None, None, None, None) == 1
    assert lib.hsr_pipeline_flush(None, None, None, None) == 1 and lib.hsr_pipeline_count(None) == -1


def test_fused_pipeline_k3_inside_k1_launch_bit_identical(torch_gpu):
    """SpectralFusion(fuse_apply=True): K3 of tile i-2 rides in the launch of K1 of tile i (hsr_srf_integrate_moments_apply,
    hsr_pipeline_create_fused).  Every tile that comes out - two submits late, the rest through drain() - carries the bits of
    its own step(): degrees 1-4, masks that come and go (the mask of the tile being FINISHED is the one K3 must use), a
    13-band table (rows of 16 floats) and 3 bands (rows of 4), odd pixel counts, the generic (unaligned) loader; uint16
    tiles through the ring kernel; the C entry refuses what the fused launch does not cover."""
    torch = torch_gpu
    import ctypes as C
    from s2_emit import SpectralFusion, _engine as eng, _native as nat
    w, good = onp.synthetic_wavelengths()
    srf13 = onp.synthetic_srf()
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    # (the last two shapes: fewer 64-pixel groups than bands - such a launch cannot carry the previous tile's fit, one
    # workgroup per band, and the executor runs that fit as a launch of its own; found by tools/dbg/stress_fused.py)
    for names_sel, gm, H, W in ((None, good, 70, 61), (("B4", "B3", "B2"), good, 64, 64), (None, None, 33, 97),
                                (None, good, 2, 158), (None, None, 1, 70)):
        srf = srf13 if names_sel is None else {k: srf13[k] for k in names_sel}
        nb = eng.build_srf_table(w, srf, gm).nb
        row = eng.padded_row(nb)
        npix = H * W
        base = torch.rand((npix * 285 + 4,), generator=g, device="cuda") * 0.6
        cubes = [base[:npix * 285].view(H, W, 285), base[1:npix * 285 + 1].view(H, W, 285).clone(),
                 base[1:npix * 285 + 1].view(H, W, 285)]                          # the last one: 4-byte aligned only
        reals = [torch.rand((H, W, row), generator=g, device="cuda") for _ in range(3)]
        masks = [None, (torch.rand(npix, generator=g, device="cuda") > 0.3).to(torch.uint8), None,
                 (torch.rand(npix, generator=g, device="cuda") > 0.6).to(torch.uint8), None]
        for deg in (1, 2, 3, 4):
            kw = dict(deg=deg, min_valid=0.0, min_count=5, apply_mask=True)
            ref = SpectralFusion(w, srf, gm, **kw)
            pipe = SpectralFusion(w, srf, gm, fuse_apply=True, **kw)
            seq = [(cubes[i % 3], reals[i % 3], masks[i % 5]) for i in range(7)]
            got = []
            for i, (c, r, m) in enumerate(seq):
                o = pipe.submit(c, r, m)
                assert (o is None) == (i < 2), (deg, i)
                if o is not None:
                    got.append(tuple(t.clone() for t in (o.pseudo, o.matched, o.moments, o.coeffs)))
            assert pipe._pipe["fused"] and pipe._pipe["S"] == 3
            got += [tuple(t.clone() for t in (o.pseudo, o.matched, o.moments, o.coeffs)) for o in pipe.drain()]
            assert len(got) == len(seq) and pipe.drain() == [] and pipe.flush() is None
            for i, ((c, r, m), gt) in enumerate(zip(seq, got)):
                want = ref.step(c, r, m, reuse_buffers=False)
                assert torch.equal(gt[0].view(torch.int32), want.pseudo.view(torch.int32)), (nb, deg, i, "pseudo")
                assert torch.equal(gt[1].view(torch.int32), want.matched.view(torch.int32)), (nb, deg, i, "matched")
                assert torch.equal(gt[2].view(torch.int64), want.moments.view(torch.int64)), (nb, deg, i, "moments")
                assert torch.equal(gt[3].view(torch.int64), want.coeffs.view(torch.int64)), (nb, deg, i, "coeffs")
            pipe.close()
    # uint16 tiles (r03, hsr_srf_integrate_moments_u16_apply): the ring kernel carries the older tile's K3 and the previous
    # tile's fit as well - same bits as step(), exact and fast arithmetic, masks, nodata; a cube the ring kernel cannot
    # load (2-byte aligned only) quietly takes the two-slot pipeline
    tiny = [eng.tile_encode_u16(torch.rand((3, 90, 285), generator=g, device="cuda") * 0.6) for _ in range(2)]   # 5 groups, 12 bands
    rt = [torch.rand((3, 90, 12), generator=g, device="cuda") for _ in range(2)]
    pt = SpectralFusion(w, srf13, good, deg=2, min_valid=0.0, min_count=5, fuse_apply=True)
    outs = [pt.submit(tiny[i % 2], rt[i % 2]) for i in range(4)]
    outs = [tuple(t.clone() for t in (o.matched, o.coeffs)) for o in outs if o is not None] + [(o.matched.clone(), o.coeffs.clone()) for o in pt.drain()]
    assert pt._pipe["fused"] and len(outs) == 4
    rf = SpectralFusion(w, srf13, good, deg=2, min_valid=0.0, min_count=5)
    for i, (mt, co) in enumerate(outs):
        want = rf.step(tiny[i % 2], rt[i % 2], reuse_buffers=False)
        assert torch.equal(mt.view(torch.int32), want.matched.view(torch.int32)) and torch.equal(co.view(torch.int64), want.coeffs.view(torch.int64)), i
    pt.close()
    raw = [eng.tile_encode_u16(torch.rand((40, 64, 285), generator=g, device="cuda") * 0.6) for _ in range(3)]
    raw[1].view(torch.int16)[3, 5, 100] = -1                                          # 65535 = nodata
    raw[2].view(torch.int16)[:, 7, :] = -1
    rus = [torch.rand((40, 64, 12), generator=g, device="cuda") for _ in range(3)]
    mus = [None, (torch.rand(40 * 64, generator=g, device="cuda") > 0.4).to(torch.uint8), None, None,
           (torch.rand(40 * 64, generator=g, device="cuda") > 0.7).to(torch.uint8)]
    for fastu in (False, True):
        for deg in (1, 3):
            kw = dict(deg=deg, min_valid=0.0, min_count=5, apply_mask=True, u16_fast=fastu)
            p16 = SpectralFusion(w, srf13, good, fuse_apply=True, **kw)
            ref = SpectralFusion(w, srf13, good, **kw)
            seq = [(raw[i % 3], rus[i % 3], mus[i % 5]) for i in range(7)]
            got = []
            for i, (c, r, m) in enumerate(seq):
                o = p16.submit(c, r, m)
                assert (o is None) == (i < 2), (fastu, deg, i)
                if o is not None:
                    got.append(tuple(t.clone() for t in (o.pseudo, o.matched, o.moments, o.coeffs)))
            assert p16._pipe["fused"] and p16._pipe["S"] == 3
            got += [tuple(t.clone() for t in (o.pseudo, o.matched, o.moments, o.coeffs)) for o in p16.drain()]
            assert len(got) == len(seq)
            for i, ((c, r, m), gt) in enumerate(zip(seq, got)):
                want = ref.step(c, r, m, reuse_buffers=False)
                assert torch.equal(gt[0].view(torch.int32), want.pseudo.view(torch.int32)), (fastu, deg, i, "pseudo")
                assert torch.equal(gt[1].view(torch.int32), want.matched.view(torch.int32)), (fastu, deg, i, "matched")
                assert torch.equal(gt[2].view(torch.int64), want.moments.view(torch.int64)), (fastu, deg, i, "moments")
                assert torch.equal(gt[3].view(torch.int64), want.coeffs.view(torch.int64)), (fastu, deg, i, "coeffs")
            p16.close()
    flat = torch.zeros(40 * 64 * 285 + 8, dtype=torch.int16, device="cuda")
    flat[1:1 + 40 * 64 * 285] = raw[0].view(torch.int16).reshape(-1)
    cu = flat[1:1 + 40 * 64 * 285].view(raw[0].dtype).view(40, 64, 285)               # 2-byte aligned
    p16 = SpectralFusion(w, srf13, good, deg=2, min_valid=0.0, min_count=5, fuse_apply=True)
    assert p16.submit(cu, rus[0]) is None
    o = p16.flush()
    assert not p16._pipe["fused"]
    want = SpectralFusion(w, srf13, good, deg=2, min_valid=0.0, min_count=5).step(cu, rus[0], reuse_buffers=False)
    assert torch.equal(o.matched.view(torch.int32), want.matched.view(torch.int32))
    # the C entry: a planar output cannot carry an apply job
    lib = nat.load()
    job = (C.c_byte * 48)()
    k = (C.c_int32 * 1)(0)
    rc = lib.hsr_srf_integrate_moments_apply(C.c_void_p(16), 64, 285, C.c_void_p(16), k, k, 1, C.c_void_p(16), 64, 1, C.c_void_p(16), 64, 1,
                                             None, 0.0, 0.0, 1, C.c_void_p(16), None, None, C.cast(job, C.c_void_p), None)
    assert rc in (1, 2) and b"hsr_apply_job" in lib.hsr_last_error() or b"apply job" in lib.hsr_last_error()


def test_padded_rows_are_owned_and_zeroed(torch_gpu):
    """Pixel-major outputs with padded rows (nb = 3 -> 4, nb = 13 -> 16): the pad columns come back as zeros, never as
    whatever the LDS staging area held - in K1, through K3 ('channels >= nb pass through'), float32 and uint16."""
    torch = torch_gpu
    from s2_emit import _engine as eng, _native as nat
    w, good = onp.synthetic_wavelengths()
    srf13 = onp.synthetic_srf()
    for names_sel, gm in ((("B4", "B3", "B2"), good), (None, None)):
        srf = srf13 if names_sel is None else {k: srf13[k] for k in names_sel}
        table = eng.build_srf_table(w, srf, gm)
        nb, row = table.nb, eng.padded_row(table.nb)
        assert row > nb
        cube = torch.rand((64 * 9 + 5, 285), device="cuda") * 0.6
        for c in (cube, eng.tile_encode_u16(cube)):
            out = torch.full((cube.shape[0], row), float("nan"), device="cuda")        # sentinel
            eng.srf_integrate(c, table, out=out, layout=nat.PIXMAJOR)
            assert torch.isfinite(out[:, :nb]).all() and (out[:, nb:] == 0).all()
            co = torch.tensor([[2.0, 0.1]] * nb, dtype=torch.float64, device="cuda")
            m = eng.poly_apply(out, co, None, None, True, nat.PIXMAJOR, nb=nb)
            assert (m[:, nb:] == 0).all()


def test_plan_device_argument_is_honoured(torch_gpu):
    """Launches go to the device (and that device's current stream) that owns the tensors, not to whatever device is
    current.  One GPU here: the explicit-device path must work, on a non-default stream too, and a helper that cannot
    switch devices must refuse a foreign tensor instead of launching on the wrong GPU."""
    torch = torch_gpu
    from s2_emit import SpectralFusion, _engine as eng
    p = _small_tiles(torch, 1, 40, 30)[0]
    plan = SpectralFusion(p.emit_w, p.srf, p.good_mask, deg=2, device="cuda:0")
    ref = plan.step(p.cube, p.real, reuse_buffers=False)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        o = plan.step(p.cube, p.real, reuse_buffers=False)
    side.synchronize()
    assert torch.equal(o.matched.view(torch.int32), ref.matched.view(torch.int32))

    class Foreign:                      # stands in for a tensor on another GPU
        is_cuda = True
        device = torch.device("cuda", torch.cuda.current_device() + 1)
    with pytest.raises(ValueError, match="current device"):
        eng._stream(torch, Foreign())
    assert (eng._stream(torch, p.cube).value or 0) == torch.cuda.current_stream().cuda_stream


def test_mosaic_8_tiles_1024_on_one_gpu(torch_gpu):
    """BASELINE configs[3]/[4] on the one GPU there is: eight resident 1024 x 1024 x 285 tiles (9.6 GB), ONE global fit
    (fuse_mosaic), properties at full size + the coefficients of one band against np.polyfit of the union."""
    torch = torch_gpu
    from s2_emit import SpectralFusion
    from s2_emit.synthetic import device_problem
    T, H, W = 8, 1024, 1024
    probs = [device_problem(H, W, 285, deg=3, seed=40 + i) for i in range(T)]
    p0 = probs[0]
    plan = SpectralFusion(p0.emit_w, p0.srf, p0.good_mask, deg=3, min_valid=0.0, min_count=50)
    coeffs, moments, outs = plan.fuse_mosaic([(p.cube, p.real) for p in probs])
    torch.cuda.synchronize()
    nb = len(plan.names)
    assert coeffs.shape == (nb, 4) and len(outs) == T
    assert float(moments[:, 0].min()) > 0.99 * T * H * W            # counts: nearly every pixel valid (x > 0, y > 0)
    # one band against NumPy on the union of all eight tiles
    b = 3
    x = np.concatenate([o.band(b, "pseudo").cpu().numpy() for o in outs]).astype(np.float64)
    y = np.concatenate([p.real[..., b].reshape(-1).cpu().numpy() for p in probs]).astype(np.float64)
    ok = (x > 0) & (y > 0)
    assert int(ok.sum()) == int(round(float(moments[b, 0])))
    ref = np.polyfit(x[ok], y[ok], 3)
    np.testing.assert_allclose(coeffs[b].cpu().numpy(), ref, rtol=2e-7, atol=1e-9)
    # every tile's matched image is the polynomial of its pseudo image (one tile bit-exact against NumPy's polyval)
    co = coeffs.cpu().numpy()
    for ti in (0, 7):
        xs = outs[ti].band(b, "pseudo").cpu().numpy()
        want = np.clip(np.polyval(co[b], xs.astype(np.float64)).astype(np.float32), 0, 1)
        assert np.array_equal(outs[ti].band(b, "matched").cpu().numpy(), want)
    # the mosaic fit equals the sum of the per-tile moments (tile order), and per-tile local fits differ from it
    local = plan.step(probs[0].cube, probs[0].real, reuse_buffers=False)
    assert not torch.equal(local.coeffs, coeffs)
    # the resident form (bench.py --tiles-per-gpu 8): batched launches, same fit
    c2, m2, outs2 = plan.fuse_mosaic([(p.cube, p.real) for p in probs], resident=True)
    torch.cuda.synchronize()
    np.testing.assert_allclose(m2.cpu().numpy(), moments.cpu().numpy(), rtol=1e-13)
    xs = np.linspace(0.0, 0.6, 40)          # the sums differ in the last bit (another tree over the tiles); the fit amplifies that
    for bb in range(nb):
        np.testing.assert_allclose(np.polyval(c2[bb].cpu().numpy(), xs), np.polyval(co[bb], xs), rtol=1e-7, atol=1e-10)
    assert torch.equal(outs2[7].pseudo.view(torch.int32), outs[7].pseudo.view(torch.int32))
    # the group pipeline (r04: one kernel per tile, one fit per step; bench.py --tiles-per-gpu 8 at N = 1) at full size: two steps, every
    # tile with the per-tile form's coefficients, moments and images bit for bit
    gp = SpectralFusion(p0.emit_w, p0.srf, p0.good_mask, deg=3, min_valid=0.0, min_count=50, fuse_apply=True, group_tiles=T)
    got = []
    for _ in range(2):
        for p in probs:
            o = gp.submit(p.cube, p.real)
            if o is not None:
                got.append((o.coeffs.clone(), o.moments.clone(), o.matched[::4099].clone(), o.pseudo[::4099].clone()))
    got += [(o.coeffs.clone(), o.moments.clone(), o.matched[::4099].clone(), o.pseudo[::4099].clone()) for o in gp.drain()]
    torch.cuda.synchronize()
    assert len(got) == 2 * T
    for k, (gc, gm, gmat, gps) in enumerate(got):
        assert torch.equal(gc.view(torch.int64), coeffs.view(torch.int64)) and torch.equal(gm.view(torch.int64), moments.view(torch.int64)), k
        assert torch.equal(gmat.view(torch.int32), outs[k % T].matched[::4099].view(torch.int32)), k
        assert torch.equal(gps.view(torch.int32), outs[k % T].pseudo[::4099].view(torch.int32)), k
    gp.close()
    del outs, outs2, probs, got
    torch.cuda.empty_cache()


def test_bench_line_carries_full_size_parity(torch_gpu):
    """bench.py as the driver runs it (fewer steps): the JSON line holds roofline (>= 20 event-bracketed launches, total
    fraction), the CPU baseline (1 thread + all cores) and max_rel_err of the FULL 1024 x 1024 tile against the
    oracle run on the same cube - C3 is oracle-checked at full size, not only through properties."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "5", "--warmup", "2", "--cpu-rows", "64"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["steps"] == 5 and line["dtype"] == "f32" and line["vs_baseline"] is None
    roof = line["roofline"]
    assert roof["kernel_launches_timed"] >= 20 and 0.2 < roof["frac"] < 1.0 and roof["total_fraction"] > roof["step_frac_of_peak"]
    assert roof["measured_read_peak"] > roof["measured_plain_read"] * 0.9
    cb = line["cpu_baseline"]
    assert cb["cores"] == 1 and cb["all_cores"]["cores"] >= 1 and cb["all_cores"]["value"] > cb["value"] * 0.5
    err = line["max_rel_err"]
    assert err["pixels_checked"] == 1024 * 1024 and err["pseudo"] < 2e-6 and err["matched"] < 1e-4, err


def test_bench_dump_outputs(torch_gpu, tmp_path):
    """bench.py --dump-outputs DIR: the last timed step's result as .npy files - whole images for a small tile (the same
    bits in two runs: the inputs are seeded), a fixed pixel sample within 64 MB for the headline tile - and the dumped
    matched image is the dumped polynomial applied to the dumped pseudo image."""
    import json, subprocess
    from conftest import ROOT
    quick = ["--steps", "3", "--warmup", "1", "--settle-ms", "0", "--no-cpu-baseline", "--no-probe", "--placement-trials", "0",
             "--cold-steps", "0", "--k1-launches", "0"]

    def run(d, *extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *quick, *extra, "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        files = {n: np.load(d / (n + ".npy")) for n in ("coeffs", "moments", "pseudo", "matched")}
        assert sorted(p.name for p in d.iterdir()) == sorted(n + ".npy" for n in files)
        assert sum(a.nbytes for a in files.values()) == line["dump_outputs"]["bytes"] <= 64 << 20
        for n, a in files.items():
            assert a.dtype == (np.float64 if n in ("coeffs", "moments") else np.float32) and np.isfinite(a).all(), n
            assert list(a.shape) == line["dump_outputs"]["files"][n]["shape"]
        nb = files["coeffs"].shape[0]
        assert files["coeffs"].shape == (nb, 4) and files["moments"].shape == (nb, 11)
        ref = onp.apply_poly_planes(files["pseudo"], files["coeffs"], None, clip=True)
        assert np.max(np.abs(files["matched"] - ref)) < 1e-5
        return files, nb

    a, nb = run(tmp_path / "a", "--height", "256", "--width", "256")
    assert a["pseudo"].shape == a["matched"].shape == (nb, 256, 256)
    b, _ = run(tmp_path / "b", "--height", "256", "--width", "256")
    for n in a:
        assert a[n].tobytes() == b[n].tobytes(), n
    c, _ = run(tmp_path / "c")
    assert c["pseudo"].shape == c["matched"].shape == (nb, 1 << 18)


def test_integration_md_stub_runs(torch_gpu):
    """The ctypes stub printed in INTEGRATION.md, exactly as a maintainer of the reference would write it (nothing
    from this package but the shared library), gives the package's own planes."""
    torch = torch_gpu
    import ctypes as C, os
    import s2_emit
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    _lib = C.CDLL(os.path.join(root, "hyperspectral_super-resolution_amd", "lib", "libhsr_mi355x.so"))
    _lib.hsr_srf_integrate.restype = C.c_int
    _lib.hsr_srf_integrate.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32,
                                       C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    _lib.hsr_last_error.restype = C.c_char_p

    def srf_integrate(cube, Wn, k0, klen):
        npix, B, nb = cube.shape[0] * cube.shape[1], cube.shape[2], Wn.shape[0]
        out = torch.empty((nb, npix), dtype=torch.float32, device=cube.device)
        rc = _lib.hsr_srf_integrate(cube.data_ptr(), npix, B, Wn.data_ptr(),
                                    k0.ctypes.data_as(C.POINTER(C.c_int32)),
                                    klen.ctypes.data_as(C.POINTER(C.c_int32)), nb,
                                    out.data_ptr(), npix, 1, None,
                                    torch.cuda.current_stream().cuda_stream)
        if rc:
            raise RuntimeError(_lib.hsr_last_error().decode())
        return out

    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths()
    R = onp.synthetic_cube(40, 30, seed=3)
    Wn64, names = onp.srf_weight_matrix(w, srf, good)
    Wn = np.ascontiguousarray(Wn64, dtype=np.float32)
    nz = [np.flatnonzero(r) for r in Wn]
    k0 = np.array([z[0] for z in nz], np.int32)
    klen = np.array([z[-1] - z[0] + 1 for z in nz], np.int32)
    planes = srf_integrate(torch.from_numpy(R).cuda(), torch.from_numpy(Wn).cuda(), k0, klen).cpu().numpy()
    ref = s2_emit.pseudo_s2_srf_integral(R, w, srf, good)
    for i, k in enumerate(names):
        assert np.array_equal(planes[i].reshape(40, 30), ref[k].astype(np.float32)), k


def test_u16_fast_arithmetic_option(torch_gpu):
    """hsr_srf_options.flags & HSR_SRF_U16_FAST: decode scale folded into the weights + packed fma.  Not bit-identical to
    the exact uint16 path any more; stated tolerance: <= 1e-6 relative against it (7e-7 observed), <= 2e-6 against the float64 oracle,
    NaN pattern (nodata pixels) identical; coefficients of a fused step within 1e-5 of the exact path's."""
    torch = torch_gpu
    from s2_emit import SpectralFusion, _engine as eng
    from s2_emit.synthetic import device_problem
    p = device_problem(100, 130, 285, deg=3, seed=9)
    u = eng.tile_encode_u16(p.cube)
    u.view(-1)[7 * 285 + 3] = 65535
    table = eng.build_srf_table(p.emit_w, p.srf, p.good_mask)
    exact = eng.srf_integrate(u, table, layout="pixmajor")
    fast = eng.srf_integrate(u, table, layout="pixmajor", opts=eng.srf_options(u16_fast=True))
    e, f = exact[:, :table.nb].cpu().numpy(), fast[:, :table.nb].cpu().numpy()
    assert np.array_equal(np.isnan(e), np.isnan(f)) and np.isnan(f[7]).all()
    ok = np.isfinite(e)
    assert not np.array_equal(e[ok], f[ok])                      # it IS a different arithmetic
    assert np.max(np.abs(f[ok] - e[ok]) / np.abs(e[ok])) < 1e-6
    R = eng.tile_decode_u16(u).cpu().numpy().reshape(100, 130, 285)
    ref = onp.pseudo_s2_srf_integral(R, p.emit_w, p.srf, p.good_mask)
    for i, k in enumerate(table.supported):
        assert _rel_err(f[:, i].reshape(100, 130), ref[k]) < 2e-6, k
    a = SpectralFusion(p.emit_w, p.srf, p.good_mask, deg=3).step(u, p.real, reuse_buffers=False)
    b = SpectralFusion(p.emit_w, p.srf, p.good_mask, deg=3, u16_fast=True).step(u, p.real, reuse_buffers=False)
    # the cubic's coefficients are ill-conditioned in the planes (cond ~1e4): 1e-6 planes -> ~1e-5 coefficients, while the
    # polynomial itself (the matched image, below) moves by < 1e-6
    np.testing.assert_allclose(b.coeffs.cpu().numpy(), a.coeffs.cpu().numpy(), rtol=2e-3, atol=2e-5)
    ma, mb = a.matched.cpu().numpy(), b.matched.cpu().numpy()
    okm = np.isfinite(ma)
    assert np.max(np.abs(ma[okm] - mb[okm])) < 1e-6
    # batches take the flag too
    tb = SpectralFusion(p.emit_w, p.srf, p.good_mask, deg=3, u16_fast=True).step_batch([u, u], [p.real, p.real])
    assert torch.equal(tb.tile(1).matched.view(torch.int32), b.matched.view(torch.int32))


def test_stream_envi_files_bil_bsq_bit_exact_with_bip_feed(torch_gpu, tmp_path):
    """SURVEY 8-f3 remainder: BIL / BSQ ENVI files go file -> pinned staging -> GPU in FILE order and are transposed there
    (hsr_interleave_to_bip) inside SpectralFusion.stream(); coefficients and images are bit-identical to feeding the
    same cube as a pixel-major array, for float32, uint16 (tile format, decoded in K1) and int16 files, ragged shapes
    included (reference loader: s2_emit/emit_io.py:7-16, transposes on the host)."""
    torch = torch_gpu
    from s2_emit import SpectralFusion, _engine as eng
    from s2_emit.emit_io import EnviCubeFile
    w, good = onp.synthetic_wavelengths()
    srf = onp.synthetic_srf()
    rng = np.random.default_rng(3)
    H, W, B = 37, 70, 285                                   # 70 samples, 285 bands: partial 64 x 64 transpose tiles
    cube = (rng.random((H, W, B)) * 0.55).astype(np.float32)
    real = rng.random((H, W, 12)).astype(np.float32)
    codes = {np.dtype(np.float32): 4, np.dtype(np.uint16): 12, np.dtype(np.int16): 2}

    def write(arr, inter, tag):
        lay = {"bip": arr, "bil": arr.transpose(0, 2, 1), "bsq": arr.transpose(2, 0, 1)}[inter]
        np.ascontiguousarray(lay).tofile(tmp_path / f"{tag}_{inter}.bin")
        (tmp_path / f"{tag}_{inter}.hdr").write_text(
            f"ENVI\nsamples = {W}\nlines = {H}\nbands = {B}\nheader offset = 0\ndata type = {codes[arr.dtype]}\n"
            f"interleave = {inter}\nbyte order = 0\n")
        return EnviCubeFile(str(tmp_path / f"{tag}_{inter}.hdr"), str(tmp_path / f"{tag}_{inter}.bin"))

    plan = SpectralFusion(w, srf, good, deg=2, min_valid=0.0)
    u16 = np.clip(np.rint(cube * 10000), 0, 65534).astype(np.uint16)
    u16[3, 5, 100] = 65535
    i16 = (u16.astype(np.int32) - 3000).astype(np.int16)
    for tag, arr in (("f32", cube), ("u16", u16), ("i16", i16)):
        feed = arr if tag != "i16" else arr.astype(np.float32)          # what the host loader would hand over
        ref = [(c.copy(), m.copy()) for _, c, m, _ in plan.stream([(feed, real)] * 3, depth=2)]
        for inter in ("bil", "bsq", "bip"):
            f = write(arr, inter, tag)
            assert f.shape == (H, W, B) and f.interleave == inter
            d = f.to_device("cuda")
            np.testing.assert_array_equal(d.cpu().numpy(), feed)                     # the transpose alone
            got = [(c.copy(), m.copy()) for _, c, m, _ in plan.stream([(f, real)] * 3, depth=2)]
            assert len(got) == 3
            for (c, m), (rc, rm) in zip(got, ref):
                assert np.array_equal(c.view(np.int64), rc.view(np.int64)), (tag, inter)
                assert np.array_equal(m.view(np.int32), rm.view(np.int32)), (tag, inter)
    # files and arrays mixed in one stream, depth 1 and 3
    f = write(cube, "bsq", "mix")
    for depth in (1, 3):
        got = [c.copy() for _, c, _, _ in plan.stream([(f, real), (cube, real), (f, real)], depth=depth)]
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[1], got[2])


def test_placement_trials_do_not_change_results(torch_gpu):
    """SpectralFusion's placement trials for the images it owns (profiles/r02_two_speeds.md: K1 is ~9 % slower when its
    output image lies in some stretches of device memory) only choose WHICH allocation is kept: results are bit-identical
    with and without them, the log shows what was timed, and small tiles skip the trials."""
    torch = torch_gpu
    from s2_emit import SpectralFusion
    from s2_emit.synthetic import device_problem
    p = device_problem(384, 256, 285, deg=3, seed=12)          # 98 304 pixels: above the 65 536-pixel threshold
    a = SpectralFusion(p.emit_w, p.srf, p.good_mask, deg=3, placement_trials=0)
    b = SpectralFusion(p.emit_w, p.srf, p.good_mask, deg=3, placement_trials=3)
    oa, ob = a.step(p.cube, p.real), b.step(p.cube, p.real)
    torch.cuda.synchronize()
    assert a.placement_log == {} and 1 <= len(b.placement_log[384 * 256]) <= 3
    assert torch.equal(oa.coeffs.view(torch.int64), ob.coeffs.view(torch.int64))
    assert torch.equal(oa.matched.view(torch.int32), ob.matched.view(torch.int32))
    assert torch.equal(oa.pseudo.view(torch.int32), ob.pseudo.view(torch.int32))
    ob2 = b.step(p.cube, p.real)                                  # second step: no more trials, same buffers
    assert ob2.pseudo.data_ptr() == ob.pseudo.data_ptr() and len(b.placement_log) == 1
    small = device_problem(64, 64, 285, deg=3, seed=13)
    b.step(small.cube, small.real)
    assert 64 * 64 not in b.placement_log
    # joint trials for a resident tile: inputs cloned next to candidate output images; the winner seeds the plan's image
    c = SpectralFusion(p.emit_w, p.srf, p.good_mask, deg=3, placement_trials=3)
    cube2, real2, log = c.place_inputs(p.cube, p.real)
    assert 1 <= len(log["joint_ms"]) <= 3 and torch.equal(cube2, p.cube) and torch.equal(real2, p.real)
    oc = c.step(cube2, real2)
    torch.cuda.synchronize()
    assert c.placement_log[384 * 256] == log["joint_ms"]          # step() ran no further trial
    assert torch.equal(oa.coeffs.view(torch.int64), oc.coeffs.view(torch.int64))
    assert torch.equal(oa.matched.view(torch.int32), oc.matched.view(torch.int32))
    assert c.place_inputs(p.cube, p.real)[2] == {}               # already placed for this tile size: a no-op
    # a spacer that cannot be allocated ends the search with what has been seen (no exception)
    d = SpectralFusion(p.emit_w, p.srf, p.good_mask, deg=3, placement_trials=3, placement_pitch_gb=400.0)
    od = d.step(p.cube, p.real)
    torch.cuda.synchronize()
    assert len(d.placement_log[384 * 256]) == 1
    assert torch.equal(oa.matched.view(torch.int32), od.matched.view(torch.int32))


@pytest.mark.gpu
def test_fused_fit_bit_identical_to_reduce_solve(torch_gpu):
    """hsr_srf_integrate_fit (slot reduction + solve folded into K1's launch: ticket per slot, the workgroup completing a
    group of slots adds it, the one completing the groups runs the butterfly, solves and re-arms the tickets) against
    hsr_srf_integrate_moments + hsr_moments_reduce_solve: same moments and coefficients bit for bit - for fewer slots
    than groups (S < 64), ragged group sizes (S = 496 with 8 reserved CUs, S = 157), every degree, masks, uint16 tiles
    (ring and single buffer), a rank-deficient band (constant x: the Jacobi path, its matrices in LDS) and an
    under-populated band (identity fallback); the tickets are left zero, so repeated launches agree too."""
    torch = torch_gpu
    from s2_emit import SpectralFusion, _engine as eng
    w, good = onp.synthetic_wavelengths()
    srf = onp.synthetic_srf()
    g = torch.Generator(device="cuda")
    g.manual_seed(21)
    cases = [((3, 50), {}), ((100, 100), {}), ((130, 300), {}), ((256, 512), {}), ((256, 512), {"reserved_cus": 8}),
             ((64, 63), {"u16_single_buffer": True})]
    for (H, W), kw in cases:
        cube = torch.rand((H, W, 285), generator=g, device="cuda") * 0.6
        real = torch.rand((H, W, 12), generator=g, device="cuda")
        real[..., 5] = -1.0                                   # below min_valid everywhere: identity fallback for band 5
        mask = (torch.rand(H * W, generator=g, device="cuda") > 0.3).to(torch.uint8)
        flat = cube.clone()
        flat[:] = 0.25                                        # every pseudo band constant: singular Gram, Jacobi path
        for deg in (1, 2, 3, 4):
            for kind in ("f32", "u16"):
                for c, m in ((cube, None), (cube, mask), (flat, None)):
                    cc = c if kind == "f32" else eng.tile_encode_u16(c)
                    a = SpectralFusion(w, srf, good, deg=deg, min_count=5, placement_trials=0, fused_fit=False, **kw)
                    b = SpectralFusion(w, srf, good, deg=deg, min_count=5, placement_trials=0, fused_fit=True, **kw)
                    oa = a.step(cc, real, m)
                    for rep in range(3):
                        ob = b.step(cc, real, m)
                        torch.cuda.synchronize()
                        tag = ((H, W), kw, deg, kind, m is not None, c is flat, rep)
                        assert torch.equal(oa.moments.view(torch.int64), ob.moments.view(torch.int64)), tag
                        assert torch.equal(oa.coeffs.view(torch.int64), ob.coeffs.view(torch.int64)), tag
                        assert torch.equal(oa.matched.view(torch.int32), ob.matched.view(torch.int32)), tag
                        assert int(b.ws.tickets.abs().sum()) == 0, tag
                    assert torch.isfinite(ob.coeffs).all()
                    assert torch.equal(ob.coeffs[5], torch.tensor([0.0] * (deg - 1) + [1.0, 0.0], dtype=torch.float64, device="cuda"))


@pytest.mark.gpu
def test_predict_cube_bad_pixel_rule_in_kernel(torch_gpu):
    """predict_cube_logit's rule for unusable pixels (Spectral_matching.ipynb raw lines 197-203: any input non-finite, or
    isclose to nodata -> NaN in every target) is part of the predict kernels' epilogue (hsr_polyfeat_predict_cube): same
    mask as torch's isfinite / isclose, clean pixels bit-identical to a call on the cleaned cube - for the kernels of
    10 inputs deg 3 (T = 5: predict103_x16_kernel; T = 70: one 96-target slice of predict103_slice_kernel<3>; T = 285: three
    such slices) and the generic kernel."""
    torch = torch_gpu
    import s2_emit
    rng = np.random.default_rng(23)
    for Cin, deg, T in ((10, 3, 5), (10, 3, 70), (10, 3, 285), (4, 2, 40)):
        N = 1500
        base = rng.random((N, 4))
        X = (600 + 4000 * np.clip(base @ rng.random((4, Cin)) / 2, 0, 1)).astype(np.float32)
        Y = onp.logit(np.clip(base @ rng.random((4, T)) / 3 + 0.01 * rng.standard_normal((N, T)), 0.001, 0.6))
        model = s2_emit.PolyRidge(degree=deg, alpha=1.0).fit(X, Y)
        H, W = 37, 41                                    # 1517 pixels: ragged last tile
        cube = (600 + 4000 * rng.random((Cin, H, W))).astype(np.float32)
        clean = torch.from_numpy(cube).cuda()
        dirty = clean.clone()
        dirty[0, 3, 4] = float("nan")
        dirty[Cin - 1, 5, 6] = float("inf")
        dirty[1, 7, 8] = float("-inf")
        dirty[2, 9, 10] = -9999.0
        dirty[3, 36, 40] = -9999.05                      # inside isclose's 1e-5 relative band of the nodata value
        dirty[2, 11, 12] = -9998.0                       # outside it: a usable (if odd) sample
        for nodata in (None, -9999.0):
            got = model.predict_cube(dirty, nodata=nodata)
            x2 = dirty.reshape(Cin, -1)
            bad = ~torch.isfinite(x2).all(dim=0)
            if nodata is not None:
                bad |= torch.isclose(x2, torch.tensor(float(nodata), device="cuda")).any(dim=0)
            assert int(bad.sum()) == (3 if nodata is None else 5)
            g2 = got.reshape(T, -1)
            assert torch.isnan(g2[:, bad]).all(), (Cin, deg, T, nodata)
            ref = model.predict_cube(torch.where(bad.reshape(1, H, W), clean, dirty), nodata=None).reshape(T, -1)
            assert torch.equal(g2[:, ~bad].view(torch.int32), ref[:, ~bad].view(torch.int32)), (Cin, deg, T, nodata)
            assert torch.isfinite(g2[:, ~bad]).all()


@pytest.mark.gpu
def test_place_batch_inputs_keeps_results(torch_gpu):
    """place_batch_inputs(): copies of a stacked batch tried in other stretches of device memory - same bytes, so the batch
    on the returned tensors is bit-identical to the batch on the originals, and step_batch() finds the cached plan."""
    torch = torch_gpu
    from s2_emit import SpectralFusion
    from s2_emit.synthetic import device_problem
    p = device_problem(64 * 4, 64, 285, deg=3, seed=9)
    cubes, reals = p.cube.reshape(4, 64, 64, 285), p.real.reshape(4, 64, 64, -1)
    a = SpectralFusion(p.emit_w, p.srf, p.good_mask, deg=3, placement_trials=0)
    b = SpectralFusion(p.emit_w, p.srf, p.good_mask, deg=3, placement_trials=3, placement_pitch_gb=1.0)
    oa = a.step_batch(cubes, reals)
    c2, r2, log = b.place_batch_inputs(cubes, reals)
    assert len(log["joint_ms"]) == 3 and torch.equal(c2, cubes) and torch.equal(r2, reals)
    nb_before = len(b._batches)
    ob = b.step_batch(c2, r2)
    torch.cuda.synchronize()
    assert len(b._batches) == nb_before                     # the placed batch was reused
    assert torch.equal(oa.coeffs.view(torch.int64), ob.coeffs.view(torch.int64))
    assert torch.equal(oa.matched.view(torch.int32), ob.matched.view(torch.int32))


@pytest.mark.gpu
def test_step_batch_other_band_counts(torch_gpu):
    """The batched slot reduction has one instantiation per band-count class (<= 8, <= 12, <= 16 bands): 3, 7 and 13
    supported bands, every tile still bit-identical to its own step()."""
    torch = torch_gpu
    from s2_emit import SpectralFusion
    w, _ = onp.synthetic_wavelengths()
    full = onp.synthetic_srf()
    names = list(full)
    g = torch.Generator(device="cuda")
    g.manual_seed(31)
    shapes = [(100, 100), (9, 40), (64, 65)]
    for pick in (names[1:4], names[:7], names):            # good_mask None: all 13 bands have support
        srf = {k: full[k] for k in pick}
        plan = SpectralFusion(w, srf, None, deg=2, min_count=5)
        nb = len(plan.names)
        assert nb == len(pick)
        row = (nb + 3) // 4 * 4
        cubes = [torch.rand((H, W, 285), generator=g, device="cuda") * 0.6 for H, W in shapes]
        reals = [torch.rand((H, W, row), generator=g, device="cuda") for H, W in shapes]
        out = plan.step_batch(cubes, reals)
        torch.cuda.synchronize()
        for i in range(len(shapes)):
            o = plan.step(cubes[i], reals[i], reuse_buffers=False)
            ti = out.tile(i)
            assert torch.equal(o.moments.view(torch.int64), ti.moments.view(torch.int64)), (nb, i)
            assert torch.equal(o.coeffs.view(torch.int64), ti.coeffs.view(torch.int64)), (nb, i)
            assert torch.equal(o.matched.view(torch.int32), ti.matched.view(torch.int32)), (nb, i)


@pytest.mark.parametrize("script,args", [("stress_fused.py", ["7", "12"]), ("stress_fused.py", ["8", "20", "tiny"]), ("stress_batch.py", ["7", "4"]), ("stress_mosaic.py", ["7", "5"]),
                                         ("stress_r03.py", ["7", "20"]), ("stress_upsample.py", ["7", "15"]), ("stress_k1.py", ["7", "15"]),
                                         ("stress_stream.py", ["7", "5"])])
def test_randomised_shapes_through_the_round3_paths(torch_gpu, script, args):
    """A short, seeded run of the randomised stress tools (tools/dbg/stress_*.py; one child process each): random tile shapes,
    band sets, degrees, masks and cube types through the fused / two-slot pipelines and the prepared step(), step_batch,
    both forms of fuse_mosaic, the rebuilt Gram / Cholesky / percentile / predict kernels, the producer upsampler and K1 -
    against the operator-by-operator path or NumPy.  Longer runs of the same tools found the two defects fixed in round 3
    (a launch of fewer workgroups than bands carrying the tail fit; the last-bit difference between the two mosaic forms)."""
    import subprocess
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dbg", script)] + args, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, (script, r.stdout[-1500:], r.stderr[-1500:])
    assert "failures: 0" in r.stdout
