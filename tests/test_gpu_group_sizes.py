"""The group pipeline - SpectralFusion(fuse_apply=True, group_tiles=T), hsr_pipeline_create_group - at the group sizes whose code no
other test runs: T = 32 (the first half of the group sum full), 33 (the first entry of the l + 32 half) and 64 (the largest group).

Two whole groups are submitted, then drain().  Every tile has its own data (seed and amplitude), masks come and go between the
tiles of the first group, the second group has none.  Two tile geometries:
  * 16 x 64 pixels with the 285-sample table (12 bands): 16 workgroups >= 12 bands, so every tile's reduction - and behind a group's
    last tile the sum over the T entries and the solve - rides in the tail of the next tile's K1 launch (csrc/hsr_fused_dev.h:
    lazy_fit); the launch record names the job-carrying instance;
  * 3 x 90 pixels: 5 workgroups < 12 bands, so the reduction and the group fit run as launches of their own (csrc/hsr_exec.hip:
    fit_standalone, hsr_moments_reduce_solve over the T entries).
Every tile that comes out is compared
  * bit for bit with fuse_mosaic() over its own group: pseudo and matched rows, the group's moments, the coefficients;
  * in the unmasked group against float64, with the bars of tests/test_fused_drain.py as they stand: pseudo planes rel 2e-6 of
    oracle_np.pseudo_s2_srf_integral (float32 accumulation of <= ~40 taps against float64); the fitted curves against
    oracle_np.fit_per_band_poly over the CONCATENATED pixels of the group, over each band's own range of x, rtol 1e-5 / atol 1e-6;
    matched planes rel 1e-4 of oracle_np.apply_poly_planes with the oracle's coefficients.
One uint16 group of 33 tiles goes through the ring kernel.
Nothing on these paths polls (the gated wait of the exchange pipeline and its time-out branch are not part of a group pipeline and
are deliberately not exercised here either); every test runs under a time limit.
"""
import ctypes as C
import warnings

import numpy as np
import pytest

from gpu_harness import torch_gpu  # noqa: F401
from oracle import oracle_np as onp

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

warnings.simplefilter("ignore")

MIN_COUNT = 5
GEOMS = {"tail": (16, 64), "standalone": (3, 90)}
_tiles = {}


def _table():
    w, good = onp.synthetic_wavelengths()
    return w, onp.synthetic_srf(), good


def _tile(geom, k, u16=False):
    """Host data of tile k of a geometry, built once: the cube (its own seed and amplitude), the float64 pseudo planes as float32,
    the targets (pixel-major) and, for k % 3 == 1, a mask."""
    key = (geom, k, u16)
    if key not in _tiles:
        H, W = GEOMS[geom]
        w, srf, good = _table()
        R = (onp.synthetic_cube(H, W, seed=1000 * list(GEOMS).index(geom) + k) * np.float32(0.5 + 0.125 * (k % 5))).astype(np.float32)
        if u16:
            R = onp.tile_decode_u16(onp.tile_encode_u16(R))
        ps = onp.pseudo_s2_srf_integral(R, w, srf, good)
        pseudo = np.stack([v for v in ps.values() if v is not None]).astype(np.float32)            # (nb, H, W)
        real = onp.synthetic_real_planes(pseudo, seed=500 + k)
        mask = (np.random.default_rng(k).random(H * W) > 0.4).astype(np.uint8) if k % 3 == 1 else None
        _tiles[key] = dict(R=R, pseudo=pseudo, real=real, real_pm=np.ascontiguousarray(np.moveaxis(real, 0, -1)), mask=mask)
    return _tiles[key]


def _rel_err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    if not fin.any():
        return 0.0
    scale = np.maximum(np.abs(ref[fin]), 1e-3 * np.max(np.abs(ref[fin])) + 1e-30)
    return float(np.max(np.abs(got[fin] - ref[fin]) / scale))


def _clone(o):
    return tuple(t.clone() for t in (o.pseudo, o.matched, o.moments, o.coeffs))


def _same_bits(torch, got, want, what):
    for g, x, part in zip(got, want, ("pseudo", "matched", "moments", "coeffs")):
        as_int = torch.int32 if g.dtype == torch.float32 else torch.int64
        assert torch.equal(g.view(as_int), x.view(as_int)), what + (part,)


def _against_oracle(got, host, deg, shape_hw, what):
    """The tiles of an unmasked group against float64: got = per tile (pseudo, matched, moments, coeffs), host = their _tile records."""
    H, W = shape_hw
    nb = host[0]["pseudo"].shape[0]
    px = np.concatenate([t["pseudo"].reshape(nb, -1) for t in host], axis=1)
    py = np.concatenate([t["real"].reshape(nb, -1) for t in host], axis=1)
    coeffs_o, counts = onp.fit_per_band_poly(px, py, np.ones(px.shape[1], bool), deg, 0.0, MIN_COUNT)
    assert counts.min() >= MIN_COUNT
    ep = em = 0.0
    for i, (gt, t) in enumerate(zip(got, host)):
        pseudo = gt[0].cpu().numpy()[:, :nb].T.reshape(nb, H, W)
        matched = gt[1].cpu().numpy()[:, :nb].T.reshape(nb, H, W)
        e1, e2 = _rel_err(pseudo, t["pseudo"]), _rel_err(matched, onp.apply_poly_planes(t["pseudo"], coeffs_o, None, clip=True))
        ep, em = max(ep, e1), max(em, e2)
        assert e1 < 2e-6, what + (i, "pseudo", e1)
        assert e2 < 1e-4, what + (i, "matched", e2)
    print(f"{what}: largest rel err over the group: pseudo {ep:.3g} (bar 2e-6), matched {em:.3g} (bar 1e-4)")
    co = got[0][3].cpu().numpy()
    for b in range(nb):
        # the curve over the band's OWN range of x in the group: that is where the data determine it
        xs = np.linspace(float(np.nanmin(px[b])), float(np.nanmax(px[b])), 50)
        np.testing.assert_allclose(np.polyval(co[b], xs), np.polyval(coeffs_o[b], xs), rtol=1e-5, atol=1e-6, err_msg=str(what + (b,)))


def _run_groups(torch, geom, T, deg, u16, groups):
    """Submit `groups` whole groups of T tiles, drain, and compare every tile; at most one group's cubes are resident at a time."""
    from s2_emit import SpectralFusion, _engine as eng, _native as nat
    lib = nat.load()
    H, W = GEOMS[geom]
    w, srf, good = _table()
    kw = dict(deg=deg, min_valid=0.0, min_count=MIN_COUNT, clip=True, apply_mask=True)
    pipe = SpectralFusion(w, srf, good, fuse_apply=True, group_tiles=T, **kw)
    ref = SpectralFusion(w, srf, good, **kw)
    nb = pipe.table.nb
    rides = lib.hsr_partial_slots(H * W, eng._opt(pipe.opts)) >= nb
    assert rides == (geom == "tail"), "16 x 64 pixels: the fit rides in the tail (hsr_partial_slots(npix) >= nb); 3 x 90: it cannot"
    got, want, host = [], [], []
    d, v, lds = C.c_int32(), C.c_int32(), C.c_int64()
    for g in range(groups):
        hs = [_tile(geom, g * T + i, u16) for i in range(T)]
        if g == groups - 1:                                   # the last group has no mask: the one the oracle covers
            hs = [dict(h, mask=None) for h in hs]
        dev = []
        for h in hs:
            c = torch.from_numpy(h["R"]).cuda()
            dev.append((eng.tile_encode_u16(c) if u16 else c, torch.from_numpy(h["real_pm"]).cuda(),
                        None if h["mask"] is None else torch.from_numpy(h["mask"]).cuda()))
        for c, r, m in dev:
            o = pipe.submit(c, r, m)
            assert (o is None) == (pipe._pipe["n"] <= T + 1)        # a tile comes out T + 1 submits late
            if o is not None:
                got.append(_clone(o))
        if rides:                                             # the K1 launch of the group's last tile: the job-carrying instance
            assert lib.hsr_srf_last_launch(C.byref(d), C.byref(v), C.byref(lds)) == 1 and (d.value, v.value) == (deg, 18 if u16 else 6)
        co, tot, outs = ref.fuse_mosaic([(c, r) for c, r, _ in dev], [m for _, _, m in dev])
        want += [(o.pseudo.clone(), o.matched.clone(), tot.clone(), co.clone()) for o in outs]
        host += hs
        del dev, outs
    st = pipe._pipe
    assert st["fused"] and st["S"] == T + 2 and st["group"] is not None
    got += [_clone(o) for o in pipe.drain()]
    assert len(got) == groups * T and pipe.drain() == []
    for k, (gt, wt) in enumerate(zip(got, want)):
        _same_bits(torch, gt, wt, (geom, T, deg, u16, k // T, k % T))
    last = slice((groups - 1) * T, groups * T)
    _against_oracle(got[last], host[last], deg, (H, W), (geom, T, deg, u16))
    pipe.close()
    ref.close()


@pytest.mark.parametrize("deg", [1, 4])
@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("T", [32, 33, 64])
def test_group_pipeline_at_group_sizes_up_to_64(torch_gpu, T, geom, deg):
    _run_groups(torch_gpu, geom, T, deg, False, 2)


def test_group_of_33_uint16_tiles(torch_gpu):
    """The same group sum behind the uint16 ring kernel (tiles quantised as the reference writer does, oracle over the decoded tiles)."""
    _run_groups(torch_gpu, "tail", 33, 3, True, 2)
