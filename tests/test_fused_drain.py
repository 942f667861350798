"""The drain of the fused pipeline (csrc/hsr_exec.hip: finish_fused, drain_apply_fit_kernel) and the timing events
bound to the fused launch.

submit() x k, then drain(): with two tiles pending the drain is two launches - K3 of the older tile with the fit of the newest one
in its tail, then K3 of the newest tile - instead of K3, reduce + solve, K3.  Every tile that comes out is compared
  * bit for bit with step() on the same tile (hsr_moments_reduce_solve and apply_rows_kernel, which the drain does not use), and
  * where the oracle covers the case (no mask) against oracle.oracle_np.fuse_lsq_reference with the tolerances of
    tests/test_gpu_parity.py::test_fused_pipeline_vs_oracle: pseudo planes rel 2e-6 (float32 accumulation of <= ~40 taps against
    float64), fitted curves rtol 1e-5 / atol 1e-6 (over each band's own range of x), matched planes rel 1e-4.
Nothing on these paths polls; every test runs under a time limit.
"""
import time
import warnings

import numpy as np
import pytest

from gpu_harness import torch_gpu  # noqa: F401
from oracle import oracle_np as onp

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

warnings.simplefilter("ignore")

MIN_COUNT = 5


def _rel_err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    if not fin.any():
        return 0.0
    scale = np.maximum(np.abs(ref[fin]), 1e-3 * np.max(np.abs(ref[fin])) + 1e-30)
    return float(np.max(np.abs(got[fin] - ref[fin]) / scale))


# name -> (H, W, B, SRF bands or None = all 13, use the good-band mask, bands expected, row length)
SHAPES = {
    "fewer_groups_than_bands": (2, 158, 285, ("B2", "B3", "B4", "B5", "B6", "B7", "B8"), True, 7, 8),   # 5 groups < 7 bands: the fallback
    "whole_groups": (64, 64, 285, None, True, 12, 12),                                                  # B is no multiple of 4
    "ragged_last_group": (33, 37, 31, None, True, None, None),
    "padded_rows": (40, 50, 285, None, False, 13, 16),
}
_problems = {}


def _problem(torch, name):
    """Two tiles of the shape, their targets, one mask and the float64 reference of each tile (clip on / off) - built once."""
    if name in _problems:
        return _problems[name]
    H, W, B, sel, use_good, nb_want, row_want = SHAPES[name]
    from s2_emit import _engine as eng
    srf13 = onp.synthetic_srf()
    srf = srf13 if sel is None else {k: srf13[k] for k in sel}
    w, good = onp.synthetic_wavelengths(B)
    gm = good if use_good else None
    nb = eng.build_srf_table(w, srf, gm).nb
    if nb_want is not None:
        assert (nb, eng.padded_row(nb)) == (nb_want, row_want)
    tiles = []
    for ti in range(2):
        R = onp.synthetic_cube(H, W, B=B, seed=40 + ti)
        ps = onp.pseudo_s2_srf_integral(R, w, srf, gm)
        names = [k for k, v in ps.items() if v is not None]
        real = onp.synthetic_real_planes(np.stack([ps[k] for k in names]).astype(np.float32), seed=7 + ti)
        tiles.append(dict(R=R, real=real, cube=torch.from_numpy(R).cuda(), real_d=torch.from_numpy(real).cuda(), oracle={}))
    rng = np.random.default_rng(5)
    mask = torch.from_numpy((rng.random(H * W) > 0.3).astype(np.uint8)).cuda()
    _problems[name] = dict(w=w, srf=srf, gm=gm, nb=nb, tiles=tiles, mask=mask, H=H, W=W)
    return _problems[name]


def _oracle(pr, ti, deg, clip):
    tl = pr["tiles"][ti]
    if (deg, clip) not in tl["oracle"]:
        tl["oracle"][(deg, clip)] = onp.fuse_lsq_reference(tl["R"], pr["w"], pr["srf"], pr["gm"], tl["real"], deg, 0.0, MIN_COUNT, clip)
    return tl["oracle"][(deg, clip)]


def _clone(o):
    return tuple(t.clone() for t in (o.pseudo, o.matched, o.moments, o.coeffs))


def _same_bits(torch, got, want, what):
    for g, x, part in zip(got, want, ("pseudo", "matched", "moments", "coeffs")):
        as_int = torch.int32 if g.dtype == torch.float32 else torch.int64
        assert torch.equal(g.view(as_int), x.view(as_int)), what + (part,)


def _against_oracle(got, ref, shape_hw, what):
    pseudo_o, coeffs_o, matched_o, _ = ref
    nb = pseudo_o.shape[0]
    H, W = shape_hw
    pseudo = got[0].cpu().numpy()[:, :nb].T.reshape(nb, H, W)
    matched = got[1].cpu().numpy()[:, :nb].T.reshape(nb, H, W)
    assert _rel_err(pseudo, pseudo_o) < 2e-6, what
    co = got[3].cpu().numpy()
    for b in range(nb):
        # the curve over the band's OWN range of x: that is where the data determine it (outside it two fits that agree on every pixel
        # may still part - a 13-band table holds bands whose range is a fraction of the image's)
        xs = np.linspace(float(np.nanmin(pseudo_o[b])), float(np.nanmax(pseudo_o[b])), 50)
        np.testing.assert_allclose(np.polyval(co[b], xs), np.polyval(coeffs_o[b], xs), rtol=1e-5, atol=1e-6, err_msg=str(what + (b,)))
    assert _rel_err(matched, matched_o) < 1e-4, what


@pytest.mark.parametrize("deg", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_drain_carries_the_bits_of_step_and_matches_the_oracle(torch_gpu, shape, deg):
    torch = torch_gpu
    from s2_emit import SpectralFusion
    pr = _problem(torch, shape)
    tiles, mask = pr["tiles"], pr["mask"]
    for clip in (True, False):
        kw = dict(deg=deg, min_valid=0.0, min_count=MIN_COUNT, clip=clip, apply_mask=True)
        ref = SpectralFusion(pr["w"], pr["srf"], pr["gm"], **kw)
        want = {(ti, m is not None): _clone(ref.step(tiles[ti]["cube"], tiles[ti]["real_d"], m, reuse_buffers=False))
                for ti in range(2) for m in (None, mask)}
        for masked in (False, True):
            for k in (1, 2, 5):     # one pending tile (nothing for the body of the drain kernel), two, two behind a running pipeline
                pipe = SpectralFusion(pr["w"], pr["srf"], pr["gm"], fuse_apply=True, **kw)
                seq = [(i % 2, masked and i % 2 == 0) for i in range(k)]        # the masks come and go from tile to tile
                got = []
                for ti, m in seq:
                    o = pipe.submit(tiles[ti]["cube"], tiles[ti]["real_d"], mask if m else None)
                    if o is not None:
                        got.append(_clone(o))
                assert pipe._pipe["fused"] and pipe._pipe["S"] == 3 and len(got) == max(0, k - 2)
                got += [_clone(o) for o in pipe.drain()]
                assert len(got) == k and pipe.drain() == []
                for i, ((ti, m), gt) in enumerate(zip(seq, got)):
                    what = (shape, deg, clip, masked, k, i)
                    _same_bits(torch, gt, want[(ti, m)], what)
                    if not m and i >= k - 2:                                    # what the drain finished, where the oracle has no mask either
                        _against_oracle(gt, _oracle(pr, ti, deg, clip), (pr["H"], pr["W"]), what)
                pipe.close()
        ref.close()


def test_drain_on_uint16_tiles(torch_gpu):
    """The drain kernel reads images and partials only, whatever the cube's format: uint16 tiles through the ring kernel, once."""
    torch = torch_gpu
    from s2_emit import SpectralFusion, _engine as eng
    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths()
    H, W, deg = 40, 64, 3
    tiles = []
    for ti in range(2):
        R = onp.tile_decode_u16(onp.tile_encode_u16(onp.synthetic_cube(H, W, seed=60 + ti)))
        ps = onp.pseudo_s2_srf_integral(R, w, srf, good)
        names = [k for k, v in ps.items() if v is not None]
        real = onp.synthetic_real_planes(np.stack([ps[k] for k in names]).astype(np.float32), seed=9 + ti)
        u = eng.tile_encode_u16(torch.from_numpy(R).cuda())
        tiles.append((R, real, u, torch.from_numpy(real).cuda()))
    kw = dict(deg=deg, min_valid=0.0, min_count=MIN_COUNT, clip=True)
    ref = SpectralFusion(w, srf, good, **kw)
    pipe = SpectralFusion(w, srf, good, fuse_apply=True, **kw)
    got = []
    for i in range(5):
        o = pipe.submit(tiles[i % 2][2], tiles[i % 2][3])
        if o is not None:
            got.append(_clone(o))
    assert pipe._pipe["fused"] and pipe._pipe["S"] == 3
    got += [_clone(o) for o in pipe.drain()]
    assert len(got) == 5
    for i, gt in enumerate(got):
        R, real, u, real_d = tiles[i % 2]
        _same_bits(torch, gt, _clone(ref.step(u, real_d, reuse_buffers=False)), ("u16", i))
        if i >= 3:
            _against_oracle(gt, onp.fuse_lsq_reference(R, w, srf, good, real, deg, 0.0, MIN_COUNT, True), (H, W), ("u16", i))
    pipe.close()
    ref.close()


def test_bound_events_bracket_the_fused_launch(torch_gpu):
    """k1_events of submit() are bound to the fused launch's dispatch: both are complete after a synchronise, their elapsed time is
    positive and no longer than a wall-clock bracket taken round the same, synchronised, launch - and the tile's bits do not change."""
    torch = torch_gpu
    from s2_emit import SpectralFusion
    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths()
    H = W = 256
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    cube = torch.rand((H, W, 285), generator=g, device="cuda") * 0.6
    real = torch.rand((H, W, 12), generator=g, device="cuda")
    kw = dict(deg=3, min_valid=0.0, min_count=50)
    pipe = SpectralFusion(w, srf, good, fuse_apply=True, **kw)
    for _ in range(3):                       # the bracketed launch carries K3 of tile 1 and the fit of tile 2
        pipe.submit(cube, real)
    assert pipe._pipe["fused"]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = pipe.submit(cube, real, k1_events=(e0, e1))
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    assert e0.query() and e1.query()
    ms = e0.elapsed_time(e1)
    print(f"bound events: {ms * 1e3:.1f} us, wall-clock bracket {wall_ms * 1e3:.1f} us")
    assert 0.0 < ms <= wall_ms
    got = [_clone(out)] + [_clone(o) for o in pipe.drain()]
    want = _clone(SpectralFusion(w, srf, good, **kw).step(cube, real, reuse_buffers=False))
    for i, gt in enumerate(got):
        _same_bits(torch, gt, want, ("events", i))
    pipe.close()
