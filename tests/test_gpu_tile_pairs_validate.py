"""fuse_tile_pairs(train_mask=..., validate=True) on an MI355X: the score kernel alone on exact data (both instances), both views
against a NumPy restatement from the device's own outputs (T = 32 and all 285 bands), the coarse view against the float64 model,
what the hold-out does to the fit, defaults that change nothing, batch bits == single-pair bits, a non-default stream and float32
inputs.  Bounds: only summation order separates the device from the restatement, so they are derived, not measured (see each
test); the observed maxima are printed (run with -s) and quoted in profiles/r07_tile_pairs_validate.md."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from gpu_harness import torch_gpu  # noqa: F401
from test_tile_pairs_host import block_mean_rule, decode_u16, g12_inputs
from test_tile_pairs_report_host import report_reference
from test_tile_pairs_validate_host import checkerboard_mask, validation_reference

pytestmark = pytest.mark.gpu

FIELDS = ("pred_coarse", "cube_coarse", "n", "rmse", "r2", "mean_ref", "sam", "n_sam", "ergas", "sam_map")
FIT_KEYS = ("mean", "scale", "Bp", "b64", "W32", "b32", "mean32", "inv32")
ANGLE_ATOL = 5e-6          # degrees: a cosine within a few ulp of 1 moves acos by up to sqrt(2 * 4 * 2^-53) rad = 1.7e-6 deg; x 3


@pytest.fixture(scope="module")
def g12():
    g = load_golden("g12_tile_pairs")
    emit, s2 = g12_inputs(g)
    return g, emit, s2


def _same_bits(a, b):
    import torch
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    width = {torch.float64: torch.int64, torch.int64: torch.int64}.get(a.dtype)
    if width is None:
        width = torch.int32 if a.element_size() == 4 else torch.uint8
    return bool((a.contiguous().view(-1).view(width) == b.contiguous().view(-1).view(width)).all())


def _dev_u16(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def _groups(out, i):
    """The group codes of pair i from the output's masks: 1 fit, 2 held out, 0 neither."""
    fit = out.mask[i].cpu().numpy().reshape(-1)
    held = out.held_out[i].cpu().numpy().reshape(-1)
    assert not (fit & held).any()
    return fit.astype(np.uint8) + 2 * held.astype(np.uint8)


def _nan_equal_close(got, ref, tol, what):
    """NaN in the same places; elsewhere |got - ref| <= tol (an array or a scalar).  -> the largest |got - ref| / tol."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=what)
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    diff = np.abs(got - ref)[ok]
    tol = np.broadcast_to(np.asarray(tol, np.float64), ref.shape)[ok]
    assert (diff <= tol).all(), (what, float(diff.max()), float((diff / tol).max()))
    return float(diff.max())


def _rel_max(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ok = np.isfinite(ref) & (ref != 0)
    return float(np.abs(got[ok] / ref[ok] - 1.0).max()) if ok.any() else 0.0


def _check_view(val, i, v, ref, seen):
    """Pair i, view v of a TilePairValidation against validation_reference's dict, with the bounds of a restatement that
    differs in summation order only: rmse, mean_ref, ergas rtol 1e-9 (n <= 1e4 terms x 2^-53, two orders of margin);
    |d r2| <= 1e-9 max(1, ss_res / (M2 + 1e-8)); angles atol 5e-6 deg on sam, 5e-6 deg + one float32 step on sam_map.
    seen collects the observed maxima."""
    c = lambda t: t[i, v].cpu().numpy()
    np.testing.assert_array_equal(c(val.n), ref["n"])
    np.testing.assert_array_equal(c(val.n_sam), ref["n_sam"])
    rel = lambda r: 1e-9 * np.abs(r)
    upd = lambda k, x: seen.__setitem__(k, max(seen.get(k, 0.0), x))
    for k in ("rmse", "mean_ref", "ergas"):
        _nan_equal_close(c(getattr(val, k)), ref[k], rel(ref[k]), k)
        upd(k + "_rel", _rel_max(c(getattr(val, k)), ref[k]))
    r2_tol = 1e-9 * np.maximum(1.0, ref["ss_res"] / (ref["m2"] + 1e-8))
    upd("r2_abs", _nan_equal_close(c(val.r2), ref["r2"], r2_tol, "r2"))
    upd("sam_abs_deg", _nan_equal_close(c(val.sam), ref["sam"], ANGLE_ATOL, "sam"))
    a32 = ref["angle"].astype(np.float32)
    upd("sam_map_abs_deg", _nan_equal_close(val.sam_map[i, v].cpu().numpy().reshape(-1), ref["angle"],
                                            ANGLE_ATOL + np.spacing(np.abs(a32)).astype(np.float64), "sam_map"))


def _score_alone(torch, pred, y, group, factor, misalign=False):
    """hsr_pair_score_f64 on host arrays pred, y (P, T, npix), group (P, npix) -> dict of host arrays.  misalign: the float arrays
    start 4 bytes past a 16-byte boundary, which sends an npix % 4 == 0 problem to the plain instance."""
    from s2_emit import _native as nat
    from s2_emit._engine import _ptr
    lib = nat.load()
    P, T, npix = pred.shape

    def dev(a):
        flat = torch.empty(a.size + 4, dtype=torch.float32, device="cuda")
        t = flat[1:1 + a.size] if misalign else flat[:a.size]
        t.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
        assert (t.data_ptr() % 16 != 0) == misalign
        return t
    pd, yd = dev(pred), dev(y)
    gd = torch.from_numpy(np.ascontiguousarray(group)).cuda()
    sw = lib.hsr_pair_score_work_bytes(npix, T) // 8
    work = torch.empty((P, sw), dtype=torch.float64, device="cuda")
    f64 = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device="cuda")
    i64 = lambda *s: torch.full(s, -7, dtype=torch.int64, device="cuda")
    n, rmse, r2, mean_ref = i64(P, 2, T), f64(P, 2, T), f64(P, 2, T), f64(P, 2, T)
    sam, n_sam, ergas = f64(P, 2), i64(P, 2), f64(P, 2)
    sam_map = torch.full((P, npix), -7.0, dtype=torch.float32, device="cuda")
    lib.hsr_pairs_last_launch(None, 0)
    nat.check(lib.hsr_pair_score_f64(_ptr(pd), T * npix, _ptr(yd), T * npix, _ptr(gd), npix, npix, T, 100.0 / factor, _ptr(work), sw,
                                     _ptr(n), _ptr(rmse), _ptr(r2), _ptr(mean_ref), 2 * T, _ptr(sam), _ptr(n_sam), _ptr(ergas), 2,
                                     _ptr(sam_map), npix, P, None), "hsr_pair_score_f64")
    record = ctypes.create_string_buffer(96)                 # the instance the alignment asks for is the one that ran
    vec = "true" if npix % 4 == 0 and not misalign else "false"
    assert lib.hsr_pairs_last_launch(record, 96) == 1
    assert record.value.decode() == f"pair_score_partial_kernel<{vec}>; pair_score_finish_kernel", record.value
    torch.cuda.synchronize()
    return dict(n=n, rmse=rmse, r2=r2, mean_ref=mean_ref, sam=sam, n_sam=n_sam, ergas=ergas, sam_map=sam_map)


@pytest.mark.parametrize("T", [40, 285])
@pytest.mark.parametrize("npix", [1000 + 37, 2000 + 36])
def test_score_kernel_on_exact_data(torch_gpu, T, npix):
    """hsr_pair_score_f64 alone on small dyadic values (multiples of 1/64 in (0, 1.2): every product and every sum of them exact
    in float64), npix a multiple of neither the 512-pixel chunk nor a lane's 8 pixels (1037: the plain instance; 2036: the
    16-byte instance), T = 40 and 285 (a partial join of 4 bands at 285), groups 0 / 1 / 2 at random, NaNs in single bands of
    pred, one constant band (M2 == 0 exactly).  n, n_sam equal; rmse, mean_ref, ergas rtol 1e-12 (exact sums, one rounding in the
    division and the square root); r2 rtol 1e-12, atol 1e-6 as the report's exact-data test; angles 5e-6 deg."""
    torch = torch_gpu
    rng = np.random.default_rng(7 + T + npix)
    P = 2
    y = (rng.integers(1, 65, (P, T, npix)) / 64.0).astype(np.float32)
    y[:, 3] = np.float32(0.375)                                         # a constant band
    pred = (y + rng.integers(-8, 9, (P, T, npix)) / 64.0).astype(np.float32)
    pred[rng.random((P, T, npix)) < 0.002] = np.nan                    # single bands of single pixels
    pred[1, :, 5] = 0.0                                                 # a zero spectrum: no angle
    group = rng.integers(0, 3, (P, npix)).astype(np.uint8)
    group[0, :600] = 1                                                  # a whole chunk of one group
    got = _score_alone(torch, pred, y, group, 6)
    worst = 0.0
    for p in range(P):
        ref = validation_reference(pred[p], y[p], group[p], 6)
        assert ref["n_sam"].min() > 0 and ref["n"].min() > 0
        c = lambda k: got[k][p].cpu().numpy()
        np.testing.assert_array_equal(c("n"), ref["n"])
        np.testing.assert_array_equal(c("n_sam"), ref["n_sam"])
        np.testing.assert_allclose(c("rmse"), ref["rmse"], rtol=1e-12)
        np.testing.assert_allclose(c("mean_ref"), ref["mean_ref"], rtol=1e-12)
        np.testing.assert_allclose(c("ergas"), ref["ergas"], rtol=1e-12)
        np.testing.assert_allclose(c("r2"), ref["r2"], rtol=1e-12, atol=1e-6)
        assert (ref["m2"][:, 3] == 0).all()
        np.testing.assert_allclose(c("r2")[:, 3], 1.0 - ref["ss_res"][:, 3] / 1e-8, rtol=1e-12)   # M2 == 0 on the device too
        np.testing.assert_allclose(c("sam"), ref["sam"], rtol=0, atol=ANGLE_ATOL)
        a32 = ref["angle"].astype(np.float32)
        worst = max(worst, _nan_equal_close(c("sam_map"), ref["angle"], ANGLE_ATOL + np.spacing(np.abs(a32)).astype(np.float64),
                                            "sam_map"))
        assert np.isnan(c("sam_map")[group[p] == 0]).all() and (p == 0 or np.isnan(c("sam_map")[5]))
    print(f"exact data T={T} npix={npix}: max |sam_map - ref| = {worst:.3e} deg")
    if npix % 4 == 0:                                                   # the plain instance on the same problem: the same bits
        plain = _score_alone(torch, pred, y, group, 6, misalign=True)
        for k in got:
            assert _same_bits(got[k], plain[k]), k


def test_holdout_kernel_codes(torch_gpu):
    """hsr_pair_holdout: mask = valid & train, group = 1 fit / 2 held out / 0; any non-zero byte of train counts as True."""
    from s2_emit import _native as nat
    from s2_emit._engine import _ptr
    torch = torch_gpu
    lib = nat.load()
    rng = np.random.default_rng(3)
    P, npix = 3, 1000 + 37
    valid = (rng.random((P, npix)) < 0.7).astype(np.uint8)
    train = (rng.integers(0, 3, (P, npix)) * 100).astype(np.uint8)      # 0, 100, 200
    vd, td = torch.from_numpy(valid).cuda(), torch.from_numpy(train).cuda()
    mask = torch.full((P, npix), 9, dtype=torch.uint8, device="cuda")
    group = torch.full((P, npix), 9, dtype=torch.uint8, device="cuda")
    nat.check(lib.hsr_pair_holdout(_ptr(vd), _ptr(td), npix, npix, _ptr(mask), _ptr(group), P, None), "hsr_pair_holdout")
    np.testing.assert_array_equal(mask.cpu().numpy(), valid & (train != 0))
    np.testing.assert_array_equal(group.cpu().numpy(), np.where(valid == 0, 0, np.where(train != 0, 1, 2)))


@pytest.mark.parametrize("bands", [32, "all"])
def test_both_views_against_restatement_from_device_outputs(torch_gpu, g12, bands):
    """T = 32 (the three pairs) and T = 285 (pair 0), a checkerboard of 10 x 10 blocks held out: every score of both views against
    validation_reference of the device's own views and masks; cube_coarse bit-equal to the block mean rule of the device cube."""
    import s2_emit
    g, emit, s2 = g12
    pairs = [0, 1, 2] if bands == 32 else [0]
    keep = checkerboard_mask(100, 100)
    out = s2_emit.fuse_tile_pairs(emit[pairs], s2[pairs], bands=bands, s2_nodata=0.0, train_mask=np.stack([keep] * len(pairs)),
                                  validate=True)
    val = out.validation
    T = len(out.bands)
    assert val.views == ("coarse", "degraded") and val.groups == ("fit", "held_out")
    assert val.n.shape == (len(pairs), 2, 2, T) and val.sam_map.shape == (len(pairs), 2, 100, 100)
    assert val.n.dtype == torch_gpu.int64 and val.rmse.dtype == torch_gpu.float64 and val.sam_map.dtype == torch_gpu.float32
    assert (out.status.cpu().numpy() == 0).all()
    seen = {}
    for i, p in enumerate(pairs):
        y = decode_u16(emit[p])[out.bands].reshape(T, -1)
        group = _groups(out, i)
        assert (group == 1).sum() >= 2900 and (group == 2).sum() >= 2900            # no group of a fitted pair is empty
        cube = out.cube[i].cpu().numpy()
        cc = val.cube_coarse[i].cpu().numpy()
        want = block_mean_rule(cube)
        np.testing.assert_array_equal(np.isnan(cc), np.isnan(want))
        np.testing.assert_array_equal(cc.view(np.int32)[~np.isnan(want)], want.view(np.int32)[~np.isnan(want)])
        for v, view in enumerate((val.pred_coarse, val.cube_coarse)):
            ref = validation_reference(view[i].cpu().numpy().reshape(T, -1), y, group, 6)
            assert ref["n"].min() > 0 and ref["n_sam"].min() > 0
            _check_view(val, i, v, ref, seen)
        print(f"pair {p} T={T}: ergas {val.ergas[i].cpu().numpy().round(4).tolist()} sam {val.sam[i].cpu().numpy().round(4).tolist()}")
    print(f"restatement T={T}: observed maxima {({k: float(f'{x:.3e}') for k, x in seen.items()})}")


def test_coarse_view_against_the_float64_model(torch_gpu, g12):
    """An independent path for the coarse view: on the fit group, rmse[:, 0, 0] against report_reference evaluated with the pair's
    float64 model on the same pixels.  |rmse(a) - rmse(b)| <= max |a - b|, and 1e-4 is the bound the g12 tests put on the float32
    predict path against the float64 reference."""
    import s2_emit
    g, emit, s2 = g12
    keep = checkerboard_mask(100, 100)
    out = s2_emit.fuse_tile_pairs(emit, s2, bands=32, s2_nodata=0.0, train_mask=np.stack([keep] * 3), validate=True)
    worst = 0.0
    for i in range(3):
        m = out.model(i)
        mask = out.mask[i].cpu().numpy().reshape(-1)
        X = out.s2_coarse[i].cpu().numpy().reshape(m.n_in, -1).T[mask]
        Y = decode_u16(emit[i])[out.bands].reshape(len(out.bands), -1).T[mask]
        _, rmse = report_reference(X, Y, m.mean_, m.scale_, m.coef_, m.intercept_, out.degree)
        got = out.validation.rmse[i, 0, 0].cpu().numpy()
        worst = max(worst, float(np.abs(got - rmse).max()))
        assert np.abs(got - rmse).max() <= 1e-4, np.abs(got - rmse).max()
        np.testing.assert_array_equal(out.validation.n[i, 0, 0].cpu().numpy(), mask.sum())
    print(f"coarse view vs float64 model: max |rmse - ref| = {worst:.3e}")


def test_holdout_means_what_it_says(torch_gpu, g12):
    """train_mask = m gives the bits of the call without a train_mask on a copy of the EMIT tiles whose held-out pixels are 65535
    in every band; valid / held_out as defined; the two groups' n sum to the valid pixels with a finite prediction."""
    import s2_emit
    torch = torch_gpu
    g, emit, s2 = g12
    keep = np.stack([checkerboard_mask(100, 100), ~checkerboard_mask(100, 100), checkerboard_mask(100, 100, 5)])
    S = _dev_u16(torch, s2)
    got = s2_emit.fuse_tile_pairs(_dev_u16(torch, emit), S, s2_nodata=0.0, train_mask=keep, validate=True, report=True)
    emit_cut = emit.copy()
    emit_cut[np.broadcast_to(~keep[:, None], emit.shape)] = 65535
    ref = s2_emit.fuse_tile_pairs(_dev_u16(torch, emit_cut), S, s2_nodata=0.0, report=True)
    plain = s2_emit.fuse_tile_pairs(_dev_u16(torch, emit), S, s2_nodata=0.0)
    for k in ("cube", "status", "n_train", "mask", "s2_coarse", "r2", "rmse"):
        assert _same_bits(getattr(got, k), getattr(ref, k)), k
    for k in FIT_KEYS:
        assert _same_bits(got._fit[k], ref._fit[k]), k
    kd = torch.from_numpy(keep).cuda()
    assert _same_bits(got.valid, plain.mask) and _same_bits(got.mask, plain.mask & kd) and _same_bits(got.held_out, plain.mask & ~kd)
    assert _same_bits(plain.valid, plain.mask) and not bool(plain.held_out.any()) and plain.validation is None
    np.testing.assert_array_equal(got.n_train.cpu().numpy(), (plain.mask & kd).sum(dim=(1, 2)).cpu().numpy())
    val = got.validation
    valid = got.valid.view(3, 1, -1)
    for v, view in enumerate((val.pred_coarse, val.cube_coarse)):
        finite = (torch.isfinite(view.view(3, 32, -1)) & valid).sum(dim=2)
        assert bool((val.n[:, v].sum(dim=1) == finite).all()), v
        assert bool((val.n[:, v, 0] > 0).all()) and bool((val.n[:, v, 1] > 0).all())


def test_defaults_change_nothing(torch_gpu, g12):
    """validate=True and an all-True train_mask leave every existing output with the bits of the plain call; validate=True does the
    same under a real train_mask."""
    import s2_emit
    torch = torch_gpu
    g, emit, s2 = g12
    E, S = _dev_u16(torch, emit), _dev_u16(torch, s2)
    ones = torch.ones((3, 100, 100), dtype=torch.bool, device="cuda")
    base = s2_emit.fuse_tile_pairs(E, S, s2_nodata=0.0, report=True)
    assert base.validation is None
    others = [s2_emit.fuse_tile_pairs(E, S, s2_nodata=0.0, report=True, validate=True),
              s2_emit.fuse_tile_pairs(E, S, s2_nodata=0.0, report=True, train_mask=ones),
              s2_emit.fuse_tile_pairs(E, S, s2_nodata=0.0, report=True, train_mask=ones.to(torch.uint8), validate=True),
              s2_emit.fuse_tile_pairs(E, S, s2_nodata=0.0, report=True, train_mask=[np.ones((100, 100), bool)] * 3)]

    def same(a, b):
        for k in ("cube", "status", "n_train", "mask", "valid", "held_out", "s2_coarse", "r2", "rmse"):
            assert _same_bits(getattr(a, k), getattr(b, k)), k
        for k in FIT_KEYS:
            assert _same_bits(a._fit[k], b._fit[k]), k
    for o in others:
        same(o, base)
    for k in FIELDS:                                                    # and the mask does not change the scores either
        assert _same_bits(getattr(others[0].validation, k), getattr(others[2].validation, k)), k
    assert not bool(others[0].validation.n[:, :, 1].any()) and bool(torch.isnan(others[0].validation.rmse[:, :, 1]).all())
    keep = torch.from_numpy(np.stack([checkerboard_mask(100, 100)] * 3)).cuda()
    same(s2_emit.fuse_tile_pairs(E, S, s2_nodata=0.0, report=True, train_mask=keep, validate=True),
         s2_emit.fuse_tile_pairs(E, S, s2_nodata=0.0, report=True, train_mask=keep))


def test_batch_bits_equal_single_pairs_any_order(torch_gpu, g12):
    """Every field of the validation carries the same bits for a pair alone and in any position of a batch; a pair without
    training pixels (status 1) has n = 0 and NaN metrics and leaves the others untouched."""
    import s2_emit
    torch = torch_gpu
    g, emit, s2 = g12
    emit4 = np.concatenate([emit, np.full((1,) + emit.shape[1:], 65535, np.uint16)])
    s24 = np.concatenate([s2, s2[:1]])
    E, S = _dev_u16(torch, emit4), _dev_u16(torch, s24)
    K = torch.from_numpy(np.stack([checkerboard_mask(100, 100, b) for b in (10, 5, 20, 10)])).cuda()
    kw = dict(s2_nodata=0.0, validate=True)
    batch = s2_emit.fuse_tile_pairs(E, S, train_mask=K, **kw)
    perm = [3, 2, 0, 1]
    permuted = s2_emit.fuse_tile_pairs([E[i] for i in perm], [S[i] for i in perm], train_mask=[K[i] for i in perm], **kw)
    singles = [s2_emit.fuse_tile_pair(E[i], S[i], train_mask=K[i], **kw) for i in range(4)]
    np.testing.assert_array_equal(batch.status.cpu().numpy(), [0, 0, 0, 1])
    bv = batch.validation
    assert not bool(bv.n[3].any()) and not bool(bv.n_sam[3].any())
    for k in ("rmse", "r2", "mean_ref", "sam", "ergas", "sam_map", "cube_coarse", "pred_coarse"):
        assert bool(torch.isnan(getattr(bv, k)[3]).all()), k
    for k in ("rmse", "r2", "mean_ref", "sam", "ergas"):
        assert bool(torch.isfinite(getattr(bv, k)[:3]).all()), k
    for i in range(4):
        for k in FIELDS:
            one = getattr(singles[i].validation, k)[0]
            assert _same_bits(getattr(bv, k)[i], one), (i, k)
            assert _same_bits(getattr(permuted.validation, k)[perm.index(i)], one), (i, k)


def test_non_default_stream_and_float32_inputs(torch_gpu, g12):
    """The same bits on a side stream; float32 EMIT / S2 with NaN and nodata samples against the restatement."""
    import s2_emit
    torch = torch_gpu
    g, emit, s2 = g12
    E, S = _dev_u16(torch, emit[:2]), _dev_u16(torch, s2[:2])
    K = torch.from_numpy(np.stack([checkerboard_mask(100, 100)] * 2)).cuda()
    ref = s2_emit.fuse_tile_pairs(E, S, s2_nodata=0.0, train_mask=K, validate=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = s2_emit.fuse_tile_pairs(E, S, s2_nodata=0.0, train_mask=K, validate=True)
    side.synchronize()
    for k in FIELDS:
        assert _same_bits(getattr(got.validation, k), getattr(ref.validation, k)), k
    for k in ("mask", "valid", "held_out", "cube"):
        assert _same_bits(getattr(got, k), getattr(ref, k)), k

    ef = decode_u16(emit[0])
    sf = s2[0].astype(np.float32)
    sel = g["bands"]
    ef[sel[5], 40, 41] = np.nan                       # an EMIT NaN: the pixel leaves both groups
    ef[sel[7], 50, 51] = -9999.0
    sf[3, 120, 130] = np.nan                          # an S2 NaN: coarse pixel (20, 21) invalid, the 10 m pixel NaN in the cube
    sf[6, 240, 250] = -1.0
    keep = checkerboard_mask(100, 100)
    out = s2_emit.fuse_tile_pair(ef, sf, emit_nodata=-9999.0, s2_nodata=-1.0, train_mask=keep, validate=True)
    assert int(out.status[0]) == 0
    valid = out.valid[0].cpu().numpy()
    assert not valid[40, 41] and not valid[50, 51] and not valid[20, 21]
    val = out.validation
    assert bool(torch.isnan(val.cube_coarse[0, :, 20, 21]).all()) and bool(torch.isnan(val.pred_coarse[0, :, 20, 21]).all())
    assert bool(torch.isnan(val.sam_map[0, :, 40, 41]).all())
    y = ef[out.bands].reshape(32, -1)
    group = _groups(out, 0)
    seen = {}
    for v, view in enumerate((val.pred_coarse, val.cube_coarse)):
        _check_view(val, 0, v, validation_reference(view[0].cpu().numpy().reshape(32, -1), y, group, 6), seen)
    print(f"float32 inputs: observed maxima {({k: float(f'{x:.3e}') for k, x in seen.items()})}")
