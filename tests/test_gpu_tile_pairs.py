"""fuse_tile_pairs on an MI355X: against fixture g12 (the notebook's per-pair flow, scikit-learn float64), and the batch's own
guarantees - batch bits == single-pair bits in any order, the prep's mask and block mean against the host rules and
hsr_block_mean, the cube against PolyRidge.predict_cube of the returned model, float32 inputs, a non-default stream."""
import numpy as np
import pytest

from conftest import load_golden
from gpu_harness import torch_gpu  # noqa: F401
from test_tile_pairs_host import block_mean_rule, decode_u16, g12_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g12():
    g = load_golden("g12_tile_pairs")
    emit, s2 = g12_inputs(g)
    return g, emit, s2


def _bits(t):
    return t.contiguous().view(-1).view(__import__("torch").int32)


def _same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    if a.dtype == __import__("torch").float64:
        return bool((a.contiguous().view(-1).view(__import__("torch").int64) ==
                     b.contiguous().view(-1).view(__import__("torch").int64)).all())
    return bool((_bits(a) == _bits(b)).all())


def test_g12_batch_against_notebook(torch_gpu, g12):
    import s2_emit
    g, emit, s2 = g12
    out = s2_emit.fuse_tile_pairs(emit, s2, bands=32, s2_nodata=0.0)
    torch_gpu.cuda.synchronize()
    assert out.cube.shape == (3, 32, 600, 600) and out.cube.dtype == torch_gpu.float32
    np.testing.assert_array_equal(out.n_train.cpu().numpy(), g["n_train"])
    np.testing.assert_array_equal(out.status.cpu().numpy(), [0, 0, 0])
    for p in range(3):
        np.testing.assert_array_equal(np.packbits(out.mask[p].cpu().numpy().reshape(-1)), g["mask_packed"][p])
        m = out.model(p)
        np.testing.assert_allclose(m.mean_, g["mean"][p], rtol=1e-12)
        np.testing.assert_allclose(m.scale_, g["scale"][p], rtol=1e-12)
        np.testing.assert_allclose(m.intercept_, g["intercept"][p], rtol=1e-6, atol=1e-7)
        pred = out.cube[p].cpu().numpy()
        np.testing.assert_allclose(pred[:, ::23, ::29], g["pred_sample"][p], rtol=0, atol=1e-4, equal_nan=True)
        np.testing.assert_allclose(pred[:, 301, :], g["pred_row_301"][p], rtol=0, atol=1e-4, equal_nan=True)
        fin = np.isfinite(pred)
        assert int((~fin).sum()) == int(g["pred_nan_count"][p]), p
        zs = np.where(fin, pred, 0).astype(np.float64)
        np.testing.assert_allclose(zs.sum(axis=(1, 2)), g["pred_band_sum"][p], rtol=2e-6)
        np.testing.assert_allclose((zs ** 2).sum(axis=(1, 2)), g["pred_band_sumsq"][p], rtol=4e-6)


def test_g12_all_285_bands(torch_gpu, g12):
    import s2_emit
    g, emit, s2 = g12
    out = s2_emit.fuse_tile_pair(emit[0], s2[0], bands="all", s2_nodata=0.0)
    assert out.cube.shape == (1, 285, 600, 600)
    assert int(out.n_train[0]) == int(g["n_train_285"]) and int(out.status[0]) == 0
    m = out.model(0)
    np.testing.assert_allclose(m.intercept_, g["intercept_285"], rtol=1e-6, atol=1e-7)
    Xs = s2[0].reshape(10, -1)[:, g["pix_285"]].T.astype(np.float32)
    np.testing.assert_allclose(m.predict(Xs), g["pred_logit_285"], rtol=0, atol=2e-4)
    cube = out.cube[0].reshape(285, -1)[:, torch_gpu.from_numpy(g["pix_285"]).cuda()].t().cpu().numpy()
    np.testing.assert_allclose(cube, s2_emit.ridge.sigmoid(g["pred_logit_285"].astype(np.float64)), rtol=0, atol=1e-4)


def test_batch_bits_equal_single_pairs_any_order(torch_gpu, g12):
    """Every pair of a batch carries the bits it has alone, in any position; a pair without training pixels gets status 1 and
    an all-NaN cube and leaves the others untouched."""
    import s2_emit
    torch = torch_gpu
    g, emit, s2 = g12
    emit4 = np.concatenate([emit, np.full((1,) + emit.shape[1:], 65535, np.uint16)])      # pair 3: no valid EMIT pixel
    s24 = np.concatenate([s2, s2[:1]])
    E, S = torch.from_numpy(emit4.view(np.int16)).cuda().view(torch.uint16), torch.from_numpy(s24.view(np.int16)).cuda().view(torch.uint16)
    batch = s2_emit.fuse_tile_pairs(E, S, s2_nodata=0.0)
    perm = [3, 2, 0, 1]
    permuted = s2_emit.fuse_tile_pairs([E[i] for i in perm], [S[i] for i in perm], s2_nodata=0.0)
    singles = [s2_emit.fuse_tile_pair(E[i], S[i], s2_nodata=0.0) for i in range(4)]
    torch.cuda.synchronize()
    np.testing.assert_array_equal(batch.status.cpu().numpy(), [0, 0, 0, 1])
    assert int(batch.n_train[3]) == 0 and bool(torch.isnan(batch.cube[3]).all())
    for i in range(4):
        one = singles[i]
        assert _same_bits(batch.cube[i], one.cube[0]), i
        assert _same_bits(permuted.cube[perm.index(i)], one.cube[0]), i
        assert int(one.status[0]) == int(batch.status[i]) and int(one.n_train[0]) == int(batch.n_train[i])
        for k in ("mean", "scale", "b64", "W32", "b32"):
            assert _same_bits(batch._fit[k][i], one._fit[k][0]), (i, k)
            assert _same_bits(permuted._fit[k][perm.index(i)], one._fit[k][0]), (i, k)


def test_prep_mask_block_mean_and_cube_against_references(torch_gpu, g12):
    """The prep's mask is flatten_pixels' on the decoded, block-meaned arrays; its block mean carries hsr_block_mean's bits where
    no sample is bad; the cube is PolyRidge.predict_cube of the returned model, bit for bit."""
    import s2_emit
    from s2_emit import _native as nat
    from s2_emit._engine import _ptr
    torch = torch_gpu
    g, emit, s2 = g12
    out = s2_emit.fuse_tile_pairs(emit, s2, s2_nodata=0.0)
    lib = nat.load()
    for p in range(3):
        X = out.s2_coarse[p].cpu().numpy()
        Y = decode_u16(emit[p])[g["bands"]]
        Xtr, _ = s2_emit.flatten_pixels(X, Y, x_nodata=0.0)
        mask = out.mask[p].cpu().numpy()
        assert mask.sum() == len(Xtr) == int(out.n_train[p])
        np.testing.assert_array_equal(mask, np.isfinite(X).all(0) & np.isfinite(Y).all(0) & ~np.isclose(X, 0.0).any(0))
        Sd = torch.from_numpy(s2[p].view(np.int16)).cuda()
        bm = torch.empty((10, 100 * 100), dtype=torch.float32, device="cuda")
        nat.check(lib.hsr_block_mean(_ptr(Sd), 2, 600 * 600, 1, 10, 100, 100, 6, 1.0, _ptr(bm), 100 * 100, 1, None), "hsr_block_mean")
        ref = bm.cpu().numpy().reshape(10, 100, 100)
        fin = np.isfinite(X)
        assert (~fin).sum() == np.isnan(block_mean_rule(s2[p], nodata=0.0)).sum()
        np.testing.assert_array_equal(X[fin].view(np.int32), ref[fin].view(np.int32))
        S32 = torch.from_numpy(s2[p].astype(np.float32)).cuda()
        direct = out.model(p).predict_cube(S32, nodata=0.0)
        assert _same_bits(out.cube[p], direct), p


def test_float32_inputs_with_nan_and_nodata(torch_gpu, g12):
    """float32 EMIT / S2 with NaNs and float nodata values: the mask follows flatten_pixels (a nodata sample in an unselected
    EMIT band keeps its pixel), the fit matches PolyRidge on the host-flattened pixels, the cube its predict_cube."""
    import s2_emit
    torch = torch_gpu
    g, emit, s2 = g12
    ef = decode_u16(emit[0])
    sf = s2[0].astype(np.float32)
    sel = g["bands"]
    ef[sel[5], 40, 41] = np.nan
    ef[sel[7], 50, 51] = -9999.0
    ef[2, 60, 61] = -9999.0                         # unselected band: pixel stays
    sf[3, 120, 130] = np.nan
    sf[6, 240, 250] = -1.0
    coarse = block_mean_rule(sf, nodata=-1.0)
    out = s2_emit.fuse_tile_pair(ef, sf, emit_nodata=-9999.0, s2_nodata=-1.0)
    X = out.s2_coarse[0].cpu().numpy()
    np.testing.assert_array_equal(np.isnan(X), np.isnan(coarse))
    Y = ef[sel]
    Xtr, Ytr = s2_emit.flatten_pixels(X, Y, x_nodata=-1.0, y_nodata=-9999.0)
    mask = out.mask[0].cpu().numpy()
    assert mask.sum() == len(Xtr) == int(out.n_train[0]) and mask[60, 61] and not mask[50, 51] and not mask[40, 41]
    ref = s2_emit.PolyRidge(3, 1.0).fit(Xtr, s2_emit.ridge.logit(Ytr.astype(np.float64)))
    m = out.model(0)
    np.testing.assert_allclose(m.mean_, ref.mean_, rtol=1e-12)
    np.testing.assert_allclose(m.scale_, ref.scale_, rtol=1e-12)
    np.testing.assert_allclose(m.intercept_, ref.intercept_, rtol=1e-6, atol=1e-7)
    direct = m.predict_cube(torch.from_numpy(sf).cuda(), nodata=-1.0)
    assert _same_bits(out.cube[0], direct)
    assert bool(torch.isnan(out.cube[0, :, 120, 130]).all()) and bool(torch.isnan(out.cube[0, :, 240, 250]).all())
    # the caller's S2 on the EMIT grid instead of the block mean: the same model when it is the block mean itself
    via = s2_emit.fuse_tile_pair(ef, sf, emit_nodata=-9999.0, s2_nodata=-1.0, s2_coarse=coarse)
    assert _same_bits(via.cube[0], out.cube[0]) and int(via.n_train[0]) == int(out.n_train[0])


def test_non_default_stream_same_bits(torch_gpu, g12):
    import s2_emit
    torch = torch_gpu
    g, emit, s2 = g12
    E = torch.from_numpy(emit[:2].view(np.int16)).cuda().view(torch.uint16)
    S = torch.from_numpy(s2[:2].view(np.int16)).cuda().view(torch.uint16)
    ref = s2_emit.fuse_tile_pairs(E, S, s2_nodata=0.0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = s2_emit.fuse_tile_pairs(E, S, s2_nodata=0.0)
    side.synchronize()
    assert _same_bits(got.cube, ref.cube)
    assert _same_bits(got._fit["b64"], ref._fit["b64"])
