"""fuse_tile_pairs(pool=...) on an MI355X: fixture g14 (the pooled scikit-learn pipeline on g12's pairs), the single-model path
(PolyRidge on the host-concatenated training pixels), the bit invariants of the pooling kernels' merge rules on a small batch,
hsr_pool_stats and hsr_pool_gram alone through ctypes, and TilePairOutput.predict."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from gpu_harness import torch_gpu  # noqa: F401
from test_gpu_tile_pairs_report import _check_close
from test_gpu_tile_pairs_validate import _check_view, _dev_u16, _groups, _same_bits
from test_tile_pairs_host import decode_u16, g12_inputs
from test_tile_pairs_pool_host import POOLINGS
from test_tile_pairs_report_host import report_reference
from test_tile_pairs_validate_host import validation_reference

pytestmark = pytest.mark.gpu

FIT_KEYS = ("mean", "scale", "Bp", "b64", "W32", "b32", "mean32", "inv32")


@pytest.fixture(scope="module")
def g12():
    g = load_golden("g12_tile_pairs")
    emit, s2 = g12_inputs(g)
    return g, emit, s2


def _held_mask(held, P=3, h=100, w=100):
    m = np.ones((P, h, w), bool)
    for p in held:
        m[p] = False
    return m


# ---- 1. g12's pairs against fixture g14, both poolings ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(POOLINGS))
def test_g12_pooled_against_g14(torch_gpu, g12, name):
    """The tolerances of test_g12_batch_against_notebook.  In pooling "010" pair 2 supplies no training pixel: n_train 0, status 0,
    a finite cube from group 0's model, and with validate=True a held_out group scored as validation_reference scores the device's
    own views (the tolerances of test_gpu_tile_pairs_validate)."""
    import s2_emit
    torch = torch_gpu
    g, emit, s2 = g12
    g14 = load_golden("g14_tile_pairs_pool")
    ids, held = POOLINGS[name]
    kw = dict(train_mask=_held_mask(held), validate=True) if held else {}
    out = s2_emit.fuse_tile_pairs(emit, s2, bands=32, s2_nodata=0.0, pool="all" if name == "all" else ids, **kw)
    torch.cuda.synchronize()
    M = max(ids) + 1
    assert out.cube.shape == (3, 32, 600, 600) and out.cube.dtype == torch.float32
    np.testing.assert_array_equal(out.pool, ids)
    assert out.pool.dtype == np.int32 and out.n_pool.dtype == torch.int64 and out.pool_status.dtype == torch.int32
    np.testing.assert_array_equal(out.n_pool.cpu().numpy(), g14[f"n_pool_{name}"])
    np.testing.assert_array_equal(out.pool_status.cpu().numpy(), [0] * M)
    np.testing.assert_array_equal(out.status.cpu().numpy(), [0, 0, 0])
    np.testing.assert_array_equal(out.n_train.cpu().numpy(), [0 if p in held else int(g["n_train"][p]) for p in range(3)])
    for grp in range(M):
        m = out.pool_model(grp)
        np.testing.assert_allclose(m.mean_, g14[f"mean_{name}"][grp], rtol=1e-12)
        np.testing.assert_allclose(m.scale_, g14[f"scale_{name}"][grp], rtol=1e-12)
        np.testing.assert_allclose(m.intercept_, g14[f"intercept_{name}"][grp], rtol=1e-6, atol=1e-7)
    for p in range(3):
        np.testing.assert_array_equal(out.model(p).intercept_, out.pool_model(ids[p]).intercept_)
        np.testing.assert_array_equal(out.model(p).mean_, out.pool_model(ids[p]).mean_)
        pred = out.cube[p].cpu().numpy()
        np.testing.assert_allclose(pred[:, ::23, ::29], g14[f"pred_sample_{name}"][p], rtol=0, atol=1e-4, equal_nan=True)
        np.testing.assert_allclose(pred[:, 301, :], g14[f"pred_row_301_{name}"][p], rtol=0, atol=1e-4, equal_nan=True)
        fin = np.isfinite(pred)
        assert int((~fin).sum()) == int(g14[f"pred_nan_count_{name}"][p]), p
        zs = np.where(fin, pred, 0).astype(np.float64)
        np.testing.assert_allclose(zs.sum(axis=(1, 2)), g14[f"pred_band_sum_{name}"][p], rtol=2e-6)
        np.testing.assert_allclose((zs ** 2).sum(axis=(1, 2)), g14[f"pred_band_sumsq_{name}"][p], rtol=4e-6)
    for p in held:                                     # a wholly held-out pair
        assert int(out.n_train[p]) == 0 and int(out.status[p]) == 0 and not bool(out.mask[p].any())
        assert int(g14[f"pred_nan_count_{name}"][p]) == 0 and bool(torch.isfinite(out.cube[p]).all())
        val = out.validation
        assert int(val.n[p, :, 0].max()) == 0 and int(val.n[p, :, 1].min()) > 0
        y = decode_u16(emit[p])[out.bands].reshape(32, -1)
        group = _groups(out, p)
        assert (group == 2).sum() == g["n_train"][p] and (group == 1).sum() == 0
        seen = {}
        for v, view in enumerate((val.pred_coarse, val.cube_coarse)):
            ref = validation_reference(view[p].cpu().numpy().reshape(32, -1), y, group, 6)
            assert ref["n"][1].min() > 0 and ref["n_sam"][1] > 0
            _check_view(val, p, v, ref, seen)
        print(f"{name} pair {p} held out: rmse {val.rmse[p, 0, 1].cpu().numpy().round(5).tolist()[:4]} .. observed {seen}")


# ---- 2. against the single-model path ---------------------------------------------------------------------------------------------
def test_pool_all_against_polyridge_on_concatenated_pixels(torch_gpu, g12):
    """pool="all": the model is PolyRidge(3, 1.0).fit on the host-concatenated training pixels (the tolerances of
    test_float32_inputs_with_nan_and_nodata) and every cube is predict_cube of that model, bit for bit."""
    import s2_emit
    torch = torch_gpu
    g, emit, s2 = g12
    out = s2_emit.fuse_tile_pairs(emit, s2, s2_nodata=0.0, pool="all")
    Xs, Ys = [], []
    for p in range(3):
        X = out.s2_coarse[p].cpu().numpy()
        Xtr, Ytr = s2_emit.flatten_pixels(X, decode_u16(emit[p])[g["bands"]], x_nodata=0.0)
        assert len(Xtr) == int(out.n_train[p])
        Xs.append(Xtr)
        Ys.append(Ytr)
    Xc, Yc = np.concatenate(Xs), np.concatenate(Ys)
    assert int(out.n_pool[0]) == len(Xc)
    ref = s2_emit.PolyRidge(3, 1.0).fit(Xc, s2_emit.ridge.logit(Yc.astype(np.float64)))
    m = out.pool_model(0)
    np.testing.assert_allclose(m.mean_, ref.mean_, rtol=1e-12)
    np.testing.assert_allclose(m.scale_, ref.scale_, rtol=1e-12)
    np.testing.assert_allclose(m.intercept_, ref.intercept_, rtol=1e-6, atol=1e-7)
    for p in range(3):
        direct = m.predict_cube(torch.from_numpy(s2[p].astype(np.float32)).cuda(), nodata=0.0)
        assert _same_bits(out.cube[p], direct), p
        assert _same_bits(out.model(p).predict_cube(torch.from_numpy(s2[p].astype(np.float32)).cuda(), nodata=0.0), direct), p


# ---- 3. bit invariants on a small batch ---------------------------------------------------------------------------------------------
SMALL = dict(bands=5, degree=2, factor=2)


@pytest.fixture(scope="module")
def small(torch_gpu):
    """5 pairs of 9 x 11 EMIT pixels (20 bands, float32 reflectance), factor 2, 4 S2 bands (float32) correlated with the targets;
    a NaN in a selected band of pair 1 and in S2 of pair 3."""
    rng = np.random.default_rng(14)
    P, B, h, w, f, nb = 5, 20, 9, 11, 2, 4
    ab = rng.random((P, 3, h, w))
    spectra = 0.1 + 0.7 * rng.random((3, B))
    resp = 500 + 2000 * rng.random((3, nb))
    emit = (np.einsum("pkij,kb->pbij", ab, spectra) / 3 + 0.01 * rng.random((P, B, h, w))).astype(np.float32)
    coarse = np.einsum("pkij,kc->pcij", ab, resp)
    s2 = (np.repeat(np.repeat(coarse, f, axis=2), f, axis=3) + 20 * rng.random((P, nb, h * f, w * f))).astype(np.float32)
    emit[1, 0, 2, 3] = np.nan                          # band 0 is selected by bands=5
    s2[3, 1, 5, 6] = np.nan
    return emit, s2


def _assert_pair_bits(a, i, b, j, what):
    assert _same_bits(a.cube[i], b.cube[j]), (what, "cube")
    for k in FIT_KEYS:
        x, y = (a._fit[k][i], b._fit[k][j]) if k != "Bp" else (a._fit[k][i, :a._fit["nf"]], b._fit[k][j, :b._fit["nf"]])
        assert _same_bits(x, y), (what, k)
    assert int(a.status[i]) == int(b.status[j]) and int(a.n_train[i]) == int(b.n_train[j]), what


def test_singleton_groups_carry_the_bits_of_no_pooling(torch_gpu, small):
    import s2_emit
    emit, s2 = small
    ref = s2_emit.fuse_tile_pairs(emit, s2, report=True, **SMALL)
    assert (ref.status.cpu().numpy() == 0).all() and int(ref.n_train[1]) == 98 and ref._fit["nf"] == 14
    for ids in (list(range(5)), [3, 0, 4, 1, 2]):
        out = s2_emit.fuse_tile_pairs(emit, s2, pool=ids, report=True, **SMALL)
        for i in range(5):
            _assert_pair_bits(out, i, ref, i, (ids, i))
            for k in FIT_KEYS:                          # the group arrays are the pair's own
                x, y = out._pool_fit[k][ids[i]], ref._fit[k][i]
                assert _same_bits(x[:14] if k == "Bp" else x, y[:14] if k == "Bp" else y), (ids, i, k)
        assert _same_bits(out.status, ref.status) and _same_bits(out.n_train, ref.n_train)
        assert _same_bits(out.r2, ref.r2) and _same_bits(out.rmse, ref.rmse)
        np.testing.assert_array_equal(out.n_pool.cpu().numpy()[ids], ref.n_train.cpu().numpy())
    one = s2_emit.fuse_tile_pair(emit[2], s2[2], **SMALL)
    for pool in ("all", [0]):
        _assert_pair_bits(s2_emit.fuse_tile_pair(emit[2], s2[2], pool=pool, **SMALL), 0, one, 0, pool)
        _assert_pair_bits(s2_emit.fuse_tile_pairs(emit[2:3], s2[2:3], pool=pool, **SMALL), 0, one, 0, pool)


def test_groups_do_not_depend_on_the_other_groups_of_the_batch(torch_gpu, small):
    """[a, b, c, d] with pool=[0, 1, 0, 1]: group 0 carries the bits of fuse_tile_pairs([a, c], pool="all"), group 1 those of
    [b, d]."""
    import s2_emit
    emit, s2 = small
    out = s2_emit.fuse_tile_pairs(emit[:4], s2[:4], pool=[0, 1, 0, 1], **SMALL)
    for grp, members in enumerate(([0, 2], [1, 3])):
        alone = s2_emit.fuse_tile_pairs(emit[members], s2[members], pool="all", **SMALL)
        for j, i in enumerate(members):
            _assert_pair_bits(out, i, alone, j, (grp, i))
        assert int(out.n_pool[grp]) == int(alone.n_pool[0]) == int(alone.n_train.sum())
        # the model is not a member's own: pooling did something
        assert not _same_bits(out._fit["b64"][members[0]], s2_emit.fuse_tile_pair(emit[members[0]], s2[members[0]], **SMALL)._fit["b64"][0])


def test_member_without_training_pixels_leaves_its_group_unchanged(torch_gpu, small):
    import s2_emit
    torch = torch_gpu
    emit, s2 = small
    base = s2_emit.fuse_tile_pairs(emit[[0, 2]], s2[[0, 2]], pool="all", **SMALL)
    for pos in (0, 1, 2):                               # the empty member first, in the middle, last
        idx = [0, 2]
        idx.insert(pos, 4)
        tm = np.ones((3, 9, 11), bool)
        tm[pos] = False
        out = s2_emit.fuse_tile_pairs(emit[idx], s2[idx], pool="all", train_mask=tm, **SMALL)
        assert int(out.n_train[pos]) == 0 and int(out.status[pos]) == 0 and bool(torch.isfinite(out.cube[pos]).all())
        for k in FIT_KEYS:
            x, y = out._pool_fit[k][0], base._pool_fit[k][0]
            assert _same_bits(x[:14] if k == "Bp" else x, y[:14] if k == "Bp" else y), (pos, k)
        assert _same_bits(out.n_pool, base.n_pool)
        others = [i for i in range(3) if i != pos]
        for j, i in enumerate(others):
            _assert_pair_bits(out, i, base, j, (pos, i))
        direct = out.pool_model(0).predict_cube(torch.from_numpy(s2[4]).cuda())
        assert _same_bits(out.cube[pos], direct)


def test_group_without_training_pixels_and_the_report(torch_gpu, small):
    """pool=[0, 1, 0, 1, 2]: group 1's members both lack training pixels (status 1, NaN cubes, NaN report), pair 4 of group 2 is
    alone, pair 2 of group 0 supplies no pixel (status 0, finite cube, NaN report).  The report of a pair scores its own training
    pixels with its group's model (report_reference, the tolerances of test_gpu_tile_pairs_report)."""
    import s2_emit
    torch = torch_gpu
    emit, s2 = small
    ids = [0, 1, 0, 1, 2]
    tm = np.ones((5, 9, 11), bool)
    tm[[1, 3, 2]] = False
    tm[0, ::2] = False                                  # pair 0 trains on its odd rows
    out = s2_emit.fuse_tile_pairs(emit, s2, pool=ids, train_mask=tm, report=True, **SMALL)
    np.testing.assert_array_equal(out.pool_status.cpu().numpy(), [0, 1, 0])
    np.testing.assert_array_equal(out.status.cpu().numpy(), [0, 1, 0, 1, 0])
    np.testing.assert_array_equal(out.n_pool.cpu().numpy(), [4 * 11, 0, 99])
    np.testing.assert_array_equal(out.n_train.cpu().numpy(), [4 * 11, 0, 0, 0, 99])
    for p in (1, 3):
        assert bool(torch.isnan(out.cube[p]).all()) and bool(torch.isnan(out.r2[p]).all()) and bool(torch.isnan(out.rmse[p]).all())
        assert bool(torch.isnan(out._fit["b64"][p]).all())
    assert bool(torch.isfinite(out.cube[2]).all()) and bool(torch.isnan(out.r2[2]).all()) and bool(torch.isnan(out.rmse[2]).all())
    # the other groups are untouched by the empty one
    g0 = s2_emit.fuse_tile_pairs(emit[[0, 2]], s2[[0, 2]], pool="all", train_mask=tm[[0, 2]], report=True, **SMALL)
    g2 = s2_emit.fuse_tile_pair(emit[4], s2[4], report=True, **SMALL)
    _assert_pair_bits(out, 0, g0, 0, "group 0, pair 0")
    _assert_pair_bits(out, 2, g0, 1, "group 0, pair 2")
    _assert_pair_bits(out, 4, g2, 0, "group 2")
    assert _same_bits(out.r2[0], g0.r2[0]) and _same_bits(out.rmse[4], g2.rmse[0])
    # a pooled group of two trained pairs: each pair's report against the restatement with the GROUP's model
    both = s2_emit.fuse_tile_pairs(emit[[0, 4]], s2[[0, 4]], pool="all", train_mask=tm[[0, 4]], report=True, **SMALL)
    m = both.pool_model(0)
    for i, p in enumerate((0, 4)):
        mask = both.mask[i].cpu().numpy().reshape(-1)
        X = both.s2_coarse[i].cpu().numpy().reshape(4, -1).T[mask]
        Y = emit[p][both.bands].reshape(5, -1).T[mask]
        r2, rmse = report_reference(X, Y, m.mean_, m.scale_, m.coef_, m.intercept_, 2)
        _check_close(both.r2[i].cpu().numpy(), both.rmse[i].cpu().numpy(), r2, rmse)
    assert not _same_bits(both.r2[0], out.r2[0])        # another model than group 0's above


# ---- 4. hsr_pool_stats alone ------------------------------------------------------------------------------------------------------
def _layout_dev(torch, ids):
    from s2_emit.pairs import pool_layout
    order, start = pool_layout(np.asarray(ids, np.int32))
    return torch.from_numpy(order).cuda(), torch.from_numpy(start).cuda(), order, start


@pytest.mark.parametrize("nb", [1, 16])
def test_pool_stats_kernel(torch_gpu, nb):
    """P = 7, M = 3, unordered ids, member 3 with n = 0, pair 2 a singleton group: against the two-pass float64 statistics of the
    concatenation at rtol 1e-12 (a Chan merge of 3 members holds a few ulp); the singleton's mean and scale carry hsr_pair_stats'
    bits."""
    torch = torch_gpu
    from s2_emit import _native as nat
    from s2_emit._engine import _ptr
    lib = nat.load()
    ids = [2, 0, 1, 0, 2, 2, 0]
    P, M, npix = 7, 3, 1500
    rng = np.random.default_rng(nb)
    x = (1000 + 300 * rng.standard_normal((P, nb, npix)) + 50 * np.arange(P)[:, None, None]).astype(np.float32)
    mask = rng.random((P, npix)) < 0.7
    mask[3] = False
    xd, md = torch.from_numpy(x).cuda(), torch.from_numpy(mask.astype(np.uint8)).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")
    stats, mean, scale = torch.empty((P, 1 + 2 * nb), **f64), torch.empty((P, nb), **f64), torch.empty((P, nb), **f64)
    n_train = torch.empty(P, dtype=torch.int64, device="cuda")
    nat.check(lib.hsr_pair_stats(_ptr(xd), _ptr(md), npix, nb, _ptr(stats), _ptr(mean), _ptr(scale), _ptr(n_train), P, None))
    order, start, _, _ = _layout_dev(torch, ids)
    gstats, gmean, gscale = torch.empty((M, 1 + 2 * nb), **f64), torch.empty((M, nb), **f64), torch.empty((M, nb), **f64)
    pmean, pscale = torch.full((P, nb), -7.0, **f64), torch.full((P, nb), -7.0, **f64)
    n_pool = torch.empty(M, dtype=torch.int64, device="cuda")
    nat.check(lib.hsr_pool_stats(_ptr(stats), nb, P, _ptr(order), _ptr(start), M, _ptr(gstats), _ptr(n_pool), _ptr(gmean),
                                 _ptr(gscale), _ptr(pmean), _ptr(pscale), None), "hsr_pool_stats")
    torch.cuda.synchronize()
    for g in range(M):
        members = [p for p in range(P) if ids[p] == g]
        cat = np.concatenate([x[p][:, mask[p]] for p in members], axis=1).astype(np.float64)     # (nb, n)
        n = cat.shape[1]
        mu = cat.mean(axis=1)
        m2 = ((cat - mu[:, None]) ** 2).sum(axis=1)
        assert int(n_pool[g]) == n and float(gstats[g, 0]) == n
        np.testing.assert_allclose(gstats[g, 1:1 + nb].cpu().numpy(), mu, rtol=1e-12)
        np.testing.assert_allclose(gstats[g, 1 + nb:].cpu().numpy(), m2, rtol=1e-12)
        np.testing.assert_allclose(gmean[g].cpu().numpy(), mu, rtol=1e-12)
        np.testing.assert_allclose(gscale[g].cpu().numpy(), np.sqrt(m2 / n), rtol=1e-12)
        for p in members:                               # every member's row, the empty member's too
            assert _same_bits(pmean[p], gmean[g]) and _same_bits(pscale[p], gscale[g]), (g, p)
    assert _same_bits(gmean[1], mean[2]) and _same_bits(gscale[1], scale[2]) and _same_bits(gstats[1], stats[2])   # the singleton
    # a group of empty members only: mean 0, scale 1, n 0
    stats0 = stats.clone()
    stats0[[0, 4, 5]] = 0.0
    nat.check(lib.hsr_pool_stats(_ptr(stats0), nb, P, _ptr(order), _ptr(start), M, _ptr(gstats), _ptr(n_pool), _ptr(gmean),
                                 _ptr(gscale), _ptr(pmean), _ptr(pscale), None), "hsr_pool_stats")
    assert int(n_pool[2]) == 0 and bool((gmean[2] == 0).all()) and bool((gscale[2] == 1).all()) and bool((gstats[2] == 0).all())
    assert bool((pmean[[0, 4, 5]] == 0).all()) and bool((pscale[[0, 4, 5]] == 1).all())
    assert _same_bits(gmean[1], mean[2])


# ---- 5. hsr_pool_gram alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("n_elems", [1, 255, 256, 257, 1037, 1038])
def test_pool_gram_kernel_is_exact_on_integers(torch_gpu, n_elems, misalign):
    """Small integers stored as doubles: every sum is exact, so the result equals NumPy's.  Padded strides; an even n_elems with
    aligned bases takes the 16-byte instance, an odd one or a base moved by 8 bytes the plain one.  P = 7, M = 3, unordered ids,
    an empty member whose values must not be added, a singleton group that carries its input bits (-0.0 included)."""
    torch = torch_gpu
    from s2_emit import _native as nat
    from s2_emit._engine import _ptr
    lib = nat.load()
    ids = [2, 0, 1, 0, 2, 2, 0]
    P, M = 7, 3
    pair_g, group_out = n_elems + 6, n_elems + 4
    rng = np.random.default_rng(n_elems)
    src = rng.integers(-1000, 1000, (P, pair_g)).astype(np.float64)
    src[2, 0] = -0.0                                    # the singleton (group 1) keeps the sign of a zero: copied, not added to 0
    cnt = np.array([[5.0, 9.0], [1.0, 9.0], [2.0, 9.0], [0.0, 9.0], [3.0, 9.0], [4.0, 9.0], [6.0, 9.0]])      # pair 3 is empty
    off = 1 if misalign else 0
    buf = torch.zeros(P * pair_g + 2, dtype=torch.float64, device="cuda")
    gd = buf[off:off + P * pair_g]
    gd.copy_(torch.from_numpy(src.reshape(-1)))
    obuf = torch.full((M * group_out + 2,), 7.5, dtype=torch.float64, device="cuda")
    od = obuf[off:off + M * group_out]
    assert (gd.data_ptr() % 16 == 8) == misalign
    order, start, _, _ = _layout_dev(torch, ids)
    cd = torch.from_numpy(cnt).cuda()
    lib.hsr_pairs_last_launch(None, 0)
    nat.check(lib.hsr_pool_gram(_ptr(gd), pair_g, n_elems, _ptr(cd), 2, P, _ptr(order), _ptr(start), M, _ptr(od), group_out, None),
              "hsr_pool_gram")
    record = ctypes.create_string_buffer(64)                 # the instance the sizes and the alignment ask for is the one that ran
    vec = "true" if n_elems % 2 == 0 and not misalign else "false"
    assert lib.hsr_pairs_last_launch(record, 64) == 1 and record.value.decode() == f"pool_gram_kernel<{vec}>", record.value
    torch.cuda.synchronize()
    got = od.cpu().numpy().reshape(M, group_out)
    for g in range(M):
        members = [p for p in range(P) if ids[p] == g and cnt[p, 0] != 0]
        want = src[members, :n_elems].sum(axis=0)
        np.testing.assert_array_equal(got[g, :n_elems], want)
        np.testing.assert_array_equal(got[g, n_elems:], 7.5)          # the padding is not written
    np.testing.assert_array_equal(got[1, :n_elems].view(np.int64), src[2, :n_elems].view(np.int64))
    assert obuf[0 if misalign else -1].item() == 7.5 and obuf[-1].item() == 7.5
    # a group whose members are all empty: zeros
    cd[[0, 4, 5], 0] = 0.0
    nat.check(lib.hsr_pool_gram(_ptr(gd), pair_g, n_elems, _ptr(cd), 2, P, _ptr(order), _ptr(start), M, _ptr(od), group_out, None),
              "hsr_pool_gram")
    assert bool((od.view(M, group_out)[2, :n_elems] == 0).all())


# ---- 6. predict ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_predict_on_tiles_without_a_partner(torch_gpu, small, dtype):
    """Q = 5 tiles of another height and width, a model_index that repeats and reorders: the bits of model(i).predict_cube, for
    uint16 and float32 tiles, with a nodata value, on a non-default stream; one pair or one group needs no model_index."""
    import s2_emit
    torch = torch_gpu
    emit, s2 = small
    out = s2_emit.fuse_tile_pairs(emit[:4], s2[:4], pool=[0, 1, 0, 1], **SMALL)
    rng = np.random.default_rng(6)
    Q, H, W = 5, 13, 21
    tiles = (500 + 2500 * rng.random((Q, 4, H, W)))
    tiles = np.round(tiles).astype(np.uint16) if dtype == "uint16" else tiles.astype(np.float32)
    tiles[1, 2, 3, 4] = 0
    if dtype == "float32":
        tiles[2, 0, 5, 5] = np.nan
    index = [3, 0, 3, 2, 1]
    as_f32 = lambda t: torch.from_numpy(t.astype(np.float32)).cuda()
    want = [out.model(i).predict_cube(as_f32(tiles[q]), nodata=0.0) for q, i in enumerate(index)]
    dev_tiles = _dev_u16(torch, tiles) if dtype == "uint16" else torch.from_numpy(tiles).cuda()
    for given in (tiles, dev_tiles, [t for t in tiles]):
        got = out.predict(given, index, s2_nodata=0.0)
        assert got.shape == (Q, 5, H, W) and got.dtype == torch.float32
        for q in range(Q):
            assert _same_bits(got[q], want[q]), q
    assert bool(torch.isnan(got[1, :, 3, 4]).all()) and int(torch.isnan(got[0]).sum()) == 0
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = out.predict(dev_tiles, np.array(index), s2_nodata=0.0)
    side.synchronize()
    assert _same_bits(on_side, got)
    with pytest.raises(ValueError, match="model_index is required"):
        out.predict(tiles)
    one_group = s2_emit.fuse_tile_pairs(emit[:2], s2[:2], pool="all", **SMALL)
    one_pair = s2_emit.fuse_tile_pair(emit[0], s2[0], **SMALL)
    for o in (one_group, one_pair):
        got = o.predict(dev_tiles)
        for q in range(Q):
            assert _same_bits(got[q], o.model(0).predict_cube(as_f32(tiles[q]))), q
