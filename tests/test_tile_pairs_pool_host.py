"""fuse_tile_pairs(pool=...) on the host side: fixture g14 (the pooled scikit-learn pipeline on g12's pairs), a float64 NumPy
restatement of the pooled fit that the GPU tests reuse, the argument checks that need no GPU, the membership arrays the pooling
kernels walk, and the declaration and registration of the new exports."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from oracle import oracle_np as onp
from test_tile_pairs_host import block_mean_rule, decode_u16, g12_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("hsr_pool_stats", "hsr_pool_gram", "hsr_pool_models")
POOLINGS = {"all": ([0, 0, 0], ()), "010": ([0, 1, 0], (2,))}      # g14: name -> (group ids, pairs with an all-False train_mask)


def pool_reference(xs, ys, masks, ids, degree=3, alpha=1.0, eps=1e-4):
    """The pooled fit restated in float64: xs[p] (nb, npix) float32 S2 on the EMIT grid, ys[p] (T, npix) float32 decoded targets,
    masks[p] (npix,) bool = the pixels pair p gives to its group's fit (valid & train_mask), ids[p] its group.  Group g is
    oracle_np.ridge_poly_fit on the concatenation, in pair order, of its members' masked pixels against logit(clip(y)).
    -> a list over the groups of dict(mean, scale, coef, intercept, degree, n_pool), None for a group without a training pixel."""
    ids = np.asarray(ids)
    out = []
    for g in range(int(ids.max()) + 1):
        members = np.flatnonzero(ids == g)
        X = np.concatenate([np.asarray(xs[p], np.float64)[:, masks[p]].T for p in members])
        Y = np.concatenate([np.asarray(ys[p], np.float64)[:, masks[p]].T for p in members])
        if len(X) == 0:
            out.append(None)
            continue
        m = onp.ridge_poly_fit(X, onp.logit(Y, eps=eps), degree=degree, alpha=alpha)
        m["n_pool"] = len(X)
        out.append(m)
    return out


def g12_pairs(g):
    """(emit, s2, xs, ys, valid) of g12: the inputs, S2 on the EMIT grid, the decoded selected targets and flatten_pixels' mask."""
    emit, s2 = g12_inputs(g)
    xs = [block_mean_rule(s2[p], nodata=0.0).reshape(10, -1) for p in range(3)]
    ys = [decode_u16(emit[p])[g["bands"]].reshape(len(g["bands"]), -1) for p in range(3)]
    valid = [np.isfinite(xs[p]).all(0) & np.isfinite(ys[p]).all(0) & ~np.isclose(xs[p], 0.0).any(0) for p in range(3)]
    return emit, s2, xs, ys, valid


@pytest.fixture(scope="module")
def g14_case():
    g12, g14 = load_golden("g12_tile_pairs"), load_golden("g14_tile_pairs_pool")
    return (g12, g14) + g12_pairs(g12)


def test_g14_within_the_size_limit_and_consistent_with_g12(g14_case):
    g12, g14 = g14_case[:2]
    assert os.path.getsize(os.path.join(GOLDEN, "g14_tile_pairs_pool.npz")) <= 1 << 20
    for name, (ids, held) in POOLINGS.items():
        np.testing.assert_array_equal(g14[f"pool_{name}"], ids)
        np.testing.assert_array_equal(g14[f"held_{name}"], list(held))
        M = max(ids) + 1
        want = [sum(int(g12["n_train"][p]) for p in range(3) if ids[p] == grp and p not in held) for grp in range(M)]
        np.testing.assert_array_equal(g14[f"n_pool_{name}"], want)
        assert g14[f"mean_{name}"].shape == (M, 10) and g14[f"intercept_{name}"].shape == (M, 32)
        assert g14[f"pred_sample_{name}"].shape == g12["pred_sample"].shape
        assert g14[f"pred_row_301_{name}"].shape == g12["pred_row_301"].shape
        np.testing.assert_array_equal(g14[f"pred_nan_count_{name}"], g12["pred_nan_count"])     # a rule of the inputs alone
    # pooling [0, 1, 0] with pair 2 held out: group 0 is pair 0's own model, group 1 pair 1's (g12 fits them from the same rows)
    np.testing.assert_allclose(g14["intercept_010"], g12["intercept"][:2], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(g14["pred_sample_010"][:2], g12["pred_sample"][:2], rtol=0, atol=1e-6, equal_nan=True)
    # the pooled model is not a pair's model: a test at 1e-4 tells them apart (ten times the tolerance on the stored sample)
    assert np.nanmax(np.abs(g14["pred_sample_all"][1] - g12["pred_sample"][1])) > 1e-3
    assert np.nanmax(np.abs(g14["pred_sample_010"][2] - g12["pred_sample"][2])) > 1e-3


def test_pool_reference_against_g14(g14_case):
    """The float64 restatement (oracle_np.ridge_poly_fit on the concatenated training pixels) against the pooled scikit-learn
    pipeline of g14: 1e-8 on the logits (the two float64 references differ by about 1e-9 here)."""
    g12, g14, emit, s2, xs, ys, valid = g14_case
    pix = g14["pix"]
    for name, (ids, held) in POOLINGS.items():
        masks = [valid[p] & (p not in held) for p in range(3)]
        ref = pool_reference(xs, ys, masks, ids)
        for grp, m in enumerate(ref):
            assert m["n_pool"] == g14[f"n_pool_{name}"][grp]
            np.testing.assert_allclose(m["mean"], g14[f"mean_{name}"][grp], rtol=1e-12)
            np.testing.assert_allclose(m["scale"], g14[f"scale_{name}"][grp], rtol=1e-12)
            np.testing.assert_allclose(m["intercept"], g14[f"intercept_{name}"][grp], rtol=1e-9, atol=1e-10)
        for p in range(3):
            Xs = s2[p].reshape(10, -1)[:, pix].T.astype(np.float64)
            ok = ~np.isclose(Xs, 0.0).any(1)
            want = g14[f"pred_logit_{name}"][p]
            np.testing.assert_array_equal(np.isnan(want).any(1), ~ok)
            got = onp.ridge_poly_predict(ref[ids[p]], Xs[ok])
            err = float(np.max(np.abs(got - want[ok])))
            print(f"{name} pair {p}: max |logit difference| {err:.2e}")
            assert err <= 1e-8, (name, p, err)


def test_pool_reference_empty_group_and_pair_order():
    rng = np.random.default_rng(3)
    xs = [rng.random((2, 30)).astype(np.float32) for _ in range(3)]
    ys = [(0.1 + 0.8 * rng.random((3, 30))).astype(np.float32) for _ in range(3)]
    full, none = np.ones(30, bool), np.zeros(30, bool)
    ref = pool_reference(xs, ys, [full, none, full], [0, 1, 0], degree=2)
    assert ref[1] is None and ref[0]["n_pool"] == 60
    alone = onp.ridge_poly_fit(np.concatenate([xs[0].T, xs[2].T]).astype(np.float64),
                               onp.logit(np.concatenate([ys[0].T, ys[2].T]).astype(np.float64)), degree=2)
    np.testing.assert_allclose(ref[0]["coef"], alone["coef"], rtol=1e-11, atol=1e-13)   # the same rows through other array layouts


def test_pool_layout_for_an_unordered_id_list():
    """order = the pairs sorted by (group, pair index), start = each group's slice of it."""
    from s2_emit.pairs import _pool_ids, pool_layout
    ids = _pool_ids([2, 0, 1, 0, 2, 2, 1], 7)
    assert ids.dtype == np.int32
    order, start = pool_layout(ids)
    assert order.dtype == np.int32 and start.dtype == np.int32
    assert order.tolist() == [1, 3, 2, 6, 0, 4, 5] and start.tolist() == [0, 2, 4, 7]
    for g in range(3):
        members = order[start[g]:start[g + 1]]
        assert (ids[members] == g).all() and (np.diff(members) > 0).all()
    np.testing.assert_array_equal(_pool_ids("all", 4), [0, 0, 0, 0])
    order, start = pool_layout(_pool_ids("all", 4))
    assert order.tolist() == [0, 1, 2, 3] and start.tolist() == [0, 4]
    order, start = pool_layout(_pool_ids(np.arange(5)[::-1].copy(), 5))
    assert order.tolist() == [4, 3, 2, 1, 0] and start.tolist() == [0, 1, 2, 3, 4, 5]


def test_bad_pool_arguments_raise_before_gpu_work(monkeypatch):
    """A wrong length, a bool, a float dtype, a negative id, a gap in the ids, a string other than "all" and a tensor that is not on
    the host raise ValueError naming `pool` from the host checks; the GPU is never asked for."""
    import torch
    import s2_emit
    from s2_emit import _native as nat

    def no_gpu():
        raise AssertionError("the GPU was asked for")

    monkeypatch.setattr(nat, "require_gpu", no_gpu)
    emit = np.zeros((3, 285, 4, 5), np.uint16)
    s2 = np.zeros((3, 10, 24, 30), np.uint16)
    bad = ([0, 0], [0, 0, 0, 0], 0, True, [True, False, True], np.zeros(3, bool), [0.0, 1.0, 0.0], np.zeros(3, np.float32),
           [0, -1, 0], [0, 2, 0], [1, 1, 1], [1, 2, 3], "each", "ALL", "", np.zeros((3, 1), np.int32), [[0, 0, 0]],
           torch.zeros(3, dtype=torch.int32, device="meta"))
    for pool in bad:
        with pytest.raises(ValueError, match="pool"):
            s2_emit.fuse_tile_pairs(emit, s2, pool=pool)
    for pool in ([0, 0], True, [1], "one", [0.0]):
        with pytest.raises(ValueError, match="pool"):
            s2_emit.fuse_tile_pair(emit[0], s2[0], pool=pool)


def test_good_pool_arguments_reach_the_gpu_request(monkeypatch):
    import torch
    import s2_emit
    from s2_emit import _native as nat

    class Asked(Exception):
        pass

    def gpu():
        raise Asked

    monkeypatch.setattr(nat, "require_gpu", gpu)
    emit = np.zeros((3, 285, 4, 5), np.uint16)
    s2 = np.zeros((3, 10, 24, 30), np.uint16)
    for pool in (None, "all", [0, 0, 0], [0, 1, 0], (2, 0, 1), np.array([1, 0, 1]), np.array([0, 1, 2], np.uint8),
                 np.zeros(3, np.int64), torch.tensor([1, 1, 0])):
        with pytest.raises(Asked):
            s2_emit.fuse_tile_pairs(emit, s2, pool=pool, report=True, validate=True)
    for pool in (None, "all", [0]):
        with pytest.raises(Asked):
            s2_emit.fuse_tile_pair(emit[0], s2[0], pool=pool)


def test_plan_carries_the_group_ids():
    from s2_emit import pairs
    emit = np.zeros((4, 285, 2, 3), np.uint16)
    s2 = np.zeros((4, 10, 2, 3), np.uint16)
    plan = pairs._plan(emit, s2, 32, 3, 1, None, pool=[1, 0, 1, 1])
    assert plan.pool.tolist() == [1, 0, 1, 1] and plan.pool.dtype == np.int32 and plan.M == 2
    plan = pairs._plan(emit, s2, 32, 3, 1, None, pool="all")
    assert plan.pool.tolist() == [0, 0, 0, 0] and plan.M == 1
    plan = pairs._plan(emit, s2, 32, 3, 1, None)
    assert plan.pool is None and plan.M == 0


def test_output_fields_default_to_none_and_predict_checks_its_arguments(monkeypatch):
    """The new fields of TilePairOutput default to None, pool_model needs a pooled output, and predict refuses a missing or
    malformed model_index and a wrong band count before the GPU is asked for."""
    import torch
    from s2_emit import TilePairOutput
    from s2_emit import _native as nat

    def no_gpu():
        raise AssertionError("the GPU was asked for")

    monkeypatch.setattr(nat, "require_gpu", no_gpu)
    fit = dict(n_in=4, nf=14, b64=torch.zeros((2, 5), dtype=torch.float64))
    out = TilePairOutput(cube=None, n_train=None, status=None, mask=None, s2_coarse=None, bands=np.arange(5), degree=2, alpha=1.0,
                         _fit=fit)
    assert out.pool is None and out.n_pool is None and out.pool_status is None
    with pytest.raises(ValueError, match="pool_model"):
        out.pool_model(0)
    tiles = np.zeros((3, 4, 6, 7), np.uint16)
    with pytest.raises(ValueError, match="model_index is required"):
        out.predict(tiles)
    for idx in ([0, 1], [0, 1, 2], [0, -1, 1], [0.0, 1.0, 0.0], torch.zeros(3, dtype=torch.int64, device="meta")):
        with pytest.raises(ValueError, match="model_index"):
            out.predict(tiles, idx)
    with pytest.raises(ValueError, match="bands"):
        out.predict(np.zeros((3, 5, 6, 7), np.uint16), [0, 1, 0])
    with pytest.raises(ValueError, match="uint16 or float32"):
        out.predict(tiles.astype(np.int32), [0, 1, 0])


def test_new_exports_declared_and_registered():
    import inspect
    import s2_emit
    from s2_emit import _native as nat
    text = open(os.path.join(ROOT, "include", "hsr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    comments = "".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/hsr.h"
        assert name in nat.SIGNATURES, f"{name} has no ctypes signature"
        assert name in comments, f"{name} is not documented in include/hsr.h"
    assert len(nat.SIGNATURES["hsr_pool_stats"][1]) == 13 and len(nat.SIGNATURES["hsr_pool_gram"][1]) == 12
    assert len(nat.SIGNATURES["hsr_pool_models"][1]) == 27
    assert nat.HSR_ABI_VERSION == 5
    lib = nat.load()
    assert lib.hsr_abi_version() == 5 and all(hasattr(lib, n) for n in NEW_EXPORTS)
    assert lib.hsr_k4_instance_count() == 31 and lib.hsr_aux_instance_count() == 32     # the new kernels are in neither record
    for fn in (s2_emit.fuse_tile_pairs, s2_emit.fuse_tile_pair):
        assert inspect.signature(fn).parameters["pool"].default is None
