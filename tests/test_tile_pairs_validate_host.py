"""fuse_tile_pairs(train_mask=..., validate=True) on the host side: a float64 NumPy restatement of the validation scores that the
GPU tests reuse (checked here on hand-built cases), the argument checks that need no GPU, the declaration and registration of
the new exports, the plane slicing of the block mean and the conditions the GPU tests put on fixture g12."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("hsr_pair_holdout", "hsr_pair_score_work_bytes", "hsr_pair_score_f64")


def validation_reference(pred, y, group, factor):
    """The scores of one pair and one view restated: pred, y (T, npix) float32, group (npix,) with 1 = fit, 2 = held out.
    Per band over S = the group's pixels with pred and y finite: d = float32(y - pred), ss_res = sum (double) d^2, mean_ref and
    the two-pass M2 of (double) y, rmse = sqrt(ss_res / n), r2 = 1 - ss_res / (M2 + 1e-8); n == 0 -> NaN.  Per pixel of a group
    with all T values finite and both spectra non-zero: the spectral angle in degrees, float64.  ergas = 100 / factor *
    sqrt(mean over the bands with n > 0 and mean_ref != 0 of (rmse / mean_ref)^2).
    -> dict: n (2, T) int64, rmse, r2, mean_ref, ss_res, m2 (2, T), sam, ergas (2,), n_sam (2,) int64, angle (npix,) float64 (NaN
    where undefined; sam_map is its float32 rounding)."""
    pred = np.asarray(pred, np.float32)
    y = np.asarray(y, np.float32)
    group = np.asarray(group)
    T, npix = pred.shape
    fin = np.isfinite(pred) & np.isfinite(y)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (y - pred).astype(np.float64)
    y64, p64 = y.astype(np.float64), pred.astype(np.float64)
    out = {k: np.full((2, T), np.nan) for k in ("rmse", "r2", "mean_ref", "ss_res", "m2")}
    out["n"] = np.zeros((2, T), np.int64)
    out["sam"], out["ergas"], out["n_sam"] = np.full(2, np.nan), np.full(2, np.nan), np.zeros(2, np.int64)
    allfin = fin.all(axis=0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dot, a, b = (y64 * p64).sum(axis=0), (y64 * y64).sum(axis=0), (p64 * p64).sum(axis=0)
        has = np.isin(group, (1, 2)) & allfin & (a > 0) & (b > 0)
        cosv = np.clip(dot / np.sqrt(a * b), -1.0, 1.0)
        angle = np.where(has, np.arccos(cosv) * (180.0 / np.pi), np.nan)
    out["angle"] = angle
    for g in range(2):
        ing = group == g + 1
        terms = []
        for j in range(T):
            S = ing & fin[j]
            n = int(S.sum())
            out["n"][g, j] = n
            if n == 0:
                continue
            ss_res = float((d[j, S] * d[j, S]).sum())
            mean = float(y64[j, S].mean())
            m2 = float(((y64[j, S] - mean) ** 2).sum())
            out["ss_res"][g, j], out["m2"][g, j], out["mean_ref"][g, j] = ss_res, m2, mean
            out["rmse"][g, j] = np.sqrt(ss_res / n)
            out["r2"][g, j] = 1.0 - ss_res / (m2 + 1e-8)
            if mean != 0.0:
                terms.append((out["rmse"][g, j] / mean) ** 2)
        if terms:
            out["ergas"][g] = 100.0 / factor * np.sqrt(np.mean(terms))
        sel = ing & has
        out["n_sam"][g] = int(sel.sum())
        if sel.any():
            out["sam"][g] = float(angle[sel].mean())
    return out


def checkerboard_mask(h, w, block=10):
    """True on the blocks of a block x block checkerboard that may train, False on the held-out ones."""
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return ((i // block + j // block) % 2) == 0


# ---- the restatement on hand-built cases -------------------------------------------------------------------------------------
def test_reference_identical_spectra():
    rng = np.random.default_rng(0)
    y = rng.random((5, 12)).astype(np.float32) + np.float32(0.1)
    r = validation_reference(y, y, np.ones(12, np.uint8), 6)
    assert (r["n"][0] == 12).all() and (r["n"][1] == 0).all()
    assert (r["rmse"][0] == 0).all() and (r["r2"][0] == 1).all()
    assert np.nanmax(r["angle"]) <= 5e-6 and r["sam"][0] <= 5e-6 and r["n_sam"][0] == 12
    assert r["ergas"][0] == 0 and np.isnan(r["ergas"][1]) and np.isnan(r["sam"][1]) and np.isnan(r["rmse"][1]).all()


def test_reference_orthogonal_and_scaled_spectra():
    y = np.array([[1.0, 0.25], [0.0, 0.5]], np.float32)          # pixel 0: (1, 0), pixel 1: (0.25, 0.5)
    p = np.array([[0.0, 0.5], [1.0, 1.0]], np.float32)           # pixel 0: (0, 1) orthogonal, pixel 1: 2 y
    r = validation_reference(p, y, np.array([1, 2], np.uint8), 6)
    assert abs(r["angle"][0] - 90.0) < 1e-12 and abs(r["sam"][0] - 90.0) < 1e-12
    assert abs(r["angle"][1]) <= 5e-6 and r["rmse"][1, 0] == 0.25 and r["rmse"][1, 1] == 0.5
    assert r["n_sam"].tolist() == [1, 1]


def test_reference_constant_band_and_ergas_by_hand():
    # band 0 constant 0.5 with errors +-0.25: ss_res = 2 / 16, M2 = 0 -> r2 = 1 - 0.25 / 1e-8; rmse 0.25, mean 0.5
    # band 1 targets 1, 3 (mean 2, M2 2) with errors 1, 1: rmse 1, r2 = 1 - 2 / (2 + 1e-8)
    y = np.array([[0.5, 0.5, 0.5, 0.5], [1.0, 3.0, 1.0, 3.0]], np.float32)
    p = y - np.array([[0.25, -0.25, 0.25, -0.25], [1.0, 1.0, 7.0, 7.0]], np.float32)
    r = validation_reference(p, y, np.array([1, 1, 0, 0], np.uint8), 6)
    assert r["m2"][0, 0] == 0.0 and r["r2"][0, 0] == 1.0 - 0.125 / 1e-8 and r["rmse"][0, 0] == 0.25
    assert r["rmse"][0, 1] == 1.0 and r["r2"][0, 1] == 1.0 - 2.0 / (2.0 + 1e-8) and r["mean_ref"][0].tolist() == [0.5, 2.0]
    # ergas = 100 / 6 * sqrt(((0.25 / 0.5)^2 + (1 / 2)^2) / 2) = 100 / 6 * 0.5
    np.testing.assert_allclose(r["ergas"][0], 100.0 / 6.0 * 0.5, rtol=1e-15)
    assert (r["n"][1] == 0).all() and np.isnan(r["angle"][2:]).all()              # group 0 pixels: in no statistic, no angle


def test_reference_nan_removes_the_pixel_from_its_band_and_from_the_angles_only():
    rng = np.random.default_rng(1)
    y = rng.random((3, 6)).astype(np.float32) + np.float32(0.1)
    p = y + np.float32(0.125)
    p[1, 2] = np.nan
    r = validation_reference(p, y, np.ones(6, np.uint8), 6)
    assert r["n"][0].tolist() == [6, 5, 6] and r["n_sam"][0] == 5 and np.isnan(r["angle"][2]) and np.isfinite(r["angle"][[0, 1, 3]]).all()
    keep = np.arange(6) != 2
    np.testing.assert_allclose(r["mean_ref"][0, 1], y[1, keep].astype(np.float64).mean(), rtol=1e-15)
    np.testing.assert_allclose(r["mean_ref"][0, 0], y[0].astype(np.float64).mean(), rtol=1e-15)
    # a band whose mean is 0 leaves ERGAS; a group with no usable band has NaN
    z = np.zeros((1, 4), np.float32)
    assert np.isnan(validation_reference(z + np.float32(0.5), z, np.ones(4, np.uint8), 6)["ergas"][0])


# ---- the interface ---------------------------------------------------------------------------------------------------------
def test_validate_and_train_mask_checked_before_gpu_work(monkeypatch):
    """A validate flag that is not a bool, or a train_mask of the wrong shape or dtype, raises ValueError naming the argument from
    the host checks; the GPU is never asked for."""
    import s2_emit
    from s2_emit import _native as nat

    def no_gpu():
        raise AssertionError("the GPU was asked for")

    monkeypatch.setattr(nat, "require_gpu", no_gpu)
    emit = np.zeros((285, 4, 5), np.uint16)
    s2 = np.zeros((10, 24, 30), np.uint16)
    for bad in (1, 0, "yes", None, 1.0, np.bool_(True)):
        with pytest.raises(ValueError, match="validate"):
            s2_emit.fuse_tile_pair(emit, s2, validate=bad)
        with pytest.raises(ValueError, match="validate"):
            s2_emit.fuse_tile_pairs(emit[None], s2[None], validate=bad)
    for bad in (np.ones((4, 6), bool), np.ones((5, 4), bool), np.ones((1, 4, 5), bool), np.ones((4, 5), np.float32),
                np.ones((4, 5), np.int64)):
        with pytest.raises(ValueError, match="train_mask"):
            s2_emit.fuse_tile_pair(emit, s2, train_mask=bad)
    for bad in (np.ones((4, 5), bool), np.ones((2, 4, 5), bool), [np.ones((4, 5), bool), np.ones((4, 5), bool)],
                np.ones((1, 4, 5), np.int32)):
        with pytest.raises(ValueError, match="train_mask"):
            s2_emit.fuse_tile_pairs(emit[None], s2[None], train_mask=bad)


def test_good_train_mask_and_validate_reach_the_gpu_request(monkeypatch):
    import s2_emit
    from s2_emit import _native as nat

    class Asked(Exception):
        pass

    def gpu():
        raise Asked

    monkeypatch.setattr(nat, "require_gpu", gpu)
    emit = np.zeros((285, 4, 5), np.uint16)
    s2 = np.zeros((10, 24, 30), np.uint16)
    for m in (np.ones((4, 5), bool), np.ones((4, 5), np.uint8)):
        with pytest.raises(Asked):
            s2_emit.fuse_tile_pair(emit, s2, train_mask=m, validate=True)
        with pytest.raises(Asked):
            s2_emit.fuse_tile_pairs([emit, emit], [s2, s2], train_mask=[m, m], validate=True)


def test_new_exports_declared_and_registered():
    from s2_emit import _native as nat
    text = open(os.path.join(ROOT, "include", "hsr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    comments = "".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/hsr.h"
        assert name in nat.SIGNATURES, f"{name} has no ctypes signature"
        assert name in comments, f"{name} is not documented in include/hsr.h"
    assert len(nat.SIGNATURES["hsr_pair_score_f64"][1]) == 24 and len(nat.SIGNATURES["hsr_pair_holdout"][1]) == 8
    assert nat.HSR_ABI_VERSION == 5
    import s2_emit
    assert "TilePairValidation" in s2_emit.__all__
    assert s2_emit.pairs.VIEWS == ("coarse", "degraded") and s2_emit.pairs.GROUPS == ("fit", "held_out")


def test_score_work_bytes_host_helper():
    """The sizing helper needs no GPU: 512-pixel chunks, per chunk T x 2 groups x 4 doubles and 4 doubles of angle sums."""
    from s2_emit import _native as nat
    lib = nat.load()
    assert lib.hsr_pair_score_work_bytes(10000, 32) == 20 * (32 * 8 + 4) * 8
    assert lib.hsr_pair_score_work_bytes(512, 1) == (8 + 4) * 8 and lib.hsr_pair_score_work_bytes(513, 1) == 2 * (8 + 4) * 8
    assert lib.hsr_pair_score_work_bytes(0, 32) == 0 and lib.hsr_pair_score_work_bytes(100, 0) == 0


def test_plane_slices_plan():
    """P T float32 planes go to hsr_block_mean in slices of whole pairs of at most 65 535 planes."""
    from s2_emit.pairs import _plane_slices
    assert _plane_slices(64, 32) == ((0, 64),)
    assert _plane_slices(64, 285) == ((0, 64),)                                   # 18 240 planes
    assert _plane_slices(229, 285) == ((0, 229),)                                 # 65 265 planes
    assert _plane_slices(230, 285) == ((0, 229), (229, 230))                      # 65 550 planes
    assert _plane_slices(500, 285) == ((0, 229), (229, 458), (458, 500))
    assert _plane_slices(3, 65535) == ((0, 1), (1, 2), (2, 3))
    for P, T in ((1, 1), (7, 3), (1000, 285), (65535, 32)):
        sl = _plane_slices(P, T)
        assert sl[0][0] == 0 and sl[-1][1] == P and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
        assert all(0 < (p1 - p0) * T <= 65535 for p0, p1 in sl) and len(sl) == -(-P // (65535 // T))
    with pytest.raises(ValueError, match="validate"):
        _plane_slices(2, 65536)


def test_block_mean_is_issued_in_slices_of_whole_pairs(monkeypatch):
    """_validate with a stand-in library: for P T > 65 535 every hsr_block_mean call takes whole pairs and at most 65 535 planes,
    at the right offsets into the cube and the coarse view; one predict call and one score call per view whatever P is."""
    import ctypes
    import torch
    from s2_emit import pairs

    calls = []

    class Lib:
        def __getattr__(self, name):
            def fn(*args):
                calls.append((name, args))
                return 12 * 8 if name == "hsr_pair_score_work_bytes" else 0
            return fn

    P, T, h, w, f, nb = 300, 285, 1, 2, 1, 2
    plan = pairs._plan(np.zeros((P, T, h, w), np.uint16), np.zeros((P, nb, h, w), np.uint16), "all", 1, f, None, False, None, True)
    assert plan.plane_slices == ((0, 229), (229, 300))
    x = torch.zeros((P, nb, h * w))
    y = torch.zeros((P, T, h * w))
    group = torch.zeros((P, h * w), dtype=torch.uint8)
    cube = torch.zeros((P, T, h * w * f * f))
    model = dict(W=torch.zeros((P, 2, T)), b=torch.zeros((P, T)), mean=torch.zeros((P, nb)), inv=torch.zeros((P, nb)))
    v = pairs._validate(Lib(), torch, ctypes.c_void_p(0), plan, pairs._FitState({}, model, x, y, group, 1), cube, None)
    names = [c[0] for c in calls]
    assert names.count("hsr_block_mean") == 2 and names.count("hsr_polyfeat_predict_cube_batched") == 1
    assert names.count("hsr_pair_score_f64") == 2
    bm = [c[1] for c in calls if c[0] == "hsr_block_mean"]
    assert [a[4] for a in bm] == [229 * T, 71 * T]                                             # planes of each call
    assert [a[0].value - cube.data_ptr() for a in bm] == [0, 229 * T * h * w * 4]              # input offsets (bytes)
    assert [a[9].value - v.cube_coarse.data_ptr() for a in bm] == [0, 229 * T * h * w * 4]     # output offsets
    assert v.n.shape == (P, 2, 2, T) and v.sam_map.shape == (P, 2, h, w) and v.views == ("coarse", "degraded")


# ---- what the GPU tests need of fixture g12 --------------------------------------------------------------------------------
def test_g12_checkerboard_leaves_both_groups_well_filled():
    """A 10 x 10 checkerboard hold-out leaves every pair of g12 (9 997, 9 996 and 6 000 valid pixels) at least 2 900 training pixels,
    above the 285 polynomial features, and a held-out group of about the same size."""
    g = load_golden("g12_tile_pairs")
    assert g["n_train"].tolist() == [9997, 9996, 6000]
    keep = checkerboard_mask(100, 100).reshape(-1)
    assert keep.sum() == 5000
    for p in range(3):
        valid = np.unpackbits(g["mask_packed"][p])[:10000].astype(bool)
        n_fit, n_held = int((valid & keep).sum()), int((valid & ~keep).sum())
        assert n_fit >= 2900 and n_held >= 2900 and n_fit + n_held == g["n_train"][p], (p, n_fit, n_held)
