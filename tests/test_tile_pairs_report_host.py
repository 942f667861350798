"""fuse_tile_pairs(report=True) on the host side: the flag's check that needs no GPU, fixture g13 (the notebook's cell 26 on
g12's pairs) and a float64 restatement of the report that the GPU tests reuse."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from oracle import oracle_np as onp
from test_tile_pairs_host import block_mean_rule, decode_u16, g12_inputs


def report_reference(Xtr, Ytr, mean, scale, coef, intercept, degree=3):
    """Cell 26 restated: z = float32(b + phi((X - mean) / scale) . coef^T) in float64, yp = sigmoid(clip(z, +-50)) in float32,
    d = y - yp in float32, sums in float64.  -> (r2 (T,), rmse (T,)); NaN for an empty training set."""
    Z = (np.asarray(Xtr, np.float64) - mean) / scale
    z = (intercept + onp.poly_features(Z, degree) @ np.asarray(coef, np.float64).T).astype(np.float32)
    zc = np.clip(z, np.float32(-50), np.float32(50))
    yp = np.float32(1) / (np.float32(1) + np.exp(-zc))
    yt = np.asarray(Ytr, np.float32)
    d = (yt - yp).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ss_res = (d * d).sum(axis=0)
        ss_tot = ((yt.astype(np.float64) - yt.astype(np.float64).mean(axis=0)) ** 2).sum(axis=0) + 1e-8
        return 1.0 - ss_res / ss_tot, np.sqrt(ss_res / len(yt))


def test_report_flag_checked_before_gpu_work(monkeypatch):
    """A report flag that is not a bool raises ValueError naming `report` from the host checks; the GPU is never asked for."""
    import s2_emit
    from s2_emit import _native as nat

    def no_gpu():
        raise AssertionError("the GPU was asked for")

    monkeypatch.setattr(nat, "require_gpu", no_gpu)
    emit = np.zeros((285, 4, 5), np.uint16)
    s2 = np.zeros((10, 24, 30), np.uint16)
    for bad in (1, 0, "yes", None, 1.0, np.bool_(True)):
        with pytest.raises(ValueError, match="report"):
            s2_emit.fuse_tile_pair(emit, s2, report=bad)
        with pytest.raises(ValueError, match="report"):
            s2_emit.fuse_tile_pairs(emit[None], s2[None], report=bad)


def test_g13_size_and_training_counts():
    assert os.path.getsize(os.path.join(GOLDEN, "g13_tile_pairs_report.npz")) <= 1 << 20
    g13, g12 = load_golden("g13_tile_pairs_report"), load_golden("g12_tile_pairs")
    np.testing.assert_array_equal(g13["n_train"], g12["n_train"])
    assert g13["r2"].shape == (3, 32) and g13["rmse"].shape == (3, 32)
    assert np.isfinite(g13["r2"]).all() and (g13["rmse"] > 0).all()


def test_g13_against_restatement_from_g12_model():
    """g13 (the notebook's cell 26, scikit-learn's model) against the float64 restatement built from g12's stored model; g12
    stores coef as float32, hence 1e-4."""
    g13, g = load_golden("g13_tile_pairs_report"), load_golden("g12_tile_pairs")
    import s2_emit
    emit, s2 = g12_inputs(g)
    for p in range(3):
        X = block_mean_rule(s2[p], nodata=0.0)
        Y = decode_u16(emit[p])[g["bands"]]
        Xtr, Ytr = s2_emit.flatten_pixels(X, Y, x_nodata=0.0)
        r2, rmse = report_reference(Xtr, Ytr, g["mean"][p], g["scale"][p], g["coef"][p], g["intercept"][p])
        np.testing.assert_allclose(r2, g13["r2"][p], rtol=0, atol=1e-4)
        np.testing.assert_allclose(rmse, g13["rmse"][p], rtol=1e-4)
