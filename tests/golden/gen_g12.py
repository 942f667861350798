"""Generate tests/golden/g12_tile_pairs.npz (build container only, with the reference present):

    python tests/golden/gen_g12.py

Fixture g12 pins s2_emit.fuse_tile_pairs: P = 3 synthetic tile pairs at the notebook's shape (EMIT 285 x 100 x 100 uint16
x 1e4 with nodata 65535, S2 10 x 600 x 600 uint16 DN with nodata 0) run through the per-pair flow of
legacy_notebooks/Spectral_matching.ipynb with the notebook's OWN functions (flatten_pixels, logit, sigmoid,
subsample_bands_evenly, predict_cube_logit, loaded by oracle.ref_loader) and the scikit-learn pipeline in float64, as g11.

One step is restated instead of run: the notebook brings S2 to the EMIT grid with GDAL's bilinear reproject (raw line 377),
which needs rasterio (absent).  Here S2 on the EMIT grid is the 6 x 6 block mean of the fine pixels (float64 sum, float32
store) and a block holding a nodata (0) sample is NaN - the rule fuse_tile_pairs implements; its GDAL parity is unpinned.

The inputs are stored as small factors (abundances, endmember spectra, S2 responses) plus fixed integer dithers and lists
of nodata positions; tests/test_tile_pairs_host.py rebuilds them with the same statements (g12_inputs).
NumPy 2.2.6 / scikit-learn 1.7.2.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_loader            # noqa: E402

warnings.simplefilter("ignore")

P, B, C, h, f = 3, 285, 10, 100, 6


def g12_inputs(g):
    """(emit (P, 285, 100, 100) uint16, s2 (P, 10, 600, 600) uint16) from the stored factors (the same statements as the test)."""
    ab = g["abund"].astype(np.float64) / 255.0                                          # (P, 3, h, h)
    bb, ii, jj = np.meshgrid(np.arange(B), np.arange(h), np.arange(h), indexing="ij")
    emit = np.empty((P, B, h, h), np.uint16)
    for p in range(P):
        refl = np.einsum("kij,kb->bij", ab[p], g["spectra"])
        dn = np.round(1e4 * refl) + ((7 * ii + 13 * jj + 5 * bb + 11 * p) % 17 - 8)
        emit[p] = np.clip(dn, 1, 9000).astype(np.uint16)
    for p, b_, i_, j_ in g["emit_nd"]:                       # b_ == -1: every band
        if b_ < 0:
            emit[p, :, i_, j_] = 65535
        else:
            emit[p, b_, i_, j_] = 65535
    i2, j2 = np.meshgrid(np.arange(h), np.arange(h), indexing="ij")
    bad2 = (3 * i2 + 7 * j2) % 5 < 2                         # pair 2: 40 % of the pixels lose one selected band
    sel = g["bands"]
    emit[2, sel[(i2 + j2) % len(sel)][bad2], i2[bad2], j2[bad2]] = 65535
    cc, fi, fj = np.meshgrid(np.arange(C), np.arange(h * f), np.arange(h * f), indexing="ij")
    s2 = np.empty((P, C, h * f, h * f), np.uint16)
    for p in range(P):
        coarse = np.einsum("kij,kc->cij", ab[p], g["s2_resp"])
        fine = np.repeat(np.repeat(coarse, f, axis=1), f, axis=2) + ((3 * fi + 5 * fj + 7 * cc + p) % 11 - 5)
        s2[p] = np.clip(np.round(fine), 1, 10000).astype(np.uint16)
    for p, c_, i_, j_ in g["s2_zero"]:
        s2[p, c_, i_, j_] = 0
    return emit, s2


def block_mean_rule(s2_u16, nodata=0.0):
    """S2 (C, H f, W f) -> (C, H, W) float32: float64 sum of the f x f samples / f^2, NaN where a sample is nodata."""
    Cn, Hf, Wf = s2_u16.shape
    v = s2_u16.astype(np.float64).reshape(Cn, Hf // f, f, Wf // f, f)
    m = (v.sum(axis=(2, 4)) / (f * f)).astype(np.float32)
    bad = np.isclose(v, nodata).any(axis=(2, 4))
    m[bad] = np.nan
    return m


def decode(emit_u16):
    return np.where(emit_u16 == 65535, np.float32(np.nan), emit_u16.astype(np.float32) * np.float32(1e-4))


def main():
    assert ref_loader.available(), "reference tree not present"
    smf = ref_loader.load_spectral_matching_functions()
    from sklearn.linear_model import Ridge
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import PolynomialFeatures, StandardScaler

    rng = np.random.default_rng(12)
    abund = (rng.random((P, 3, 20, 20)) * 255)
    abund = np.repeat(np.repeat(abund, 5, axis=2), 5, axis=3) + rng.random((P, 3, h, h)) * 40
    abund = np.clip(abund, 0, 255).astype(np.uint8)                                 # (P, 3, 100, 100)
    wl = np.linspace(0, 1, B)
    spectra = np.stack([0.05 + 0.4 * wl, 0.3 - 0.2 * wl + 0.05 * np.sin(9 * wl), 0.1 + 0.3 * np.exp(-((wl - 0.6) / 0.15) ** 2)])
    s2_resp = 600 + 2200 * rng.random((3, C))
    bands = smf["subsample_bands_evenly"](B, 32).astype(np.int32)
    assert 1 not in bands
    emit_nd = np.array([[0, -1, 5, 7], [0, int(bands[3]), 10, 20], [0, 1, 30, 40], [1, -1, 99, 99]])
    s2_zero = np.array([[1, 0, 0, 0], [1, 4, 300, 301], [1, 9, 599, 17], [0, 2, 123, 456]])
    g = dict(abund=abund, spectra=spectra, s2_resp=s2_resp, bands=bands, emit_nd=emit_nd, s2_zero=s2_zero)
    emit, s2 = g12_inputs(g)

    out = dict(g)
    n_train, masks, means, scales, coefs, intercepts = [], [], [], [], [], []
    samples, rows, nan_counts, bsum, bsumsq = [], [], [], [], []
    for p in range(P):
        X = block_mean_rule(s2[p])                                                     # (10, 100, 100) float32
        Yall = decode(emit[p])                                                         # (285, 100, 100) float32
        Y = Yall[bands]
        Xtr, Ytr = smf["flatten_pixels"](X, Y, x_nodata=0.0, y_nodata=None)
        Xf, Yf = X.reshape(C, -1).T, Y.reshape(len(bands), -1).T
        mask = np.isfinite(Xf).all(1) & np.isfinite(Yf).all(1) & ~np.isclose(Xf, 0.0).any(1)
        assert mask.sum() == len(Xtr)
        model = Pipeline([("scaler", StandardScaler()), ("poly", PolynomialFeatures(degree=3, include_bias=False)),
                          ("ridge", Ridge(alpha=1.0))])
        model.fit(Xtr.astype(np.float64), smf["logit"](Ytr.astype(np.float64), eps=1e-4))
        pred = smf["predict_cube_logit"](model, s2[p].astype(np.float32), nodata=0.0)   # (32, 600, 600) float32
        fin = np.isfinite(pred)
        n_train.append(len(Xtr))
        masks.append(np.packbits(mask))
        means.append(model.named_steps["scaler"].mean_)
        scales.append(model.named_steps["scaler"].scale_)
        coefs.append(model.named_steps["ridge"].coef_.astype(np.float32))          # float32: the file stays under 1 MiB
        intercepts.append(model.named_steps["ridge"].intercept_)
        samples.append(pred[:, ::23, ::29])
        rows.append(pred[:, 301, :])
        nan_counts.append((~fin).sum())
        bsum.append(np.where(fin, pred, 0).sum(axis=(1, 2), dtype=np.float64))
        bsumsq.append((np.where(fin, pred, 0).astype(np.float64) ** 2).sum(axis=(1, 2)))
        print(f"pair {p}: n_train {len(Xtr)}, NaN at 10 m {nan_counts[-1]}")
        if p == 0:                                                                     # all 285 bands as targets
            Y285 = Yall
            Xa, Ya = smf["flatten_pixels"](X, Y285, x_nodata=0.0, y_nodata=None)
            m285 = Pipeline([("scaler", StandardScaler()), ("poly", PolynomialFeatures(degree=3, include_bias=False)),
                             ("ridge", Ridge(alpha=1.0))])
            m285.fit(Xa.astype(np.float64), smf["logit"](Ya.astype(np.float64), eps=1e-4))
            pix = (np.arange(257) * 1399) % (h * f * h * f)                            # 257 fine pixels
            Xs = s2[p].reshape(C, -1)[:, pix].T.astype(np.float32)
            ok = ~np.isclose(Xs, 0.0).any(1)
            out.update(n_train_285=np.int64(len(Xa)), intercept_285=m285.named_steps["ridge"].intercept_, pix_285=pix,
                       pred_logit_285=np.where(ok[:, None], m285.predict(Xs.astype(np.float64)), np.nan).astype(np.float32))
    out.update(n_train=np.array(n_train, np.int64), mask_packed=np.stack(masks), mean=np.stack(means), scale=np.stack(scales),
               coef=np.stack(coefs), intercept=np.stack(intercepts), pred_sample=np.stack(samples), pred_row_301=np.stack(rows),
               pred_nan_count=np.array(nan_counts, np.int64), pred_band_sum=np.stack(bsum), pred_band_sumsq=np.stack(bsumsq))
    path = os.path.join(HERE, "g12_tile_pairs.npz")
    np.savez_compressed(path, **out)
    print(f"g12_tile_pairs.npz  {os.path.getsize(path)/1024:.1f} KiB")


if __name__ == "__main__":
    main()
