"""Generate tests/golden/g14_tile_pairs_pool.npz (build container only, with the reference present):

    python tests/golden/gen_g14.py

Fixture g14 pins fuse_tile_pairs(pool=...): ONE model per group of tile pairs, fitted on the training pixels of all the group's
members and applied to every member.  The inputs are g12's three pairs (rebuilt from its stored factors by gen_g12.g12_inputs),
pooled two ways:
    "all"  pool="all": one model from the training pixels of the three pairs;
    "010"  pool=[0, 1, 0] with pair 2's train_mask all False: group 0 is fitted on pair 0 alone and also applied to pair 2 (a
           wholly held-out pair), group 1 is pair 1.
Each group is fitted as gen_g12.py fits a pair - the notebook's functions (flatten_pixels, logit, predict_cube_logit) through
oracle.ref_loader, the scikit-learn pipeline in float64 - on the CONCATENATION of its members' training pixels in pair order.
Stored per pooling k: mean_k, scale_k (M, 10), intercept_k (M, 32), n_pool_k (M,), and per pair the strided prediction sample,
row 301, the NaN count and the per-band sums and sums of squares as g12 stores them, plus the model's float64 logits at 48 fine
pixels (pix) for the float64 restatement of tests/test_tile_pairs_pool_host.py.  NumPy 2.2.6 / scikit-learn 1.7.2.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from oracle import ref_loader                                         # noqa: E402
from gen_g12 import C, P, block_mean_rule, decode, f, g12_inputs, h   # noqa: E402

warnings.simplefilter("ignore")

POOLINGS = {"all": ([0, 0, 0], ()), "010": ([0, 1, 0], (2,))}         # name -> (group ids, pairs whose train_mask is all False)
NPIX_LOGIT = 48


def main():
    assert ref_loader.available(), "reference tree not present"
    smf = ref_loader.load_spectral_matching_functions()
    from sklearn.linear_model import Ridge
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import PolynomialFeatures, StandardScaler

    g = dict(np.load(os.path.join(HERE, "g12_tile_pairs.npz")))
    emit, s2 = g12_inputs(g)
    bands = g["bands"]
    train = []
    for p in range(P):
        Xtr, Ytr = smf["flatten_pixels"](block_mean_rule(s2[p]), decode(emit[p])[bands], x_nodata=0.0, y_nodata=None)
        assert len(Xtr) == g["n_train"][p]
        train.append((Xtr.astype(np.float64), smf["logit"](Ytr.astype(np.float64), eps=1e-4)))
    pix = (np.arange(NPIX_LOGIT) * 7499 + 17) % (h * f * h * f)
    out = dict(pix=pix)
    for name, (ids, held) in POOLINGS.items():
        M = max(ids) + 1
        models, n_pool = [], []
        for grp in range(M):
            members = [p for p in range(P) if ids[p] == grp and p not in held]
            X = np.concatenate([train[p][0] for p in members])
            Y = np.concatenate([train[p][1] for p in members])
            model = Pipeline([("scaler", StandardScaler()), ("poly", PolynomialFeatures(degree=3, include_bias=False)),
                              ("ridge", Ridge(alpha=1.0))])
            model.fit(X, Y)
            models.append(model)
            n_pool.append(len(X))
        samples, rows, nan_counts, bsum, bsumsq, logits = [], [], [], [], [], []
        for p in range(P):
            model = models[ids[p]]
            pred = smf["predict_cube_logit"](model, s2[p].astype(np.float32), nodata=0.0)   # (32, 600, 600) float32
            fin = np.isfinite(pred)
            samples.append(pred[:, ::23, ::29])
            rows.append(pred[:, 301, :])
            nan_counts.append((~fin).sum())
            bsum.append(np.where(fin, pred, 0).sum(axis=(1, 2), dtype=np.float64))
            bsumsq.append((np.where(fin, pred, 0).astype(np.float64) ** 2).sum(axis=(1, 2)))
            Xs = s2[p].reshape(C, -1)[:, pix].T.astype(np.float32)
            ok = ~np.isclose(Xs, 0.0).any(1)
            logits.append(np.where(ok[:, None], model.predict(Xs.astype(np.float64)), np.nan))
            print(f"{name}: pair {p} from group {ids[p]} (n_pool {n_pool[ids[p]]}), NaN at 10 m {nan_counts[-1]}")
        out.update({f"pool_{name}": np.array(ids, np.int32), f"held_{name}": np.array(held, np.int32),
                    f"n_pool_{name}": np.array(n_pool, np.int64),
                    f"mean_{name}": np.stack([m.named_steps["scaler"].mean_ for m in models]),
                    f"scale_{name}": np.stack([m.named_steps["scaler"].scale_ for m in models]),
                    f"intercept_{name}": np.stack([m.named_steps["ridge"].intercept_ for m in models]),
                    f"pred_sample_{name}": np.stack(samples), f"pred_row_301_{name}": np.stack(rows),
                    f"pred_nan_count_{name}": np.array(nan_counts, np.int64), f"pred_band_sum_{name}": np.stack(bsum),
                    f"pred_band_sumsq_{name}": np.stack(bsumsq), f"pred_logit_{name}": np.stack(logits)})
    path = os.path.join(HERE, "g14_tile_pairs_pool.npz")
    np.savez_compressed(path, **out)
    print(f"g14_tile_pairs_pool.npz  {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()
