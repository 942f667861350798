"""Generate tests/golden/g13_tile_pairs_report.npz (build container only, with the reference present):

    python tests/golden/gen_g13.py

Fixture g13 pins fuse_tile_pairs(report=True): the fit report of legacy_notebooks/Spectral_matching.ipynb (cell 26: predict
the training pixels, sigmoid, per-band R^2 and RMSE against the raw targets) on g12's three pairs.  The inputs are g12's
(rebuilt from its stored factors by gen_g12.g12_inputs), each pair is fitted as gen_g12.py fits it (the notebook's functions
through oracle.ref_loader, scikit-learn in float64), and the notebook's own cell 26 is executed from the .ipynb JSON with
``model``, ``sigmoid``, ``X_train`` (float64) and ``Y_train`` (float32, as flatten_pixels returns it) in scope.  None of the
notebook's text is stored here.  The cell sums in float32; the GPU sums in float64, so tests compare with tolerances.
"""
from __future__ import annotations

import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from oracle import ref_loader                                         # noqa: E402
from gen_g12 import C, P, block_mean_rule, decode, g12_inputs         # noqa: E402

warnings.simplefilter("ignore")


def report_cell() -> str:
    path = os.path.join(ref_loader.REFERENCE_ROOT, "legacy_notebooks", "Spectral_matching.ipynb")
    nb = json.load(open(path))
    cells = [c for c in nb["cells"] if c["cell_type"] == "code" and "r2_per_band.append" in "".join(c["source"])]
    assert len(cells) == 1, len(cells)
    return "".join(cells[0]["source"])


def main():
    assert ref_loader.available(), "reference tree not present"
    smf = ref_loader.load_spectral_matching_functions()
    from sklearn.linear_model import Ridge
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import PolynomialFeatures, StandardScaler

    g = dict(np.load(os.path.join(HERE, "g12_tile_pairs.npz")))
    emit, s2 = g12_inputs(g)
    bands = g["bands"]
    code = compile(report_cell(), "Spectral_matching.ipynb:cell26", "exec")
    r2, rmse, n_train = [], [], []
    for p in range(P):
        X = block_mean_rule(s2[p])
        Y = decode(emit[p])[bands]
        Xtr, Ytr = smf["flatten_pixels"](X, Y, x_nodata=0.0, y_nodata=None)
        assert Xtr.shape[1] == C and Ytr.dtype == np.float32
        model = Pipeline([("scaler", StandardScaler()), ("poly", PolynomialFeatures(degree=3, include_bias=False)),
                          ("ridge", Ridge(alpha=1.0))])
        model.fit(Xtr.astype(np.float64), smf["logit"](Ytr.astype(np.float64), eps=1e-4))
        scope = dict(np=np, model=model, sigmoid=smf["sigmoid"], X_train=Xtr.astype(np.float64), Y_train=Ytr)
        exec(code, scope)
        r2.append(scope["r2_per_band"])
        rmse.append(scope["rmse_per_band"])
        n_train.append(len(Xtr))
        print(f"pair {p}: n_train {len(Xtr)}, R2 {min(r2[-1]):.4f} .. {max(r2[-1]):.4f}, RMSE {min(rmse[-1]):.2e} .. {max(rmse[-1]):.2e}")
    assert np.array_equal(n_train, g["n_train"])
    path = os.path.join(HERE, "g13_tile_pairs_report.npz")
    np.savez_compressed(path, r2=np.array(r2, np.float64), rmse=np.array(rmse, np.float64), n_train=np.array(n_train, np.int64))
    print(f"g13_tile_pairs_report.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
