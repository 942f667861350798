"""Generate tests/golden/g17_affine.npz (build container only, with the reference present):

    python tests/golden/gen_g17.py

Fixture g17 pins s2_emit.affine: ``fit_ot_affine_rgb`` and ``apply_affine_rgb`` run from the notebook itself
(Pairs_EMIT_S2_demo-2.ipynb, the cell after reproject_stack_to_grid) - the two FunctionDef nodes taken out of the cell's source by
AST and executed; none of their text is stored here.

PARITY UNPINNED SUB-STEP: POT (``import ot``) is absent offline.  The executed namespace gets an ``ot`` object whose ``dist`` and
``sinkhorn`` are the oracle's ``sqeuclidean_cost`` and ``sinkhorn_knopp`` (oracle/oracle_np.py), POT's documented algorithm
restated - as for the fixtures of fit_ot_poly_rgb.  Everything else is the notebook's own code: the order of the two ``choice``
draws, the row filters, the barycentric projection, np.linalg.lstsq, the apply with and without a mask.

Contents (seeded; NumPy 2.2.6): a 40 x 36 pair with values outside [0, 1], a mask of ~85 %, a NaN and an inf inside the mask.
    src, ref (40, 36, 3) float32, mask (40, 36) bool
    A, t                          fit_ot_affine_rgb(src, ref, mask, n_samples=600, seed=3)
    A_one, t_one, mask_one        the identity case: a mask with one pixel
    At_hand                       a hand-made (A, t) with zero entries, so that inf * 0 occurs
    out_fit_mask, out_fit_nomask, out_hand_mask, out_hand_nomask      apply_affine_rgb with the fitted / hand-made map
    W_gray (4, 3)                 np.linalg.lstsq directly on all usable masked rows of (gray, ref), gray = src's first channel three
                                  times (rank 2; not stored, a test repeats the channel): the minimum-norm solution
"""
from __future__ import annotations

import ast
import json
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import oracle_np as onp                                   # noqa: E402
from oracle import ref_loader                                         # noqa: E402

warnings.simplefilter("ignore")
H, W = 40, 36


def load_notebook_functions():
    path = os.path.join(ref_loader.REFERENCE_ROOT, "Pairs_EMIT_S2_demo-2.ipynb")
    cells = json.load(open(path))["cells"]
    src = next("".join(c["source"]) for c in cells if c["cell_type"] == "code" and "def fit_ot_affine_rgb" in "".join(c["source"]))
    tree = ast.parse(src, filename=path)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("fit_ot_affine_rgb", "apply_affine_rgb")]
    assert len(fns) == 2
    ot = types.SimpleNamespace(dist=lambda X, Y, metric="sqeuclidean": onp.sqeuclidean_cost(X, Y),
                               sinkhorn=lambda a, b, M, reg, numItermax, stopThr: onp.sinkhorn_knopp(a, b, M, reg, numItermax, stopThr))
    ns = {"np": np, "ot": ot}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return ns["fit_ot_affine_rgb"], ns["apply_affine_rgb"]


def main():
    assert ref_loader.available(), "reference tree not present"
    fit, apply = load_notebook_functions()
    rng = np.random.default_rng(17)
    src = (rng.random((H, W, 3)) * 1.3 - 0.15).astype(np.float32)
    M = np.array([[0.8, 0.1, -0.05], [0.15, 0.7, 0.1], [-0.1, 0.2, 0.9]])
    ref = (np.clip(src.astype(np.float64), 0, 1) ** 0.9 @ M + [0.03, -0.02, 0.05] + 0.02 * rng.standard_normal((H, W, 3))).astype(np.float32)
    mask = rng.random((H, W)) < 0.85
    mask[3, 4] = mask[10, 20] = mask[30, 7] = True
    mask[0, 0] = False
    src[3, 4, 1] = np.nan
    src[10, 20, 0] = np.inf
    ref[30, 7, 2] = -np.inf
    src[0, 0] = [np.nan, 2.0, -1.0]                                        # outside the mask: passes through
    A, t = fit(src, ref, mask, n_samples=600, seed=3)
    mask_one = np.zeros((H, W), bool)
    mask_one[5, 5] = True
    A_one, t_one = fit(src, ref, mask_one, n_samples=600, seed=3)
    At_hand = np.array([1.2, 0.0, 0.3, 0.0, 0.9, 0.0, -0.4, 0.0, 1.1, 0.0, 0.1, -0.3])
    Ah, th = At_hand[:9].reshape(3, 3), At_hand[9:]
    gray = np.repeat(src[..., :1], 3, axis=2).copy()
    ok = mask & np.isfinite(gray).all(axis=2) & np.isfinite(ref).all(axis=2)
    Xg = gray[ok].astype(np.float64)
    W_gray, *_ = np.linalg.lstsq(np.concatenate([Xg, np.ones((len(Xg), 1))], axis=1), ref[ok].astype(np.float64), rcond=None)
    out = dict(src=src, ref=ref, mask=mask, A=A, t=t, mask_one=mask_one, A_one=A_one, t_one=t_one, At_hand=At_hand,
               out_fit_mask=apply(src, A, t, mask), out_fit_nomask=apply(src, A, t), out_hand_mask=apply(src, Ah, th, mask),
               out_hand_nomask=apply(src, Ah, th), W_gray=W_gray)
    # what the fixture is there for
    assert 0.8 < mask.mean() < 0.9 and (src < 0).any() and (src > 1).any()
    assert np.array_equal(A_one, np.eye(3)) and not t_one.any() and A.shape == (3, 3) and t.shape == (3,)
    assert np.isnan(out["out_hand_mask"][10, 20]).any() and out["out_fit_mask"].dtype == np.float32
    assert np.isnan(out["out_fit_nomask"][0, 0]).all() and np.isnan(out["out_fit_mask"][0, 0, 0]) and out["out_fit_mask"][0, 0, 1] == 2.0
    assert np.linalg.matrix_rank(np.concatenate([Xg, np.ones((len(Xg), 1))], axis=1)) == 2
    print("mask", float(mask.mean()), "A", A, "t", t)
    path = os.path.join(HERE, "g17_affine.npz")
    np.savez_compressed(path, **out)
    print(f"g17_affine.npz  {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) <= 100 * 1024


if __name__ == "__main__":
    main()
