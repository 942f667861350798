"""Generate tests/golden/g16_ortho.npz (build container only, with the reference present):

    python tests/golden/gen_g16.py

Fixture g16 pins s2_emit.ortho: the geometry-lookup-table gather of an EMIT swath with its quality and band masks.
``apply_glt`` (EMIT_data/emit_tools.py:153-181) runs from the reference file itself - ONE function node taken out by AST, as the
module imports netCDF4, xarray and s3fs - and none of its text is stored here.  RESTATED, because they sit inside I/O code:
    the GLT build          np.nan_to_num(np.stack([glt_x, glt_y], axis=-1), nan=0).astype(int)     (emit_tools.py:199-201,
                           emit_proj.py:683-687), here ``build_glt``;
    the mask statements    data[qmask == 1] = -9999; data[unpacked_bmask == 1] = -9999              (emit_tools.py:115-119) and
                           np.unpackbits(bmask, axis=-1)[:, :, 0:285]                               (:317-319), here ``masked_swath``;
    quality_mask's lines   np.sum(mask[:, :, quality_bands], axis=-1); qmask[qmask > 1] = 1         (:296-297);
    the in-bounds rule     valid & (0 <= glt - 1 < raw shape), dropped = valid - kept               (emit_proj.py:691-717), here
                           ``drop_out_of_bounds``: the entries it drops are set to no data BEFORE apply_glt sees them (apply_glt
                           alone would raise or wrap); the decrement is done in int64 so that INT32_MIN cannot wrap.

Contents (seeded):
    swath285 (6, 5, 285), swath3 (6, 5, 3) float32: values over the whole range from a pool of random bit patterns - NaN with
             payloads, +-inf, -0.0, denormals among them.
    glt_x, glt_y (9, 11) float64 with NaN -> glt_mixed: no data in x only, in y only and in both; many cells on one swath pixel;
             swath pixels that no cell references.  glt_nodata (all 0), glt_valid (every cell valid), glt_drop = glt_mixed with
             entries cols + 1, rows + 1, negatives, INT32_MAX and INT32_MIN.
    qmask    (6, 5) uint8 over {0, 1, 2, 255};  bmask (6, 5, 36) uint8, bits at bands 0, 7, 8, 15, 283, 284 and the pad bits
             285-287;  mask_cube (6, 5, 8), quality_bands -> qmask_cube.
Stored: the inputs; apply_glt's result for swath285 on glt_mixed with no mask / qmask / band mask / both, on glt_nodata,
glt_valid and glt_drop (with its dropped count), for swath3 on glt_mixed with no mask and with qmask; two windows of glt_drop
(both masks) with their dropped counts.  NumPy 2.2.6.
"""
from __future__ import annotations

import ast
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_loader                                         # noqa: E402

warnings.simplefilter("ignore")

ROWS, COLS, GH, GW, BMASK_BYTES = 6, 5, 9, 11, 36
I32_MAX, I32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min
MASK_BITS = (0, 7, 8, 15, 283, 284, 285, 286, 287)
WINDOWS = np.array([[1, 2, 5, 7], [8, 10, 1, 1]], np.int32)           # row_off, col_off, height, width
SPECIAL_BITS = [0x7fc00000, 0x7fc12345, 0xffc00001, 0x7f800001, 0x7f800000, 0xff800000, 0x80000000, 0x00000000, 0x00000001,
                0x80000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0xff7fffff]


def load_apply_glt():
    path = os.path.join(ref_loader.REFERENCE_ROOT, "EMIT_data", "emit_tools.py")
    tree = ast.parse(open(path).read(), filename=path)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "apply_glt")
    ns = {"np": np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["apply_glt"]


def swath(rng, bands):
    """Values from a pool of 4096 random bit patterns and the special ones, -9999 and 0.25 (the pool keeps the file small)."""
    pool = np.concatenate([rng.integers(0, 1 << 32, 4096 - len(SPECIAL_BITS) - 2, dtype=np.uint64).astype(np.uint32),
                           np.array(SPECIAL_BITS, np.uint32), np.array([-9999.0, 0.25], np.float32).view(np.uint32)])
    bits = pool[rng.integers(0, len(pool), (ROWS, COLS, bands))]
    bits[0, 0, :len(SPECIAL_BITS)] = np.array(SPECIAL_BITS, np.uint32)[:bands]
    return bits.view(np.float32)


def glt_xy(rng):
    """One-based columns (x) and rows (y) as the netCDF stores them: float64, NaN where there is no data."""
    x = rng.integers(1, COLS + 1, (GH, GW)).astype(np.float64)
    y = rng.integers(1, ROWS + 1, (GH, GW)).astype(np.float64)
    x[2:5, 3:7], y[2:5, 3:7] = 2.0, 3.0                  # twelve cells on swath pixel (row 2, col 1)
    ref = (y == 6.0) & (x == 5.0)                         # the last swath pixel: referenced by no cell
    x[ref] = 4.0
    x[0, 0:3] = np.nan                                    # x only
    y[1, 4:6] = np.nan                                    # y only
    x[8, 8:], y[8, 8:] = np.nan, np.nan                   # both
    x[0, 10], y[0, 10] = 5.0, 1.0                         # corners of the swath
    x[8, 0], y[8, 0] = 1.0, 6.0
    x[7, 5], y[7, 5] = 1.0, 1.0                           # swath pixel (0, 0): the special values
    return x, y


def build_glt(glt_x, glt_y):
    return np.nan_to_num(np.stack([glt_x, glt_y], axis=-1), nan=0).astype(int).astype(np.int32)


def drop_grid(glt):
    g = glt.copy()
    g[3, 0] = (COLS + 1, 2)
    g[3, 1] = (2, ROWS + 1)
    g[3, 2] = (-1, 2)
    g[4, 0] = (2, -3)
    g[4, 1] = (I32_MAX, 1)
    g[4, 2] = (1, I32_MAX)
    g[5, 0] = (I32_MIN, 1)
    g[5, 1] = (1, I32_MIN)
    g[5, 2] = (I32_MIN, I32_MAX)
    g[6, 0] = (COLS + 1, 0)                               # out of bounds in x, no data in y: no data, not dropped
    g[8, 10] = (COLS + 1, ROWS + 1)                       # the cell of the 1 x 1 window
    g[1, 2] = (COLS, ROWS)                                # the last swath pixel, in bounds
    return g


def masked_swath(data, qmask, bmask):
    out = data.copy()
    if qmask is not None:
        out[qmask == 1] = -9999
    if bmask is not None:
        unpacked = np.unpackbits(bmask, axis=-1)[:, :, 0:285][:, :, :data.shape[-1]]
        out[unpacked == 1] = -9999
    return out


def drop_out_of_bounds(glt, raw_h, raw_w):
    """-> (the table with the dropped entries set to no data, dropped)."""
    valid = np.all(glt != 0, axis=-1)
    glt0 = glt.astype(np.int64)
    glt0[valid] -= 1
    in_bounds = (glt0[..., 1] >= 0) & (glt0[..., 1] < raw_h) & (glt0[..., 0] >= 0) & (glt0[..., 0] < raw_w)
    valid2 = valid & in_bounds
    kept = glt.copy()
    kept[valid & ~in_bounds] = 0
    return kept, int(np.count_nonzero(valid) - np.count_nonzero(valid2))


def main():
    assert ref_loader.available(), "reference tree not present"
    apply_glt = load_apply_glt()
    rng = np.random.default_rng(16)
    s285, s3 = swath(rng, 285), swath(rng, 3)
    glt_x, glt_y = glt_xy(rng)
    mixed = build_glt(glt_x, glt_y)
    nodata_grid = np.zeros((GH, GW, 2), np.int32)
    valid_grid = np.stack([rng.integers(1, COLS + 1, (GH, GW)), rng.integers(1, ROWS + 1, (GH, GW))], axis=-1).astype(np.int32)
    drop = drop_grid(mixed)
    qmask = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=(ROWS, COLS), p=[0.4, 0.3, 0.15, 0.15])
    qmask[2, 1], qmask[0, 0] = 1, 0
    unpacked = np.zeros((ROWS, COLS, BMASK_BYTES * 8), np.uint8)
    for i, b in enumerate(MASK_BITS):
        unpacked[:, :, b] = rng.random((ROWS, COLS)) < (0.5 if b < 285 else 0.8)
        unpacked[i % ROWS, i % COLS, b] = 1
    unpacked[0, 0, :] = 0
    unpacked[5, 3, :] = 1                                                  # a pixel with every bit set, the pad bits too
    bmask = np.packbits(unpacked, axis=-1)
    cube = (rng.random((ROWS, COLS, 8)) < 0.3).astype(np.float32)
    cube[:, :, 5] = rng.random((ROWS, COLS)).astype(np.float32)           # a data band
    quality_bands = np.array([0, 1, 3, 4], np.int64)
    qmask_cube = np.sum(cube[:, :, quality_bands], axis=-1)
    qmask_cube[qmask_cube > 1] = 1

    out = dict(swath285=s285, swath3=s3, glt_x=glt_x, glt_y=glt_y, glt_mixed=mixed, glt_nodata=nodata_grid, glt_valid=valid_grid,
               glt_drop=drop, qmask=qmask, bmask=bmask, mask_cube=cube, quality_bands=quality_bands, qmask_cube=qmask_cube,
               windows=WINDOWS)
    for tag, q, b in (("plain", None, None), ("q", qmask, None), ("b", None, bmask), ("qb", qmask, bmask)):
        out[f"out285_{tag}"] = apply_glt(masked_swath(s285, q, b), mixed)
    out["out3_plain"] = apply_glt(s3, mixed)
    out["out3_q"] = apply_glt(masked_swath(s3, qmask, None), mixed)
    out["out285_nodata"] = apply_glt(s285, nodata_grid)
    out["out285_valid"] = apply_glt(s285, valid_grid)
    kept, dropped = drop_out_of_bounds(drop, ROWS, COLS)
    out["out285_drop"], out["dropped_drop"] = apply_glt(s285, kept), np.int64(dropped)
    both = masked_swath(s285, qmask, bmask)
    for k, (r0, c0, h, w) in enumerate(WINDOWS):
        kept, dropped = drop_out_of_bounds(drop[r0:r0 + h, c0:c0 + w], ROWS, COLS)
        out[f"out285_win{k}"], out[f"dropped_win{k}"] = apply_glt(both, kept), np.int64(dropped)
    # what the fixture is there for
    assert np.isnan(glt_x).any() and (np.isnan(glt_x) != np.isnan(glt_y)).any() and (np.isnan(glt_x) & np.isnan(glt_y)).any()
    v = np.all(mixed != 0, axis=-1)
    used = set(map(tuple, mixed[v][:, ::-1] - 1))
    assert len(used) < ROWS * COLS and ((mixed[..., 0] == 2) & (mixed[..., 1] == 3)).sum() >= 12
    assert out["dropped_drop"] == 10 and out["dropped_win1"] == 1 and out["dropped_win0"] > 0
    assert out["out285_plain"].dtype == np.float32 and out["out285_plain"].shape == (GH, GW, 285)
    bits = out["out285_plain"].view(np.uint32)
    assert all((bits == s).any() for s in SPECIAL_BITS), "a special value is referenced by no cell"
    assert set(np.unique(qmask)) == {0, 1, 2, 255}
    assert (out["out285_q"].view(np.uint32) != bits).any() and (out["out285_b"].view(np.uint32) != bits).any()
    print("valid cells", int(v.sum()), "of", GH * GW, "; swath pixels referenced", len(used), "of", ROWS * COLS,
          "; dropped", int(out["dropped_drop"]), int(out["dropped_win0"]), int(out["dropped_win1"]))
    path = os.path.join(HERE, "g16_ortho.npz")
    np.savez_compressed(path, **out)
    print(f"g16_ortho.npz  {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) <= 800 * 1024


if __name__ == "__main__":
    main()
