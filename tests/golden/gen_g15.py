"""Generate tests/golden/g15_scene_tiles.npz (build container only, with the reference present):

    python tests/golden/gen_g15.py

Fixture g15 pins s2_emit.scenes: the black-pixel scan, the window selection and the tile extraction of the reference's
tiles_helpers/utils.py.  ``is_black_mask`` (:201-220) runs from the reference file itself - ONE function node taken out by AST, as
the module imports rasterio - and the uint16 quantisation (:362-374) through oracle.ref_loader.load_tile_quantiser; none of their
text is stored here.  The window loop of find_valid_paired_tiles (:256-302) reads its tiles through rasterio and is restated.

Scenes (seeded):
    emit     (7, 37, 45) float32, nodata -9999: reflectance-like values with a nodata border, one window all -0.01, one all zero,
             and scattered pixels of every class the scan has to tell apart - each predicate true in every band / in all but the
             last / in all but the first, nodata and -0.01 mixed across bands, NaN, +-inf, and the float32 values next to both
             edges of every tolerance: (float)v +- tol and +-(float)1e-6, one ulp inside, on, and one ulp outside.
    u16      (4, 20, 26) uint16 over {0, 1, 2, 65535}, nodata 65535.
    s2       (3, 111, 135) uint16 = 3 x the emit scene's size, with zero patches of several sizes; the tests also use its
             (90, 110) corner, an S2 scene SMALLER than scale x EMIT, whose last window row and column are skipped.
Stored: the scenes; the packed black masks (emit with and without its nodata value, u16, s2) and the counts of the 8 x 8 (s2:
24 x 24) window grids; per setting k of SETTINGS the windows, the kept windows' indices and their black fractions; the quantised
EMIT tiles of setting 1.  NumPy 2.2.6.
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

BANDS, H, W, TILE, SCALE = 7, 37, 45, 8, 3
NODATA, MASKED, ATOL, ZERO = -9999.0, -0.01, 1e-3, 1e-6
# (S2 scene: "full" or "small", max_black_frac, max_tiles)
SETTINGS = [("full", 0.0, None), ("full", 0.1, None), ("full", 0.5, 3), ("full", 1.0, None), ("small", 0.1, None),
            ("small", 1.0, 5)]


def load_is_black_mask():
    path = os.path.join(ref_loader.REFERENCE_ROOT, "tiles_helpers", "utils.py")
    tree = ast.parse(open(path).read(), filename=path)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "is_black_mask")
    ns = {"np": np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["is_black_mask"]


def edge_values():
    """The float32 values next to every edge of the three tests."""
    out = []
    for v in (NODATA, MASKED):
        vf, tol = np.float32(v), np.float32(ATOL + 1e-5 * abs(v))
        for edge in (np.float32(vf + tol), np.float32(vf - tol)):
            out += [edge, np.nextafter(edge, np.float32(np.inf)), np.nextafter(edge, np.float32(-np.inf))]
    z = np.float32(ZERO)
    for edge in (z, -z):
        out += [edge, np.nextafter(edge, np.float32(np.inf)), np.nextafter(edge, np.float32(-np.inf))]
    return out


def emit_scene(rng):
    a = rng.uniform(0.02, 0.7, size=(BANDS, H, W)).astype(np.float32)
    a[:, :2, :] = NODATA                                   # a nodata border: rows 0-1, columns 43-44
    a[:, :, 43:] = NODATA
    a[:, 8:16, 16:24] = MASKED                             # window (1, 2) all masked
    a[:, 24:32, 0:8] = 0.0                                 # window (3, 0) all zero
    a[:, 34:, 5:20] = NODATA                               # black pixels below the last window row: never counted
    nd, mk, zr, ok = np.float32(NODATA), np.float32(MASKED), np.float32(0.0), np.float32(0.3)
    classes = [np.full(BANDS, v, np.float32) for v in (nd, mk, zr)]
    for v in (nd, mk, zr):
        last = np.full(BANDS, v, np.float32)
        last[-1] = ok
        first = np.full(BANDS, v, np.float32)
        first[0] = ok
        classes += [last, first]
    mixed = np.full(BANDS, nd, np.float32)
    mixed[1::2] = mk
    mixed2 = np.full(BANDS, mk, np.float32)
    mixed2[-1] = zr
    classes += [mixed, mixed2]
    for v in (np.nan, np.inf, -np.inf):
        classes.append(np.full(BANDS, v, np.float32))
        one = np.full(BANDS, nd, np.float32)
        one[3] = v
        classes.append(one)
    classes += [np.full(BANDS, v, np.float32) for v in edge_values()]
    # three pixels per class at scattered places of rows 2-23 (windows rows 0-2), columns 0-42; rows 16-23 keep columns 24+ clean
    spots = [(y, x) for y in range(2, 24) for x in range(0, 43) if not (8 <= y < 16 and 16 <= x < 24) and not (y >= 16 and x >= 24)]
    pick = rng.permutation(len(spots))[:3 * len(classes)]
    for k, s in enumerate(pick):
        y, x = spots[s]
        a[:, y, x] = classes[k % len(classes)]
    return a


def u16_scene(rng):
    a = rng.choice(np.array([0, 1, 2, 65535], np.uint16), size=(4, 20, 26), p=[0.45, 0.1, 0.05, 0.4])
    a[:, :4, :4] = 0
    a[:, 4:8, 8:12] = 65535
    a[:, 8:12, 12:16] = 1
    a[:, 16:, :] = 65535
    a[0, 17, 3] = 0
    return a


def s2_scene(rng):
    a = rng.integers(1, 3000, size=(3, H * SCALE, W * SCALE)).astype(np.uint16)
    a[:, 48:72, 0:24] = 0                                  # S2 window (2, 0) all zero
    a[:, 50:60, 30:40] = 0                                 # 100 of 576 pixels of window (2, 1)
    a[:, 72:96, 48:72] = 0                                 # window (3, 2)
    a[:, 80, 100:104] = 0                                  # 4 pixels of window (3, 4)
    a[:, 60:66, 110:118] = 0                               # 48 pixels of window (2, 4)
    a[0, 70, 75] = 0                                       # one band only: not black
    return a


def windows_of(h_e, w_e, h_s, w_s):
    """The reference's window loop (:256-277) as rows of [col_e, row_e, w, h, col_s, row_s, w_s, h_s]."""
    ts, out = TILE * SCALE, []
    for row_e in range(0, h_e - TILE + 1, TILE):
        for col_e in range(0, w_e - TILE + 1, TILE):
            row_s, col_s = row_e * SCALE, col_e * SCALE
            if row_s + ts > h_s or col_s + ts > w_s:
                continue
            out.append([col_e, row_e, TILE, TILE, col_s, row_s, ts, ts])
    return np.array(out, dtype=np.int32)


def counts_of(mask, t):
    ny, nx = mask.shape[0] // t, mask.shape[1] // t
    return mask[:ny * t, :nx * t].reshape(ny, t, nx, t).sum(axis=(1, 3)).astype(np.int32)


def main():
    assert ref_loader.available(), "reference tree not present"
    black = load_is_black_mask()
    quantise = ref_loader.load_tile_quantiser()
    rng = np.random.default_rng(15)
    emit, u16, s2 = emit_scene(rng), u16_scene(rng), s2_scene(rng)
    m_emit = black(emit, nodata=NODATA)
    m_emit0 = black(emit, nodata=None)
    m_u16 = black(u16, nodata=65535)
    m_u160 = black(u16, nodata=None)
    out = dict(emit=emit, u16=u16, s2=s2, nodata=np.float64(NODATA),
               mask_emit=np.packbits(m_emit), mask_emit_none=np.packbits(m_emit0), mask_u16=np.packbits(m_u16),
               mask_u16_none=np.packbits(m_u160), counts_emit=counts_of(m_emit, TILE), counts_emit_none=counts_of(m_emit0, TILE),
               counts_u16=counts_of(m_u16, 4), counts_u16_none=counts_of(m_u160, 4),
               settings=np.array([[s == "small", f, -1 if m is None else m] for s, f, m in SETTINGS], dtype=np.float64))
    print("emit black", m_emit.sum(), "without nodata", m_emit0.sum(), "u16 black", m_u16.sum(), "/", m_u160.sum())
    for name, scene in (("full", s2), ("small", s2[:, :90, :110])):
        m = black(scene, nodata=None)
        out[f"mask_s2_{name}"] = np.packbits(m)
        out[f"counts_s2_{name}"] = counts_of(m, TILE * SCALE)
        out[f"windows_{name}"] = windows_of(H, W, scene.shape[1], scene.shape[2])
    for k, (name, frac, max_tiles) in enumerate(SETTINGS):
        scene = s2 if name == "full" else s2[:, :90, :110]
        kept, fracs = [], []
        for i, (ce, re, we, he, cs, rs, ws, hs) in enumerate(out[f"windows_{name}"]):
            eb = black(emit[:, re:re + he, ce:ce + we], nodata=NODATA)        # :279-286 on the windows' arrays
            sb = black(scene[:, rs:rs + hs, cs:cs + ws], nodata=None)
            ef, sf = eb.sum() / eb.size, sb.sum() / sb.size
            if ef <= frac and sf <= frac:
                kept.append(i)
                fracs.append((ef, sf))
                if max_tiles is not None and len(kept) >= max_tiles:
                    break
        out[f"kept_{k}"] = np.array(kept, dtype=np.int32)
        out[f"fracs_{k}"] = np.array(fracs, dtype=np.float64).reshape(-1, 2)
        print(f"setting {k} {name} frac {frac} max {max_tiles}: kept {kept}")
    wins = out["windows_full"][out["kept_1"]]
    out["emit_u16_tiles_1"] = np.stack([quantise(emit[:, re:re + he, ce:ce + we], src_nodata=NODATA)
                                        for ce, re, we, he, *_ in wins])
    path = os.path.join(HERE, "g15_scene_tiles.npz")
    np.savez_compressed(path, **out)
    print(f"g15_scene_tiles.npz  {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) <= 800 * 1024


if __name__ == "__main__":
    main()
