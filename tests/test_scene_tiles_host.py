"""s2_emit.scenes on the host side: the window loop and the selection against fixture g15 (the reference's is_black_mask and its
restated loop), the float32 / float64 restatement of np.isclose's arithmetic that the GPU tests reuse, every argument check that
needs no GPU, and the declaration and registration of the new exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("hsr_scene_black_counts", "hsr_scene_gather_tiles", "hsr_scene_mosaic")
NEW_NAMES = ("find_valid_paired_tiles", "extract_tile_pairs", "mosaic_tiles", "fuse_scene", "scene_windows", "select_tiles", "Window",
             "SceneOutput")
TILE, SCALE = 8, 3                     # g15's grid


def black_rule(arr, nodata=None, masked_val=-0.01, nodata_atol=1e-3, zero_atol=1e-6):
    """is_black_mask's arithmetic spelled out, as NumPy 2 evaluates np.isclose(arr, v, atol=a) with v a Python float: float32 arrays
    wholly in float32 (|x - (float)v| <= (float)(a + 1e-5 |v|) & isfinite(v) | x == (float)v, |x| < (float)zero_atol), integer
    arrays in float64."""
    ft = np.float32 if arr.dtype == np.float32 else np.float64
    x = arr.astype(ft, copy=False)

    def close(v):
        with np.errstate(invalid="ignore"):
            return (np.abs(x - ft(v)) <= ft(nodata_atol + 1e-5 * abs(v))) & np.isfinite(v) | (x == ft(v))

    out = close(masked_val).all(0) | (np.abs(x) < ft(zero_atol)).all(0)
    return out | close(nodata).all(0) if nodata is not None else out


def window_counts(mask, th, tw):
    ny, nx = mask.shape[0] // th, mask.shape[1] // tw
    return mask[:ny * th, :nx * tw].reshape(ny, th, nx, tw).sum(axis=(1, 3)).astype(np.int32)


def g15_mask(g, key, shape):
    return np.unpackbits(g[key])[:shape[0] * shape[1]].reshape(shape).astype(bool)


def g15_settings(g):
    """(k, S2 scene, its name, max_black_frac, max_tiles) of every setting of the fixture."""
    for k, (small, frac, mt) in enumerate(g["settings"]):
        s2 = g["s2"][:, :90, :110] if small else g["s2"]
        yield k, s2, "small" if small else "full", float(frac), None if mt < 0 else int(mt)


@pytest.fixture(scope="module")
def g15():
    return load_golden("g15_scene_tiles")


def test_scene_windows_and_select_tiles_against_g15(g15):
    from s2_emit import scenes
    g = g15
    _, he, we = g["emit"].shape
    for k, s2, name, frac, max_tiles in g15_settings(g):
        windows = scenes.scene_windows(he, we, s2.shape[1], s2.shape[2], TILE, SCALE)
        flat = np.array([tuple(we_) + tuple(ws_) for we_, ws_ in windows], dtype=np.int32)
        np.testing.assert_array_equal(flat, g[f"windows_{name}"])
        tiles = scenes.select_tiles(windows, g["counts_emit"], g[f"counts_s2_{name}"], TILE, SCALE, frac, max_tiles)
        kept = g[f"kept_{k}"]
        assert [t["idx"] for t in tiles] == list(range(len(kept)))
        assert [windows.index((t["emit_window"], t["s2_window"])) for t in tiles] == kept.tolist()
        fr = np.array([(t["emit_black_frac"], t["s2_black_frac"]) for t in tiles], dtype=np.float64).reshape(-1, 2)
        np.testing.assert_array_equal(fr, g[f"fracs_{k}"])
    assert len(g["windows_small"]) < len(g["windows_full"]) == 20


def test_black_rule_restatement_against_g15(g15):
    """The rule the scan kernel implements and the reference-sized GPU case is compared with, against is_black_mask itself."""
    g = g15
    nd = float(g["nodata"])
    for key, arr, nodata in (("mask_emit", g["emit"], nd), ("mask_emit_none", g["emit"], None), ("mask_u16", g["u16"], 65535),
                             ("mask_u16_none", g["u16"], None), ("mask_s2_full", g["s2"], None)):
        want = g15_mask(g, key, arr.shape[1:])
        np.testing.assert_array_equal(black_rule(arr, nodata), want, err_msg=key)
    want = g15_mask(g, "mask_emit", g["emit"].shape[1:])
    np.testing.assert_array_equal(window_counts(want, TILE, TILE), g["counts_emit"])
    assert 0 < want.sum() < want.size and g15_mask(g, "mask_emit_none", want.shape).sum() < want.sum()


def _tile(r, c, t=TILE, s=SCALE):
    from s2_emit.scenes import Window
    return {"idx": 0, "emit_window": Window(c, r, t, t), "s2_window": Window(c * s, r * s, t * s, t * s)}


def test_argument_checks_need_no_gpu():
    """Every shape, dtype and range error is raised before any GPU work (this machine has none)."""
    import s2_emit
    from s2_emit import scenes
    e = np.zeros((7, 37, 45), np.float32)
    s = np.zeros((3, 111, 135), np.uint16)
    bad = [
        (lambda: s2_emit.find_valid_paired_tiles(e, s, 38, SCALE), "larger than"),
        (lambda: s2_emit.find_valid_paired_tiles(e, s, 0, SCALE), "emit_tile_size"),
        (lambda: s2_emit.find_valid_paired_tiles(e, s, TILE, 0), "scale"),
        (lambda: s2_emit.find_valid_paired_tiles(e, s, TILE, 2.5), "scale"),
        (lambda: s2_emit.find_valid_paired_tiles(e.astype(np.float64), s, TILE, SCALE), "uint16 or float32"),
        (lambda: s2_emit.find_valid_paired_tiles(e, s.astype(np.int32), TILE, SCALE), "uint16 or float32"),
        (lambda: s2_emit.find_valid_paired_tiles(e[0], s, TILE, SCALE), "(bands, H, W)"),
        (lambda: s2_emit.find_valid_paired_tiles(e, s, TILE, SCALE, max_tiles=0), "max_tiles"),
        (lambda: s2_emit.find_valid_paired_tiles(e, s, TILE, SCALE, max_black_frac="x"), "max_black_frac"),
        (lambda: s2_emit.find_valid_paired_tiles(e, s, TILE, SCALE, emit_nodata="x"), "emit_nodata"),
        (lambda: scenes.scene_windows(37, 45, 111, 135, 46, 3), "larger than"),
        (lambda: scenes.select_tiles(scenes.scene_windows(37, 45, 111, 135, TILE, SCALE), np.zeros((2, 2), np.int32),
                                     np.zeros((4, 5), np.int32), TILE, SCALE), "not a window"),
        (lambda: scenes.select_tiles([], np.zeros((4, 5)), np.zeros((4, 5), np.int32), TILE, SCALE), "integer arrays"),
        (lambda: s2_emit.extract_tile_pairs(e, s, []), "non-empty list"),
        (lambda: s2_emit.extract_tile_pairs(e, s, [_tile(32, 0)]), "outside"),
        (lambda: s2_emit.extract_tile_pairs(e, s, [_tile(0, 40)]), "outside"),
        (lambda: s2_emit.extract_tile_pairs(e, s, [_tile(0, 0), _tile(8, 8, t=4)]), "share one size"),
        (lambda: s2_emit.extract_tile_pairs(e, s, [{"idx": 0}]), "emit_window"),
        (lambda: s2_emit.extract_tile_pairs(e.astype(np.float64), s, [_tile(0, 0)]), "uint16 or float32"),
        (lambda: s2_emit.extract_tile_pairs(e, s, [_tile(0, 0)], emit_nodata_u16=70000), "emit_nodata_u16"),
        (lambda: s2_emit.mosaic_tiles(np.zeros((2, 4, 24, 24), np.float32), [_tile(0, 0)], (111, 135)), "2 cubes"),
        (lambda: s2_emit.mosaic_tiles(np.zeros((1, 4, 24, 24), np.float64), [_tile(0, 0)], (111, 135)), "float32"),
        (lambda: s2_emit.mosaic_tiles(np.zeros((1, 4, 12, 24), np.float32), [_tile(0, 0)], (111, 135)), "the cubes are"),
        (lambda: s2_emit.mosaic_tiles(np.zeros((1, 4, 24, 24), np.float32), [_tile(0, 0)], (20, 135)), "outside"),
        (lambda: s2_emit.mosaic_tiles(np.zeros((2, 4, 24, 24), np.float32), [_tile(0, 0), _tile(0, 0)], (111, 135)), "share"),
        (lambda: s2_emit.mosaic_tiles(np.zeros((1, 4, 24, 24), np.float32),
                                      [{"s2_window": scenes.Window(5, 0, 24, 24)}], (111, 135)), "not on the"),
        (lambda: s2_emit.fuse_scene(e, s, tile=38, factor=SCALE), "larger than"),
        (lambda: s2_emit.fuse_scene(e, s, tile=TILE, factor=0), "scale"),
        (lambda: s2_emit.fuse_scene(e, s, tile=TILE, factor=SCALE, bands=8), "bands"),          # the scene has 7
        (lambda: s2_emit.fuse_scene(e, np.zeros((17, 111, 135), np.uint16), tile=TILE, factor=SCALE, bands=4), "17 bands"),
        (lambda: s2_emit.fuse_scene(e, s, tile=TILE, factor=SCALE, bands=4, degree=4), "degree"),
        (lambda: s2_emit.fuse_scene(e, s, tile=TILE, factor=SCALE, bands=4, batch=0), "batch"),
        (lambda: s2_emit.fuse_scene(e.astype(np.float16), s, tile=TILE, factor=SCALE, bands=4), "uint16 or float32"),
    ]
    for call, text in bad:
        with pytest.raises(ValueError) as err:
            call()
        assert text in str(err.value), (text, str(err.value))
    # an S2 scene too small for a single window pair: an empty list, and no GPU is asked for
    assert s2_emit.find_valid_paired_tiles(e, s[:, :20, :20], TILE, SCALE) == []


def test_c_entry_points_refuse_bad_arguments():
    """HSR_REQUIRE comes before any HIP call, so the refusals and their error text are reachable without a GPU."""
    from s2_emit import _native as nat
    lib = nat.load()
    p, st = C.c_void_p(64), C.c_void_p(0)

    def refused(rc, text):
        assert rc != 0 and text in lib.hsr_last_error().decode(), (rc, lib.hsr_last_error())

    refused(lib.hsr_scene_gather_tiles(p, 2, 3, 10, 10, p, 1, 2, 2, 1, 1e4, 0, 0.0, 65535, p, st), "encode quantises float32")
    refused(lib.hsr_scene_gather_tiles(p, 0, 3, 10, 10, p, 1, 2, 2, 1, 1e4, 0, 0.0, 0, p, st), "nodata_u16")
    refused(lib.hsr_scene_gather_tiles(p, 1, 3, 10, 10, p, 1, 2, 2, 0, 1e4, 0, 0.0, 65535, p, st), "dtype=1")
    refused(lib.hsr_scene_gather_tiles(p, 0, 3, 10, 10, p, 1, 11, 2, 0, 1e4, 0, 0.0, 65535, p, st), "bad shape")
    refused(lib.hsr_scene_gather_tiles(p, 0, 3, 10, 10, None, 1, 2, 2, 0, 1e4, 0, 0.0, 65535, p, st), "NULL")
    refused(lib.hsr_scene_black_counts(p, 0, 3, 10, 10, 11, 2, 0, 0.0, -0.01, 1e-3, 1e-6, p, st), "bad shape")
    refused(lib.hsr_scene_black_counts(p, 3, 3, 10, 10, 2, 2, 0, 0.0, -0.01, 1e-3, 1e-6, p, st), "dtype=3")
    refused(lib.hsr_scene_black_counts(p, 0, 3, 10, 10, 2, 2, 0, 0.0, -0.01, 1e-3, 1e-6, None, st), "NULL")
    refused(lib.hsr_scene_mosaic(p, 1, 3, 4, 4, p, 10, 10, p, 3, 2, 0.0, 1, st), "bad shape")
    refused(lib.hsr_scene_mosaic(None, 1, 3, 4, 4, p, 10, 10, p, 2, 2, 0.0, 1, st), "NULL")
    refused(lib.hsr_scene_mosaic(p, 1, 0, 4, 4, p, 10, 10, p, 2, 2, 0.0, 1, st), "bad shape")


def test_exports_declared_registered_and_additive():
    import s2_emit
    from s2_emit import _native as nat
    lib = nat.load()
    text = open(os.path.join(ROOT, "include", "hsr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/hsr.h"
        assert name in nat.SIGNATURES, f"{name} has no ctypes signature"
        assert name in comments, f"{name} is not documented in include/hsr.h"
    assert [len(nat.SIGNATURES[n][1]) for n in NEW_EXPORTS] == [14, 16, 14]
    # purely additive: the ABI version and both launch records are what they were
    assert lib.hsr_abi_version() == 5 == nat.HSR_ABI_VERSION
    assert lib.hsr_aux_instance_count() == 32 and lib.hsr_k4_instance_count() == 31
    for name in NEW_NAMES:
        assert name in s2_emit.__all__ and hasattr(s2_emit, name), name
    assert s2_emit.__all__[:13] == s2_emit._REFERENCE_SURFACE and len(set(s2_emit.__all__)) == len(s2_emit.__all__)
    assert s2_emit.Window._fields == ("col_off", "row_off", "width", "height")
    assert s2_emit.SceneOutput._fields == ("cube", "tiles", "n_train", "status", "bands")
