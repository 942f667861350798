"""Overlapping windows and the feathered mosaic on the host side: the strided window walk and the selection on cell counts against
direct implementations, the blend plan (lattice pitch, start table, refusals), the stack-size arithmetic, every refusal of
hsr_scene_mosaic_blend, its declaration and registration - and the float64 restatement of its definition that the GPU tests
compare the kernel with."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORT = "hsr_scene_mosaic_blend"


# ---- the definition of hsr_scene_mosaic_blend (include/hsr.h) in float64 -----------------------------------------------------------
def tent(n):
    r = np.arange(n)
    return np.minimum(r + 1, n - r).astype(np.float64)


def blend_ref64(cubes, start, sy, sx, H, W):
    """cubes (P, T, th, tw) float32, start (ny, nx) -> a dict of (T, H, W) arrays: ``mean`` = sum w v / sum w in float64 (NaN where
    n == 0), ``absmean`` = sum w |v| / sum w, ``n`` the values that are not NaN, ``cover`` the cubes over the pixel, ``one`` the
    bits of the value the kernel has to COPY where n <= 1: the one value that is not NaN, or - n == 0 - the contributor visited
    last.  The cells are walked in ascending start row, then ascending start column: every pixel's visiting order."""
    P, T, th, tw = cubes.shape
    w = np.outer(tent(th), tent(tw))
    num, den, absnum = (np.zeros((T, H, W)) for _ in range(3))
    n, cover = np.zeros((T, H, W), np.int64), np.zeros((T, H, W), np.int64)
    one = np.zeros((T, H, W), np.uint32)
    for j in range(start.shape[0]):
        for i in range(start.shape[1]):
            e = int(start[j, i])
            if e < 0 or e >= P or j * sy + th > H or i * sx + tw > W:
                continue
            win = (slice(None), slice(j * sy, j * sy + th), slice(i * sx, i * sx + tw))
            v = cubes[e]
            ok = ~np.isnan(v)
            v64 = np.where(ok, v, 0.0).astype(np.float64)
            one[win] = np.where(ok | (n[win] == 0), v.view(np.uint32), one[win])
            num[win] += ok * w * v64
            absnum[win] += ok * w * np.abs(v64)
            den[win] += ok * w
            n[win] += ok
            cover[win] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        return dict(mean=num / den, absmean=absnum / den, n=n, cover=cover, one=one)


def check_blend(got, ref, K, fill):
    """The whole contract on one result: ``fill``'s bits where nothing covers, the copied bits where n <= 1, NaN exactly where a
    covered element has n == 0, and |got - mean| <= (K + 2) 2^-24 sum w |v| / sum w everywhere else (at most K roundings of a
    running sum that never exceeds sum w |v|, the division's and one spare; the weights and their sum are exact).  Returns the
    largest error over the bound."""
    bits = np.ascontiguousarray(got).view(np.uint32)
    n, cover = ref["n"], ref["cover"]
    np.testing.assert_array_equal(bits[cover == 0], np.full(int((cover == 0).sum()), np.float32(fill).view(np.uint32)))
    copied = (cover > 0) & (n <= 1)
    np.testing.assert_array_equal(bits[copied], ref["one"][copied])
    np.testing.assert_array_equal(np.isnan(got)[cover > 0], (n == 0)[cover > 0])
    many = n >= 2
    err = np.abs(got[many].astype(np.float64) - ref["mean"][many])
    bound = (K + 2) * 2.0 ** -24 * ref["absmean"][many]
    assert (err <= bound).all(), (float(err.max()), float((err / np.maximum(bound, 1e-300)).max()))
    return float((err / np.maximum(bound, 1e-300)).max()) if many.any() else 0.0


# ---- the window walk with a stride ------------------------------------------------------------------------------------------------
HE, WE, HS, WS, TILE, SCALE = 43, 62, 258, 372, 20, 6


def test_scene_windows_with_a_stride():
    from s2_emit import scenes
    plain = scenes.scene_windows(HE, WE, HS, WS, TILE, SCALE)
    assert scenes.scene_windows(HE, WE, HS, WS, TILE, SCALE, stride=None) == plain
    assert scenes.scene_windows(HE, WE, HS, WS, TILE, SCALE, stride=TILE) == plain and len(plain) == 6
    for s in (20, 10, 5, 4):
        want = []
        for r in range(0, HE - TILE + 1, s):
            for c in range(0, WE - TILE + 1, s):
                if (r + TILE) * SCALE <= HS and (c + TILE) * SCALE <= WS:
                    want.append((scenes.Window(c, r, TILE, TILE), scenes.Window(c * SCALE, r * SCALE, TILE * SCALE, TILE * SCALE)))
        assert scenes.scene_windows(HE, WE, HS, WS, TILE, SCALE, stride=s) == want
    assert len(scenes.scene_windows(HE, WE, HS, WS, TILE, SCALE, stride=10)) == 15
    # an S2 scene one pixel short of the last window row: those pairs are skipped, as in the plain walk
    assert len(scenes.scene_windows(HE, WE, 40 * SCALE - 1, WS, TILE, SCALE, stride=10)) == 10
    for bad in (7, 0, 21, -10, 2.5, True):
        with pytest.raises(ValueError, match="stride"):
            scenes.scene_windows(HE, WE, HS, WS, TILE, SCALE, stride=bad)


def test_select_tiles_on_cell_counts():
    """Random black masks: the cell sums of a window are its own count, so fractions, idx and max_tiles equal a direct walk."""
    from s2_emit import scenes
    rng = np.random.default_rng(5)
    for s in (20, 10, 5, 4):
        me, ms = rng.random((HE, WE)) < 0.02, rng.random((HS, WS)) < 0.02
        me[:14, 30:], ms[150:, :130] = True, True
        cs = s * SCALE
        ec = me[:HE // s * s, :WE // s * s].reshape(HE // s, s, WE // s, s).sum(axis=(1, 3)).astype(np.int32)
        sc = ms[:HS // cs * cs, :WS // cs * cs].reshape(HS // cs, cs, WS // cs, cs).sum(axis=(1, 3)).astype(np.int32)
        windows = scenes.scene_windows(HE, WE, HS, WS, TILE, SCALE, stride=s)
        for frac, max_tiles in ((0.0, None), (0.05, None), (0.3, None), (0.3, 3), (1.0, None)):
            want = []
            for we, ws in windows:
                ne = int(me[we.row_off:we.row_off + TILE, we.col_off:we.col_off + TILE].sum())
                ns = int(ms[ws.row_off:ws.row_off + TILE * SCALE, ws.col_off:ws.col_off + TILE * SCALE].sum())
                fe, fs = ne / (TILE * TILE), ns / (TILE * SCALE * TILE * SCALE)
                if fe <= frac and fs <= frac and (max_tiles is None or len(want) < max_tiles):
                    want.append({"idx": len(want), "emit_window": we, "s2_window": ws, "emit_black_frac": fe, "s2_black_frac": fs})
            got = scenes.select_tiles(windows, ec, sc, TILE, SCALE, frac, max_tiles, stride=s)
            assert got == want, (s, frac, max_tiles)
        assert 0 < len(scenes.select_tiles(windows, ec, sc, TILE, SCALE, 0.3, stride=s)) < len(windows)
    # stride=None and stride=tile read the same window counts
    plain = scenes.scene_windows(HE, WE, HS, WS, TILE, SCALE)
    ec, sc = rng.integers(0, 3, (2, 3)).astype(np.int32), rng.integers(0, 3, (2, 3)).astype(np.int32)
    assert scenes.select_tiles(plain, ec, sc, TILE, SCALE, 0.0025, stride=TILE) == scenes.select_tiles(plain, ec, sc, TILE, SCALE, 0.0025)
    off =[(scenes.Window(5, 0, TILE, TILE), scenes.Window(30, 0, TILE * SCALE, TILE * SCALE))]      # column 5 is on no cell of 10
    with pytest.raises(ValueError, match="not a window"):
        scenes.select_tiles(off, np.zeros((4, 6), np.int32), np.zeros((4, 6), np.int32), TILE, SCALE, stride=10)
    last = [(scenes.Window(50, 30, TILE, TILE), scenes.Window(300, 180, TILE * SCALE, TILE * SCALE))]   # its second cell row is missing
    with pytest.raises(ValueError, match="not a window"):
        scenes.select_tiles(last, np.zeros((4, 6), np.int32), np.zeros((4, 6), np.int32), TILE, SCALE, stride=10)
    with pytest.raises(ValueError, match="stride"):
        scenes.select_tiles([], np.zeros((4, 6), np.int32), np.zeros((4, 6), np.int32), TILE, SCALE, stride=7)


# ---- the blend plan ---------------------------------------------------------------------------------------------------------------
def _tiles(origins, th, tw):
    from s2_emit.scenes import Window
    return [{"s2_window": Window(c, r, tw, th)} for r, c in origins]


def test_plan_blend():
    from s2_emit import scenes
    org = [(8, 4), (0, 0), (4, 12), (12, 28)]
    start, sy, sx, H, W, th, tw = scenes._plan_blend((4, 3, 8, 8), "float32", _tiles(org, 8, 8), (23, 36))
    assert (sy, sx, H, W, th, tw) == (4, 4, 23, 36, 8, 8) and start.dtype == np.int32 and start.shape == (4, 8)
    want = np.full((4, 8), -1, np.int32)
    want[2, 1], want[0, 0], want[1, 3], want[3, 7] = 0, 1, 2, 3
    np.testing.assert_array_equal(start, want)
    # the pitch is the largest that divides the tile and every origin: rows 0 and 6 of 6-row tiles -> 6; columns 0, 2, 8 -> 2
    start, sy, sx, *_ = scenes._plan_blend((3, 1, 6, 6), "float32", _tiles([(0, 0), (6, 2), (0, 8)], 6, 6), (23, 31))
    assert (sy, sx) == (6, 2) and start.shape == (3, 13) and start[1, 1] == 1 and start[0, 4] == 2
    # tiles on the plain grid: one window over every pixel
    _, sy, sx, *_ = scenes._plan_blend((2, 1, 6, 8), "float32", _tiles([(6, 16), (12, 0)], 6, 8), (23, 36))
    assert (sy, sx) == (6, 8)
    def big():                         # two 4096 x 4096 tiles at half stride: the weights of a pixel add up to 2^24 at most
        return scenes._plan_blend((2, 1, 4096, 4096), "float32", _tiles([(0, 0), (2048, 2048)], 4096, 4096), (8192, 8192))

    bad = [
        (lambda: scenes._plan_blend((2, 3, 8, 8), "float32", _tiles([(4, 4), (4, 4)], 8, 8), (23, 36)), "share"),
        (lambda: scenes._plan_blend((2, 3, 8, 8), "float32", _tiles([(0, 0), (1, 1)], 8, 8), (23, 36)), "8 x 8 = 64 windows"),
        (lambda: scenes._plan_blend((2, 3, 8, 12), "float32", _tiles([(0, 0), (2, 2)], 8, 12), (30, 37)), "4 x 6 = 24 windows"),
        (lambda: scenes._plan_blend((1, 3, 8, 8), "float32", _tiles([(16, 0)], 8, 8), (23, 36)), "outside"),
        (lambda: scenes._plan_blend((1, 3, 8, 8), "float32", _tiles([(0, 32)], 8, 8), (23, 36)), "outside"),
        (lambda: scenes._plan_blend((2, 3, 8, 8), "float32", _tiles([(0, 0)], 8, 8), (23, 36)), "2 cubes"),
        (lambda: scenes._plan_blend((1, 3, 8, 8), "float64", _tiles([(0, 0)], 8, 8), (23, 36)), "float32"),
        (lambda: scenes._plan_blend((1, 3, 4, 8), "float32", _tiles([(0, 0)], 8, 8), (23, 36)), "the cubes are"),
        (lambda: scenes._plan_blend((1, 8, 8), "float32", _tiles([(0, 0)], 8, 8), (23, 36)), "(P, T, th, tw)"),
    ]
    for call, text in bad:
        with pytest.raises(ValueError) as err:
            call()
        assert text in str(err.value), (text, str(err.value))
    # 16 windows over a pixel and a weight sum of exactly 2^24 are the limits: allowed
    _, sy, sx, *_ = scenes._plan_blend((2, 3, 8, 8), "float32", _tiles([(0, 0), (1, 4)], 8, 8), (23, 36))
    assert (sy, sx) == (1, 4)
    _, sy, sx, *_ = big()
    assert (sy, sx) == (2048, 2048)
    with pytest.raises(ValueError) as err:
        scenes._plan_blend((2, 1, 4098, 4096), "float32", _tiles([(0, 0), (2049, 2048)], 4098, 4096), (8196, 8192))
    assert "4 x ceil(4098 / 2) x ceil(4096 / 2) = 16785408 > 2^24" in str(err.value)


def test_blend_stack_bytes():
    from s2_emit import scenes
    assert scenes._blend_stack_bytes(1, 1, 1, 1) == 4
    assert scenes._blend_stack_bytes(15, 4, 120, 120) == 15 * 4 * 120 * 120 * 4 == 3456000
    # the half-stride window set of a 1242 x 1280 EMIT scene, 32 bands: 23 x 24 windows of 600 x 600 - beyond 32 bits
    assert scenes._blend_stack_bytes(23 * 24, 32, 600, 600) == 25436160000

    class Cuda:                        # 1 MB free on the device and 2.5 MB more that torch's allocator holds unused
        mem_get_info = staticmethod(lambda dev: (1000000, 64000000))
        memory_reserved = staticmethod(lambda dev: 3000000)
        memory_allocated = staticmethod(lambda dev: 500000)

    class Torch:
        cuda = Cuda

    scenes._check_blend_stack(Torch, None, 15, 4, 120, 120)                # 3 456 000 <= 3 500 000
    with pytest.raises(ValueError) as err:
        scenes._check_blend_stack(Torch, None, 16, 4, 120, 120)
    for text in ("3686400 bytes", "3500000 are free", "fewer bands", "larger stride", "max_tiles"):
        assert text in str(err.value), (text, str(err.value))


def test_argument_checks_need_no_gpu():
    import s2_emit
    e = np.zeros((7, 43, 62), np.float32)
    s = np.zeros((3, 258, 372), np.float32)
    cubes = np.zeros((1, 3, 8, 8), np.float32)
    bad = [
        (lambda: s2_emit.find_valid_paired_tiles(e, s, TILE, SCALE, stride=7), "stride=7"),
        (lambda: s2_emit.find_valid_paired_tiles(e, s, TILE, SCALE, stride=40), "stride=40"),
        (lambda: s2_emit.find_valid_paired_tiles(e, s, TILE, SCALE, stride=0), "stride=0"),
        (lambda: s2_emit.mosaic_tiles(cubes, _tiles([(0, 0)], 8, 8), (23, 36), blend="linear"), "blend='linear'"),
        (lambda: s2_emit.mosaic_tiles(cubes, _tiles([(0, 0)], 8, 8), (23, 36), blend=True), "blend=True"),
        (lambda: s2_emit.mosaic_tiles(cubes, _tiles([(16, 0)], 8, 8), (23, 36), blend="feather"), "outside"),
        (lambda: s2_emit.mosaic_tiles(np.zeros((2, 3, 8, 8), np.float32), _tiles([(0, 0), (1, 1)], 8, 8), (23, 36), blend="feather"),
         "64 windows"),
        (lambda: s2_emit.fuse_scene(e, s, tile=TILE, factor=SCALE, bands=4, stride=7), "stride=7"),
        (lambda: s2_emit.fuse_scene(e, s, tile=TILE, factor=SCALE, bands=4, stride=10, blend="mean"), "blend='mean'"),
        (lambda: s2_emit.fuse_scene(e, s, tile=TILE, factor=SCALE, bands=4, blend="mean"), "blend='mean'"),
        (lambda: s2_emit.fuse_scene(e, s, tile=TILE, factor=SCALE, bands=4, stride=4), "5 x 5 = 25 windows"),
        (lambda: s2_emit.fuse_scene(e, s, tile=TILE, factor=SCALE, bands=4, stride=10, batch=0), "batch"),
    ]
    for call, text in bad:
        with pytest.raises(ValueError) as err:
            call()
        assert text in str(err.value), (text, str(err.value))
    # an S2 scene too small for a single window pair: an empty list, and no GPU is asked for
    assert s2_emit.find_valid_paired_tiles(e, s[:, :20, :20], TILE, SCALE, stride=10) == []


# ---- the C entry ------------------------------------------------------------------------------------------------------------------
def test_c_entry_refuses_bad_arguments():
    """HSR_REQUIRE comes before any HIP call, so every refusal and its text is reachable without a GPU."""
    from s2_emit import _native as nat
    lib = nat.load()
    p, st = C.c_void_p(64), C.c_void_p(0)

    def call(cubes=p, P=4, T=3, th=8, tw=8, sy=4, sx=4, start=p, ny=4, nx=8, out=p, H=23, W=36):
        return lib.hsr_scene_mosaic_blend(cubes, P, T, th, tw, sy, sx, start, ny, nx, out, H, W, 0.0, st)

    def refused(rc, text):
        assert rc != 0 and text in lib.hsr_last_error().decode(), (rc, lib.hsr_last_error())
        return rc

    codes = {}
    for kw in (dict(cubes=None), dict(start=None), dict(out=None)):
        codes["null"] = refused(call(**kw), "NULL pointer")
    for name in ("P", "T", "th", "tw", "sy", "sx", "ny", "nx", "H", "W"):
        for v in (0, -1):
            codes["size"] = refused(call(**{name: v}), "bad shape")
    codes["pitch"] = refused(call(sy=3), "does not divide")
    refused(call(sx=3), "does not divide")
    refused(call(th=6, sy=4), "does not divide")
    codes["K"] = refused(call(sy=1, sx=2), "8 x 4 = 32 windows")
    refused(call(th=17, tw=1, sy=1, sx=1), "17 x 1 = 17 windows")
    codes["weights"] = refused(call(th=4098, tw=4096, sy=2049, sx=2048, H=8196, W=8192), "above 2^24")
    refused(call(th=1 << 30, tw=1 << 30, sy=1 << 30, sx=1 << 30, H=5, W=5), "above 2^24")
    codes["T"] = refused(call(T=65536), "T=65536")
    codes["cells"] = refused(call(ny=1 << 16, nx=1 << 15), "lattice cells")
    assert codes["null"] == codes["size"] == codes["pitch"] == 1, codes                # HSR_ERR_INVALID
    assert codes["K"] == codes["weights"] == codes["T"] == codes["cells"] == 2, codes  # HSR_ERR_UNSUPPORTED


def test_export_declared_registered_and_additive():
    from s2_emit import _native as nat
    lib = nat.load()
    text = open(os.path.join(ROOT, "include", "hsr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    assert hasattr(lib, EXPORT), f"{EXPORT} is not exported"
    assert re.search(r"\b%s\s*\(" % EXPORT, code), f"{EXPORT} is not declared in include/hsr.h"
    assert EXPORT in comments, f"{EXPORT} is not documented in include/hsr.h"
    assert EXPORT in nat.SIGNATURES and len(nat.SIGNATURES[EXPORT][1]) == 15
    assert lib.hsr_abi_version() == 5 == nat.HSR_ABI_VERSION
    assert lib.hsr_aux_instance_count() == 32 and lib.hsr_k4_instance_count() == 31
