"""s2_emit.scenes on an MI355X: the black-pixel scan against fixture g15 (the reference's is_black_mask) and, at the reference's
sizes, against the float32 / float64 restatement of test_scene_tiles_host.black_rule; the tile gather against host slicing, the
codec and the fixture's quantised tiles; the mosaic against a NumPy assembly; fuse_scene against fuse_tile_pairs on host-sliced
pairs.  Every comparison is exact."""
import numpy as np
import pytest

from conftest import load_golden
from gpu_harness import torch_gpu  # noqa: F401
from scene_cases import assemble as _assemble            # hsr_scene_mosaic in NumPy, shared with the instance tests
from test_scene_tiles_host import SCALE, TILE, black_rule, g15_mask, g15_settings, window_counts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g15():
    return load_golden("g15_scene_tiles")


def _dev(a, torch):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16) if a.dtype == np.uint16 else torch.from_numpy(a).cuda()


def _host(t, torch):
    t = t.contiguous()
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.uint16 else t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _scan(torch, scene, th, tw, nodata=None, masked_val=-0.01, nodata_atol=1e-3, zero_atol=1e-6):
    """hsr_scene_black_counts through s2_emit.scenes' wrapper -> the (H // th, W // tw) counts on the host."""
    from s2_emit import _native as nat, scenes
    from s2_emit._engine import _stream
    from s2_emit.pairs import _stack_dev
    dev = torch.device("cuda", torch.cuda.current_device())
    shape, dt = scenes._scene(scene, "scene")
    d = _stack_dev(scene, torch, dev)
    counts = torch.full((shape[1] // th, shape[2] // tw), -7, dtype=torch.int32, device=dev)          # the call zeroes it
    scenes._scan(nat.load(), _stream(torch), d, dt, shape, th, tw, scenes._nodata(nodata, "nodata"), masked_val, nodata_atol,
                 zero_atol, counts)
    return counts.cpu().numpy()


# ---- 1. the scan at the smallest shapes: 7 x 37 x 45, tile 8 - 4 x 5 windows, 5-pixel remainders, rows no multiple of 64 -------
def test_scan_float32_against_is_black_mask(torch_gpu, g15):
    """Every pixel class of gen_g15.emit_scene, with and without a nodata value; tile 8 (a wave touches up to six windows of a row),
    tile 1 (one window per pixel: up to 45 windows a wave), one 37 x 45 window, and a 5 x 3 tile."""
    g, torch = g15, torch_gpu
    emit, nd = g["emit"], float(g["nodata"])
    for nodata, key in ((nd, "emit"), (None, "emit_none")):
        mask = g15_mask(g, f"mask_{key}", emit.shape[1:])
        np.testing.assert_array_equal(_scan(torch, emit, TILE, TILE, nodata), g[f"counts_{key}"])
        np.testing.assert_array_equal(_scan(torch, emit, 1, 1, nodata), mask.astype(np.int32))
        np.testing.assert_array_equal(_scan(torch, emit, 37, 45, nodata), [[mask.sum()]])
        np.testing.assert_array_equal(_scan(torch, emit, 5, 3, nodata), window_counts(mask, 5, 3))


def test_scan_uint16_against_is_black_mask(torch_gpu, g15):
    g, torch = g15, torch_gpu
    u16 = g["u16"]
    for nodata, key in ((65535, "u16"), (None, "u16_none")):
        mask = g15_mask(g, f"mask_{key}", u16.shape[1:])
        np.testing.assert_array_equal(_scan(torch, u16, 4, 4, nodata), g[f"counts_{key}"])
        np.testing.assert_array_equal(_scan(torch, u16, 1, 1, nodata), mask.astype(np.int32))
        np.testing.assert_array_equal(_scan(torch, u16, 20, 26, nodata), [[mask.sum()]])
    np.testing.assert_array_equal(_scan(torch, g["s2"], TILE * SCALE, TILE * SCALE), g["counts_s2_full"])


def test_find_valid_paired_tiles_against_g15(torch_gpu, g15):
    """The two scans, the one copy to the host and the selection, for every setting of the fixture (NumPy and device inputs)."""
    import s2_emit
    g, torch = g15, torch_gpu
    emit_d = _dev(g["emit"], torch)
    for k, s2, name, frac, max_tiles in g15_settings(g):
        for e, s in ((g["emit"], s2), (emit_d, _dev(s2, torch))):
            tiles = s2_emit.find_valid_paired_tiles(e, s, TILE, SCALE, frac, max_tiles, emit_nodata=float(g["nodata"]))
            wins = np.array([tuple(t["emit_window"]) + tuple(t["s2_window"]) for t in tiles], dtype=np.int32).reshape(-1, 8)
            np.testing.assert_array_equal(wins, g[f"windows_{name}"][g[f"kept_{k}"]])
            assert [t["idx"] for t in tiles] == list(range(len(tiles)))
            fr = np.array([(t["emit_black_frac"], t["s2_black_frac"]) for t in tiles], dtype=np.float64).reshape(-1, 2)
            np.testing.assert_array_equal(fr, g[f"fracs_{k}"])


# ---- 2. one case at the reference's sizes ----------------------------------------------------------------------------------------
def test_scan_reference_sizes(torch_gpu):
    """285 x 200 x 200 float32 with a black border and 10 x 1200 x 1200 uint16, tile 100, scale 6: 2 x 2 windows, a row of 200
    pixels is three full waves and a part of one, and black regions read all 285 bands in groups."""
    import s2_emit
    from s2_emit import scenes
    torch = torch_gpu
    rng = np.random.default_rng(7)
    emit = rng.random((285, 200, 200), dtype=np.float32) * 0.6 + 0.02
    emit[:, :37, :] = -9999.0                              # the border
    emit[:, :, 171:] = -9999.0
    emit[:, 120:150, 40:90] = -0.01
    emit[:, 150:160, 40:90] = 0.0
    emit[284, 50:60, 50:60] = -9999.0                      # the LAST band only: not black
    emit[:, 60:70, 50:60] = -9999.0
    emit[284, 60:70, 50:60] = 0.3                          # all but the last band: not black
    emit[:, 100:105, 100:110] = -0.01
    emit[100, 100:105, 100:110] = -9999.0                  # mixed predicates: not black
    s2 = rng.integers(1, 4000, size=(10, 1200, 1200)).astype(np.uint16)
    s2[:, :200, :] = 0
    s2[:, 700:760, 100:1000] = 0
    s2[9, 800:900, 800:900] = 0                            # one band only
    me, ms = black_rule(emit, -9999.0), black_rule(s2, None)
    ce, cs = window_counts(me, 100, 100), window_counts(ms, 600, 600)
    assert 0 < me.sum() < me.size and not me[50:70, 50:60].any() and not me[100:105, 100:110].any()
    emit_d, s2_d = _dev(emit, torch), _dev(s2, torch)
    np.testing.assert_array_equal(_scan(torch, emit_d, 100, 100, -9999.0), ce)
    np.testing.assert_array_equal(_scan(torch, s2_d, 600, 600), cs)
    tiles = s2_emit.find_valid_paired_tiles(emit_d, s2_d, 100, 6, 0.45, emit_nodata=-9999.0)
    want = scenes.select_tiles(scenes.scene_windows(200, 200, 1200, 1200, 100, 6), ce, cs, 100, 6, 0.45)
    assert tiles == want and 0 < len(tiles) < 4


def test_scan_waves_that_walk_several_rows(torch_gpu):
    """2 x 4300 x 1100 uint16, windows of 301 x 500: above 32 Ki waves the library gives a wave several consecutive rows (here 4) and
    the wave carries its window counts across them; 301 is odd, so the row groups straddle the window rows, and half of the
    pixels are black."""
    rng = np.random.default_rng(11)
    scene = (rng.random((2, 4300, 1100)) < 0.3).astype(np.uint16)
    scene[:, 1000:1700, 200:900] = 0
    mask = black_rule(scene, None)
    assert 0.4 < mask.mean() < 0.7
    np.testing.assert_array_equal(_scan(torch_gpu, scene, 301, 500), window_counts(mask, 301, 500))
    np.testing.assert_array_equal(_scan(torch_gpu, scene, 1000, 7), window_counts(mask, 1000, 7))


# ---- 3. the gather -------------------------------------------------------------------------------------------------------------------
ORIGINS = [(0, 0), (1, 3), (2, 4), (1, 3)]                             # odd and even columns, a duplicate


def _gather(torch, scene, origins, th, tw, encode=None):
    from s2_emit import _native as nat, scenes
    from s2_emit._engine import _stream
    from s2_emit.pairs import _stack_dev
    dev = torch.device("cuda", torch.cuda.current_device())
    out = scenes._gather(nat.load(), torch, _stream(torch), _stack_dev(scene, torch, dev), str(scene.dtype), scene.shape,
                         np.array(origins, dtype=np.int32), th, tw, encode)
    return _host(out, torch)


def _encode_u16(torch, tile, scale, has_nd, nd, nd16):
    """hsr_tile_encode_u16 on one contiguous float32 tile."""
    from s2_emit import _native as nat
    from s2_emit._engine import _ptr, _stream
    x = torch.from_numpy(np.ascontiguousarray(tile)).cuda()
    out = torch.empty(x.shape, dtype=torch.int16, device=x.device)
    nat.check(nat.load().hsr_tile_encode_u16(_ptr(x), x.numel(), scale, has_nd, nd, nd16, _ptr(out), _stream(torch)), "encode")
    return out.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("th,tw", [(6, 8), (5, 7), (3, 4)])
def test_gather_bits_equal_host_slicing(torch_gpu, th, tw):
    """(5, 15, 19) scenes: tw % 4 == 0 takes the vector instance (row segments at every alignment: odd columns and a row pitch of 19
    samples), 7 the plain one; the last origin touches the last row and column."""
    torch = torch_gpu
    rng = np.random.default_rng(3)
    f32 = rng.standard_normal((5, 15, 19)).astype(np.float32) * 0.3
    f32[1, 2, 3], f32[2, 4, 5], f32[0, 1, 4], f32[3, 14, 18] = np.nan, np.inf, -9999.0, -0.0
    u16 = rng.integers(0, 65536, size=(5, 15, 19)).astype(np.uint16)
    origins = ORIGINS + [(15 - th, 19 - tw), (15 - th, 0), (0, 19 - tw)]
    for scene in (f32, u16):
        got = _gather(torch, scene, origins, th, tw)
        want = np.stack([scene[:, r:r + th, c:c + tw] for r, c in origins])
        assert got.dtype == scene.dtype and got.shape == want.shape
        np.testing.assert_array_equal(_bits(got), _bits(want))
    enc = (10000.0, 1, -9999.0, 65535)
    got = _gather(torch, f32, origins, th, tw, enc)
    assert got.dtype == np.uint16
    for k, (r, c) in enumerate(origins):
        np.testing.assert_array_equal(got[k], _encode_u16(torch, f32[:, r:r + th, c:c + tw], *enc))
    got = _gather(torch, f32, origins[:2], th, tw, (2000.0, 0, 0.0, 4000))
    np.testing.assert_array_equal(got[1], _encode_u16(torch, f32[:, 1:1 + th, 3:3 + tw], 2000.0, 0, 0.0, 4000))


def test_extract_tile_pairs_against_g15(torch_gpu, g15):
    """The fixture's quantised EMIT tiles (the reference's statements) and the S2 windows, for the tiles of setting 1; without
    emit_uint16 the EMIT stack keeps the scene's bits; an encode request on a uint16 scene is refused by the library."""
    import s2_emit
    from s2_emit import _native as nat
    g, torch = g15, torch_gpu
    emit, s2, nd = g["emit"], g["s2"], float(g["nodata"])
    tiles = s2_emit.find_valid_paired_tiles(emit, s2, TILE, SCALE, 0.1, emit_nodata=nd)
    emits, s2s = s2_emit.extract_tile_pairs(emit, s2, tiles, emit_nodata=nd)
    assert emits.dtype == torch.uint16 and s2s.dtype == torch.uint16 and emits.is_cuda and s2s.is_cuda
    np.testing.assert_array_equal(_host(emits, torch), g["emit_u16_tiles_1"])
    wins = g["windows_full"][g["kept_1"]]
    np.testing.assert_array_equal(_host(s2s, torch), np.stack([s2[:, rs:rs + hs, cs:cs + ws] for *_, cs, rs, ws, hs in wins]))
    raw, _ = s2_emit.extract_tile_pairs(_dev(emit, torch), _dev(s2, torch), tiles, emit_uint16=False)
    assert raw.dtype == torch.float32
    np.testing.assert_array_equal(_bits(_host(raw, torch)), _bits(np.stack([emit[:, re:re + he, ce:ce + we] for ce, re, we, he, *_ in wins])))
    same, _ = s2_emit.extract_tile_pairs(s2, s2, [dict(t, emit_window=t["s2_window"]) for t in tiles])   # uint16 "EMIT": copied as it is
    np.testing.assert_array_equal(_host(same, torch), _host(s2s, torch))
    with pytest.raises(nat.HsrError, match="encode quantises float32"):
        _gather(torch, g["u16"], [(0, 0)], 4, 4, (10000.0, 0, 0.0, 65535))


# ---- 4. the mosaic -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,tw", [(36, 8), (31, 8), (36, 6), (30, 7)])
def test_mosaic_bits_equal_numpy_assembly(torch_gpu, W, tw):
    """T = 3, H = 23, th = 6: 3 x 4 windows, a 5-row strip below and a strip right of them ((36, 8) is the 16-byte instance, the
    others the plain one).  Cubes, NaN fill (bits 0x7fc00000), -2 and an out-of-range slot left at the sentinel, with and without
    fill_rest."""
    from s2_emit import _native as nat, scenes
    from s2_emit._engine import _stream
    torch = torch_gpu
    T, H, th = 3, 23, 6
    rng = np.random.default_rng(W * 10 + tw)
    cubes = rng.standard_normal((4, T, th, tw)).astype(np.float32)
    cubes[1, 0, 2, 3] = np.nan
    cubes.view(np.uint32)[2, 1, 0, 0] = 0x7fc12345                   # a NaN payload is data: copied, not canonicalised
    slot = np.full((H // th, W // tw), -1, dtype=np.int32)
    slot.flat[:8] = [0, 3, -2, 1, 2, 0, 9, -2]                       # cube 0 twice; 9: no such cube
    pre = np.full((T, H, W), -123.5, dtype=np.float32)
    for fill, fill_rest in ((np.float32(np.nan), True), (np.float32(7.25), False)):
        out = torch.from_numpy(pre).cuda()
        scenes._mosaic_into(nat.load(), torch, _stream(torch), torch.from_numpy(cubes).cuda(), out, slot, th, tw, float(fill), fill_rest)
        want = _assemble(cubes, slot, pre, th, tw, fill, fill_rest)
        got = out.cpu().numpy()
        np.testing.assert_array_equal(_bits(got), _bits(want))
        assert (got == -123.5).any() and (not fill_rest or np.isnan(got[:, 18:, :]).all())
    assert np.float32(np.nan).view(np.uint32) == 0x7fc00000


def test_mosaic_tiles_public(torch_gpu):
    import s2_emit
    torch = torch_gpu
    W = s2_emit.Window
    cubes = np.random.default_rng(1).standard_normal((2, 2, 6, 8)).astype(np.float32)
    tiles = [{"s2_window": W(16, 6, 8, 6)}, {"s2_window": W(0, 12, 8, 6)}]
    got = s2_emit.mosaic_tiles(torch.from_numpy(cubes).cuda(), tiles, (23, 36)).cpu().numpy()
    slot = np.full((3, 4), -1, dtype=np.int32)
    slot[1, 2], slot[2, 0] = 0, 1
    want = _assemble(cubes, slot, np.zeros((2, 23, 36), np.float32), 6, 8, np.float32(np.nan), True)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    got0 = s2_emit.mosaic_tiles(cubes, tiles, (23, 36), fill=0.0).cpu().numpy()
    np.testing.assert_array_equal(_bits(got0), _bits(_assemble(cubes, slot, np.ones((2, 23, 36), np.float32), 6, 8, np.float32(0), True)))


# ---- 5. fuse_scene ---------------------------------------------------------------------------------------------------------------------
T20, F = 20, 6


@pytest.fixture(scope="module")
def scene_pair():
    """EMIT (12, 43, 62) float32 and S2 (3, 258, 372) float32: 2 x 3 windows of 20 x 20 at factor 6 with remainders on both sides;
    window (0, 1) is black on the EMIT side (all -0.01), window (1, 2) on the S2 side (all zero)."""
    rng = np.random.default_rng(20)
    h, w = 43, 62
    yy, xx = np.mgrid[0:h * F, 0:w * F].astype(np.float32)
    s2 = np.stack([0.25 + 0.2 * np.sin(yy / (9 + 3 * c) + c) * np.cos(xx / (11 + 2 * c)) for c in range(3)]).astype(np.float32)
    s2 += rng.normal(0, 0.01, s2.shape).astype(np.float32)
    coarse = s2.reshape(3, h, F, w, F).mean(axis=(2, 4))
    emit = np.stack([0.1 + 0.05 * b / 12 + (0.6 + 0.02 * b) * coarse[b % 3] + 0.2 * coarse[(b + 1) % 3] ** 2 for b in range(12)])
    emit = np.clip(emit + rng.normal(0, 0.003, emit.shape), 0.01, 0.95).astype(np.float32)
    emit[:, 0:20, 20:40] = -0.01
    s2[:, 120:240, 240:360] = 0.0
    emit[:, 5, 5] = np.nan                                 # an unusable pixel inside a kept window
    return emit, s2


def _check_fused(torch, out, emit, s2, kw):
    """out.cube against fuse_tile_pairs on the host-sliced pairs of out.tiles, NaN everywhere else."""
    import s2_emit
    cube = out.cube.cpu().numpy()
    assert cube.shape == (4, s2.shape[1], s2.shape[2]) and cube.dtype == np.float32
    e = np.stack([emit[:, t["emit_window"].row_off:t["emit_window"].row_off + T20,
                       t["emit_window"].col_off:t["emit_window"].col_off + T20] for t in out.tiles])
    s = np.stack([s2[:, t["s2_window"].row_off:t["s2_window"].row_off + T20 * F,
                     t["s2_window"].col_off:t["s2_window"].col_off + T20 * F] for t in out.tiles])
    ref = s2_emit.fuse_tile_pairs(e, s, bands=4, degree=2, factor=F, **kw)
    rc = ref.cube.cpu().numpy()
    rest = np.ones(cube.shape[1:], bool)
    for k, t in enumerate(out.tiles):
        win = (slice(t["s2_window"].row_off, t["s2_window"].row_off + T20 * F),
               slice(t["s2_window"].col_off, t["s2_window"].col_off + T20 * F))
        np.testing.assert_array_equal(_bits(cube[(slice(None),) + win]), _bits(rc[k]))
        rest[win] = False
    assert np.isnan(cube[:, rest]).all() and rest.any()
    np.testing.assert_array_equal(out.n_train.cpu().numpy(), ref.n_train.cpu().numpy())
    np.testing.assert_array_equal(out.status.cpu().numpy(), ref.status.cpu().numpy())
    np.testing.assert_array_equal(out.bands, ref.bands)
    return cube, ref


def test_fuse_scene_against_fuse_tile_pairs(torch_gpu, scene_pair):
    """batch=2.  With the default max_black_frac the two black windows are rejected: 4 pairs in two batches, NaN in the rejected
    windows and the remainder.  With max_black_frac=1 all 6 windows are kept - three batches, the first fills the remainder only -
    and the black ones hold whatever fuse_tile_pairs makes of such a pair.  Then device inputs with max_tiles=1."""
    import s2_emit
    from s2_emit import scenes
    torch = torch_gpu
    emit, s2 = scene_pair
    windows = scenes.scene_windows(43, 62, 258, 372, T20, F)
    ce, cs = window_counts(black_rule(emit), T20, T20), window_counts(black_rule(s2), T20 * F, T20 * F)
    assert len(windows) == 6 and ce.tolist() == [[0, 400, 0], [0, 0, 0]] and cs.tolist() == [[0, 0, 0], [0, 0, 14400]]
    for frac, kept in ((0.0, 4), (1.0, 6)):
        out = s2_emit.fuse_scene(emit, s2, tile=T20, factor=F, max_black_frac=frac, batch=2, bands=4, degree=2)
        assert out.tiles == scenes.select_tiles(windows, ce, cs, T20, F, frac) and len(out.tiles) == kept
        cube, _ = _check_fused(torch, out, emit, s2, {})
        if frac == 0.0:
            assert (out.status.cpu().numpy() == 0).all() and (out.n_train.cpu().numpy() > 300).all()
            assert np.isfinite(cube[:, 130, 10]).all() and np.isnan(cube[:, 10, 130]).all() and np.isnan(cube[:, 130, 250]).all()
    dev = s2_emit.fuse_scene(_dev(emit, torch), _dev(s2, torch), tile=T20, factor=F, batch=64, bands=4, degree=2, max_tiles=1)
    assert len(dev.tiles) == 1 and dev.tiles[0]["emit_window"] == s2_emit.Window(0, 0, T20, T20)
    _check_fused(torch, dev, emit, s2, {})


def test_fuse_scene_without_a_valid_window(torch_gpu, scene_pair):
    import s2_emit
    emit, s2 = scene_pair
    out = s2_emit.fuse_scene(np.full_like(emit, -0.01), s2, tile=T20, factor=F, bands=4, degree=2)
    assert out.tiles == [] and out.n_train.numel() == 0 and out.status.numel() == 0 and len(out.bands) == 4
    cube = out.cube.cpu().numpy()
    assert cube.shape == (4, 258, 372) and np.isnan(cube).all()
