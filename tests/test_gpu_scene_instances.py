"""Every kernel instance of csrc/hsr_scene.hip - the black-pixel scan, the tile gather, the mosaic and the feathered mosaic - on an
MI355X, row by row of the tables of tests/scene_cases.py, against the references stated there.

The entry points are called through ctypes.  Every output lies `off` bytes past a 256-byte boundary in a buffer filled with a
sentinel byte, between two guard zones (Buf of gpu_harness.py): what a call does not own must come back untouched.
After every call the library's launch record (hsr_scene_last_launch) is read and compared with the instance the row expects, a
name computed by scene_cases' mirror of the selection rules.  Every comparison is exact - integers or bits - except the blend's
pixels under two or more values, which are held to the derived bound (K + 2) 2^-24 sum w |v| / sum w (check_blend).  The last
test checks that the rows reached every name hsr_scene_instance_name enumerates.  What the rows claim about themselves (which
pixels count, which loops make a second trip, ...) is checked without a GPU in test_scene_instances_host.py."""
import numpy as np
import pytest

import scene_cases as sc
from gpu_harness import FILL, SENT32, Buf, LaunchLog, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from gpu_harness import lib as _lib
from family_runners import bits as _bits, run_blend, run_gather, run_mosaic, scan_call
from test_scene_blend_host import check_blend

pytestmark = pytest.mark.gpu

LOG = LaunchLog("hsr_scene_last_launch")
WORST = {}                       # K -> largest blend error over its bound
F32, U16 = sc.F32, sc.U16


# =============================================================================================================================
# scan
# =============================================================================================================================
def _scan(torch, sb, scene, th, tw, **kw):
    """hsr_scene_black_counts on the scene in Buf `sb` -> the (H // th, W // tw) counts."""
    return scan_call(torch, sb, scene, th, tw, LOG, **kw)


@pytest.mark.parametrize("dtype", [F32, U16], ids=["float32", "uint16"])
@pytest.mark.parametrize("bands", sc.DECIDING_BANDS)
def test_scan_deciding_band(torch_gpu, dtype, bands):
    """Regions that are black in every band but one, at every position of the band loop's groups of 8 and for every band count
    round them, under every predicate; waves with one live lane and with none."""
    scene, _, _ = sc.deciding_scene(dtype, bands)
    sb = Buf(torch_gpu, scene.nbytes, 0, scene)
    for kw, _ in sc.DECIDING_SETTINGS[dtype]:
        mask = sc.black_mask_np(scene, **kw)
        for th, tw in sc.scan_tilings(*sc.DECIDING_HW):
            got = _scan(torch_gpu, sb, scene, th, tw, **kw)
            np.testing.assert_array_equal(got, sc.window_counts(mask, th, tw), err_msg=f"{kw} tile {th} x {tw}")
    sb.get(np.uint8)


def test_scan_float32_tolerance_edges(torch_gpu):
    """Samples one, two and three float32 steps on either side of nodata +- tol, masked_val +- tol and +-zero_atol, -0.0,
    denormals, NaN and +-Inf, with finite and non-finite nodata values: the mask itself (tile 1 x 1) and its sum."""
    scene, _ = sc.f32_edge_scene()
    _, H, W = scene.shape
    sb = Buf(torch_gpu, scene.nbytes, 0, scene)
    for call in sc.F32_EDGE_CALLS:
        mask = sc.black_mask_np(scene, **sc.ref_kwargs(call))
        got = _scan(torch_gpu, sb, scene, 1, 1, **call)
        bad = np.argwhere(got != mask)
        assert not len(bad), (call, [(tuple(p), [float(v) for v in scene[:, p[0], p[1]]]) for p in bad[:5]])
        np.testing.assert_array_equal(_scan(torch_gpu, sb, scene, H, W, **call), [[mask.sum()]])
        np.testing.assert_array_equal(_scan(torch_gpu, sb, scene, 5, 3, **call), sc.window_counts(mask, 5, 3))


def test_scan_uint16_tolerance_edges(torch_gpu):
    scene = sc.u16_edge_scene()
    sb = Buf(torch_gpu, scene.nbytes, 0, scene)
    for call in sc.U16_EDGE_CALLS:
        mask = sc.black_mask_np(scene, **call)
        got = _scan(torch_gpu, sb, scene, 1, 1, **call)
        bad = np.argwhere(got != mask)
        assert not len(bad), (call, [(tuple(p), scene[:, p[0], p[1]].tolist()) for p in bad[:5]])
        np.testing.assert_array_equal(_scan(torch_gpu, sb, scene, 2, 70, **call), [[mask.sum()]])


@pytest.mark.parametrize("dtype", [F32, U16], ids=["float32", "uint16"])
def test_scan_ignores_the_remainder_strips(torch_gpu, dtype):
    """Black pixels right of and below the window grid change nothing."""
    black, valid = sc.strip_scenes(dtype)
    th, tw = sc.STRIP_TILE
    want = sc.scan_ref(black, th, tw)
    for scene in (black, valid):
        sb = Buf(torch_gpu, scene.nbytes, 0, scene)
        np.testing.assert_array_equal(_scan(torch_gpu, sb, scene, th, tw), want)


def test_scan_float32_several_rows_per_wave(torch_gpu):
    """1 x 2100 x 1024 float32, half black: 33 600 waves, so a wave walks two rows and carries two window counts across them -
    the same window (one window), a second one (a window row per row; 7-row windows of a wave's width), evictions (3 x 5)."""
    scene = sc.large_f32_scene()
    H, W = sc.LARGE_HW
    mask = sc.black_mask_np(scene, nodata=-9999.0)
    sb = Buf(torch_gpu, scene.nbytes, 0, scene)
    for th, tw in sc.LARGE_TILINGS:
        assert sc.scan_rows_per_wave(H, W, th, tw) == 2
        got = _scan(torch_gpu, sb, scene, th, tw, nodata=-9999.0)
        np.testing.assert_array_equal(got, sc.window_counts(mask, th, tw), err_msg=f"tile {th} x {tw}")


# =============================================================================================================================
# gather
# =============================================================================================================================
@pytest.mark.parametrize("name", list(sc.GATHER_ROWS))
def test_gather_rows(torch_gpu, name):
    row = sc.GATHER_ROWS[name]
    c = sc.gather_case_of(row)
    got = run_gather(torch_gpu, row, c, LOG)
    np.testing.assert_array_equal(_bits(got[c["inside"]]), _bits(c["want"][c["inside"]]))


# =============================================================================================================================
# mosaic
# =============================================================================================================================
@pytest.mark.parametrize("name", list(sc.MOSAIC_ROWS))
def test_mosaic_rows(torch_gpu, name):
    T, H, W, th, tw, P, out_off, cubes_off, fills = sc.MOSAIC_ROWS[name]
    cubes, slot = sc.mosaic_case(name)
    pre = np.frombuffer(bytes([FILL]) * (T * H * W * 4), np.float32).reshape(T, H, W)
    for fill, fill_rest in fills:
        got = run_mosaic(torch_gpu, sc.MOSAIC_ROWS[name], (cubes, slot), LOG, fill, fill_rest)
        want = sc.assemble(cubes, slot, pre, th, tw, fill, fill_rest)
        np.testing.assert_array_equal(got, _bits(want))
        assert (got == SENT32).any() or name == "z-limit"


# =============================================================================================================================
# blend
# =============================================================================================================================
def _blend(torch, name, case, fill):
    return run_blend(torch, sc.BLEND_ROWS[name], case, LOG, fill)


@pytest.mark.parametrize("name", list(sc.BLEND_ROWS))
def test_blend_rows(torch_gpu, name):
    case = sc.blend_case(name)
    K = case["K"]
    fills = (np.float32(np.nan), np.float32(7.25)) if sc.BLEND_ROWS[name]["T"] == 3 else (np.float32(np.nan),)
    for fill in fills:
        got = _blend(torch_gpu, name, case, fill)
        WORST[K] = max(WORST.get(K, 0.0), check_blend(got, case["ref"], K, fill))
    if sc.BLEND_ROWS[name]["kind"] == "nofit":
        assert (got.view(np.uint32) == np.float32(7.25).view(np.uint32)).all()
    print(f"blend {name} K={K}: largest error / bound = {WORST[K]:.3f} so far")


@pytest.mark.parametrize("name", [n for n, r in sc.BLEND_ROWS.items() if r["kind"] == "lattice" and not r["out_off"] and not r["cubes_off"]])
def test_blend_of_a_constant_is_the_constant(torch_gpu, name):
    """Cubes that are 0.5 everywhere: the weighted sums are exact, so every covered pixel is 0.5 bit for bit, for every K."""
    case = sc.blend_const_case(name)
    got = _blend(torch_gpu, name, case, np.float32(np.nan))
    cover = case["ref"]["cover"]
    assert (got.view(np.uint32)[cover > 0] == np.float32(0.5).view(np.uint32)).all() and np.isnan(got[cover == 0]).all()
    check_blend(got, case["ref"], case["K"], np.float32(np.nan))


# =============================================================================================================================
# another stream
# =============================================================================================================================
def test_chain_on_a_side_stream(torch_gpu):
    """find_valid_paired_tiles -> extract_tile_pairs -> mosaic_tiles, plain and feathered, under torch.cuda.stream(side) on scenes
    that a preceding kernel of that stream writes: the bits of the same chain on the default stream."""
    import s2_emit
    torch = torch_gpu
    rng = np.random.default_rng(9)
    emit = rng.uniform(0.05, 0.6, (5, 43, 62)).astype(np.float32)
    s2 = rng.uniform(0.05, 0.6, (3, 129, 186)).astype(np.float32)
    emit[:, 0:20, 20:40] = -0.01
    s2[:, 60:120, 120:180] = 0.0
    emit[2, 5, 5] = np.nan

    def chain(E, S, stride):
        tiles = s2_emit.find_valid_paired_tiles(E, S, 20, 3, 0.3, emit_nodata=-9999.0, stride=stride)
        emits, s2s = s2_emit.extract_tile_pairs(E, S, tiles, emit_nodata=-9999.0)
        image = s2_emit.mosaic_tiles(s2s, tiles, (129, 186), blend=None if stride is None else "feather")
        return tiles, emits.view(torch.int16), s2s, image

    e0, s0 = torch.from_numpy(emit).cuda(), torch.from_numpy(s2).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for stride in (None, 10):
        want = chain(e0, s0, stride)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            busy = torch.ones((2048, 2048), device="cuda")
            for _ in range(4):                                             # keeps the stream busy while the chain is enqueued
                busy = busy @ busy * (1.0 / 2048)
            E, S = torch.empty_like(e0), torch.empty_like(s0)
            E.copy_(e0 * busy[0, 0])                                       # x 1.0: written by this stream, behind the products
            S.copy_(s0 * busy[1, 1])
            got = chain(E, S, stride)
        side.synchronize()
        assert got[0] == want[0] and len(got[0]) >= 2
        for g, w in zip(got[1:], want[1:]):
            assert g.shape == w.shape and torch.equal(g.contiguous().view(torch.int32 if g.dtype == torch.float32 else g.dtype),
                                                      w.contiguous().view(torch.int32 if w.dtype == torch.float32 else w.dtype))
        assert np.isfinite(got[3].cpu().numpy()).any()


# =============================================================================================================================
# completeness
# =============================================================================================================================
def test_rows_reach_every_instance(torch_gpu):
    lib = _lib()
    assert lib.hsr_scene_instance_count() == 20
    table = {lib.hsr_scene_instance_name(i).decode() for i in range(20)}
    assert len(table) == 20
    assert LOG.seen == table, (sorted(table - LOG.seen), sorted(LOG.seen - table))
    print("scene instances seen: %d of %d" % (len(LOG.seen & table), len(table)))
    print("blend: largest error / bound per K: " + ", ".join(f"K={k}: {WORST[k]:.3f}" for k in sorted(WORST)))
