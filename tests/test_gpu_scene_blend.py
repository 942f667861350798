"""Overlapping windows and the feathered mosaic on an MI355X: hsr_scene_mosaic_blend against the float64 restatement of its
definition (test_scene_blend_host.blend_ref64) under the bound (K + 2) 2^-24 sum w |v| / sum w, its exact properties bit for bit,
the seam it is there to remove, and fuse_scene with a stride against the chain of its parts."""
import numpy as np
import pytest

from gpu_harness import torch_gpu  # noqa: F401
from test_scene_blend_host import blend_ref64, check_blend

pytestmark = pytest.mark.gpu

T = 3


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _blend(torch, cubes, start, sy, sx, H, W, fill, misalign=False):
    """hsr_scene_mosaic_blend through s2_emit.scenes' wrapper; misalign: the stack starts one float past a 16-byte boundary."""
    from s2_emit import _native as nat, scenes
    from s2_emit._engine import _stream
    P, T_, th, tw = cubes.shape
    flat = torch.empty(cubes.size + 4, dtype=torch.float32, device="cuda")
    off = 1 if misalign else 0
    dev = flat[off:off + cubes.size].view(P, T_, th, tw)
    dev.copy_(torch.from_numpy(cubes))
    assert dev.data_ptr() % 16 == 4 * off
    out = torch.full((T_, H, W), -123.5, dtype=torch.float32, device="cuda")
    scenes._blend_into(nat.load(), torch, _stream(torch), dev, out, start, sy, sx, th, tw, float(fill))
    return out.cpu().numpy()


def make_case(th, tw, sy, sx, H, W, seed):
    """A start table with a spare row and column of cells (their windows leave the output) in which about 20 % of the usable
    cells are empty, one usable cell names a cube that does not exist and one spare cell names a real cube; cubes in (0, 1) with
    5 % NaN, a NaN payload among them, and one output pixel under several windows whose every contributor is NaN."""
    rng = np.random.default_rng(seed)
    ny, nx = (H - th) // sy + 2, (W - tw) // sx + 2
    start = np.full((ny, nx), -1, np.int32)
    ky, kx = th // sy, tw // sx
    used = rng.random((ny - 1, nx - 1)) >= 0.2
    used[:max(ky, 2), :max(kx, 2)] = True                 # cell (ky - 1, kx - 1) lies under all K windows
    used[ny - 2, nx - 2] = False                          # holds the cube that does not exist
    P = int(used.sum())
    start[:ny - 1, :nx - 1][used] = rng.permutation(P)    # the stack order is unrelated to the position
    start[ny - 2, nx - 2] = P + 3
    start[ny - 1, 1] = 0                                  # a real cube whose window would leave the output: ignored
    start[0, nx - 1] = 1
    cubes = rng.random((P, T, th, tw), dtype=np.float32) * 0.98 + 0.01
    cubes[rng.random(cubes.shape) < 0.05] = np.nan
    cubes.view(np.uint32)[start[0, 0], 1, 0, 0] = 0x7fc12345      # under one window only: its bits are the result
    # pixel (sy, sx) lies under the windows that start at cells (0, 0), (0, 1), (1, 0), (1, 1) at least: NaN in all of its
    # contributors in plane 0
    for j in range(ny - 1):
        for i in range(nx - 1):
            r, c = sy - j * sy, sx - i * sx
            if used[j, i] and 0 <= r < th and 0 <= c < tw:
                cubes[start[j, i], 0, r, c] = np.nan
    return cubes, start, ky * kx


CASES = [  # th, tw, sy, sx, H, W, misalign: the instance, K
    (8, 8, 4, 4, 23, 36, False),       # vector, K = 4, remainder strips below and right
    (6, 6, 3, 2, 23, 31, False),       # scalar, K = 6 (unrolled to 8)
    (8, 12, 2, 4, 30, 37, False),      # scalar (W is odd), K = 12 (unrolled to 16)
    (8, 8, 4, 4, 23, 36, True),        # the vector shape on a misaligned stack: the scalar instance
]


@pytest.mark.parametrize("th,tw,sy,sx,H,W,misalign", CASES)
def test_blend_against_float64(torch_gpu, th, tw, sy, sx, H, W, misalign):
    cubes, start, K = make_case(th, tw, sy, sx, H, W, seed=th * 100 + tw + sy)
    ref = blend_ref64(cubes, start, sy, sx, H, W)
    n, cover = ref["n"], ref["cover"]
    # the case holds what it is meant to: holes, single and multiple coverage, an all-NaN pixel under several windows, the bad entries
    assert (cover == 0).any() and (cover == 1).any() and (cover == K).any() and (n == 1).any() and (n >= 2).any()
    assert cover[0, sy, sx] >= 2 and n[0, sy, sx] == 0
    assert (start >= len(cubes)).sum() == 1 and (start[-1] >= 0).any() and (start[:, -1] >= 0).any()
    assert ref["one"][1, 0, 0] == 0x7fc12345 and cover[1, 0, 0] == 1
    worst = 0.0
    for fill in (np.float32(np.nan), np.float32(7.25)):
        got = _blend(torch_gpu, cubes, start, sy, sx, H, W, fill, misalign)
        worst = max(worst, check_blend(got, ref, K, fill))
    print(f"blend {th}x{tw} pitch {sy}x{sx} K={K}: largest error / bound = {worst:.3f}")


def _tiles(origins, th, tw):
    from s2_emit.scenes import Window
    return [{"s2_window": Window(c, r, tw, th)} for r, c in origins]


def test_feather_on_grid_tiles_is_the_plain_mosaic(torch_gpu):
    """Tiles that do not overlap: one window over every pixel, so every element is a copy - the bits of mosaic_tiles()."""
    import s2_emit
    rng = np.random.default_rng(1)
    for th, tw, W in ((6, 8, 36), (6, 7, 30)):
        org = [(6, 2 * tw), (12, 0), (0, tw), (6, 0)]
        cubes = rng.standard_normal((4, 2, th, tw)).astype(np.float32)
        cubes[1, 0, 2, 3] = np.nan
        cubes.view(np.uint32)[2, 1, 0, 0] = 0x7fc12345
        for fill in (float("nan"), 0.5):
            plain = s2_emit.mosaic_tiles(cubes, _tiles(org, th, tw), (23, W), fill=fill).cpu().numpy()
            feather = s2_emit.mosaic_tiles(cubes, _tiles(org, th, tw), (23, W), fill=fill, blend="feather").cpu().numpy()
            np.testing.assert_array_equal(_bits(feather), _bits(plain))
        assert (_bits(feather) == 0x7fc12345).sum() == 1


def test_feather_does_not_depend_on_the_tile_order(torch_gpu):
    import s2_emit
    rng = np.random.default_rng(2)
    org = [(r, c) for r in (0, 4, 8, 12) for c in (0, 4, 8, 16, 20, 28) if (r, c) != (4, 8)]
    cubes = rng.random((len(org), T, 8, 8), dtype=np.float32)
    cubes[rng.random(cubes.shape) < 0.05] = np.nan
    first = s2_emit.mosaic_tiles(cubes, _tiles(org, 8, 8), (23, 36), blend="feather").cpu().numpy()
    assert np.isfinite(first).any() and np.isnan(first[:, 20:, :]).all()
    for seed in (3, 4):
        p = np.random.default_rng(seed).permutation(len(org))
        again = s2_emit.mosaic_tiles(cubes[p], _tiles([org[k] for k in p], 8, 8), (23, 36), blend="feather").cpu().numpy()
        np.testing.assert_array_equal(_bits(again), _bits(first))


def test_seam_becomes_a_ramp(torch_gpu):
    """Two 8 x 8 cubes of constants a = 0.25 and b = 0.75 at columns 0 and 4: in columns 4 .. 7 the column weights are 4, 3, 2, 1
    against 1, 2, 3, 4 (the row weight is common), so the result is a + (b - a) k / 5 for k = 1 .. 4: the linear ramp from column
    3 to column 8 with step (b - a) / (tw / 2 + 1) = 0.1, within the kernel's bound (K = 2), and flat outside.  The plain mosaic
    cannot take these tiles at all."""
    import s2_emit
    a, b = np.float32(0.25), np.float32(0.75)
    cubes = np.stack([np.full((T, 8, 8), a), np.full((T, 8, 8), b)]).astype(np.float32)
    tiles = _tiles([(0, 0), (0, 4)], 8, 8)
    got = s2_emit.mosaic_tiles(cubes, tiles, (8, 12), blend="feather").cpu().numpy().astype(np.float64)
    step = (float(b) - float(a)) / (8 / 2 + 1)
    assert step == 0.1
    want = np.full(12, float(a))
    want[3:9] = float(a) + step * np.arange(6)
    want[8:] = float(b)
    bound = (2 + 2) * 2.0 ** -24 * want                                # the values are positive: sum w |v| / sum w is the mean
    assert got.shape == (T, 8, 12) and (np.abs(got - want) <= bound).all(), np.abs(got - want).max()
    assert (got[:, :, :4] == a).all() and (got[:, :, 8:] == b).all() and (np.diff(got[0, 0, 3:9]) > 0.0999).all()
    with pytest.raises(ValueError, match="not on the"):
        s2_emit.mosaic_tiles(cubes, tiles, (8, 12))


# ---- fuse_scene with a stride ---------------------------------------------------------------------------------------------------------
T20, F = 20, 6


@pytest.fixture(scope="module")
def scene_pair():
    """The pair of test_gpu_scene_tiles: EMIT (12, 43, 62) float32 and S2 (3, 258, 372) float32, windows of 20 x 20 at factor 6;
    EMIT rows 0 .. 19 x columns 20 .. 39 are black (-0.01), S2 rows 120 .. 239 x columns 240 .. 359 are zero."""
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
    emit[:, 5, 5] = np.nan
    return emit, s2


@pytest.fixture(scope="module")
def fused(torch_gpu, scene_pair):
    """fuse_scene(stride=10) once, for the tests below: (batch=2 result, batch=64 result)."""
    import s2_emit
    emit, s2 = scene_pair
    kw = dict(tile=T20, factor=F, stride=10, bands=4, degree=2)
    return s2_emit.fuse_scene(emit, s2, batch=2, **kw), s2_emit.fuse_scene(emit, s2, batch=64, **kw)


def test_fuse_scene_stride_against_its_parts(torch_gpu, scene_pair, fused):
    import s2_emit
    emit, s2 = scene_pair
    out = fused[0]
    tiles = s2_emit.find_valid_paired_tiles(emit, s2, T20, F, stride=10)
    # 3 x 5 windows at stride 10.  With max_black_frac = 0 the black EMIT block rejects rows 0, 10 x columns 10, 20, 30 and the
    # zero S2 block rows 10, 20 x columns 30, 40: six windows are left
    assert out.tiles == tiles
    assert [(t["emit_window"].row_off, t["emit_window"].col_off) for t in tiles] == [(0, 0), (0, 40), (10, 0), (20, 0), (20, 10), (20, 20)]
    assert [t["idx"] for t in tiles] == list(range(6))
    assert all(t["s2_window"] == s2_emit.Window(t["emit_window"].col_off * F, t["emit_window"].row_off * F, T20 * F, T20 * F) and
               t["emit_black_frac"] == 0.0 and t["s2_black_frac"] == 0.0 for t in tiles)
    emits, s2s = s2_emit.extract_tile_pairs(emit, s2, tiles, emit_uint16=False)
    ref = s2_emit.fuse_tile_pairs(emits, s2s, bands=4, degree=2, factor=F)
    want = s2_emit.mosaic_tiles(ref.cube, tiles, s2.shape[1:], blend="feather").cpu().numpy()
    cube = out.cube.cpu().numpy()
    assert cube.shape == (4, 258, 372) and cube.dtype == np.float32
    np.testing.assert_array_equal(_bits(cube), _bits(want))
    np.testing.assert_array_equal(out.n_train.cpu().numpy(), ref.n_train.cpu().numpy())
    np.testing.assert_array_equal(out.status.cpu().numpy(), ref.status.cpu().numpy())
    np.testing.assert_array_equal(out.bands, ref.bands)
    assert len(out.n_train) == len(tiles) and (out.status.cpu().numpy() == 0).all()
    reached = np.zeros(cube.shape[1:], bool)
    for t in tiles:
        w = t["s2_window"]
        reached[w.row_off:w.row_off + w.height, w.col_off:w.col_off + w.width] = True
    assert (~reached).any() and np.isnan(cube[:, ~reached]).all() and np.isfinite(cube[:, reached]).mean() > 0.99
    # one, two and three kept windows over a pixel all occur; under one window the cube's own bits stand
    cover = np.zeros(cube.shape[1:], int)
    for t in tiles:
        w = t["s2_window"]
        cover[w.row_off:w.row_off + w.height, w.col_off:w.col_off + w.width] += 1
    assert sorted(np.unique(cover)) == [0, 1, 2, 3]
    rc = ref.cube.cpu().numpy()
    alone = cover[0:120, 240:360] == 1                                  # the window at EMIT (0, 40), tile 1, overlaps no other
    assert alone.all()
    np.testing.assert_array_equal(_bits(cube[:, 0:120, 240:360]), _bits(rc[1]))


def test_fuse_scene_stride_does_not_depend_on_the_batch(torch_gpu, fused):
    a, b = fused
    assert a.tiles == b.tiles
    np.testing.assert_array_equal(_bits(a.cube.cpu().numpy()), _bits(b.cube.cpu().numpy()))
    np.testing.assert_array_equal(a.n_train.cpu().numpy(), b.n_train.cpu().numpy())
    np.testing.assert_array_equal(a.status.cpu().numpy(), b.status.cpu().numpy())


def test_fuse_scene_stride_equal_to_the_tile_is_the_plain_path(torch_gpu, scene_pair):
    import s2_emit
    emit, s2 = scene_pair
    kw = dict(tile=T20, factor=F, batch=2, bands=4, degree=2)
    plain, strided = s2_emit.fuse_scene(emit, s2, **kw), s2_emit.fuse_scene(emit, s2, stride=T20, **kw)
    assert plain.tiles == strided.tiles and len(plain.tiles) == 4
    np.testing.assert_array_equal(_bits(strided.cube.cpu().numpy()), _bits(plain.cube.cpu().numpy()))
    np.testing.assert_array_equal(strided.n_train.cpu().numpy(), plain.n_train.cpu().numpy())
    np.testing.assert_array_equal(strided.status.cpu().numpy(), plain.status.cpu().numpy())
    # an explicit feather on the same windows: one window over every pixel, so the same bits through the blend kernel
    feather = s2_emit.fuse_scene(emit, s2, stride=T20, blend="feather", **kw)
    assert feather.tiles == plain.tiles
    np.testing.assert_array_equal(_bits(feather.cube.cpu().numpy()), _bits(plain.cube.cpu().numpy()))
