"""s2_emit.clouds on an MI355X: scl_metrics / count_cloud_pixels against the restated reference (cloud_utils.py), the mask, coarse
and cube functions against tests/scl_cases.py's references, and fuse_scene_clear against the chain written out by hand, bit for
bit; an all-clear SCL gives fuse_scene's cube; a planted cloud no longer spoils the fit.  Every comparison but the last is an
equality; the last is a relation between two measured values, without a threshold."""
import numpy as np
import pytest

import scl_cases as sc
from gpu_harness import bits_equal, torch_gpu  # noqa: F401  (torch_gpu: the fixture)

pytestmark = pytest.mark.gpu
KW = dict(tile=sc.T20, factor=sc.F, bands=sc.BANDS_OUT, degree=sc.DEGREE)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the reference's statistics --------------------------------------------------------------------------------------------------------
def test_scl_metrics_and_count_cloud_pixels(torch_gpu):
    import s2_emit
    torch = torch_gpu
    rng = np.random.default_rng(5)
    planes = [rng.choice(np.arange(12, dtype=np.uint8), size=(137, 211), p=[.05, .01, .04, .05, .3, .2, .1, .05, .08, .06, .04, .02]),
              np.zeros((5, 7), np.uint8), np.full((33, 65), 9, np.uint8), sc.scene_scl(1), sc.scene_scl(2)]
    for scl in planes:
        for shadows in (False, True):
            want = sc.metrics_ref(scl, s2_emit.SCL_NAMES, shadows)
            for arg in (scl, torch.from_numpy(scl.copy()).cuda()):
                got = s2_emit.scl_metrics(arg, shadows)
                assert list(got) == list(want)
                for key in want:
                    assert got[key] == want[key] or (key == "cloud_frac_valid" and np.isnan(got[key]) and np.isnan(want[key])), (key, got, want)
                    assert type(got[key]) is type(want[key]) or key == "cloud_frac_valid", key
        assert s2_emit.count_cloud_pixels(scl) == sc.cloud_pixels_ref(scl, s2_emit.CLOUD_CLASSES)
    # a strided view, values above 11, and the per-window form
    big = rng.choice(sc.VALUES, size=(70, 300)).astype(np.uint8)
    view = torch.from_numpy(big).cuda()[3:60, 7:250]
    sub = big[3:60, 7:250]
    got, want = s2_emit.scl_metrics(view), sc.metrics_ref(sub, s2_emit.SCL_NAMES)
    other = sum(v for k, v in want["class_counts"].items() if k in ("12", "31", "32", "255"))
    assert {k: got[k] for k in got if k != "class_counts"} == {k: want[k] for k in want if k != "class_counts"}
    assert got["class_counts"].pop("other") == other and all(want["class_counts"][k] == v for k, v in got["class_counts"].items())
    per = s2_emit.scl_metrics(view, True, tile=(10, 64))
    ref = sc.counts_ref(sub, 10, 64).astype(np.int64)
    np.testing.assert_array_equal(per["class_counts"], ref[..., :13])
    np.testing.assert_array_equal(per["total_px"], np.full((5, 3), 640))
    np.testing.assert_array_equal(per["cloud_px"], ref[..., [3, 8, 9, 10]].sum(axis=-1))
    np.testing.assert_array_equal(per["valid_px"], 640 - ref[..., 0])
    np.testing.assert_array_equal(per["cloud_frac_valid"], per["cloud_px"] / per["valid_px"])


def test_mask_coarse_and_cube_functions(torch_gpu):
    import s2_emit
    torch = torch_gpu
    scl = sc.mask_plane("random-0.05-disc-r5")
    for kw, ref in ((dict(buffer=5), sc.dilate_ref(scl, sc.GROW, sc.FLAT, 5, sc.DISC)),
                    (dict(buffer=2, shape="square", include_shadows=True, flat_classes=()), sc.dilate_ref(scl, sc.GROW | 8, 0, 2, sc.SQUARE)),
                    (dict(classes=(4, 40), flat_classes=(0, 255)), sc.dilate_ref(scl, 1 << 4, 1, 0, sc.DISC))):
        np.testing.assert_array_equal(s2_emit.cloud_mask(scl, **kw).cpu().numpy(), ref)
    out = torch.full((70, 160), 7, dtype=torch.uint8, device="cuda")
    m = s2_emit.cloud_mask(torch.from_numpy(scl.copy()).cuda(), buffer=5, out=out[:, 3:153])
    np.testing.assert_array_equal(m.cpu().numpy(), sc.dilate_ref(scl, sc.GROW, sc.FLAT, 5, sc.DISC))
    assert (out[:, :3] == 7).all() and (out[:, 153:] == 7).all()
    for k, frac, cell in ((6, 0.0, None), (3, 0.5, (4, 5)), (16, 1.0, 2), (2, 0.25, 7)):
        clear, win = s2_emit.coarse_clear_mask(m, k, max_bad_frac=frac, cell=cell)
        c = (cell, cell) if isinstance(cell, int) else cell
        rc, _, rw = sc.coarse_ref(m.cpu().numpy(), k, int(np.floor(frac * k * k)), c)
        np.testing.assert_array_equal(clear.cpu().numpy(), rc)
        assert (win is None) == (cell is None) and (win is None or np.array_equal(win.cpu().numpy(), rw))
    for name in ("up1-nan", "up2-nan", "up2-fill"):
        T, H, W, rs, bs, up, fill, _ = sc.APPLY_ROWS[name]
        c = sc.apply_case(name)
        cube = torch.from_numpy(c["cube"].copy()).cuda()
        assert s2_emit.mask_cube(cube, c["mask"], fill=fill) is cube
        bits_equal(cube.cpu().numpy(), c["ref"], name)
        wide = torch.full((T, H + 2, W + 5), 3.25, dtype=torch.float32, device="cuda")
        wide[:, 1:H + 1, 2:W + 2] = torch.from_numpy(c["cube"].copy()).cuda()
        s2_emit.mask_cube(wide[:, 1:H + 1, 2:W + 2], torch.from_numpy(c["mask"].copy()).cuda(), fill=fill)
        bits_equal(wide[:, 1:H + 1, 2:W + 2].cpu().numpy(), c["ref"], name + " view")
        edge = wide.cpu().numpy().copy()
        edge[:, 1:H + 1, 2:W + 2] = 3.25
        assert (edge == 3.25).all()
    with pytest.raises(ValueError, match="neither"):
        s2_emit.mask_cube(torch.zeros((1, 10, 10), device="cuda"), np.zeros((4, 4), np.uint8))


# ---- fuse_scene_clear ------------------------------------------------------------------------------------------------------------------
def _by_hand(torch, name):
    """cloud_mask -> coarse_clear_mask -> find_valid_paired_tiles filtered by the NumPy cloud fraction -> extract_tile_pairs ->
    fuse_tile_pairs(train_mask=) -> mosaic_tiles -> NumPy masking."""
    import s2_emit
    buffer, shape, up, stride, frac = sc.DRIVER_ROWS[name]
    emit, s2 = sc.scene_pair()
    scl = sc.scene_scl(up)
    mask = s2_emit.cloud_mask(scl, buffer=buffer, shape=shape)
    clear, _ = s2_emit.coarse_clear_mask(mask, sc.F // up)
    clear_h = clear.cpu().numpy()
    tiles = []
    for t in s2_emit.find_valid_paired_tiles(emit, s2, sc.T20, sc.F, stride=stride):
        w = t["emit_window"]
        cf = int((clear_h[w.row_off:w.row_off + sc.T20, w.col_off:w.col_off + sc.T20] == 0).sum()) / sc.T20 ** 2
        if cf <= frac:
            tiles.append(dict(t, idx=len(tiles), cloud_frac=cf))
    emits, s2s = s2_emit.extract_tile_pairs(emit, s2, tiles, emit_uint16=False)
    tm = np.stack([clear_h[t["emit_window"].row_off:t["emit_window"].row_off + sc.T20,
                           t["emit_window"].col_off:t["emit_window"].col_off + sc.T20] for t in tiles])
    out = s2_emit.fuse_tile_pairs(emits, s2s, bands=sc.BANDS_OUT, degree=sc.DEGREE, factor=sc.F, train_mask=tm)
    cube = s2_emit.mosaic_tiles(out.cube, tiles, s2.shape[1:], blend="feather" if stride else None).cpu().numpy()
    raw = cube.copy()
    m = np.repeat(np.repeat(mask.cpu().numpy() != 0, up, axis=0), up, axis=1)[:258, :372]
    cube[:, m] = np.nan
    return dict(tiles=tiles, cube=cube, raw=raw, out=out, mask=mask.cpu().numpy(), clear=clear_h, under=m)


@pytest.mark.parametrize("name", list(sc.DRIVER_ROWS))
def test_fuse_scene_clear_against_the_chain_by_hand(torch_gpu, name):
    import s2_emit
    torch = torch_gpu
    buffer, shape, up, stride, frac = sc.DRIVER_ROWS[name]
    emit, s2 = sc.scene_pair()
    c, hand = sc.driver_case(name), _by_hand(torch, name)
    np.testing.assert_array_equal(hand["mask"], c["mask"])
    np.testing.assert_array_equal(hand["clear"], c["clear"])
    assert [(t["emit_window"].row_off, t["emit_window"].col_off, t["cloud_frac"]) for t in hand["tiles"]] == c["kept"]
    for args in ((emit, s2, sc.scene_scl(up)), tuple(torch.from_numpy(a.copy()).cuda() for a in (emit, s2, sc.scene_scl(up)))):
        out = s2_emit.fuse_scene_clear(*args, max_cloud_frac=frac, buffer=buffer, shape=shape, stride=stride, batch=2, **KW)
        assert out.tiles == hand["tiles"]
        bits_equal(out.cube.cpu().numpy(), hand["cube"], name)
        np.testing.assert_array_equal(out.mask.cpu().numpy(), c["mask"])
        np.testing.assert_array_equal(out.clear.cpu().numpy(), c["clear"])
        np.testing.assert_array_equal(out.n_train.cpu().numpy(), hand["out"].n_train.cpu().numpy())
        np.testing.assert_array_equal(out.n_train.cpu().numpy(), c["train"])
        np.testing.assert_array_equal(out.status.cpu().numpy(), np.zeros(len(c["kept"]), np.int32))
        np.testing.assert_array_equal(out.bands, hand["out"].bands)
    cube = out.cube.cpu().numpy()
    assert np.isnan(cube[:, hand["under"]]).all()                              # NaN under the buffered mask ...
    assert np.isfinite(cube[:, ~hand["under"]]).any() and np.isfinite(hand["raw"][:, hand["under"]]).any()   # ... which held predictions
    raw = s2_emit.fuse_scene_clear(emit, s2, sc.scene_scl(up), max_cloud_frac=frac, buffer=buffer, shape=shape, stride=stride,
                                   mask_output=False, **KW)
    bits_equal(raw.cube.cpu().numpy(), hand["raw"], name + " unmasked")
    one = s2_emit.fuse_scene_clear(emit, s2, sc.scene_scl(up), max_cloud_frac=frac, buffer=buffer, shape=shape, stride=stride, max_tiles=1, **KW)
    assert one.tiles == hand["tiles"][:1]


def test_all_clear_scl_gives_fuse_scenes_cube(torch_gpu):
    import s2_emit
    emit, s2 = sc.scene_pair()
    for stride in (None, 10):
        plain = s2_emit.fuse_scene(emit, s2, stride=stride, batch=3, **KW)
        for up in (1, 2):
            scl = np.full((-(-258 // up), -(-372 // up)), 4, np.uint8)
            out = s2_emit.fuse_scene_clear(emit, s2, scl, mask_output=False, buffer=8, stride=stride, batch=3, **KW)
            np.testing.assert_array_equal(_bits(out.cube.cpu().numpy()), _bits(plain.cube.cpu().numpy()))
            assert [dict(t, cloud_frac=0.0) for t in plain.tiles] == out.tiles
            np.testing.assert_array_equal(out.n_train.cpu().numpy(), plain.n_train.cpu().numpy())
            assert not out.mask.any() and out.clear.all()
            masked = s2_emit.fuse_scene_clear(emit, s2, scl, buffer=8, stride=stride, batch=3, **KW)      # nothing to blank either
            np.testing.assert_array_equal(_bits(masked.cube.cpu().numpy()), _bits(plain.cube.cpu().numpy()))
    none = s2_emit.fuse_scene_clear(emit, s2, np.full((258, 372), 9, np.uint8), **KW)                     # all cloud: nothing is kept
    assert none.tiles == [] and np.isnan(none.cube.cpu().numpy()).all() and none.mask.all() and not none.clear.any()
    assert none.n_train.numel() == 0 and none.cube.shape == (4, 258, 372)


def test_planted_cloud_no_longer_spoils_the_fit(torch_gpu):
    """The S2 patch under a cloud of SCL class 9 over about a fifth of window (0, 0) is replaced by a bright flat value; EMIT, acquired
    at another time, is untouched.  RMSE against the EMIT tile over the CLEAR cells of that window, of the cube averaged back to the
    EMIT grid:  fuse_scene_clear (buffer 2)  <  fuse_scene  - a relation, no threshold.  Both values are printed (they go into
    profiles/r22_scl.md).  The cube is NaN exactly under the buffered mask, inside the kept windows."""
    import s2_emit
    emit, s2 = sc.scene_pair()
    scl = sc.scene_scl(1)
    s2 = s2.copy()
    s2[:, scl == 9] = 0.9
    cloudy = s2_emit.fuse_scene(emit, s2, **KW)
    clear = s2_emit.fuse_scene_clear(emit, s2, scl, buffer=2, **KW)
    assert cloudy.tiles[0]["emit_window"] == clear.tiles[0]["emit_window"] == s2_emit.Window(0, 0, sc.T20, sc.T20)
    cells = clear.clear.cpu().numpy()[:sc.T20, :sc.T20] != 0
    cells &= np.isfinite(emit[:, :sc.T20, :sc.T20]).all(axis=0)
    assert 0.15 < 1 - cells.mean() < 0.35
    target = emit[clear.bands][:, :sc.T20, :sc.T20]
    rmse = []
    for out in (clear, cloudy):
        win = out.cube.cpu().numpy()[:, :sc.T20 * sc.F, :sc.T20 * sc.F].astype(np.float64)
        back = win.reshape(len(out.bands), sc.T20, sc.F, sc.T20, sc.F).mean(axis=(2, 4))
        assert np.isfinite(back[:, cells]).all()
        rmse.append(float(np.sqrt(np.mean((back[:, cells] - target[:, cells]) ** 2))))
    print(f"planted cloud: RMSE over the clear cells of the window, fuse_scene_clear {rmse[0]:.6f}, fuse_scene {rmse[1]:.6f}")
    assert rmse[0] < rmse[1]
    under = clear.mask.cpu().numpy() != 0
    kept = np.zeros_like(under)
    for t in clear.tiles:
        w = t["s2_window"]
        kept[w.row_off:w.row_off + w.height, w.col_off:w.col_off + w.width] = True
    nan = np.isnan(clear.cube.cpu().numpy()).all(axis=0)
    assert np.array_equal(nan[kept], under[kept]) and nan[~kept].all()
