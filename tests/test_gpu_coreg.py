"""coregister_scene end to end on an MI355X: a 48 x 48 EMIT / 288 x 288 S2 pair of tests/coreg_cases.py, displaced by a translation
and by an affine field, float32 and uint16, with a planted decoy window.

Against the reference chain of coreg_cases (long double surfaces -> float64 peaks -> np.linalg.lstsq):
  tie-point statuses equal the reference's (the table's margins make the peaks the same);
  shifts within 2 bar (|l - r| + |den|) / den^2 of the reference's - the surface bar carried through the parabola - on rows with
  |den| >= 1e-3 (tests/test_coreg_host.py checks that this is every row);
  the model within its bar plus that shift error carried through the least squares (|pinv(X)| times the per-record bound);
  the warped scene bit-equal to the NumPy warp UNDER THE KERNEL'S OWN MODEL;
  the output goes into find_valid_paired_tiles unchanged in type;
  the chain on device tensors issues no blocking synchronisation (torch's sync debug mode set to "error").

The same on a rectangular pair (48 x 60 EMIT, an S2 scene five rows longer than 6 x 48), and the parts of the public functions
beyond the plain call: an EMIT mask in every form and an S2 nodata value, grid= and the max_points thinning, NumPy scenes in and
out, scenes and outputs that are views, and the three ways to the identity (no model)."""
import numpy as np
import pytest

import coreg_cases as cc
import s2_emit
from gpu_harness import bits_equal, same_bits, torch_gpu  # noqa: F401  (torch_gpu: the fixture)

pytestmark = pytest.mark.gpu


def _scenes(torch, c, dtype):
    """(emit scene (3, he, we) with the matching band at 1, S2 scene (2, hs, ws) with the matching band at 0), on the device."""
    emit = np.stack([c["emit"] * 0.5, c["emit"], 1.0 - c["emit"]]).astype(np.float32)
    other = np.roll(c["s2"], 17, axis=1)
    s2 = np.stack([c["s2"], other])
    return torch.from_numpy(emit).cuda(), torch.from_numpy(s2).cuda(), s2


def _pinv_bound(table, err, hs, ws, kind_used):
    """|delta coefficient| <= |pinv(X)| @ |delta d| in the scaled coordinates, per shift component: (2, 3)."""
    use, X, _ = cc._design(table, hs, ws)
    if kind_used == 1:
        P = np.abs(np.linalg.pinv(X))
    else:
        P = np.zeros((3, int(use.sum())))
        P[0] = 1.0 / use.sum()
    return np.stack([P @ err[use, 0], P @ err[use, 1]])


@pytest.mark.parametrize("dtype", ["f32", "u16"])
@pytest.mark.parametrize("name", list(cc.E2E_MODELS))
def test_coregister_scene(torch_gpu, name, dtype):
    _coregister_scene(torch_gpu, name, dtype, False)


@pytest.mark.parametrize("dtype", ["f32", "u16"])
@pytest.mark.parametrize("name", list(cc.E2E_MODELS))
def test_coregister_scene_rectangular(torch_gpu, name, dtype):
    """The same assertions on the 48 x 60 EMIT / 293 x 360 S2 pair: he != we, and an S2 scene five rows longer than f he."""
    _coregister_scene(torch_gpu, name, dtype, True)


def _coregister_scene(torch, name, dtype, rect):
    c = cc.e2e_case(name, dtype, rect)
    p = c["params"]
    emit_t, s2_t, s2_np = _scenes(torch, c, dtype)
    kw = dict(emit_band=1, s2_band=0, factor=p["f"], window=p["w"], step=p["step"], max_shift=p["R"],
              min_valid_frac=p["min_valid_frac"], min_score=p["min_score"], model=name, reject_px=p["reject_px"])
    out = s2_emit.coregister_scene(emit_t, s2_t, **kw)                       # warm-up: code objects, the allocator's blocks
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = s2_emit.coregister_scene(emit_t, s2_t, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert isinstance(out, s2_emit.CoregOutput) and out.s2.is_cuda and out.s2.dtype == s2_t.dtype and out.s2.shape == s2_t.shape
    assert out.s2.data_ptr() != s2_t.data_ptr() and out.model.params.is_cuda and out.tie_points.table.is_cuda
    assert np.array_equal(out.tie_points.origins.cpu().numpy(), c["origins"])
    # tie points
    surface, table, model = (t.cpu().numpy() for t in (out.tie_points.surface, out.tie_points.table, out.model.params))
    fin = np.isfinite(c["surface"])
    assert np.array_equal(np.isfinite(surface), fin) and (np.abs(surface - c["surface"])[fin] <= c["bar"][fin]).all()
    assert np.array_equal(table[:, 7], c["table"][:, 7]) and table[cc.DECOY, 7] == cc.OUTLIER
    bound, den_min = cc.shift_bar(c["surface"], c["bar"], c["table0"], p["R"])
    admitted = (c["table"][:, 7] == cc.OK) & (den_min >= 1e-3)
    assert admitted.sum() == len(table) - 1
    err = np.abs(table[:, 2:4] - c["table"][:, 2:4])
    print(f"{name} {dtype}: largest shift difference {err[admitted].max():.3g} S2 pixels, bound {bound[admitted].max():.3g}")
    assert (err[admitted] <= bound[admitted]).all()
    assert np.array_equal(table[:, [0, 1]], c["table"][:, [0, 1]]) and np.array_equal(table[:, 6], c["table"][:, 6])
    # the model
    assert (model[9], model[8]) == (c["model"][9], c["model"][8]) == (1 if name == "affine" else 0, len(table) - 1)
    diff = np.abs(cc.scaled_coefficients(model, c["hs"], c["ws"]) - c["coef"])
    allowed = c["model_bar"] + _pinv_bound(c["table"], bound, c["hs"], c["ws"], model[9])
    print(f"{name} {dtype}: largest coefficient difference {diff.max():.3g}, allowed {allowed.max():.3g}")
    assert (diff <= allowed).all()
    # the warp, under the kernel's own model
    fill = float("nan") if dtype == "f32" else 0.0
    want, _ = cc.warp_ref(s2_np, model, None, fill)
    got = out.s2.cpu().numpy()
    if dtype == "f32":
        bits_equal(got, want, f"{name} warp")
    else:
        assert np.array_equal(got, want)
    assert out.model.max_abs_shift == p["R"] + 1 and cc.warp_instance(dtype, out.model.max_abs_slope).endswith("LDS>")
    # the corrected band lines up with EMIT again: outside the border and the decoy window its block mean IS the EMIT band up to
    # the residual shift (<= 0.25 S2 pixel, 1 / 24 of an EMIT pixel) and the spline - the reference warp gives 0.99999 - while
    # the uncorrected band is 2.7 - 4.3 S2 pixels off (0.76 / 0.89, on the square pair and on the rectangular one)
    if dtype == "f32":
        keep = np.ones((p["he"], p["we"]), bool)
        keep[:3] = keep[-3:] = keep[:, :3] = keep[:, -3:] = False
        i0, j0 = c["origins"][cc.DECOY]
        keep[i0:i0 + p["w"], j0:j0 + p["w"]] = False

        def corr(plane):
            bm = plane[:p["he"] * p["f"], :p["we"] * p["f"]].reshape(p["he"], p["f"], p["we"], p["f"]).mean(axis=(1, 3))
            return np.corrcoef(bm[keep], c["emit"][keep])[0, 1]
        assert corr(got[0]) > 0.999 > 0.95 > corr(s2_np[0])
    # into the next stage, unchanged in type
    tiles = s2_emit.find_valid_paired_tiles(emit_t, out.s2, emit_tile_size=16, scale=p["f"], max_black_frac=1.0)
    before = s2_emit.find_valid_paired_tiles(emit_t, s2_t, emit_tile_size=16, scale=p["f"], max_black_frac=1.0)
    assert len(tiles) == len(before) == 9 and [t.keys() for t in tiles] == [t.keys() for t in before]
    assert (out.tie_points.s2_shape, tuple(out.s2.shape[1:])) == ((c["hs"], c["ws"]),) * 2


def test_stages_on_arrays_and_views(torch_gpu):
    """NumPy in gives NumPy out; a band view of a scene and a precomputed EMIT plane pass without a copy; warp_scene into `out`."""
    torch = torch_gpu
    c, p = cc.e2e_case("translation", "f32"), cc.E2E
    emit_t, s2_t, s2_np = _scenes(torch, c, "f32")
    kw = dict(window=p["w"], step=p["step"], factor=p["f"], max_shift=p["R"])
    tp = s2_emit.match_windows(emit_t[1], s2_t[0], **kw)
    tp_np = s2_emit.match_windows(c["emit"], c["s2"], **kw)
    assert isinstance(tp_np.table, np.ndarray) and np.array_equal(tp.table.cpu().numpy(), tp_np.table)
    assert np.array_equal(tp.surface.cpu().numpy(), tp_np.surface, equal_nan=True)
    sm = s2_emit.fit_shift_model(tp, model="translation")
    sm_np = s2_emit.fit_shift_model(tp_np, model="translation")                          # array records: the host twin
    assert np.array_equal(tp.table.cpu().numpy()[:, 7], tp_np.table[:, 7]) and tp_np.table[cc.DECOY, 7] == cc.OUTLIER
    assert np.abs(sm.params.cpu().numpy() - sm_np.params).max() <= 1e-12
    out = torch.full_like(s2_t, -5.0)
    res = s2_emit.warp_scene(s2_t, sm, out=out)
    assert res.data_ptr() == out.data_ptr()
    bits_equal(out.cpu().numpy(), cc.warp_ref(s2_np, sm.params.cpu().numpy(), None, float("nan"))[0], "warp into out")
    same = s2_emit.warp_scene(s2_np, sm)
    assert isinstance(same, np.ndarray)
    bits_equal(same, out.cpu().numpy(), "warp of an array")
    full = s2_emit.coregister_scene(None, s2_t, emit_band=emit_t[1], s2_band=0, model="translation", **kw)   # a precomputed plane
    bits_equal(full.s2.cpu().numpy(), out.cpu().numpy(), "coregister_scene with an EMIT plane")
    with pytest.raises(s2_emit.HsrError, match="aliases"):
        s2_emit.warp_scene(s2_t, sm, out=s2_t)


# ---- the parts of the public functions beyond the plain call: masks, nodata, grids, arrays, views, the identity --------------------------
def _match_kw(p):
    return dict(window=p["w"], step=p["step"], factor=p["f"], max_shift=p["R"], min_valid_frac=p["min_valid_frac"], min_score=p["min_score"])


def _same_tie_points(a, b, what):
    """Two TiePoints, device or array: origins, surfaces and records bit for bit."""
    get = lambda t: t if isinstance(t, np.ndarray) else t.cpu().numpy()                      # noqa: E731
    assert np.array_equal(get(a.origins), get(b.origins)), what
    same_bits(get(a.surface), get(b.surface), what + ": surface")
    same_bits(get(a.table), get(b.table), what + ": records")


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_emit_mask_and_s2_nodata(torch_gpu, dtype):
    """match_windows and coregister_scene with an EMIT mask in every form it may take and an S2 nodata value (NaN and inf beside it
    for float32): the surfaces within the bars of surface_ref under the same mask and nodata, NaN in the same places; the records
    bit-equal to peaks_ref of the device's own surfaces, with the reference's statuses; the warp bit-equal under the device's
    model with the same nodata.  The device path issues no blocking synchronisation."""
    torch = torch_gpu
    c = cc.masked_case(dtype)
    p, he, we = c["params"], c["params"]["he"], c["params"]["we"]
    emit_t, s2_t, s2_np = _scenes(torch, c, dtype)
    mask_t = torch.from_numpy(c["mask"].copy()).cuda()
    kw = _match_kw(p)
    tp = s2_emit.match_windows(emit_t[1], s2_t[0], emit_mask=mask_t, s2_nodata=c["nodata"], **kw)
    surface, table = tp.surface.cpu().numpy(), tp.table.cpu().numpy()
    assert np.array_equal(tp.origins.cpu().numpy(), c["origins"])
    fin = np.isfinite(c["surface"])
    assert np.array_equal(np.isfinite(surface), fin) and np.array_equal(np.isnan(surface), ~fin)
    err = np.abs(surface - c["surface"])[fin]
    print(f"masked {dtype}: {int(fin.sum())} finite entries, worst |err| / bar {np.max(err / c['bar'][fin]):.3g}")
    assert (err <= c["bar"][fin]).all()
    same_bits(table, cc.peaks_ref(surface, c["origins"], p["w"], p["f"], p["R"], he, we, c["hs"], c["ws"], p["min_score"]), "records")
    assert np.array_equal(table[:, 7], c["table0"][:, 7]) and set(table[:, 7]) == {cc.OK, cc.NO_SCORE} and (table[:, 7] != cc.OK).sum() >= 3
    # the same mask in its other forms
    wide = torch.ones((he, we + 7), dtype=torch.uint8, device="cuda")
    wide[:, 3:3 + we] = mask_t
    assert wide[:, 3:3 + we].stride(0) == we + 7
    forms = {"bool tensor": mask_t != 0, "bool array": c["mask"] != 0, "uint8 array": c["mask"], "column slice": wide[:, 3:3 + we],
             "bool column slice": (wide != 0)[:, 3:3 + we]}
    for what, m in forms.items():
        _same_tie_points(s2_emit.match_windows(emit_t[1], s2_t[0], emit_mask=m, s2_nodata=c["nodata"], **kw), tp, what)
    strided = torch.ones((he, 2 * we), dtype=torch.uint8, device="cuda")[:, ::2]
    assert strided.shape == mask_t.shape
    with pytest.raises(ValueError, match="emit_mask"):
        s2_emit.match_windows(emit_t[1], s2_t[0], emit_mask=strided, s2_nodata=c["nodata"], **kw)
    with pytest.raises(ValueError, match="emit_mask"):
        s2_emit.match_windows(emit_t[1], s2_t[0], emit_mask=mask_t[:-1], s2_nodata=c["nodata"], **kw)
    # without the mask, and without the nodata value, the surfaces are others
    for other in (s2_emit.match_windows(emit_t[1], s2_t[0], s2_nodata=c["nodata"], **kw),
                  s2_emit.match_windows(emit_t[1], s2_t[0], emit_mask=mask_t, **kw)):
        o = other.surface.cpu().numpy()
        assert not np.array_equal(np.isfinite(o), fin) or (np.abs(o - c["surface"])[fin] > c["bar"][fin]).any()
    # the whole chain, on the device, without a blocking synchronisation
    ckw = dict(kw, emit_band=1, s2_band=0, emit_mask=mask_t, s2_nodata=c["nodata"], model="translation")
    ckw.pop("step")
    out = s2_emit.coregister_scene(emit_t, s2_t, step=p["step"], **ckw)                          # warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = s2_emit.coregister_scene(emit_t, s2_t, step=p["step"], **ckw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    same_bits(out.tie_points.surface.cpu().numpy(), surface, "surface of the chain")
    got_t, model = out.tie_points.table.cpu().numpy(), out.model.params.cpu().numpy()
    want_t, want_m, coef, mbar = cc.model_ref(table, 0, 1, 1.0, c["hs"], c["ws"])                # the reference fit of the device's records
    assert np.array_equal(got_t[:, 7], want_t[:, 7]) and got_t[cc.DECOY, 7] == cc.OUTLIER and (model[9], model[8]) == (0, want_m[8])
    assert np.abs(cc.scaled_coefficients(model, c["hs"], c["ws"]) - coef).max() <= mbar
    fill = float("nan") if dtype == "f32" else float(c["nodata"])
    want, raw = cc.warp_ref(s2_np, model, c["nodata"], fill)
    assert np.isnan(raw).sum() > 2 * (~cc.s2_valid(s2_np, c["nodata"])).sum()                    # the nodata costs its neighbourhood
    if dtype == "f32":
        bits_equal(out.s2.cpu().numpy(), want, "warp with nodata")
    else:
        assert np.array_equal(out.s2.cpu().numpy(), want)


def test_grid_forms_and_thinning(torch_gpu):
    """grid= as a list, an int64 array and a device tensor; max_points below the full grid: the origins are tie_point_grid's and
    every record equals the matching row of the full run bit for bit."""
    torch = torch_gpu
    c = cc.e2e_case("translation", "f32", True)
    p = c["params"]
    emit_t, s2_t, _ = _scenes(torch, c, "f32")
    kw = _match_kw(p)
    full = s2_emit.match_windows(emit_t[1], s2_t[0], **kw)
    origins, surface, table = (t.cpu().numpy() for t in (full.origins, full.surface, full.table))
    assert np.array_equal(origins, c["origins"]) and len(origins) == 35
    pick = [31, 4, 17, 0, 34, 12]
    sub = origins[pick]
    grids = {"list": [tuple(int(v) for v in r) for r in sub], "int64 array": sub.astype(np.int64),
             "device tensor": torch.from_numpy(sub.astype(np.int64)).cuda(), "int32 device tensor": torch.from_numpy(sub.copy()).cuda()}
    for what, g in grids.items():
        tp = s2_emit.match_windows(emit_t[1], s2_t[0], grid=g, **kw)
        assert tp.origins.dtype == torch.int32 and np.array_equal(tp.origins.cpu().numpy(), sub), what
        same_bits(tp.surface.cpu().numpy(), surface[pick], what + ": surface")
        same_bits(tp.table.cpu().numpy(), table[pick], what + ": records")
    # an origin outside the planes among them: its record says so, the others are what they were
    tp = s2_emit.match_windows(emit_t[1], s2_t[0], grid=[(1, 1), (41, 1), (1, 53), (9, 41)], **kw)
    t = tp.table.cpu().numpy()
    assert list(t[:, 7]) == [cc.OK, cc.OUTSIDE, cc.OUTSIDE, cc.OK] and np.isnan(tp.surface.cpu().numpy()[1:3]).all()
    same_bits(t[[0, 3]], table[[0, cc.DECOY]], "records beside outside origins")
    for n in (10, 1, 34):
        want = s2_emit.tie_point_grid(p["he"], p["we"], c["hs"], c["ws"], window=p["w"], step=p["step"], factor=p["f"], max_shift=p["R"],
                                      max_points=n)
        tp = s2_emit.match_windows(emit_t[1], s2_t[0], max_points=n, **kw)
        got = tp.origins.cpu().numpy()
        assert len(want) == n and np.array_equal(got, want)
        rows = [int(np.flatnonzero((origins == o).all(axis=1))[0]) for o in got]
        assert len(set(rows)) == n
        same_bits(tp.surface.cpu().numpy(), surface[rows], f"max_points={n}: surface")
        same_bits(tp.table.cpu().numpy(), table[rows], f"max_points={n}: records")
    out = s2_emit.coregister_scene(emit_t, s2_t, emit_band=1, s2_band=0, model="translation", max_points=10, **kw)
    assert out.tie_points.table.shape == (10, 8) and out.model.params.cpu().numpy()[8] <= 10


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_arrays_in_arrays_out(torch_gpu, dtype):
    """coregister_scene on NumPy scenes: every field comes back as an array, bit-equal to the run on device tensors."""
    torch = torch_gpu
    c = cc.e2e_case("affine", dtype, True)
    p = c["params"]
    emit_t, s2_t, s2_np = _scenes(torch, c, dtype)
    emit_np = emit_t.cpu().numpy()
    assert s2_np.dtype == (np.uint16 if dtype == "u16" else np.float32)
    kw = dict(_match_kw(p), emit_band=1, s2_band=0, model="affine", reject_px=p["reject_px"])
    dev = s2_emit.coregister_scene(emit_t, s2_t, **kw)
    arr = s2_emit.coregister_scene(emit_np, s2_np, **kw)
    assert isinstance(arr, s2_emit.CoregOutput) and isinstance(arr.s2, np.ndarray) and arr.s2.dtype == s2_np.dtype
    assert isinstance(arr.model.params, np.ndarray) and arr.model.params.shape == (10,) and arr.model.params.dtype == np.float64
    assert all(isinstance(v, np.ndarray) for v in (arr.tie_points.table, arr.tie_points.surface, arr.tie_points.origins))
    assert arr.tie_points.origins.dtype == np.int32 and arr.tie_points.s2_shape == (c["hs"], c["ws"]) == dev.tie_points.s2_shape
    _same_tie_points(arr.tie_points, dev.tie_points, "array run")
    same_bits(arr.model.params, dev.model.params.cpu().numpy(), "params")
    assert (arr.model.max_abs_shift, arr.model.max_abs_slope) == (dev.model.max_abs_shift, dev.model.max_abs_slope)
    assert np.array_equal(arr.s2.view(np.uint8), dev.s2.cpu().numpy().view(np.uint8))
    assert arr.tie_points.table[cc.DECOY, 7] == cc.OUTLIER and arr.model.params[9] == 1
    # a read-only array, and an EMIT plane given as an array beside a device scene
    ro = s2_np.copy()
    ro.setflags(write=False)
    again = s2_emit.coregister_scene(None, ro, **dict(kw, emit_band=emit_np[1]))
    assert np.array_equal(again.s2.view(np.uint8), arr.s2.view(np.uint8))


def test_scene_views_and_out(torch_gpu):
    """S2 scenes that are views - a band gap, a wider row stride, a non-unit column stride (copied) - give the bits of their
    contiguous clones; an `out` that is a view is filled and nothing around it is written."""
    torch = torch_gpu
    c = cc.e2e_case("affine", "f32", True)
    p = c["params"]
    emit_t, s2_t, s2_np = _scenes(torch, c, "f32")
    hs, ws = c["hs"], c["ws"]
    kw = dict(_match_kw(p), emit_band=1, s2_band=0, model="affine")
    four = torch.stack([s2_t[0], s2_t[1], s2_t[1] * 0.5, s2_t[0] + 1.0])
    interleaved = torch.stack([s2_t, s2_t + 3.0], dim=-1)                                        # (2, hs, ws, 2)
    views = {"band gap": four[::2], "row stride": s2_t[:, :, 3:-2], "band gap and row stride": four[::2, :, :-3],
             "column stride": interleaved[..., 0]}
    plain = s2_emit.coregister_scene(emit_t, s2_t, **kw)
    assert views["band gap"].stride(0) == 2 * hs * ws and views["row stride"].stride(1) == ws and views["column stride"].stride(2) == 2
    for what, v in views.items():
        assert not v.is_contiguous(), what
        a, b = s2_emit.coregister_scene(emit_t, v, **kw), s2_emit.coregister_scene(emit_t, v.clone(memory_format=torch.contiguous_format), **kw)
        assert a.s2.shape == v.shape and a.tie_points.s2_shape == tuple(v.shape[1:])
        _same_tie_points(a.tie_points, b.tie_points, what)
        same_bits(a.model.params.cpu().numpy(), b.model.params.cpu().numpy(), what + ": params")
        bits_equal(a.s2.cpu().numpy(), b.s2.cpu().numpy(), what + ": warped scene")
        if what in ("band gap", "column stride"):                                               # band 0 is the plain scene's
            _same_tie_points(a.tie_points, plain.tie_points, what + " against the plain scene")
            bits_equal(a.s2[0].cpu().numpy(), plain.s2[0].cpu().numpy(), what + ": band 0 against the plain scene")
            assert a.model.params.cpu().numpy()[9] == 1
    big = torch.full((4, hs + 2, ws + 9), -7.0, dtype=torch.float32, device="cuda")
    out = big[::2, 1:-1, 4:4 + ws]
    assert out.shape == s2_t.shape and (out.stride(0), out.stride(1)) == (2 * (hs + 2) * (ws + 9), ws + 9)
    res = s2_emit.coregister_scene(emit_t, s2_t, out=out, **kw)
    assert res.s2.data_ptr() == out.data_ptr() and res.s2.stride() == out.stride()
    bits_equal(out.cpu().numpy(), plain.s2.cpu().numpy(), "out view")
    around = torch.ones_like(big, dtype=torch.bool)
    around[::2, 1:-1, 4:4 + ws] = False
    assert (big[around] == -7.0).all() and int(around.sum()) == big.numel() - out.numel()
    sm = plain.model
    u16 = torch.from_numpy(np.round(np.clip(s2_np, 0, 1) * 10000).astype(np.uint16)).cuda()
    big16 = torch.from_numpy(np.full((2, hs, ws + 3), 777, np.uint16)).cuda()
    s2_emit.warp_scene(u16, sm, out=big16[:, :, 2:2 + ws])
    after = big16.cpu().numpy()
    assert np.array_equal(after[:, :, 2:2 + ws], cc.warp_ref(u16.cpu().numpy(), sm.params.cpu().numpy(), None, 0.0)[0])
    assert (after[:, :, :2] == 777).all() and (after[:, :, 2 + ws:] == 777).all()
    with pytest.raises(ValueError, match="out"):
        s2_emit.warp_scene(s2_t, sm, out=interleaved[..., 1])


@pytest.mark.parametrize("way", ["min-points", "no-window", "masked"])
@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_identity_outcomes(torch_gpu, dtype, way):
    """The three ways to no model - min_points above the usable tie points, a scene too small for one window (no tie point at all),
    a wholly masked EMIT plane: the zero model with kind_used -1, nothing raises, and the output is the input where it is valid and
    fill elsewhere (NaN for float32; for uint16 the nodata value, so the scene as it was)."""
    torch = torch_gpu
    c = cc.masked_case(dtype)
    p = c["params"]
    emit_t, s2_t, s2_np = _scenes(torch, c, dtype)
    kw = dict(_match_kw(p), emit_band=1, s2_band=0, s2_nodata=c["nodata"])
    if way == "min-points":
        kw.update(min_points=33, emit_mask=c["mask"])                                            # 35 tie points, 32 of them usable
    elif way == "masked":
        kw["emit_mask"] = torch.zeros(emit_t.shape[1:], dtype=torch.bool, device="cuda")
    else:
        emit_t = emit_t[:, :7, :40].contiguous()                                                 # 7 rows: no 8 x 8 window
        s2_t, s2_np = s2_t[:, 170:212, 60:300].contiguous(), np.ascontiguousarray(s2_np[:, 170:212, 60:300])
    invalid = ~cc.s2_valid(s2_np, c["nodata"])
    assert invalid.sum() > 100 and (dtype == "u16" or (np.isnan(s2_np).any() and np.isinf(s2_np).any()))
    for model in ("affine", "translation"):
        out = s2_emit.coregister_scene(emit_t, s2_t, model=model, **kw)
        params, table = out.model.params.cpu().numpy(), out.tie_points.table.cpu().numpy()
        assert params[9] == -1 and not params[:9].any() and params.shape == (10,)
        P = {"min-points": 35, "masked": 35, "no-window": 0}[way]
        assert table.shape == (P, 8) and out.tie_points.surface.shape == (P, 13, 13) and out.tie_points.origins.shape == (P, 2)
        if way == "masked":
            assert (table[:, 7] == cc.NO_SCORE).all() and np.isnan(out.tie_points.surface.cpu().numpy()).all()
        if way == "min-points":
            assert np.array_equal(table[:, 7], c["table0"][:, 7]) and (table[:, 7] == cc.OK).sum() == 32   # no fit: no rejection pass
        got = out.s2.cpu().numpy()
        assert got.shape == s2_np.shape and got.dtype == s2_np.dtype and out.s2.data_ptr() != s2_t.data_ptr()
        if dtype == "f32":
            assert np.isnan(got[invalid]).all() and np.array_equal(got[~invalid].view(np.uint32), s2_np[~invalid].view(np.uint32))
        else:
            assert (got[invalid] == c["nodata"]).all() and np.array_equal(got, s2_np)
    # the stages one by one on arrays: the host twin gives the same zero model
    if way == "no-window":
        tp = s2_emit.match_windows(emit_t[1].cpu().numpy(), s2_np[0], **_match_kw(p))
        assert tp.table.shape == (0, 8) and tp.surface.shape == (0, 13, 13) and tp.origins.shape == (0, 2)
        sm = s2_emit.fit_shift_model(tp)
        assert sm.params[9] == -1 and not sm.params[:9].any()
