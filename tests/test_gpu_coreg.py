"""coregister_scene end to end on an MI355X: a 48 x 48 EMIT / 288 x 288 S2 pair of tests/coreg_cases.py, displaced by a translation
and by an affine field, float32 and uint16, with a planted decoy window.

Against the reference chain of coreg_cases (long double surfaces -> float64 peaks -> np.linalg.lstsq):
  tie-point statuses equal the reference's (the table's margins make the peaks the same);
  shifts within 2 bar (|l - r| + |den|) / den^2 of the reference's - the surface bar carried through the parabola - on rows with
  |den| >= 1e-3 (tests/test_coreg_host.py checks that this is every row);
  the model within its bar plus that shift error carried through the least squares (|pinv(X)| times the per-record bound);
  the warped scene bit-equal to the NumPy warp UNDER THE KERNEL'S OWN MODEL;
  the output goes into find_valid_paired_tiles unchanged in type;
  the chain on device tensors issues no blocking synchronisation (torch's sync debug mode set to "error")."""
import numpy as np
import pytest

import coreg_cases as cc
import s2_emit
from gpu_harness import bits_equal, torch_gpu  # noqa: F401  (torch_gpu: the fixture)

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
    torch = torch_gpu
    c, p = cc.e2e_case(name, dtype), cc.E2E
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
    # the uncorrected band is 2.7 - 4.3 S2 pixels off (0.76 / 0.89)
    if dtype == "f32":
        keep = np.ones((p["he"], p["we"]), bool)
        keep[:3] = keep[-3:] = keep[:, :3] = keep[:, -3:] = False
        i0, j0 = c["origins"][cc.DECOY]
        keep[i0:i0 + p["w"], j0:j0 + p["w"]] = False

        def corr(plane):
            bm = plane.reshape(p["he"], p["f"], p["we"], p["f"]).mean(axis=(1, 3))
            return np.corrcoef(bm[keep], c["emit"][keep])[0, 1]
        assert corr(got[0]) > 0.999 > 0.95 > corr(s2_np[0])
    # into the next stage, unchanged in type
    tiles = s2_emit.find_valid_paired_tiles(emit_t, out.s2, emit_tile_size=16, scale=p["f"], max_black_frac=1.0)
    before = s2_emit.find_valid_paired_tiles(emit_t, s2_t, emit_tile_size=16, scale=p["f"], max_black_frac=1.0)
    assert len(tiles) == len(before) == 9 and [t.keys() for t in tiles] == [t.keys() for t in before]


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
