"""The public affine colour functions on an MI355X: fit_ot_affine_rgb / apply_affine_rgb against fixture g17 (the notebook's own
functions), ot_match_rgb_sinkhorn_pot with GPU tensors against the oracle, fit_affine_rgb against np.linalg.lstsq, and
match_pair(model="affine") against a float64 restatement composed from the oracle's planes and the references of
tests/affine_cases.py.

Bars:
  maps      fitted (A, t) against a reference (A, t) as the largest difference of the two maps over the 9 x 9 x 9 grid of [0, 1]^3:
            OT fits of the public functions at 5e-5, the bar tests/test_gpu_parity.py:1340-1345 holds this family to (device
            Sinkhorn against the oracle's restatement of POT's documented algorithm); least-squares fits at
            affine_cases.solve_bar (64 kappa eps max(1, |W|)).
  apply     bit-equal to affine_cases.apply_ref; against the notebook's matmul in g17, 2^-24 + 8 eps (|x| |A| + |t|).
  driver    images at 60 m under valid60 and at 10 m under mask10 atol 1e-5, NaNs of the 10 m image in the same places, the map
            atol 2e-6 - IMAGE_ATOL and CURVE_ATOL of tests/test_gpu_match_pair_cases.py:37-38, applied there at :119-122.
"""
import warnings

import numpy as np
import pytest

import affine_cases as ac
import match_pair_cases as mpc
from conftest import load_golden
from gpu_harness import bits_equal, same_bits, torch_gpu  # noqa: F401
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

OT_ATOL = 5e-5
IMAGE_ATOL, CURVE_ATOL = 1e-5, 2e-6
IDENTITY = np.concatenate([np.eye(3), np.zeros((1, 3))])


def _W(A, t):
    A = A.cpu().numpy() if hasattr(A, "cpu") else np.asarray(A)
    t = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    assert A.shape == (3, 3) and t.shape == (3,) and A.dtype == np.float64 and t.dtype == np.float64
    return np.concatenate([A, t[None, :]])


def test_fit_ot_affine_rgb_against_g17(torch_gpu):
    torch = torch_gpu
    import s2_emit
    g = load_golden("g17_affine")
    src, ref, mask = g["src"], g["ref"], g["mask"]
    A, t = s2_emit.fit_ot_affine_rgb(src, ref, mask, n_samples=600, seed=3)
    assert isinstance(A, np.ndarray) and isinstance(t, np.ndarray)
    diff = ac.grid_diff(_W(A, t), _W(g["A"], g["t"]))
    print(f"fit_ot_affine_rgb vs g17: {diff:.3g} (bar {OT_ATOL})")
    assert diff <= OT_ATOL
    At, tt = s2_emit.fit_ot_affine_rgb(torch.from_numpy(src).cuda(), torch.from_numpy(ref).cuda(), torch.from_numpy(mask).cuda(),
                                       n_samples=600, seed=3)
    assert At.is_cuda and tt.is_cuda
    same_bits(_W(At, tt), _W(A, t), "tensor input against NumPy input")
    # too few rows: the identity, for both input kinds
    A1, t1 = s2_emit.fit_ot_affine_rgb(src, ref, g["mask_one"], n_samples=600, seed=3)
    assert np.array_equal(_W(A1, t1), IDENTITY) and np.array_equal(_W(g["A_one"], g["t_one"]), IDENTITY)
    A1, t1 = s2_emit.fit_ot_affine_rgb(torch.from_numpy(src).cuda(), torch.from_numpy(ref).cuda(), torch.from_numpy(g["mask_one"]).cuda())
    assert A1.is_cuda and np.array_equal(_W(A1, t1), IDENTITY)


def test_apply_affine_rgb_against_g17(torch_gpu):
    torch = torch_gpu
    import s2_emit
    g = load_golden("g17_affine")
    src, mask = g["src"], g["mask"]
    rows = src.reshape(-1, 3)
    x64 = np.abs(np.nan_to_num(rows.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0))
    for tag, A, t in (("fit", g["A"], g["t"]), ("hand", g["At_hand"][:9].reshape(3, 3), g["At_hand"][9:])):
        At = np.concatenate([A.reshape(-1), t])
        for mtag, m in (("mask", mask), ("nomask", None)):
            before = src.copy()
            got = s2_emit.apply_affine_rgb(src, A, t, m)
            assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == src.shape
            np.testing.assert_array_equal(src.view(np.uint32), before.view(np.uint32))                 # the input is not modified
            bits_equal(got.reshape(-1, 3), ac.apply_ref(rows, At, None if m is None else m.reshape(-1), None, 1), f"{tag} {mtag}")
            want = g[f"out_{tag}_{mtag}"]
            assert np.array_equal(np.isnan(got), np.isnan(want))
            bound = 2.0 ** -24 + 8 * ac.EPS * (x64 @ np.abs(A) + np.abs(t)).reshape(src.shape)
            ok = ~np.isnan(want)
            assert (np.abs(got.astype(np.float64) - want)[ok] <= bound[ok]).all(), (tag, mtag)
            xt = torch.from_numpy(src).cuda()
            gt = s2_emit.apply_affine_rgb(xt, torch.from_numpy(A).cuda(), torch.from_numpy(t).cuda(),
                                          None if m is None else torch.from_numpy(m).cuda())
            assert gt.is_cuda and gt.dtype == torch.float32 and gt.data_ptr() != xt.data_ptr()
            bits_equal(gt.cpu().numpy(), got, f"{tag} {mtag}: tensor input against NumPy input")
            bits_equal(xt.cpu().numpy(), src, "the input tensor is not modified")
    # channels beyond the third pass through as float32
    for extra in (1, 2):
        wide = np.concatenate([src, np.full(src.shape[:2] + (extra,), 0.25, np.float64).astype(np.float32) + np.arange(extra, dtype=np.float32)], axis=2)
        got = s2_emit.apply_affine_rgb(wide.astype(np.float64), g["A"], g["t"], mask)
        assert got.dtype == np.float32 and got.shape == wide.shape
        bits_equal(got[..., :3], ac.apply_ref(rows, np.concatenate([g["A"].reshape(-1), g["t"]]), mask.reshape(-1), None, 1).reshape(src.shape),
                   "wide")
        bits_equal(got[..., 3:], wide[..., 3:], "channels beyond the third")


def test_ot_match_rgb_sinkhorn_pot_with_tensors(torch_gpu):
    """The inputs of test_ot_color_transfer_and_ot_fit_vs_oracle (tests/test_gpu_parity.py:1326) as GPU tensors."""
    torch = torch_gpu
    import s2_emit
    rng = np.random.default_rng(77)
    H, W = 48, 40
    src = rng.random((H, W, 3)) ** 1.5
    ref = np.clip(0.8 * src[..., ::-1] + 0.1 + 0.03 * rng.standard_normal((H, W, 3)), 0, 1)
    mask = rng.random((H, W)) > 0.15
    src[2, 3, 1] = np.nan
    src, ref = src.astype(np.float32), ref.astype(np.float32)
    xt, yt, mt = torch.from_numpy(src).cuda(), torch.from_numpy(ref).cuda(), torch.from_numpy(mask).cuda()
    got_t = s2_emit.ot_match_rgb_sinkhorn_pot(xt, yt, mt, n_samples=700, seed=3)
    assert got_t.is_cuda and got_t.dtype == torch.float32 and tuple(got_t.shape) == src.shape
    got = got_t.cpu().numpy()
    want = onp.ot_match_rgb_sinkhorn_pot(src, ref, mask, n_samples=700, seed=3)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    d = float(np.max(np.abs(got[~np.isnan(want)].astype(np.float64) - want[~np.isnan(want)])))
    print(f"ot_match_rgb_sinkhorn_pot (tensors) vs oracle: {d:.3g} (bar {OT_ATOL})")
    np.testing.assert_allclose(got[~np.isnan(want)], want[~np.isnan(want)], rtol=0, atol=OT_ATOL)
    bits_equal(xt.cpu().numpy(), src, "the source tensor is not modified")
    # too few rows: a clone of the source
    tiny = torch.zeros((H, W), dtype=torch.bool, device="cuda")
    tiny[0, 0] = True
    clone = s2_emit.ot_match_rgb_sinkhorn_pot(xt, yt, tiny)
    assert clone.is_cuda and clone.data_ptr() != xt.data_ptr()
    bits_equal(clone.cpu().numpy(), src, "tiny mask")


def test_fit_affine_rgb_against_lstsq(torch_gpu):
    torch = torch_gpu
    import s2_emit
    g = load_golden("g17_affine")
    src, ref, mask = g["src"], g["ref"], g["mask"]
    for lohi_s, lohi_r in ((None, None), (ac.LOHI_PLAIN, ac.LOHI_Y)):
        xs, ys = ac.stretch(src.reshape(-1, 3), lohi_s), ac.stretch(ref.reshape(-1, 3), lohi_r)
        ok = ac.usable(src.reshape(-1, 3), ref.reshape(-1, 3), mask.reshape(-1))
        xs, ys = xs[ok].astype(np.float64), ys[ok].astype(np.float64)
        W = ac.lstsq_ref(xs, ys, 200)
        bar, kappa = ac.solve_bar(xs, W)
        A, t = s2_emit.fit_affine_rgb(src, ref, mask, lohi_src=lohi_s, lohi_ref=lohi_r)
        diff = ac.grid_diff(_W(A, t), W)
        print(f"fit_affine_rgb (stretch {lohi_s is not None}): diff {diff:.3g}, kappa {kappa:.3g}, ratio {diff * 64 / bar:.2f} of 64")
        assert diff <= bar
        At, tt = s2_emit.fit_affine_rgb(torch.from_numpy(src).cuda(), torch.from_numpy(ref).cuda(), torch.from_numpy(mask).cuda(),
                                        lohi_src=lohi_s, lohi_ref=None if lohi_r is None else torch.from_numpy(lohi_r).cuda())
        assert At.is_cuda
        same_bits(_W(At, tt), _W(A, t), "tensor input against NumPy input")
    A, t = s2_emit.fit_affine_rgb(src, ref, mask, min_count=int(ok.sum()) + 1)
    assert np.array_equal(_W(A, t), IDENTITY)                                                          # below min_count
    assert not np.array_equal(_W(*s2_emit.fit_affine_rgb(src, ref, mask, min_count=int(ok.sum()))), IDENTITY)


def _driver_reference(name):
    """match_pair(model="affine") restated in float64 from the oracle's float32 planes, masks and limits of the row."""
    c, inp, o = mpc.CASES[name], mpc.inputs(name), mpc.oracle(name)
    H, W, f = c["H"], c["W"], c["f"]
    v, m10 = o["valid60"].reshape(-1), o["mask10"].reshape(-1)
    e60 = o["emit_60m"].reshape(3, -1).T
    e10 = o["emit_10m"].reshape(3, -1).T
    s60 = o["s2_60m"].reshape(3, -1).T
    en, sn = ac.stretch(e60, o["lohi_emit_60m"]), ac.stretch(s60, o["lohi_s2_60m"])
    if c["use_ot"]:
        kw = inp["kwargs"]
        s = onp._ot_samples(en.reshape(H, W, 3), sn.reshape(H, W, 3), o["valid60"], kw["n_samples"], 0, 2)
        X, Y = s
        Wm = ac.lstsq_ref(X, onp.ot_barycentric_targets(X, Y, 0.05, 300, 1e-6), 0)
    else:
        Wm = ac.lstsq_ref(en[v].astype(np.float64), sn[v].astype(np.float64), 200)
    At = Wm.reshape(-1)
    return dict(W=Wm, m60=ac.apply_ref(e60, At, v, o["lohi_emit_60m"], 2).reshape(H, W, 3),
                m10=ac.apply_ref(e10, At, m10, o["lohi_emit_10m"], 2).reshape(H * f, W * f, 3))


@pytest.mark.parametrize("name", ["anchor_lsq", "anchor_ot"])
def test_match_pair_affine(torch_gpu, name):
    import s2_emit
    c, inp, o = mpc.CASES[name], mpc.inputs(name), mpc.oracle(name)
    ref = _driver_reference(name)
    kw = {k: v for k, v in inp["kwargs"].items() if k != "deg"}
    got = s2_emit.match_pair(inp["R"], inp["w"], inp["srf"], inp["good"], inp["s2_hi"], inp["factor"], model="affine", **kw)
    assert set(got) == {"affine_A", "affine_t", "emit_rgb_matched_60m", "s2_rgb_60m_n", "valid60", "emit_rgb_10m_matched", "mask10",
                        "lohi_emit_60m", "lohi_s2_60m", "lohi_emit_10m"}
    v, m10 = o["valid60"], o["mask10"]
    np.testing.assert_array_equal(got["valid60"], v)
    np.testing.assert_array_equal(got["mask10"], m10)
    np.testing.assert_array_equal(got["s2_rgb_60m_n"], o["s2_rgb_60m_n"])
    dmap = ac.grid_diff(_W(got["affine_A"], got["affine_t"]), ref["W"])
    d60 = float(np.max(np.abs(got["emit_rgb_matched_60m"][v].astype(np.float64) - ref["m60"][v])))
    d10 = float(np.max(np.abs(got["emit_rgb_10m_matched"][m10].astype(np.float64) - ref["m10"][m10])))
    print(f"\nmatch_pair affine {name}: map {dmap:.2e} (bar {CURVE_ATOL:.0e})  60 m {d60:.2e}  10 m {d10:.2e} (bar {IMAGE_ATOL:.0e})")
    assert dmap <= CURVE_ATOL and d60 <= IMAGE_ATOL and d10 <= IMAGE_ATOL
    assert np.array_equal(np.isnan(got["emit_rgb_10m_matched"]), np.isnan(ref["m10"]))
    assert not np.array_equal(_W(got["affine_A"], got["affine_t"]), IDENTITY)
    fin = np.isfinite(got["emit_rgb_10m_matched"])
    assert got["emit_rgb_10m_matched"][fin].min() >= 0 and got["emit_rgb_10m_matched"][fin].max() <= 1       # clip_mode 2
    again = s2_emit.match_pair(inp["R"], inp["w"], inp["srf"], inp["good"], inp["s2_hi"], inp["factor"], model="affine", **kw)
    for k in got:
        np.testing.assert_array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(again[k]).view(np.uint8), err_msg=k)


def test_match_pair_default_model_is_poly(torch_gpu):
    import s2_emit
    inp = mpc.inputs("anchor_lsq")
    args = (inp["R"], inp["w"], inp["srf"], inp["good"], inp["s2_hi"], inp["factor"])
    a = s2_emit.match_pair(*args, **inp["kwargs"])
    b = s2_emit.match_pair(*args, **inp["kwargs"], model="poly")
    assert list(a) == list(b) and "coeffs" in a and "affine_A" not in a
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape
        np.testing.assert_array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8), err_msg=k)
    with pytest.raises(ValueError, match="model"):
        s2_emit.match_pair(*args, **inp["kwargs"], model="spline")
