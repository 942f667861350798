"""s2_emit.match_pair - the reference driver (poly_regression.py:96-172) on three streams - against the float64 restatement
oracle.oracle_np.match_pair_reference, over the case table of tests/match_pair_cases.py (tests/test_match_pair_table.py checks on
the CPU that every row is what the table says).

Per row, on the same arrays:
  masks      valid60 and mask10 equal the oracle's; the planted pixels are false in valid60, the block of the -0.01 pixel true in mask10
  integers   s2_rgb_60m_n bit-identical (u8 / u16 sums are integers, the float32 rows hold multiples of 2^-12: exact in any order)
  limits     lohi_s2_60m == np.percentile(float32 block mean under valid60, [2, 98]) exactly;
             lohi_emit_60m / lohi_emit_10m within 2e-6 * max|plane| of np.percentile of the oracle's float32 planes under valid60 /
             mask10 - an order statistic moves by no more than the largest change of a sample, and a relative 2e-6 is the bar
             tests/test_gpu_k1_instances.py holds the K1 planes to
  curves     np.polyval over linspace(0, 1, 33), atol 2e-6 per channel    } the bars of test_match_pair_reference_driver, whose
  images     60 m under valid60 and 10 m under mask10, atol 1e-5; NaNs    } comment gives the stage-by-stage budget (a factor of 10
             of the 10 m image in the same places                         } is left); test_match_pair_table.py prints how far the
                                                                            oracle itself moves under a K1 error at its bar
  rule       rows below 200 valid pixels: coeffs exactly [0, .., 1, 0] and the matched images the bits of the clipped stretch (K3 without
             a polynomial on the same planes and limits); rows at 200 / 218: not the identity
  repeat     a second call returns the bits of the first for every key; rows 2 and 6 also from inside a non-default current stream
             with work queued in front (nothing waits on the host)
Every test prints its largest differences before it asserts.
"""
import warnings

import numpy as np
import pytest

from gpu_harness import torch_gpu  # noqa: F401
import match_pair_cases as mpc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

warnings.simplefilter("ignore")

KEYS = ("coeffs", "emit_rgb_matched_60m", "s2_rgb_60m_n", "valid60", "emit_rgb_10m_matched", "mask10",
        "lohi_emit_60m", "lohi_s2_60m", "lohi_emit_10m")
LIMIT_REL = 2e-6        # of max |plane|: the K1 bar
CURVE_ATOL = 2e-6
IMAGE_ATOL = 1e-5


def _host(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in res.items()}


def _call(torch, name):
    """One call of the driver on the row's inputs; the result as the driver returns it."""
    import s2_emit
    c, inp = mpc.CASES[name], mpc.inputs(name)
    R, s2 = inp["R"], inp["s2_hi"]
    extra = {}
    if c["device_inputs"]:
        H, W, B = R.shape
        wide = torch.zeros((H, W + 5, B), dtype=torch.float32, device="cuda")
        wide[:, 2:W + 2] = torch.from_numpy(R.copy()).cuda()
        R = wide[:, 2:W + 2]                                      # a slice of a wider tensor: rows are not adjacent
        assert not R.is_contiguous()
        s2 = torch.from_numpy(s2.copy()).cuda()
        extra["as_numpy"] = False
    return s2_emit.match_pair(R, inp["w"], inp["srf"], inp["good"], s2, inp["factor"], **inp["kwargs"], **extra)


def _same_bits(a, b, what):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        as_int = {4: np.int32, 8: np.int64}.get(a[k].dtype.itemsize, np.uint8)
        np.testing.assert_array_equal(a[k].view(as_int), b[k].view(as_int), err_msg=f"{what}: {k}")


@pytest.mark.parametrize("name", list(mpc.CASES))
def test_match_pair_case_vs_oracle(torch_gpu, name):
    torch = torch_gpu
    c, inp, ref = mpc.CASES[name], mpc.inputs(name), mpc.oracle(name)
    H, W, f, deg = c["H"], c["W"], c["f"], c["deg"]
    raw = _call(torch, name)
    assert set(raw) == set(KEYS)
    if c["device_inputs"]:
        assert all(type(v).__module__.startswith("torch") and v.is_cuda for v in raw.values())
    else:
        assert all(isinstance(v, np.ndarray) for v in raw.values())
    got = _host(raw)
    assert got["coeffs"].shape == (3, deg + 1) and got["coeffs"].dtype == np.float64
    assert got["emit_rgb_matched_60m"].shape == (H, W, 3) and got["emit_rgb_10m_matched"].shape == (H * f, W * f, 3)
    for k in ("lohi_emit_60m", "lohi_s2_60m", "lohi_emit_10m"):
        assert got[k].shape == (3, 2) and got[k].dtype == np.float64, k

    # ---- figures first
    xs = np.linspace(0, 1, 33)
    v, m10 = ref["valid60"], ref["mask10"]
    d_curve = max(float(np.max(np.abs(np.polyval(got["coeffs"][ch], xs) - np.polyval(ref["coeffs"][ch], xs)))) for ch in range(3))
    d60 = float(np.max(np.abs(got["emit_rgb_matched_60m"][v].astype(np.float64) - ref["emit_rgb_matched_60m"][v])))
    d10 = float(np.max(np.abs(got["emit_rgb_10m_matched"][m10].astype(np.float64) - ref["emit_rgb_10m_matched"][m10])))
    dl60 = float(np.max(np.abs(got["lohi_emit_60m"] - ref["lohi_emit_60m"]))) / ref["absmax_emit_60m"]
    dl10 = float(np.max(np.abs(got["lohi_emit_10m"] - ref["lohi_emit_10m"]))) / ref["absmax_emit_10m"]
    dls = float(np.max(np.abs(got["lohi_s2_60m"] - ref["lohi_s2_60m"])))
    print(f"\nMPCASE {name}: curves {d_curve:.2e} (bar {CURVE_ATOL:.0e})  60 m {d60:.2e} (bar {IMAGE_ATOL:.0e})  10 m {d10:.2e} (bar {IMAGE_ATOL:.0e})  "
          f"lohi_emit_60m {dl60:.2e}  lohi_emit_10m {dl10:.2e} (bar {LIMIT_REL:.0e} of max|plane|)  lohi_s2_60m {dls:.1e} (bar 0)  "
          f"masks differ at {int((got['valid60'] != v).sum())} / {int((got['mask10'] != m10).sum())} pixels", flush=True)

    # ---- masks and the integer path
    assert got["valid60"].dtype == np.bool_ and got["mask10"].dtype == np.bool_
    np.testing.assert_array_equal(got["valid60"], v)
    np.testing.assert_array_equal(got["mask10"], m10)
    assert int(got["valid60"].sum()) == c["n_valid"]
    for kind, (i, j) in mpc.planted(c).items():
        assert not got["valid60"][i, j], kind
        if kind == "neg":
            assert got["mask10"][i * f:(i + 1) * f, j * f:(j + 1) * f].all()
    if c["s2_bad"] is not None:
        _, i, j, _ = c["s2_bad"]
        assert not got["valid60"][i // f, j // f] and got["mask10"][i, j]
    np.testing.assert_array_equal(got["s2_rgb_60m_n"], ref["s2_rgb_60m_n"])

    # ---- limits
    np.testing.assert_array_equal(got["lohi_s2_60m"], ref["lohi_s2_60m"])
    assert dl60 <= LIMIT_REL and dl10 <= LIMIT_REL, (dl60, dl10)

    # ---- curves and images
    for ch in range(3):
        np.testing.assert_allclose(np.polyval(got["coeffs"][ch], xs), np.polyval(ref["coeffs"][ch], xs), rtol=0, atol=CURVE_ATOL)
    np.testing.assert_allclose(got["emit_rgb_matched_60m"][v], ref["emit_rgb_matched_60m"][v], rtol=0, atol=IMAGE_ATOL)
    np.testing.assert_allclose(got["emit_rgb_10m_matched"][m10], ref["emit_rgb_10m_matched"][m10], rtol=0, atol=IMAGE_ATOL)
    assert np.array_equal(np.isnan(got["emit_rgb_10m_matched"]), np.isnan(ref["emit_rgb_10m_matched"]))

    # ---- the 200-pixel rule
    ident = np.zeros((3, deg + 1))
    ident[:, -2] = 1.0
    if name in mpc.IDENTITY_ROWS:
        np.testing.assert_array_equal(got["coeffs"], ident)
        # the matched images are the clipped stretches: K3 without a polynomial on the driver's own planes and limits, bit for bit
        from s2_emit import _engine as eng, _native as nat
        PM = nat.PIXMAJOR
        table = eng.build_srf_table(inp["w"], {b: inp["srf"][b] for b in c["rgb_bands"]}, inp["good"])
        emit = eng.srf_integrate(torch.from_numpy(inp["R"].copy()).cuda(), table, layout=PM)
        st60 = eng.poly_apply_stretch_only(emit, torch.from_numpy(got["lohi_emit_60m"]).cuda(), PM, nb=3)
        np.testing.assert_array_equal(got["emit_rgb_matched_60m"], st60[:, :3].reshape(H, W, 3).cpu().numpy())
        emit10 = eng.bilinear_upsample(emit, H, W, f, layout=PM, nb=3)
        st10 = eng.poly_apply_stretch_only(emit10, torch.from_numpy(got["lohi_emit_10m"]).cuda(), PM, nb=3)
        np.testing.assert_array_equal(got["emit_rgb_10m_matched"], st10[:, :3].reshape(H * f, W * f, 3).cpu().numpy())
    else:
        assert not np.array_equal(got["coeffs"], ident)
    if name in mpc.FIT_AT_THE_RULE:
        assert float(np.max(np.abs(got["coeffs"] - ident))) > 1e-3            # a fit in earnest, not the identity with noise on it

    # ---- a second call: the same bits for every key
    _same_bits(_host(_call(torch, name)), got, "second call")
    if c["other_stream"]:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            junk = torch.rand((4096, 4096), device="cuda")
            for _ in range(20):                              # work in front of the call on this stream
                junk = junk * 1.0001 + 0.5
            other = _call(torch, name)
        st.synchronize()
        _same_bits(_host(other), got, "non-default current stream")


def test_match_pair_argument_errors(torch_gpu):
    import s2_emit
    inp = mpc.inputs("anchor_lsq")
    args = (inp["R"], inp["w"], inp["srf"], inp["good"])
    with pytest.raises(ValueError, match="s2_rgb_hi must be"):
        s2_emit.match_pair(*args, inp["s2_hi"][:-1], inp["factor"], **inp["kwargs"])
    with pytest.raises(ValueError, match="s2_rgb_hi must be"):
        s2_emit.match_pair(*args, inp["s2_hi"], 3, **inp["kwargs"])
    with pytest.raises(ValueError, match="B99"):
        s2_emit.match_pair(*args, inp["s2_hi"], inp["factor"], **{**inp["kwargs"], "rgb_bands": ("B4", "B99", "B2")})
