"""The case table of tests/match_pair_cases.py under the oracle alone (CPU): every row is what its comment says it is.

tests/test_gpu_match_pair_cases.py runs s2_emit.match_pair over the same table on the GPU; here oracle_np.match_pair_reference
is asked for the facts the rows were chosen for - the valid-pixel counts on both sides of the 200-pixel rule, which rows leave the
one-workgroup select, what the planted spectra do to valid60 and mask10, and that the float32 S2 images hold exact data.
"""
import warnings

import numpy as np
import pytest

import match_pair_cases as mpc
from oracle import oracle_np as onp

warnings.simplefilter("ignore")


@pytest.mark.parametrize("name", list(mpc.CASES))
def test_row_is_what_the_table_says(name):
    c, inp, ref = mpc.CASES[name], mpc.inputs(name), mpc.oracle(name)
    H, W, f = c["H"], c["W"], c["f"]
    v, m10 = ref["valid60"], ref["mask10"]
    assert v.shape == (H, W) and m10.shape == (H * f, W * f) and inp["s2_hi"].shape == (H * f, W * f, 3)
    # counts: after the spectra alone, and after the S2 image too
    e = ref["emit_60m"]
    emit_valid = np.isfinite(e).all(axis=0) & (e[c["rgb_bands"].index(c["positive_band"])] > 0)
    assert int(emit_valid.sum()) == c["n_emit_valid"] == H * W - len(c["plant"])
    assert int(v.sum()) == c["n_valid"] == c["n_emit_valid"] - (c["s2_bad"] is not None)
    # which select the 60 m images take
    assert (H * W > mpc.TINY_MAX_PIX) == (name == "select_multi_wg_f2")
    # the planted spectra: all false in valid60; NaN / +Inf take their bilinear neighbourhood out of mask10, -0.01 takes nothing
    up = lambda m: np.repeat(np.repeat(m, f, 0), f, 1)
    lost = np.zeros((H, W), bool)
    for kind, (i, j) in mpc.planted(c).items():
        assert not v[i, j], kind
        block = m10[i * f:(i + 1) * f, j * f:(j + 1) * f]
        if kind == "neg":
            assert np.isfinite(e[:, i, j]).all() and block.all()
        else:
            assert not np.isfinite(e[:, i, j]).all() and not block.any()
            lost[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2] = True          # a tap reaches one coarse pixel to each side
    assert m10[~up(lost)].all() and (len(c["plant"]) < 3 or not m10.all())
    if c["s2_bad"] is not None:
        _, i, j, _ = c["s2_bad"]
        assert emit_valid[i // f, j // f] and not v[i // f, j // f] and m10[i, j]
        assert int((emit_valid & ~v).sum()) == 1
    if name == "factor1_f32_s2_nan":
        # mask10 and valid60 part at the -0.01 pixel, at the S2 NaN pixel and at the three zero-weight neighbours of the +Inf spectrum
        ci, cj = mpc.planted(c)["inf"]
        assert sorted(map(tuple, np.argwhere(m10 != v))) == sorted([(H - 1, W - 1), (5, 7), (ci - 1, cj - 1), (ci - 1, cj), (ci, cj - 1)])
    if c["dtype"] == "f32":
        s2 = inp["s2_hi"]
        fin = np.isfinite(s2)
        assert s2.dtype == np.float32 and np.array_equal(s2[fin] * 4096, np.rint(s2[fin] * 4096)) and s2[fin].min() >= 0 and s2[fin].max() <= 1
    else:
        assert inp["s2_hi"].dtype == {"u8": np.uint8, "u16": np.uint16}[c["dtype"]]
    # the fallback: exactly the identity below 200 samples, a fit from 200 on
    ident = np.zeros((3, c["deg"] + 1))
    ident[:, -2] = 1.0
    assert (c["n_valid"] < mpc.MIN_FIT) == (name in mpc.IDENTITY_ROWS) == bool(np.array_equal(ref["coeffs"], ident))
    if name in ("ot_192_identity", "ot_218_fit"):
        assert c["use_ot"] and c["n_valid"] < mpc.N_SAMPLES                   # all rows are drawn
    # no degenerate stretch anywhere: the limits are apart by a tenth of the image's range at least
    for k in ("lohi_emit_60m", "lohi_s2_60m", "lohi_emit_10m"):
        assert np.isfinite(ref[k]).all() and (ref[k][:, 1] - ref[k][:, 0] > 0.05).all(), k


def test_the_table_holds_the_counts_at_the_rule():
    counts = {n: mpc.CASES[n]["n_valid"] for n in mpc.CASES}
    assert (counts["count_200_fit"], counts["count_199_identity"], counts["ot_192_identity"], counts["ot_218_fit"]) == (200, 199, 192, 218)
    assert (mpc.CASES["deg4_207_s2_inf"]["n_emit_valid"], counts["deg4_207_s2_inf"]) == (207, 206)


def test_bands_keywords_default_to_the_drivers_own():
    """rgb_bands / positive_band of the oracle driver: the defaults are the bits of the call without them."""
    inp = mpc.inputs("anchor_lsq")
    kw = {k: x for k, x in inp["kwargs"].items() if k not in ("rgb_bands", "positive_band")}
    plain = onp.match_pair_reference(inp["R"], inp["w"], inp["srf"], inp["good"], inp["s2_hi"], inp["factor"], **kw)
    for k, x in plain.items():
        np.testing.assert_array_equal(x, mpc.oracle("anchor_lsq")[k], err_msg=k)
    other = mpc.oracle("bands_b8_b4_b3")
    assert not np.array_equal(other["coeffs"], plain["coeffs"])


def test_sensitivity_figures(capsys):
    """Prints (pytest -s) how far the oracle's own outputs move when its K1 planes are disturbed by a relative 2e-6, next to the bars
    of the GPU test: curves 2e-6, images 1e-5.  Figures, not assertions - except that no mask may move."""
    with capsys.disabled():
        for name, c in mpc.CASES.items():
            s = mpc.sensitivity(name, draws=3 if c["H"] * c["W"] < 20000 else 1)
            print(f"\n  {name:22s} curves {s['curves']:.2e}  60 m {s['image_60m']:.2e}  10 m {s['image_10m']:.2e}", end="")
            assert not s["masks_moved"], name
