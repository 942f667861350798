"""The case table of the reference driver (s2_emit.match_pair == poly_regression.py:96-172) and the builders of its inputs.

Shared by tests/test_gpu_match_pair_cases.py (the driver on the GPU against oracle.oracle_np.match_pair_reference) and
tests/test_match_pair_table.py (the oracle alone: what the table claims about every row - valid-pixel counts, which select path
a row takes, what the planted spectra do to the masks).  Not a test module itself; everything here is NumPy.

Inputs of a row, as tests/test_gpu_parity.py::test_match_pair_reference_driver builds them: oracle_np.synthetic_cube /
synthetic_wavelengths / synthetic_srf; the real S2 image is the oracle's own RGB planes repeated f x f,
nan_to_num(nan=0.1, posinf=0.1), clipped at 0, / 0.45, ** 0.8, plus Gaussian noise of 6/255, clipped to [0, 1], then stored as
  u8   x 255                                  src_scale 1/255
  u16  x 10 000                               src_scale 1e-4
  f32  rounded to multiples of 2^-12          src_scale 1.0   (float32 block sums of such values are exact in any order;
                                                               tests/test_gpu_aux_instances.py holds block_mean to bit-equality on them)
Planted spectra (``plant``): "nan" one NaN sample at pixel (0, 0); "inf" one +Inf sample at the centre pixel; "neg" the whole
spectrum -0.01 at the last pixel (positive band <= 0: invalid at 60 m but finite, so it stays in mask10 and in the 10 m limits).
"""
import functools

import numpy as np

from oracle import oracle_np as onp

ALL3 = ("nan", "inf", "neg")
TINY_MAX_PIX = 32 * 1024          # kTinyMaxPix of csrc/hsr_select.hip: up to here one workgroup selects a channel
MIN_FIT = 200                     # the minimum-count rule of both fit branches
N_SAMPLES = 600                   # OT rows, as the existing driver test
NAN_SAMPLE, INF_SAMPLE = 50, 20   # 751 nm: outside the support of B2 / B3 / B4; 529 nm: inside B3's


def _case(H, W, f, dtype, fit, deg, n_valid, plant=ALL3, s2_bad=None, n_emit_valid=None, seed=0, **other):
    """``n_emit_valid``: pixels whose spectrum is valid, before the S2 image is looked at (default: the same as n_valid).
    ``s2_bad``: (kind, fine row, fine column, channel) of one non-finite S2 pixel."""
    case = dict(H=H, W=W, f=f, dtype=dtype, use_ot=(fit == "ot"), deg=deg, n_valid=n_valid, plant=tuple(plant), s2_bad=s2_bad,
                n_emit_valid=n_valid if n_emit_valid is None else n_emit_valid, seed=seed, rgb_bands=("B4", "B3", "B2"),
                positive_band="B2", device_inputs=False, other_stream=False)
    case.update(other)
    return case


# name -> (H, W, factor, S2 dtype, fit, deg, valid pixels at 60 m, ...).  What a row is there for stands next to it.
CASES = {
    # 1. the geometry of the existing driver test, kept as the anchor
    "anchor_lsq": _case(40, 36, 6, "u8", "lsq", 3, 1437, seed=21),
    "anchor_ot": _case(40, 36, 6, "u8", "ot", 4, 1437, seed=21),
    # 2. 34 560 pixels at 60 m > kTinyMaxPix: both 60 m selects take the multi-workgroup path, side by side on two streams; the 10 m
    #    chain is short next to them.  Also called from a non-default current stream.
    "select_multi_wg_f2": _case(192, 180, 2, "u8", "lsq", 3, 34557, seed=2, other_stream=True),
    # 3. the reference's own tile size, factor 3, uint16, src_scale 1e-4
    "tile_110x100_f3_u16": _case(110, 100, 3, "u16", "lsq", 4, 10997, seed=3),
    # 4. one row / one column: the edge clamp of the upsampler acts on every output row / column
    "one_row": _case(1, 230, 6, "u8", "lsq", 3, 227, seed=4),
    "one_column_u16": _case(230, 1, 2, "u16", "lsq", 2, 227, seed=5),
    # 5. factor 1: block mean and upsampler copy every finite value (the second tap of each axis has weight 0, and 0 x a non-finite
    #    neighbour is NaN: the pixels left of / above the +Inf spectrum leave mask10 with it).  One NaN in the S2 image at a pixel that
    #    is valid otherwise: valid60 is false there through the block mean alone.
    "factor1_f32_s2_nan": _case(33, 47, 1, "f32", "lsq", 1, 33 * 47 - 4, s2_bad=("nan", 5, 7, 1), n_emit_valid=33 * 47 - 3, seed=6),
    # 6. factor 10: 225 pixels at 60 m against 22 500 at 10 m (the chains' lengths reversed against row 2); W and W * f both odd.
    #    Also called from a non-default current stream.
    "factor10_odd": _case(25, 9, 10, "u8", "lsq", 2, 222, seed=7, other_stream=True),
    # 7. degree 4 just above the count rule: 207 spectra are valid, and one S2 fine pixel is +Inf inside a block of its own (fine pixel
    #    (26, 57) of block (4, 9)), which leaves 206 pixels in valid60 - still a fit.  (15 x 14 - 3 planted = 207 is the count before
    #    the S2 image is looked at; the +Inf block cannot also be one of the three planted pixels and "of its own".)
    "deg4_207_s2_inf": _case(15, 14, 6, "f32", "lsq", 4, 206, s2_bad=("inf", 26, 57, 1), n_emit_valid=207, seed=8),
    # 8. exactly 200 valid pixels (nothing planted): a fit, not the identity
    "count_200_fit": _case(10, 20, 6, "u8", "lsq", 4, 200, plant=(), seed=9),
    # 9. 199 valid pixels (one -0.01 spectrum): coeffs exactly [0, 0, 0, 1, 0], matched images = the clipped stretches
    "count_199_identity": _case(10, 20, 6, "u8", "lsq", 4, 199, plant=("neg",), seed=9),
    # 10. / 11. the OT branch on both sides of its rule; n_samples = 600 exceeds both row counts, so all rows are drawn
    "ot_192_identity": _case(15, 13, 6, "u8", "ot", 4, 192, seed=10),
    "ot_218_fit": _case(17, 13, 6, "u8", "ot", 2, 218, seed=11),
    # 12. other bands than the defaults
    "bands_b8_b4_b3": _case(40, 36, 6, "u8", "lsq", 3, 1437, seed=21, rgb_bands=("B8", "B4", "B3"), positive_band="B3"),
    # 13. the cube as a non-contiguous GPU tensor (a slice of a wider one), the S2 image as a GPU tensor, as_numpy=False
    "device_inputs_u16": _case(40, 36, 6, "u16", "lsq", 3, 1437, seed=13, device_inputs=True),
}
IDENTITY_ROWS = ("count_199_identity", "ot_192_identity")
FIT_AT_THE_RULE = ("count_200_fit", "ot_218_fit")

SRC_SCALE = {"u8": 1.0 / 255.0, "u16": 1e-4, "f32": 1.0}


def planted(case):
    """{"nan" | "inf" | "neg": (row, column)} of the spectra planted in this row."""
    H, W = case["H"], case["W"]
    where = {"nan": (0, 0), "inf": (H // 2, W // 2), "neg": (H - 1, W - 1)}
    return {k: where[k] for k in case["plant"]}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(R, w, srf, good, s2_hi, src_scale, kwargs) of a row, built once; callers must not write to the arrays."""
    c = CASES[name]
    H, W, f = c["H"], c["W"], c["f"]
    srf = onp.synthetic_srf()
    w, good = onp.synthetic_wavelengths()
    R = onp.synthetic_cube(H, W, seed=c["seed"])
    for kind, (i, j) in planted(c).items():
        if kind == "nan":
            R[i, j, NAN_SAMPLE] = np.nan
        elif kind == "inf":
            R[i, j, INF_SAMPLE] = np.inf
        else:
            R[i, j, :] = -0.01
    rng = np.random.default_rng(100 + c["seed"])
    ps = onp.pseudo_s2_srf_integral(R, w, {b: srf[b] for b in c["rgb_bands"]}, good)
    rgb60 = np.stack([ps[b] for b in c["rgb_bands"]], -1)
    hi = np.repeat(np.repeat(np.nan_to_num(rgb60, nan=0.1, posinf=0.1), f, 0), f, 1)
    img = np.clip((np.clip(hi, 0, None) / 0.45) ** 0.8 + rng.normal(0, 6.0 / 255.0, hi.shape), 0, 1)
    if c["dtype"] == "u8":
        s2_hi = np.rint(img * 255).astype(np.uint8)
    elif c["dtype"] == "u16":
        s2_hi = np.rint(img * 10000).astype(np.uint16)
    else:
        s2_hi = (np.rint(img * 4096) / 4096).astype(np.float32)
    if c["s2_bad"] is not None:
        kind, i, j, ch = c["s2_bad"]
        s2_hi[i, j, ch] = np.nan if kind == "nan" else np.inf
    kwargs = dict(deg=c["deg"], use_ot=c["use_ot"], n_samples=N_SAMPLES, src_scale=SRC_SCALE[c["dtype"]],
                  rgb_bands=c["rgb_bands"], positive_band=c["positive_band"])
    for a in (R, s2_hi):
        a.setflags(write=False)
    return dict(R=R, w=w, srf=srf, good=good, s2_hi=s2_hi, factor=f, kwargs=kwargs)


def _planes(name, perturb=None):
    """The float32 planes the oracle driver works on, in (red, green, blue) order: K1 at 60 m, its bilinear upsampling, the block mean
    of the S2 image times src_scale.  ``perturb(planes64)`` disturbs the float64 K1 planes first (sensitivity())."""
    inp, c = inputs(name), CASES[name]
    ps = onp.pseudo_s2_srf_integral(inp["R"], inp["w"], {b: inp["srf"][b] for b in c["rgb_bands"]}, inp["good"])
    p64 = np.stack([ps[b] for b in c["rgb_bands"]], 0)
    if perturb is not None:
        p64 = perturb(p64)
    emit60 = p64.astype(np.float32)
    s2_60 = onp.block_mean(np.ascontiguousarray(np.moveaxis(inp["s2_hi"], -1, 0)), inp["factor"])
    s2_60 *= float(inp["kwargs"]["src_scale"])
    return emit60, onp.bilinear_upsample(emit60, inp["factor"]), s2_60


def _limits(planes, mask):
    return np.array([np.percentile(p[mask], [2, 98]) for p in planes], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """match_pair_reference of a row plus what the driver's three limit tensors are compared with: np.percentile at 2 / 98 of the
    oracle's float32 planes under valid60 (60 m) / mask10 (10 m), and max |plane| under the mask per tensor.  Built once."""
    inp = inputs(name)
    ref = onp.match_pair_reference(inp["R"], inp["w"], inp["srf"], inp["good"], inp["s2_hi"], inp["factor"], **inp["kwargs"])
    emit60, emit10, s2_60 = _planes(name)
    v, m10 = ref["valid60"], ref["mask10"]
    ref = dict(ref)
    ref["lohi_emit_60m"] = _limits(emit60, v)
    ref["lohi_s2_60m"] = _limits(s2_60, v)
    ref["lohi_emit_10m"] = _limits(emit10, m10)
    ref["absmax_emit_60m"] = float(np.max(np.abs(emit60[:, v])))
    ref["absmax_emit_10m"] = float(np.max(np.abs(emit10[:, m10])))
    ref["emit_60m"], ref["emit_10m"], ref["s2_60m"] = emit60, emit10, s2_60
    return ref


def sensitivity(name, rel=2e-6, draws=3):
    """How far the oracle's own outputs move when its K1 planes are disturbed by a random relative ``rel`` (2e-6 is the bar
    tests/test_gpu_k1_instances.py holds K1 to): the largest change, over ``draws`` draws, of the curves on linspace(0, 1, 33), of the
    matched 60 m image under valid60 and of the matched 10 m image under mask10, and whether a mask changed.  A figure to print next
    to the bars of the GPU test (2e-6, 1e-5, 1e-5), not an assertion."""
    inp, ref = inputs(name), oracle(name)
    xs = np.linspace(0, 1, 33)
    worst = [0.0, 0.0, 0.0]
    masks_moved = False
    real = onp.pseudo_s2_srf_integral
    for d in range(draws):
        rng = np.random.default_rng(1000 + d)

        def disturbed(R, emit_w, srf_dict, good_mask=None):
            return {k: None if p is None else p * (1.0 + rel * rng.uniform(-1, 1, p.shape)) for k, p in real(R, emit_w, srf_dict, good_mask).items()}

        onp.pseudo_s2_srf_integral = disturbed
        try:
            got = onp.match_pair_reference(inp["R"], inp["w"], inp["srf"], inp["good"], inp["s2_hi"], inp["factor"], **inp["kwargs"])
        finally:
            onp.pseudo_s2_srf_integral = real
        masks_moved |= not (np.array_equal(got["valid60"], ref["valid60"]) and np.array_equal(got["mask10"], ref["mask10"]))
        v, m10 = ref["valid60"] & got["valid60"], ref["mask10"] & got["mask10"]
        worst[0] = max(worst[0], max(float(np.max(np.abs(np.polyval(got["coeffs"][ch], xs) - np.polyval(ref["coeffs"][ch], xs)))) for ch in range(3)))
        worst[1] = max(worst[1], float(np.max(np.abs(got["emit_rgb_matched_60m"][v].astype(np.float64) - ref["emit_rgb_matched_60m"][v]))))
        worst[2] = max(worst[2], float(np.max(np.abs(got["emit_rgb_10m_matched"][m10].astype(np.float64) - ref["emit_rgb_10m_matched"][m10]))))
    return dict(curves=worst[0], image_60m=worst[1], image_10m=worst[2], masks_moved=masks_moved)

