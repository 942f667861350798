"""CPU oracle for the s2_emit SRF + polynomial-regression path.  TEST INFRASTRUCTURE ONLY.

This module is a NumPy restatement of the reference algorithm, written to follow the
reference's operation order literally so that it agrees with it to the last bits.  It is the
*checker*, never the product: only ``tests/``, ``__graft_entry__.smoke()`` and the
``cpu_baseline`` leg of ``bench.py`` may import it.  The shipped package
(``hyperspectral_super-resolution_amd/s2_emit``) never imports anything from ``oracle/``.

Pinning: the reference ships no tests or golden vectors, so the oracle is
pinned against outputs of the reference functions themselves, imported by path in the build
container by ``oracle/ref_loader.py`` and frozen into ``tests/golden/*.npz`` by
``tests/golden/gen_golden.py``.  ``tests/test_oracle_golden.py`` re-checks the oracle against
those fixtures on every run.  Two sub-steps stay **parity unpinned** because their third-party
implementation is absent from the container and from the reference tree:
  * the Sinkhorn transport plan (POT ``ot.dist`` / ``ot.sinkhorn``, unpinned dependency), and
  * the GDAL ``reproject`` resamplers between the phases (rasterio absent).
They are restated from the published algorithm and checked by invariants only.

Each function cites the reference lines it follows (paths relative to the reference root).
NumPy's own ``interp`` / ``percentile`` / ``polyfit`` / ``polyval`` are the reference's
third-party arithmetic (requirements.txt:3) and are called directly, exactly as it calls them.
"""
from __future__ import annotations

from itertools import combinations_with_replacement
from typing import Dict, Optional, Tuple

import numpy as np

S2_BANDS_13 = ["B1", "B2", "B3", "B4", "B5", "B6", "B7", "B8", "B8A", "B9", "B10", "B11", "B12"]  # s2_emit/srf.py:11


# ---------------------------------------------------------------------------------------------
# a2: SRF band integration  (s2_emit/synth.py:9-45)
# ---------------------------------------------------------------------------------------------
def _trapezoid_last_axis(y: np.ndarray, x: np.ndarray) -> np.ndarray:
    """numpy.trapz(y, x=x, axis=-1) as NumPy computes it: sum(d * (y[1:] + y[:-1]) / 2)."""
    d = np.diff(x)
    return (d * (y[..., 1:] + y[..., :-1]) / 2.0).sum(axis=-1)


def band_response_on_emit(emit_w, lam_srf, rsp_srf, good_mask=None) -> np.ndarray:
    """SRF of one band resampled on the EMIT wavelength grid (synth.py:25,33-35)."""
    w = np.asarray(emit_w).astype(float)
    r = np.interp(w, lam_srf, rsp_srf, left=0.0, right=0.0)
    if good_mask is not None:
        r = r * np.asarray(good_mask).astype(float)
    return r


def pseudo_s2_srf_integral(R, emit_w, srf_dict, good_mask=None) -> Dict[str, Optional[np.ndarray]]:
    """Literal restatement of synth.py:9-45 (float64 temporaries, one full-cube pass per band)."""
    out: Dict[str, Optional[np.ndarray]] = {}
    emit_w = np.asarray(emit_w).astype(float)                                  # synth.py:25
    if R.ndim != 3:                                                            # synth.py:27-28
        raise ValueError(f"R must be (H,W,B). Got shape {R.shape}")
    if emit_w.ndim != 1 or emit_w.shape[0] != R.shape[-1]:                     # synth.py:29-30
        raise ValueError(f"emit_w must be (B,) matching R bands. Got {emit_w.shape} vs {R.shape[-1]}")
    for band, (lam_srf, rsp_srf) in srf_dict.items():                          # synth.py:32
        r = band_response_on_emit(emit_w, lam_srf, rsp_srf, good_mask)         # synth.py:33-35
        if np.all(r == 0):                                                     # synth.py:37-39
            out[band] = None
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            num = _trapezoid_last_axis(R * r[None, None, :], emit_w)           # synth.py:41
        den = _trapezoid_last_axis(r, emit_w)                                  # synth.py:42
        out[band] = num / (den + 1e-32)                                        # synth.py:43
    return out


def srf_weight_matrix(emit_w, srf_dict, good_mask=None) -> Tuple[np.ndarray, list]:
    """Weight-matrix form of the same integral: out_b = sum_k R_k * Wn[b,k].

    Returns (Wn (nb_supported, B) float64, names of supported bands in dict order).
    Used by tests to check the algebraic identity the device kernel relies on.
    """
    w = np.asarray(emit_w).astype(float)
    d = np.diff(w)
    half = (np.concatenate([[0.0], d]) + np.concatenate([d, [0.0]])) / 2.0
    rows, names = [], []
    for band, (lam, rsp) in srf_dict.items():
        r = band_response_on_emit(w, lam, rsp, good_mask)
        if np.all(r == 0):
            continue
        c = r * half
        rows.append(c / (_trapezoid_last_axis(r, w) + 1e-32))
        names.append(band)
    return np.asarray(rows, dtype=np.float64).reshape(len(rows), w.shape[0]), names


def pseudo_s2_rgb(pseudo_s2, order=("B4", "B3", "B2")) -> np.ndarray:
    """synth.py:47-58."""
    chans = []
    for b in order:
        x = pseudo_s2.get(b, None)
        if x is None:
            raise ValueError(f"Band {b} is None/missing in pseudo_s2.")
        chans.append(x)
    return np.stack(chans, axis=-1)


# ---------------------------------------------------------------------------------------------
# a4 / a10: percentile stretches and histogram matching  (s2_emit/color.py)
# ---------------------------------------------------------------------------------------------
def robust_norm(x, pmin=2, pmax=98):
    """color.py:6-8."""
    lo, hi = np.nanpercentile(x, [pmin, pmax])
    return np.clip((x - lo) / (hi - lo + 1e-12), 0, 1)


def robust_norm_rgb(img, mask, pmin=2, pmax=98):
    """color.py:10-23 (unmasked pixels become NaN)."""
    y = np.zeros_like(img, dtype=float)
    for c in range(3):
        lo, hi = np.percentile(img[..., c][mask], [pmin, pmax])
        cc = (img[..., c] - lo) / (hi - lo + 1e-12)
        cc[~mask] = np.nan
        y[..., c] = np.clip(cc, 0, 1)
    return y


def apply_shared_percentile_stretch(img, mask, pmin=2, pmax=98, channels: Optional[int] = None):
    """color.py:25-34; ``channels`` generalises the hard-coded 3 to nb planes (SURVEY.md 8 intro)."""
    out = np.zeros_like(img, dtype=np.float32)
    for c in range(3 if channels is None else channels):
        lo, hi = np.percentile(img[..., c][mask], [pmin, pmax])
        out[..., c] = np.clip((img[..., c] - lo) / (hi - lo + 1e-12), 0, 1)
    return out


def percentile_limits(plane, mask, pmin=2, pmax=98):
    """The (lo, hi) pair of color.py:31-32 for one channel, float64."""
    lo, hi = np.percentile(plane[mask], [pmin, pmax])
    return float(lo), float(hi)


def _hist_match_channel(src, ref, mask):
    """color.py:36-53."""
    src_vals = src[mask].ravel()
    ref_vals = ref[mask].ravel()
    s_values, s_idx, s_counts = np.unique(src_vals, return_inverse=True, return_counts=True)
    r_values, r_counts = np.unique(ref_vals, return_counts=True)
    s_q = np.cumsum(s_counts).astype(np.float64)
    s_q /= (s_q[-1] + 1e-32)
    r_q = np.cumsum(r_counts).astype(np.float64)
    r_q /= (r_q[-1] + 1e-32)
    matched = np.interp(s_q, r_q, r_values)[s_idx].reshape(src_vals.shape)
    out = src.copy()
    out[mask] = matched
    return out


def histogram_match_rgb(src_rgb, ref_rgb, mask):
    """color.py:55-63."""
    out = src_rgb.copy()
    for c in range(3):
        out[..., c] = _hist_match_channel(out[..., c], ref_rgb[..., c], mask)
    return np.clip(out, 0, 1)


# ---------------------------------------------------------------------------------------------
# Sinkhorn (POT restated; PARITY UNPINNED - POT is not installed and not pinned by the reference)
# ---------------------------------------------------------------------------------------------
def sqeuclidean_cost(X, Y):
    """ot.dist(X, Y, metric='sqeuclidean'): ||x||^2 + ||y||^2 - 2 x.y, clipped at 0 (POT docs)."""
    a2 = np.einsum("ij,ij->i", X, X)[:, None]
    b2 = np.einsum("ij,ij->i", Y, Y)[None, :]
    return np.maximum(a2 + b2 - 2.0 * X.dot(Y.T), 0.0)


def sinkhorn_knopp(a, b, M, reg, numItermax=1000, stopThr=1e-9):
    """POT ``sinkhorn_knopp`` as documented: K = exp(-M/reg); v <- b/(K^T u); u <- a/(K v);
    every 10th iteration err = ||v * (K^T u) - b||_2, stop when err < stopThr; on a numerical
    breakdown keep the previous (u, v).  Returns u[:,None] * K * v[None,:].
    """
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    K = np.exp(M / (-reg))
    u = np.full(a.shape[0], 1.0 / a.shape[0])
    v = np.full(b.shape[0], 1.0 / b.shape[0])
    for ii in range(numItermax):
        uprev, vprev = u, v
        KtU = K.T.dot(u)
        v = b / KtU
        u = a / K.dot(v)
        if (np.any(KtU == 0) or np.any(np.isnan(u)) or np.any(np.isnan(v))
                or np.any(np.isinf(u)) or np.any(np.isinf(v))):
            u, v = uprev, vprev
            break
        if ii % 10 == 0:
            tmp2 = np.einsum("i,ij,j->j", u, K, v)
            err = np.linalg.norm(tmp2 - b)
            if err < stopThr:
                break
    return u[:, None] * K * v[None, :]


def _ot_samples(src_rgb, ref_rgb, mask, n_samples, seed, min_rows):
    """Shared head of fit_ot_poly_rgb / ot_match_rgb_sinkhorn_pot (poly_regression.py:31-47)."""
    rng = np.random.default_rng(seed)
    X_all = src_rgb[mask].reshape(-1, 3).astype(np.float64)
    Y_all = ref_rgb[mask].reshape(-1, 3).astype(np.float64)
    X_all = X_all[np.isfinite(X_all).all(axis=1)]
    Y_all = Y_all[np.isfinite(Y_all).all(axis=1)]
    if X_all.shape[0] < min_rows or Y_all.shape[0] < min_rows:
        return None
    ns = min(n_samples, X_all.shape[0])
    nt = min(n_samples, Y_all.shape[0])
    X = X_all[rng.choice(X_all.shape[0], size=ns, replace=False)]
    Y = Y_all[rng.choice(Y_all.shape[0], size=nt, replace=False)]
    return X, Y


def ot_barycentric_targets(X, Y, reg=0.05, numItermax=300, stopThr=1e-6):
    """poly_regression.py:49-56."""
    ns, nt = X.shape[0], Y.shape[0]
    a = np.full(ns, 1.0 / ns, dtype=np.float64)
    b = np.full(nt, 1.0 / nt, dtype=np.float64)
    P = sinkhorn_knopp(a, b, sqeuclidean_cost(X, Y), reg, numItermax=numItermax, stopThr=stopThr)
    return (P @ Y) / (P.sum(axis=1, keepdims=True) + 1e-32)


def ot_match_rgb_sinkhorn_pot(src_rgb, ref_rgb, mask, n_samples=5_000, reg=0.05, numItermax=300, stopThr=1e-6, seed=0):
    """color.py:65-116: OT barycentric targets + affine least squares, applied inside the mask
    (Sinkhorn sub-step parity unpinned, see module docstring)."""
    s = _ot_samples(src_rgb, ref_rgb, mask, n_samples, seed, 2)
    if s is None:                                                              # color.py:88-89
        return src_rgb.copy()
    X, Y = s
    Ybar = ot_barycentric_targets(X, Y, reg, numItermax, stopThr)
    X_aug = np.concatenate([X, np.ones((X.shape[0], 1))], axis=1)              # color.py:106-109
    Wm, *_ = np.linalg.lstsq(X_aug, Ybar, rcond=None)
    A, t = Wm[:3, :], Wm[3, :]
    out = src_rgb.copy().astype(np.float32)                                    # color.py:111-116
    Xm = out[mask].reshape(-1, 3).astype(np.float64)
    Xm2 = np.clip(Xm @ A + t, 0.0, 1.0)
    out[mask] = Xm2.reshape(out[mask].shape).astype(np.float32)
    return out


# ---------------------------------------------------------------------------------------------
# a5 / a6: polynomial fit and apply  (s2_emit/poly_regression.py:16-84)
# ---------------------------------------------------------------------------------------------
def fit_ot_poly_rgb(src_rgb, ref_rgb, mask, deg=2, n_samples=5000, reg=0.05, numItermax=300,
                    stopThr=1e-6, seed=0):
    """poly_regression.py:16-62 (Sinkhorn sub-step parity unpinned, see module docstring)."""
    s = _ot_samples(src_rgb, ref_rgb, mask, n_samples, seed, 200)
    coeffs = np.zeros((3, deg + 1), dtype=np.float64)
    if s is None:                                                              # :38-41
        coeffs[:, -2] = 1.0
        return coeffs
    X, Y = s
    Ybar = ot_barycentric_targets(X, Y, reg, numItermax, stopThr)
    for c in range(3):                                                         # :59-60
        coeffs[c] = np.polyfit(X[:, c], Ybar[:, c], deg=deg)
    return coeffs


def polyfit_channels(X, Ybar, deg):
    """The step (vi) of a5 on explicit (x, ybar) columns: one np.polyfit per channel."""
    return np.stack([np.polyfit(X[:, c], Ybar[:, c], deg=deg) for c in range(X.shape[1])])


def apply_poly_rgb(rgb, coeffs, mask=None):
    """poly_regression.py:65-84; channel count taken from coeffs (reference hard-codes 3)."""
    out = rgb.copy().astype(np.float32)
    nch = len(coeffs)
    if mask is None:
        for c in range(nch):
            out[..., c] = np.polyval(coeffs[c], out[..., c])
        return np.clip(out, 0.0, 1.0)
    for c in range(nch):
        x = out[..., c]
        y = np.polyval(coeffs[c], x)
        x2 = x.copy()
        x2[mask] = y[mask]
        out[..., c] = x2
    return np.clip(out, 0.0, 1.0)


# ---------------------------------------------------------------------------------------------
# a8: per-band least squares over all valid pixels
#     (Pairs_EMIT_S2_demo-2.ipynb cell 72, raw lines 4484-4510), degree generalised.
# ---------------------------------------------------------------------------------------------
def per_band_valid(x, y, valid_mask, min_valid=0.0):
    return valid_mask & np.isfinite(x) & np.isfinite(y) & (x > min_valid) & (y > min_valid)


def fit_per_band_poly(pseudo_stack, real_stack, valid_mask, deg=1, min_valid=0.0, min_count=50):
    """Per band k: polyfit over every valid pixel; fewer than ``min_count`` -> identity."""
    nb = pseudo_stack.shape[0]
    coeffs = np.zeros((nb, deg + 1), dtype=np.float64)
    counts = np.zeros(nb, dtype=np.int64)
    for k in range(nb):
        x, y = pseudo_stack[k], real_stack[k]
        with np.errstate(invalid="ignore"):
            vk = per_band_valid(x, y, valid_mask, min_valid)
        x1 = x[vk].astype(np.float64)
        y1 = y[vk].astype(np.float64)
        counts[k] = x1.size
        if x1.size < min_count:
            coeffs[k, -2] = 1.0
        else:
            coeffs[k] = np.polyfit(x1, y1, deg=deg)
    return coeffs, counts


def calibrate_pseudo_to_real_linear(pseudo_stack, real_stack, valid_mask, min_valid=0.0):
    """Notebook cell 72 verbatim semantics: deg 1, corrected = (x*a + b) as float32."""
    coeffs, _ = fit_per_band_poly(pseudo_stack, real_stack, valid_mask, 1, min_valid, 50)
    corrected = np.zeros_like(pseudo_stack, dtype=np.float32)
    params = []
    for k in range(pseudo_stack.shape[0]):
        a, b = coeffs[k]
        corrected[k] = (pseudo_stack[k] * a + b).astype(np.float32)
        params.append((float(a), float(b)))
    return corrected, params


def apply_poly_planes(planes, coeffs, mask=None, clip=True):
    """apply_poly_rgb semantics on a band-major (nb,H,W) stack (what the device pipeline uses)."""
    hw_last = np.moveaxis(np.asarray(planes), 0, -1)
    if clip:
        res = apply_poly_rgb(hw_last, coeffs, mask)
    else:
        res = hw_last.copy().astype(np.float32)
        for c in range(len(coeffs)):
            y = np.polyval(coeffs[c], res[..., c])
            if mask is None:
                res[..., c] = y
            else:
                x2 = res[..., c].copy()
                x2[mask] = y[mask]
                res[..., c] = x2
    return np.ascontiguousarray(np.moveaxis(res, -1, 0))


# ---------------------------------------------------------------------------------------------
# a7: the pipeline of poly_regression.py:96-139 on a grid-aligned synthetic pair
#     ("per-band least squares" flavour: no OT, every valid pixel, nb bands).
# ---------------------------------------------------------------------------------------------
def fuse_lsq_reference(R, emit_w, srf_dict, good_mask, real_planes, deg, min_valid=0.0,
                       min_count=50, clip=True):
    """SRF -> per-band all-valid-pixel polyfit -> apply.  The C1..C3 workload, reference-ordered.

    real_planes: (nb_supported, H, W) real-S2 planes for the supported bands, dict order.
    Returns (pseudo (nb,H,W) f32, coeffs (nb,deg+1) f64, matched (nb,H,W) f32, names).
    """
    ps = pseudo_s2_srf_integral(R, emit_w, srf_dict, good_mask)
    names = [b for b, v in ps.items() if v is not None]
    pseudo = np.stack([ps[b] for b in names], axis=0).astype(np.float32)       # poly_regression.py:104
    valid = np.ones(pseudo.shape[1:], dtype=bool)
    coeffs, _ = fit_per_band_poly(pseudo, real_planes, valid, deg, min_valid, min_count)
    fitmask = None
    matched = apply_poly_planes(pseudo, coeffs, fitmask, clip=clip)
    return pseudo, coeffs, matched, names


# ---------------------------------------------------------------------------------------------
# a9: multivariate fusion variant (legacy_notebooks/Spectral_matching.ipynb)
# ---------------------------------------------------------------------------------------------
def logit(p, eps=1e-4):
    """Spectral_matching.ipynb raw line 174-176."""
    p = np.clip(p, eps, 1 - eps)
    return np.log(p / (1 - p))


def sigmoid(z):
    """Spectral_matching.ipynb raw line 178-181."""
    z = np.clip(z, -50, 50)
    return 1.0 / (1.0 + np.exp(-z))


def poly_feature_exponents(n_inputs: int, degree: int) -> np.ndarray:
    """Exponent table of sklearn PolynomialFeatures(degree, include_bias=False): degree-major,
    combinations_with_replacement order.  (n_features, n_inputs) int."""
    rows = []
    for d in range(1, degree + 1):
        for comb in combinations_with_replacement(range(n_inputs), d):
            e = np.zeros(n_inputs, dtype=np.int64)
            for i in comb:
                e[i] += 1
            rows.append(e)
    return np.stack(rows)


def poly_features(Z, degree: int) -> np.ndarray:
    expo = poly_feature_exponents(Z.shape[1], degree)
    out = np.ones((Z.shape[0], expo.shape[0]), dtype=Z.dtype)
    for f, e in enumerate(expo):
        for i, p in enumerate(e):
            for _ in range(int(p)):
                out[:, f] *= Z[:, i]
    return out


def ridge_poly_fit(X, Y, degree=3, alpha=1.0):
    """StandardScaler -> PolynomialFeatures(degree, no bias) -> Ridge(alpha, intercept) in float64
    (Spectral_matching.ipynb raw lines 475-490).  Returns dict(mean, scale, coef, intercept)."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    mean = X.mean(axis=0)
    scale = X.std(axis=0)
    scale[scale == 0] = 1.0
    Phi = poly_features((X - mean) / scale, degree)
    pm, ym = Phi.mean(axis=0), Y.mean(axis=0)
    Pc, Yc = Phi - pm, Y - ym
    G = Pc.T @ Pc
    G[np.diag_indices_from(G)] += alpha
    coef = np.linalg.solve(G, Pc.T @ Yc).T            # (n_targets, n_features)
    return dict(mean=mean, scale=scale, coef=coef, intercept=ym - coef @ pm, degree=degree)


def ridge_poly_predict(model, X):
    Z = (np.asarray(X, dtype=np.float64) - model["mean"]) / model["scale"]
    return poly_features(Z, int(model["degree"])) @ model["coef"].T + model["intercept"]


def predict_cube_logit(model, X_bhw, nodata=None):
    """Spectral_matching.ipynb raw lines 192-213: (C,H,W) -> (T,H,W) float32 = sigmoid(float32(model(px))); pixels with a
    non-finite input, or an input np.isclose to ``nodata``, stay NaN in every target.  (The notebook hard-codes 32 targets
    and predicts in batches of 200 000 pixels; neither changes a value.)"""
    C, H, W = X_bhw.shape
    X = X_bhw.reshape(C, -1).T
    valid = np.isfinite(X).all(axis=1)
    if nodata is not None:
        valid &= ~(np.isclose(X, nodata).any(axis=1))
    T = model["coef"].shape[0]
    Y = np.full((X.shape[0], T), np.nan, dtype=np.float32)
    y_logit = ridge_poly_predict(model, X[valid]).astype(np.float32)
    Y[valid] = sigmoid(y_logit).astype(np.float32)
    return Y.T.reshape(T, H, W)


# ---------------------------------------------------------------------------------------------
# f1: grid-aligned resamplers (integer factor) - GDAL parity unpinned, see module docstring
# ---------------------------------------------------------------------------------------------
def block_mean(planes, factor: int):
    """'average' resampling of an exactly aligned (C, H*f, W*f) stack onto the coarse grid."""
    C, H, W = planes.shape
    return planes.reshape(C, H // factor, factor, W // factor, factor).mean(axis=(2, 4), dtype=np.float64).astype(np.float32)


def bilinear_upsample(planes, factor: int):
    """Pixel-centre-aligned separable bilinear upsampling by an integer factor with edge clamp
    (what GDAL bilinear does for interior pixels of an aligned grid)."""
    C, H, W = planes.shape

    def taps(n):
        pos = (np.arange(n * factor) + 0.5) / factor - 0.5
        i0 = np.floor(pos).astype(np.int64)
        t = pos - i0
        return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), t

    r0, r1, tr = taps(H)
    c0, c1, tc = taps(W)
    p = planes.astype(np.float64)
    top = p[:, r0][:, :, c0] * (1 - tc) + p[:, r0][:, :, c1] * tc
    bot = p[:, r1][:, :, c0] * (1 - tc) + p[:, r1][:, :, c1] * tc
    return (top * (1 - tr)[None, :, None] + bot * tr[None, :, None]).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# uint16 tile format
# ---------------------------------------------------------------------------------------------
def tile_encode_u16(emit_tile, src_nodata=None, emit_scale=10000.0, emit_nodata_u16=65535) -> np.ndarray:
    """Quantisation of an EMIT tile as the reference writer does it (tiles_helpers/utils.py:362-374):
    float32 product, round half to even, int32 cast (x86 semantics for out-of-range values), clip to
    [0, nodata-1]; non-finite / source-nodata samples -> nodata.  Pinned by tests/golden/g10_tile_u16.npz."""
    emit = np.asarray(emit_tile).astype(np.float32)
    valid = np.isfinite(emit)
    if src_nodata is not None:
        valid &= emit != src_nodata
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(emit * np.float32(emit_scale))
        inrange = (r >= -2147483648.0) & (r < 2147483648.0)          # NaN compares False
        q = np.where(inrange, r, 0.0).astype(np.int64)
    q = np.where(inrange, q, np.iinfo(np.int32).min)                 # cvttss2si "integer indefinite"
    q = np.clip(q, 0, int(emit_nodata_u16) - 1)
    out = np.full(emit.shape, int(emit_nodata_u16), dtype=np.uint16)
    out[valid] = q[valid].astype(np.uint16)
    return out


def tile_decode_u16(u16, scale=None, nodata=65535) -> np.ndarray:
    """uint16 tile -> float32 reflectance, the consumers' convention (Pairs_EMIT_S2_demo-2.ipynb cell 65:
    ``out *= float(s2_scale)`` on a float32 array, s2_scale = 1e-4): float32(u) * float32(scale);
    nodata samples become NaN (they are excluded by every validity mask downstream).  The reference has no
    decoder of its own for the EMIT tiles: this convention is the documented one, parity unpinned."""
    u = np.asarray(u16)
    sc = np.float32(1e-4) if scale is None else np.float32(scale)
    out = u.astype(np.float32) * sc
    if nodata is not None:
        out[u == nodata] = np.nan
    return out


def match_pair_reference(R, emit_w, srf_dict, good_mask, s2_rgb_hi, factor=6, deg=4, use_ot=True,
                         n_samples=5000, reg=0.05, numItermax=300, stopThr=1e-6, seed=0, src_scale=1.0 / 255.0,
                         rgb_bands=("B4", "B3", "B2"), positive_band="B2"):
    """poly_regression.py:96-172 on in-memory aligned arrays, statement by statement; the two GDAL warps
    are the aligned-grid restatements above (unpinned).  ``rgb_bands`` (red, green, blue) and ``positive_band``
    generalise the driver's hard-coded B4 / B3 / B2 and its ``B2 > 0``; the defaults are the driver's."""
    pseudo = pseudo_s2_srf_integral(R, emit_w, srf_dict, good_mask)                                   # :101
    stack_order = tuple(rgb_bands)[::-1]                                                              # the driver stacks B2, B3, B4
    emit_sim_60m = np.stack([pseudo[b] for b in stack_order], axis=0).astype(np.float32)              # :103-104
    with np.errstate(invalid="ignore"):
        valid60 = np.isfinite(emit_sim_60m).all(axis=0) & (emit_sim_60m[stack_order.index(positive_band)] > 0)   # :106
    s2_planes = np.ascontiguousarray(np.moveaxis(np.asarray(s2_rgb_hi), -1, 0))
    s2_real_60m = block_mean(s2_planes, factor)                                                        # :110-116
    s2_real_60m *= float(src_scale)
    valid60 = valid60 & np.isfinite(s2_real_60m).all(axis=0)                                           # :118
    emit_rgb_60m = np.transpose(emit_sim_60m[[2, 1, 0], ...], (1, 2, 0))                               # :122
    s2_rgb_60m = np.transpose(s2_real_60m[[0, 1, 2], ...], (1, 2, 0))                                  # :124
    emit_rgb_n = apply_shared_percentile_stretch(emit_rgb_60m, valid60)                                # :126
    s2_rgb_n = apply_shared_percentile_stretch(s2_rgb_60m, valid60)                                    # :127
    if use_ot:
        coeffs = fit_ot_poly_rgb(emit_rgb_n, s2_rgb_n, valid60, deg=deg, n_samples=n_samples, reg=reg,
                                 numItermax=numItermax, stopThr=stopThr, seed=seed)                    # :129-137
    else:
        x = np.moveaxis(emit_rgb_n, -1, 0)
        y = np.moveaxis(s2_rgb_n, -1, 0)
        coeffs = np.zeros((3, deg + 1))
        for c in range(3):
            xs, ys = x[c][valid60].astype(np.float64), y[c][valid60].astype(np.float64)
            if xs.size < 200:
                coeffs[c, -2] = 1.0
            else:
                coeffs[c] = np.polyfit(xs, ys, deg)
    emit_rgb_matched_60m = apply_poly_rgb(emit_rgb_n, coeffs, mask=valid60)                            # :139
    emit_sim_10m = bilinear_upsample(emit_sim_60m, factor)                                             # :150-155
    emit_rgb_10m = np.transpose(emit_sim_10m[[2, 1, 0], ...], (1, 2, 0))                               # :157
    mask10 = np.isfinite(emit_rgb_10m).all(axis=-1)                                                    # :159
    emit_rgb_10m_n = apply_shared_percentile_stretch(emit_rgb_10m, mask10)                             # :161
    emit_rgb_10m_matched = apply_poly_rgb(emit_rgb_10m_n, coeffs, mask=mask10)                         # :162
    return dict(coeffs=coeffs, emit_rgb_matched_60m=emit_rgb_matched_60m, s2_rgb_60m_n=s2_rgb_n, valid60=valid60,
                emit_rgb_10m_matched=emit_rgb_10m_matched, mask10=mask10)


# ---------------------------------------------------------------------------------------------
# Synthetic inputs of SURVEY.md 8(d) (NumPy, for the small parity cases and the CPU baseline)
# ---------------------------------------------------------------------------------------------
S2A_CENTRES = [443, 490, 560, 665, 705, 740, 783, 842, 865, 945, 1375, 1610, 2190]
S2A_WIDTHS = [20, 65, 35, 30, 15, 15, 20, 115, 20, 20, 30, 90, 180]


def synthetic_srf(threshold=1e-3):
    lam = np.arange(300.0, 2600.0, 1.0)
    srf = {}
    for name, c, fwhm in zip(S2_BANDS_13, S2A_CENTRES, S2A_WIDTHS):
        r = np.exp(-0.5 * ((lam - c) / (fwhm / 2.3548200450309493)) ** 2)
        m = r > threshold
        srf[name] = (lam[m].copy(), r[m].copy())
    return srf


def synthetic_wavelengths(B=285):
    w = np.linspace(381.00558, 2492.9, B, dtype=np.float32)
    wf = w.astype(float)
    good = ~(((wf > 1320) & (wf < 1440)) | ((wf > 1770) & (wf < 1970)))
    return w, good


def synthetic_cube(H, W, B=285, seed=0):
    rng = np.random.default_rng(seed)
    w, _ = synthetic_wavelengths(B)
    t = (w.astype(float) - 381.0) / (2493.0 - 381.0)
    E = np.stack([0.08 + 0.35 * np.exp(-((t - 0.25) / 0.3) ** 2),
                  0.05 + 0.45 * t * np.exp(-t * 1.5) * 2.0,
                  0.30 - 0.2 * t + 0.05 * np.sin(6 * t)])
    A = rng.random((H, W, 3))
    A /= A.sum(axis=-1, keepdims=True)
    R = A @ E + 0.005 * rng.standard_normal((H, W, B))
    return np.clip(R, -0.01, 0.6).astype(np.float32)


def synthetic_real_planes(pseudo, seed=1):
    """y_b = clip(g_b * x_b^gamma_b + o_b + 0.01 N(0,1), 0, 1) on the same grid."""
    rng = np.random.default_rng(seed)
    nb = pseudo.shape[0]
    g = 0.8 + 0.4 * rng.random(nb)
    gam = 0.8 + 0.4 * rng.random(nb)
    o = 0.02 * rng.random(nb)
    x = np.clip(pseudo.astype(np.float64), 1e-6, None)
    y = g[:, None, None] * x ** gam[:, None, None] + o[:, None, None] + 0.01 * rng.standard_normal(pseudo.shape)
    return np.clip(y, 0, 1).astype(np.float32)
