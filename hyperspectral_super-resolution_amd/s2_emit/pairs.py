"""Tile pairs -> the fused 10 m cube: the per-pair flow of legacy_notebooks/Spectral_matching.ipynb for a batch of pairs.

One pair is what ``tiles_helpers/utils.py:223-395`` writes: an EMIT tile (285, h, w) - uint16 reflectance x 1e4 with nodata
65535, or float32 reflectance - and an S2 tile (10, h f, w f).  The notebook reads the pair (raw lines 265-266), keeps 32
evenly spaced EMIT bands (``subsample_bands_evenly``, :327), brings S2 to the EMIT grid (:377), drops unusable pixels
(``flatten_pixels``, :410, def :108-126), fits ``StandardScaler -> PolynomialFeatures(3) -> Ridge(1.0)`` on
``logit(clip(y, 1e-4, 1 - 1e-4))`` (:434, :475-490) and predicts the (32, h f, w f) cube with ``predict_cube_logit`` (:561).

Here the whole flow of P pairs of one shape is a fixed number of launches on the current stream, whatever P is
(csrc/hsr_pairs.hip, csrc/hsr_ridge.hip, csrc/hsr_gram.hip, csrc/hsr_chol.hip): pair prep (block mean, band gather and decode, mask),
masked scaler statistics, masked expand, Gram, assembly, P Cholesky factorisations side by side, model read-out and the
10 m prediction; with ``report=True`` two more launches score each fit on its own training pixels (the notebook's cell 26:
per-band R^2 and RMSE of sigmoid(model(X_train)) against the raw targets).  ``train_mask`` keeps pixels out of the fit (one more
launch) and ``validate=True`` scores the result against the EMIT tile on the fit and the held-out pixels, for the model applied
to S2 on the EMIT grid and for the 10 m cube averaged back to it (see ``TilePairValidation``).  Nothing synchronises with the host and no pixel crosses PCIe for device inputs.  A pair's arithmetic
does not depend on the batch: ``fuse_tile_pairs`` of a batch gives the bits of ``fuse_tile_pair`` of each of its pairs.

S2 -> EMIT grid: an f x f block mean (float64 sum of the f^2 samples, stored as float32: the bits of ``hsr_block_mean``);
a coarse pixel whose block holds a non-finite or ``s2_nodata`` sample is NaN and so leaves the training set.  The
notebook's GDAL bilinear ``reproject`` is NOT reproduced (rasterio is absent, that parity is unpinned); a caller who has
S2 on the EMIT grid already (e.g. from GDAL) passes it as ``s2_coarse`` and reproduces the notebook exactly.
"""
from __future__ import annotations

import operator
from collections import namedtuple
from dataclasses import dataclass, field
from typing import Any, Optional

import numpy as np

from . import _native as nat
from ._engine import _ptr, _stream
from .ridge import PolyRidge, _is_torch, _nodata_args, _predict_batched, check_fit_features, ridge_dims, subsample_bands_evenly

_DTYPES = {"uint16": 2, "float32": 0}      # hsr_pair_prep's dtype codes
_MAX_FACTOR = 64                           # hsr_pair_prep's bound on the S2 / EMIT pixel ratio
_MAX_PLANES = 65535                        # hsr_block_mean's bound on the planes of one call
VIEWS = ("coarse", "degraded")
GROUPS = ("fit", "held_out")


def _dtype_name(a) -> str:
    return str(a.dtype).replace("torch.", "")


def _describe(x, what: str, ndim: int):
    """(batched shape, dtype name) of a cube or a batch of cubes: a (P, ...) array / tensor or a list of (...) ones."""
    if isinstance(x, (list, tuple)):
        if not x:
            raise ValueError(f"{what}: empty list")
        shapes = {tuple(e.shape) for e in x}
        dts = {_dtype_name(e) for e in x}
        if len(shapes) != 1 or len(dts) != 1:
            raise ValueError(f"{what}: the pairs of a batch must share one shape and dtype, got {sorted(shapes)} {sorted(dts)}")
        shape, dt = (len(x),) + shapes.pop(), dts.pop()
    else:
        shape, dt = tuple(x.shape), _dtype_name(x)
    if len(shape) != ndim + 1:
        raise ValueError(f"{what}: expected (P, {', '.join('abc'[:ndim])}) / a list of {ndim}-d cubes, got shape {shape}")
    return shape, dt


def _bands_index(bands, nbands: int) -> np.ndarray:
    if isinstance(bands, str):
        if bands != "all":
            raise ValueError(f"bands={bands!r}: an int, an index array or 'all'")
        return np.arange(nbands, dtype=np.int32)
    if isinstance(bands, (bool, np.bool_)):
        raise ValueError("bands: a bool is not a band count")
    if isinstance(bands, (int, np.integer)):
        if not 1 <= int(bands) <= nbands:
            raise ValueError(f"bands={bands}: keep between 1 and {nbands} of the EMIT bands")
        return subsample_bands_evenly(nbands, int(bands)).astype(np.int32)
    idx = np.asarray(bands)
    if idx.ndim != 1 or idx.size == 0 or idx.dtype.kind not in "iu":
        raise ValueError(f"bands: a non-empty 1-d integer index array, got {idx.dtype} of shape {idx.shape}")
    if idx.min() < 0 or idx.max() >= nbands:
        raise ValueError(f"bands: indices must lie in [0, {nbands}), got [{idx.min()}, {idx.max()}]")
    return idx.astype(np.int32)


@dataclass
class _Plan:
    P: int
    nbands: int
    h: int
    w: int
    nb: int
    factor: int
    bands: np.ndarray
    emit_dtype: str
    s2_dtype: str
    plane_slices: tuple = ()


def _plane_slices(P: int, T: int, limit: int = _MAX_PLANES):
    """The pairs [p0, p1) of each hsr_block_mean call over a (P, T, ...) cube seen as P T planes: whole pairs, at most ``limit``
    planes a call, so the number of calls is ceil(P / floor(limit / T))."""
    if not 1 <= T <= limit:
        raise ValueError(f"validate: {T} target bands, the block mean takes at most {limit} planes a call")
    step = limit // T
    return tuple((p0, min(p0 + step, P)) for p0 in range(0, P, step))


def _plan(emits, s2s, bands, degree, factor, s2_coarse, report=False, train_mask=None, validate=False) -> _Plan:
    """Every check that needs no GPU: shapes, dtypes, the factor, the bands, the size of the ridge system, the report and
    validate flags and the training mask."""
    if not isinstance(report, bool):
        raise ValueError(f"report={report!r}: must be True or False")
    if not isinstance(validate, bool):
        raise ValueError(f"validate={validate!r}: must be True or False")
    try:
        f = operator.index(factor)
    except TypeError:
        raise ValueError(f"factor={factor!r}: the S2 / EMIT pixel ratio must be an integer") from None
    if f < 1:
        raise ValueError(f"factor={f}: must be >= 1")
    if f > _MAX_FACTOR:
        raise ValueError(f"factor={f}: the pair prep takes at most {_MAX_FACTOR}")
    if not 1 <= int(degree) <= 3:
        raise ValueError(f"degree={degree}: 1, 2 or 3")
    (P, B, h, w), edt = _describe(emits, "emit", 3)
    (P2, nb, H, W), sdt = _describe(s2s, "s2", 3)
    if P2 != P:
        raise ValueError(f"{P} EMIT tiles but {P2} S2 tiles")
    if edt not in _DTYPES or sdt not in _DTYPES:
        raise ValueError(f"emit is {edt}, s2 is {sdt}: each must be uint16 or float32")
    if (H, W) != (h * f, w * f):
        raise ValueError(f"s2 is {H} x {W} but emit {h} x {w} at factor {f} needs {h * f} x {w * f}")
    if not 1 <= nb <= nat.HSR_MAX_BANDS:
        raise ValueError(f"s2 has {nb} bands: 1 .. {nat.HSR_MAX_BANDS} supported")
    check_fit_features(nb, degree)
    if s2_coarse is not None:
        cshape, cdt = _describe(s2_coarse, "s2_coarse", 3)
        if cshape != (P, nb, h, w) or cdt != "float32":
            raise ValueError(f"s2_coarse: expected float32 {(P, nb, h, w)}, got {cdt} {cshape}")
    if train_mask is not None:
        mshape, mdt = _describe(train_mask, "train_mask", 2)
        if mshape != (P, h, w) or mdt not in ("bool", "uint8"):
            raise ValueError(f"train_mask: expected bool or uint8 {(P, h, w)}, got {mdt} {mshape}")
    idx = _bands_index(bands, B)
    return _Plan(P, B, h, w, nb, f, idx, edt, sdt, _plane_slices(P, len(idx)) if validate else ())


def _stack_dev(x, torch, dev):
    """A (P, ...) contiguous device tensor from a batch tensor / array or a list of cubes (stacked ON the device; uint16 is
    moved as int16 bits, which every torch operation supports)."""
    def one(e):
        if _is_torch(e):
            return e
        a = np.ascontiguousarray(e)
        return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)

    if isinstance(x, (list, tuple)):
        if all(not _is_torch(e) for e in x):                     # NumPy pairs: stacked on the host, copied once
            return _stack_dev(np.stack([np.asarray(e) for e in x]), torch, dev)
        parts = [one(e).to(dev) for e in x]
        parts = [p.view(torch.int16) if p.dtype == torch.uint16 else p for p in parts]
        out = torch.stack(parts)
    else:
        out = one(x).to(dev)
        if out.dtype == torch.uint16:
            out = out.view(torch.int16)
    return out.contiguous()


_BANDS_CACHE: dict = {}


def _bands_dev(idx: np.ndarray, torch, dev):
    key = (idx.tobytes(), str(dev))
    t = _BANDS_CACHE.get(key)
    if t is None:
        t = _BANDS_CACHE[key] = torch.from_numpy(idx.copy()).to(dev)
    return t


@dataclass
class TilePairValidation:
    """``fuse_tile_pairs(validate=True).validation`` (device tensors): two views of the prediction on the EMIT grid, each scored
    against the decoded EMIT targets for two groups of pixels.  Axes V = ``views``, G = ``groups``.

    views    ("coarse", "degraded"): the pair's model applied to ``s2_coarse`` (what the fit was trained to do), and the 10 m
             ``cube`` averaged over each f x f block (``hsr_block_mean``'s arithmetic; a NaN sample makes the block NaN) - the
             consistency half of Wald's protocol;
    groups   ("fit", "held_out"): ``mask``, and ``held_out`` = ``valid & ~train_mask``;
    pred_coarse, cube_coarse  (P, T, h, w) float32, the two views themselves;
    n        (P, V, G, T) int64, the group's pixels with a finite prediction and target in the band;
    rmse, r2, mean_ref  (P, V, G, T) float64 over those: d = y - p in float32, rmse = sqrt(mean d^2), mean_ref = mean y,
             r2 = 1 - sum d^2 / (sum (y - mean_ref)^2 + 1e-8), sums in float64; NaN where n == 0;
    sam, n_sam  (P, V, G) float64 / int64: the mean spectral angle in degrees over the group's pixels that have one (every band
             of prediction and target finite, neither spectrum zero) and their count;
    ergas    (P, V, G) float64 = 100 / factor * sqrt(mean over the bands with n > 0 and mean_ref != 0 of (rmse / mean_ref)^2);
    sam_map  (P, V, h, w) float32, the angle of every such pixel, NaN elsewhere.
    A pair with ``status != 0`` has an all-NaN cube: n = 0 and NaN throughout."""
    pred_coarse: Any
    cube_coarse: Any
    n: Any
    rmse: Any
    r2: Any
    mean_ref: Any
    sam: Any
    n_sam: Any
    ergas: Any
    sam_map: Any
    views: tuple = VIEWS
    groups: tuple = GROUPS


@dataclass
class TilePairOutput:
    """What ``fuse_tile_pairs`` returns (device tensors, nothing copied to the host):

    cube     (P, T, h f, w f) float32 = sigmoid(clip(model(S2 at 10 m), +-50)), NaN where predict_cube_logit leaves NaN (a
             non-finite or ``s2_nodata`` input) and everywhere for a pair without training pixels;
    n_train  (P,) int64, the pixels the fit used: those that survived the flatten rule and, if given, ``train_mask``;
    status   (P,) int32: 0 fitted, 1 no training pixel, 2 non-positive Cholesky pivot (e.g. alpha = 0 and training pixels
             that all carry one S2 vector); a pair with status != 0 has NaN intercepts (``model(i).intercept_``), an all-NaN
             cube and NaN ``r2`` / ``rmse``, while its other fit outputs are whatever the failed solve left;
    mask     (P, h, w) bool, the pixels the fit used: ``valid & train_mask``;
    valid    (P, h, w) bool, flatten_pixels' rule on the EMIT grid (equal to ``mask`` without a ``train_mask``);
    held_out (P, h, w) bool = ``valid & ~train_mask`` (all False without a ``train_mask``);
    validation  a ``TilePairValidation`` with ``validate=True`` (else None);
    s2_coarse (P, nb, h, w) float32, S2 on the EMIT grid as the fit saw it (the block mean, or the caller's ``s2_coarse``);
    bands    (T,) the EMIT band indices of the targets;
    r2, rmse (P, T) float64 with ``report=True`` (else None): the fit scored on its own training pixels as the notebook's cell 26
             does - yp = sigmoid(clip(float32(model(X_train)), +-50)) in float32, d = y - yp against the decoded targets,
             r2 = 1 - sum d^2 / (sum (y - mean y)^2 + 1e-8), rmse = sqrt(mean d^2), sums in float64; NaN where status != 0.
    ``model(i)`` is pair i's model as a ``PolyRidge`` (its host attributes are copied on first access)."""
    cube: Any
    n_train: Any
    status: Any
    mask: Any
    s2_coarse: Any
    bands: np.ndarray
    degree: int
    alpha: float
    _fit: dict = field(repr=False, default_factory=dict)
    r2: Any = None
    rmse: Any = None
    valid: Any = None
    held_out: Any = None
    validation: Optional[TilePairValidation] = None

    def model(self, i: int) -> PolyRidge:
        f = self._fit
        m = PolyRidge(self.degree, self.alpha)
        m.n_in, m.n_feat, m.n_targets = f["n_in"], f["nf"], len(self.bands)
        m._fit64 = (f["mean"][i], f["scale"][i], f["Bp"][i, :f["nf"]], f["b64"][i])
        m._dev = dict(W=f["W32"][i], b=f["b32"][i], mean=f["mean32"][i], inv=f["inv32"][i])
        return m


# What the fit of fuse_tile_pairs (steps 1 - 5) hands to the steps that read it: fit = TilePairOutput._fit; model = the predict
# kernels' float32 operands W, b, mean, inv (tensors of fit); x (P, nb, npix) float32 S2 on the EMIT grid; y (P, T, npix) float32
# decoded targets; group (P, npix) uint8: 1 fit, 2 held out, 0 neither; degree.
_FitState = namedtuple("_FitState", "fit model x y group degree")


def fuse_tile_pairs(emits, s2s, *, bands=32, degree: int = 3, alpha: float = 1.0, factor: int = 6,
                    emit_nodata: Optional[float] = None, s2_nodata: Optional[float] = None, s2_coarse=None,
                    eps: float = 1e-4, report: bool = False, train_mask=None, validate: bool = False) -> TilePairOutput:
    """P tile pairs -> their fused 10 m cubes (see the module docstring).

    emits: (P, bands, h, w) uint16 (decoded as ``u == 65535 ? NaN : float32(u) * 1e-4f``) or float32 reflectance (with an
    optional ``emit_nodata``, tested with the isclose rule); s2s: (P, nb, h f, w f) uint16 DN or float32 (optional
    ``s2_nodata``).  Device tensors, NumPy arrays (copied once) or lists of per-pair cubes (stacked on the device).
    bands: an int (evenly subsampled, ``subsample_bands_evenly``), an index array or ``"all"``.
    report: also score every pair's fit on its training pixels (``r2`` / ``rmse`` of the output); two more launches, no host
    sync, and every other output keeps the bits it has without the report.
    train_mask: (P, h, w) bool / uint8 (array, tensor or list of (h, w) ones): the fit uses ``valid & train_mask``; ``n_train``,
    ``status`` and the report follow that mask, the other valid pixels are ``held_out``.
    validate: also score the prediction against the EMIT tile (``validation``, see ``TilePairValidation``); a fixed number of
    launches more, no host sync, and every other output keeps its bits."""
    plan = _plan(emits, s2s, bands, degree, factor, s2_coarse, report, train_mask, validate)
    torch = nat.require_gpu()
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    P, nb, h, w, f = plan.P, plan.nb, plan.h, plan.w, plan.factor
    T, npix, npix10 = len(plan.bands), h * w, h * w * f * f
    E = _stack_dev(emits, torch, dev)
    S = _stack_dev(s2s, torch, dev)
    Sc = _stack_dev(s2_coarse, torch, dev) if s2_coarse is not None else None
    Tm = _stack_dev(train_mask, torch, dev) if train_mask is not None else None
    st = _stream(torch)
    nat.check(lib.hsr_polyfeat_prepare(nb, int(degree)), "hsr_polyfeat_prepare")
    dims = ridge_dims(nb, degree, T)
    nf, na, ldq, npad, kpad = dims.nf, dims.na, dims.ldq, dims.npad, dims.kpad
    f64 = dict(dtype=torch.float64, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)

    # 1. pair prep: block mean, band gather / decode, training mask
    x = torch.empty((P, nb, npix), **f32)
    y = torch.empty((P, T, npix), **f32)
    mask = torch.empty((P, npix), dtype=torch.uint8, device=dev)
    src, src_dt, pair_s, fac = (Sc, 0, nb * npix, 0) if Sc is not None else (S, _DTYPES[plan.s2_dtype], S.stride(0), f)
    nat.check(lib.hsr_pair_prep(_ptr(E), _DTYPES[plan.emit_dtype], E.stride(0), plan.nbands, _ptr(_bands_dev(plan.bands, torch, dev)),
                                T, _ptr(src), src_dt, pair_s, nb, h, w, fac, *_nodata_args(emit_nodata), *_nodata_args(s2_nodata),
                                _ptr(x), _ptr(y), _ptr(mask), P, st), "hsr_pair_prep")
    valid = group = mask                               # without a train_mask: one array, codes 0 / 1
    if Tm is not None:                                 # the fit's mask = the rule's & the caller's; 1 fit, 2 held out
        Tm = Tm.view(torch.uint8) if Tm.dtype == torch.bool else Tm
        mask = torch.empty_like(valid)
        group = torch.empty_like(valid)
        nat.check(lib.hsr_pair_holdout(_ptr(valid), _ptr(Tm), npix, npix, _ptr(mask), _ptr(group), P, st), "hsr_pair_holdout")
    # 2. StandardScaler over the training pixels
    stats = torch.empty((P, 1 + 2 * nb), **f64)
    mean = torch.empty((P, nb), **f64)
    scale = torch.empty((P, nb), **f64)
    n_train = torch.empty(P, dtype=torch.int64, device=dev)
    nat.check(lib.hsr_pair_stats(_ptr(x), _ptr(mask), npix, nb, _ptr(stats), _ptr(mean), _ptr(scale), _ptr(n_train), P, st),
              "hsr_pair_stats")
    # 3. [1 | Phi | logit(y)] rows of the training pixels, zero rows for the others; 4. their Gram
    Q = torch.empty((P, npix, ldq), **f64)
    nat.check(lib.hsr_pair_expand_f64(_ptr(x), nb * npix, _ptr(mean), _ptr(scale), nb, _ptr(y), T * npix, _ptr(mask), npix, npix,
                                      nb, int(degree), T, float(eps), _ptr(Q), ldq, npix * ldq, na, P, st), "hsr_pair_expand_f64")
    wq = lib.hsr_gram_work_bytes(na, ldq, npix) // 8
    work = torch.empty((P, wq), **f64)
    G = torch.empty((P, na, ldq), **f64)
    nat.check(lib.hsr_gram_f64_batched(_ptr(Q), ldq, na, ldq, npix, npix * ldq, _ptr(work), wq, _ptr(G), ldq, na * ldq, P, st),
              "hsr_gram_f64_batched")
    # 5. centred ridge systems, P Cholesky factorisations side by side, model read-out
    Gp = torch.empty((P, npad, npad), **f64)
    Bp = torch.empty((P, npad, T), **f64)
    info = torch.empty(P, dtype=torch.int32, device=dev)
    nat.check(lib.hsr_ridge_assemble_batched(_ptr(G), ldq, na * ldq, na, nf, T, float(alpha), _ptr(Gp), npad, npad * npad, _ptr(Bp),
                                             T, npad * T, _ptr(info), P, st), "hsr_ridge_assemble_batched")
    cw = lib.hsr_chol_work_bytes(npad) // 8
    cwork = torch.empty((P, cw), **f64)
    nat.check(lib.hsr_chol_solve_f64_batched(_ptr(Gp), npad, npad, npad * npad, _ptr(Bp), T, T, npad * T, _ptr(cwork), _ptr(info), P,
                                             st), "hsr_chol_solve_f64_batched")
    b64 = torch.empty((P, T), **f64)
    W32 = torch.empty((P, kpad, T), **f32)
    b32 = torch.empty((P, T), **f32)
    mean32 = torch.empty((P, nb), **f32)
    inv32 = torch.empty((P, nb), **f32)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    nat.check(lib.hsr_ridge_finish_batched(_ptr(G), na * ldq, na, nf, T, _ptr(Bp), T, npad * T, _ptr(mean), _ptr(scale), nb, nb, kpad,
                                           _ptr(b64), _ptr(b32), T, _ptr(W32), kpad * T, _ptr(mean32), _ptr(inv32), nb, _ptr(info),
                                           _ptr(status), P, st), "hsr_ridge_finish_batched")
    r2 = rmse = None
    if report:                                         # the notebook's cell 26 on the rows Q the fit read
        rw = lib.hsr_pair_report_work_bytes(npix, T) // 8
        rwork = torch.empty((P, rw), **f64)
        r2 = torch.empty((P, T), **f64)
        rmse = torch.empty((P, T), **f64)
        nat.check(lib.hsr_pair_report_f64(_ptr(Q), ldq, npix * ldq, na, npix, _ptr(b64), T, _ptr(Bp), T, npad * T, nf, _ptr(y),
                                          T * npix, _ptr(mask), npix, T, _ptr(status), _ptr(rwork), rw, _ptr(r2), _ptr(rmse), T, P,
                                          st), "hsr_pair_report_f64")
    # 6. the 10 m prediction: predict_cube_logit's rule for unusable pixels, per pair
    if plan.s2_dtype == "uint16":                      # DN as float32 (exact), from the int16 bits
        Xf = (S.to(torch.int32) & 0xFFFF).to(torch.float32)
    else:
        Xf = S
    Xf = Xf.reshape(P, nb, npix10)
    fit = dict(n_in=nb, nf=nf, mean=mean, scale=scale, Bp=Bp, b64=b64, W32=W32, b32=b32, mean32=mean32, inv32=inv32)
    state = _FitState(fit, dict(W=W32, b=b32, mean=mean32, inv=inv32), x, y, group, int(degree))
    cube = _predict_batched(lib, st, state.degree, state.model, _ptr(Xf), 1, npix10, nb * npix10, npix10, P, 1, True, s2_nodata,
                            torch.empty((P, T, npix10), **f32))
    validation = _validate(lib, torch, st, plan, state, cube, s2_nodata) if validate else None
    held = (group == 2) if Tm is not None else torch.zeros_like(mask, dtype=torch.bool)
    mask_b = mask.view(P, h, w).bool()
    valid_b = mask_b if Tm is None else valid.view(P, h, w).bool()
    return TilePairOutput(cube=cube.view(P, T, h * f, w * f), n_train=n_train, status=status, mask=mask_b,
                          s2_coarse=x.view(P, nb, h, w), bands=plan.bands, degree=int(degree), alpha=float(alpha), _fit=fit,
                          r2=r2, rmse=rmse, valid=valid_b, held_out=held.view(P, h, w), validation=validation)


def _validate(lib, torch, st, plan, state, cube, s2_nodata) -> TilePairValidation:
    """The two views on the EMIT grid and their scores: one predict launch, one block mean per slice of planes, two launches per
    view (csrc/hsr_pairs.hip); the launch count depends on ceil(P T / 65535) only."""
    x, y, group = state.x, state.y, state.group
    P, nb, h, w, f = plan.P, plan.nb, plan.h, plan.w, plan.factor
    T, npix, npix10 = len(plan.bands), h * w, h * w * f * f
    dev = x.device
    f64 = dict(dtype=torch.float64, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)
    views = torch.empty((2, P, T, npix), dtype=torch.float32, device=dev)
    pred, coarse = views[0], views[1]
    _predict_batched(lib, st, state.degree, state.model, _ptr(x), 1, npix, nb * npix, npix, P, 1, True, s2_nodata, pred)
    for p0, p1 in plan.plane_slices:
        nat.check(lib.hsr_block_mean(_ptr(cube[p0:p1]), 0, npix10, 1, (p1 - p0) * T, h, w, f, 1.0, _ptr(coarse[p0:p1]), npix, 1, st),
                  "hsr_block_mean")
    V, G = len(VIEWS), len(GROUPS)
    n = torch.empty((P, V, G, T), **i64)
    rmse = torch.empty((P, V, G, T), **f64)
    r2 = torch.empty((P, V, G, T), **f64)
    mean_ref = torch.empty((P, V, G, T), **f64)
    sam = torch.empty((P, V, G), **f64)
    n_sam = torch.empty((P, V, G), **i64)
    ergas = torch.empty((P, V, G), **f64)
    sam_map = torch.empty((P, V, npix), dtype=torch.float32, device=dev)
    sw = lib.hsr_pair_score_work_bytes(npix, T) // 8
    work = torch.empty((P, sw), **f64)
    for v in range(V):
        nat.check(lib.hsr_pair_score_f64(_ptr(views[v]), T * npix, _ptr(y), T * npix, _ptr(group), npix, npix, T, 100.0 / f,
                                         _ptr(work), sw, _ptr(n[:, v]), _ptr(rmse[:, v]), _ptr(r2[:, v]), _ptr(mean_ref[:, v]),
                                         V * G * T, _ptr(sam[:, v]), _ptr(n_sam[:, v]), _ptr(ergas[:, v]), V * G,
                                         _ptr(sam_map[:, v]), V * npix, P, st), "hsr_pair_score_f64")
    return TilePairValidation(pred_coarse=pred.view(P, T, h, w), cube_coarse=coarse.view(P, T, h, w), n=n, rmse=rmse, r2=r2,
                              mean_ref=mean_ref, sam=sam, n_sam=n_sam, ergas=ergas, sam_map=sam_map.view(P, V, h, w))


def fuse_tile_pair(emit, s2, *, bands=32, degree: int = 3, alpha: float = 1.0, factor: int = 6,
                   emit_nodata: Optional[float] = None, s2_nodata: Optional[float] = None, s2_coarse=None,
                   eps: float = 1e-4, report: bool = False, train_mask=None, validate: bool = False) -> TilePairOutput:
    """One tile pair: emit (bands, h, w), s2 (nb, h f, w f) -> a TilePairOutput with P = 1 (``cube[0]`` is (T, h f, w f)).
    The same launches as ``fuse_tile_pairs``, so a pair gives the same bits alone as in any batch."""
    batch = lambda a: None if a is None else ([a] if not _is_torch(a) and not isinstance(a, np.ndarray) else a[None])
    return fuse_tile_pairs(batch(emit), batch(s2), bands=bands, degree=degree, alpha=alpha, factor=factor,
                           emit_nodata=emit_nodata, s2_nodata=s2_nodata, s2_coarse=batch(s2_coarse), eps=eps, report=report,
                           train_mask=batch(train_mask), validate=validate)
