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

``pool=`` shares one model among a group of pairs: M groups, each fitted on the training pixels of all its members and applied to
every member, also to members that were kept out of the fit as a whole (``train_mask`` all False) - with ``validate=True`` that
is generalisation to unseen tiles, where hold-out inside a tile measures interpolation.  Nothing is concatenated: a group's
StandardScaler is a Chan merge of its members' ``[n, mean, M2]`` (``hsr_pool_stats``), every member's rows are expanded with the
group's mean and scale, so the group's Gram is the sum of its members' Grams (``hsr_pool_gram``), M systems are assembled,
factorised and read out instead of P, and one launch hands every pair a copy of its group's model in the per-pair layout that
the report, predict and validate steps read (``hsr_pool_models``): three launches more than without pooling, whatever P and M
are.  Merges walk a group's members in pair-index order, skip members without training pixels and copy the first one, so
singleton groups give the bits of ``pool=None`` and a group does not depend on the other groups of its batch.
``TilePairOutput.predict`` applies the fitted models to S2 tiles that have no EMIT partner.

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
    pool: Optional[np.ndarray] = None          # (P,) int32 group ids 0 .. M-1, None without pooling
    M: int = 0


def _plane_slices(P: int, T: int, limit: int = _MAX_PLANES):
    """The pairs [p0, p1) of each hsr_block_mean call over a (P, T, ...) cube seen as P T planes: whole pairs, at most ``limit``
    planes a call, so the number of calls is ceil(P / floor(limit / T))."""
    if not 1 <= T <= limit:
        raise ValueError(f"validate: {T} target bands, the block mean takes at most {limit} planes a call")
    step = limit // T
    return tuple((p0, min(p0 + step, P)) for p0 in range(0, P, step))


def _pool_ids(pool, P: int) -> np.ndarray:
    """``pool`` -> the (P,) int32 group ids 0 .. M-1 (host data only; see ``fuse_tile_pairs``)."""
    if isinstance(pool, str):
        if pool != "all":
            raise ValueError(f"pool={pool!r}: None, 'all' or a sequence of {P} group ids")
        return np.zeros(P, dtype=np.int32)
    if _is_torch(pool):
        if pool.device.type != "cpu":
            raise ValueError("pool: the group ids are host data (a list or a NumPy array); reading a device tensor would need a "
                             "host sync")
        pool = pool.numpy()
    if isinstance(pool, (bool, np.bool_)):
        raise ValueError("pool: a bool is not a list of group ids")
    try:
        ids = np.asarray(pool)
    except Exception:
        raise ValueError(f"pool={pool!r}: None, 'all' or a sequence of {P} group ids") from None
    if ids.dtype.kind not in "iu":
        raise ValueError(f"pool: the group ids must be integers, got {ids.dtype}")
    if ids.shape != (P,):
        raise ValueError(f"pool: expected {P} group ids, one per pair, got shape {ids.shape}")
    if ids.min() < 0:
        raise ValueError(f"pool: negative group id {int(ids.min())}")
    used = np.unique(ids)
    if int(used[-1]) != len(used) - 1:
        raise ValueError(f"pool: the group ids must be exactly 0 .. M-1, each used at least once; got {len(used)} distinct ids "
                         f"up to {int(used[-1])}")
    return ids.astype(np.int32)


def pool_layout(ids: np.ndarray):
    """(order, start) of the group ids ``ids`` (P,), values 0 .. M-1: order (P,) int32 = the pairs sorted by (group, pair index),
    start (M + 1,) int32 = each group's slice of order.  What the pooling kernels walk (include/hsr.h)."""
    ids = np.asarray(ids, dtype=np.int64)
    order = np.argsort(ids, kind="stable").astype(np.int32)
    start = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=int(ids.max()) + 1))]).astype(np.int32)
    return order, start


def _plan(emits, s2s, bands, degree, factor, s2_coarse, report=False, train_mask=None, validate=False, pool=None) -> _Plan:
    """Every check that needs no GPU: shapes, dtypes, the factor, the bands, the size of the ridge system, the report and
    validate flags, the training mask and the pooling."""
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
    ids = _pool_ids(pool, P) if pool is not None else None
    return _Plan(P, B, h, w, nb, f, idx, edt, sdt, _plane_slices(P, len(idx)) if validate else (), ids,
                 int(ids.max()) + 1 if ids is not None else 0)


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


_POOL_CACHE: dict = {}


def _pool_dev(ids: np.ndarray, torch, dev):
    """(order, start, group_of) int32 device tensors of the group ids, uploaded once per id list and device."""
    key = (ids.tobytes(), str(dev))
    t = _POOL_CACHE.get(key)
    if t is None:
        order, start = pool_layout(ids)
        t = _POOL_CACHE[key] = tuple(torch.from_numpy(a.copy()).to(dev) for a in (order, start, ids))
    return t


_INDEX_CACHE: dict = {}


def _index_dev(idx: np.ndarray, torch, dev):
    key = (idx.tobytes(), str(dev))
    t = _INDEX_CACHE.get(key)
    if t is None:
        t = _INDEX_CACHE[key] = torch.from_numpy(idx.copy()).to(dev)
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
    ``model(i)`` is pair i's model as a ``PolyRidge`` (its host attributes are copied on first access).

    With ``pool=`` (else None): pool (P,) NumPy int32, each pair's group; n_pool (M,) int64, the training pixels of each group;
    pool_status (M,) int32, the status of each group's fit.  ``status`` is then the group's status per pair, ``n_train`` stays each
    pair's own count, ``model(i)`` is the model of pair i's group and ``pool_model(g)`` that of group g; ``r2`` / ``rmse`` score a
    pair's own training pixels with its group's model and are NaN for a pair that supplied none.
    ``predict(s2s, model_index)`` applies the fitted models to S2 tiles that have no EMIT partner."""
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
    pool: Optional[np.ndarray] = None
    n_pool: Any = None
    pool_status: Any = None
    _pool_fit: Optional[dict] = field(repr=False, default=None)

    def _model_of(self, f: dict, i: int) -> PolyRidge:
        m = PolyRidge(self.degree, self.alpha)
        m.n_in, m.n_feat, m.n_targets = f["n_in"], f["nf"], len(self.bands)
        m._fit64 = (f["mean"][i], f["scale"][i], f["Bp"][i, :f["nf"]], f["b64"][i])
        m._dev = dict(W=f["W32"][i], b=f["b32"][i], mean=f["mean32"][i], inv=f["inv32"][i])
        return m

    def model(self, i: int) -> PolyRidge:
        return self._model_of(self._fit, i)

    def pool_model(self, g: int) -> PolyRidge:
        """Group g's model (``pool=`` only): the one every member's cube comes from."""
        if self._pool_fit is None:
            raise ValueError("pool_model: this output was not fitted with pool=")
        return self._model_of(self._pool_fit, g)

    def predict(self, s2s, model_index=None, s2_nodata: Optional[float] = None):
        """Apply fitted models to Q S2 tiles that have no EMIT partner: s2s (Q, nb, H, W) uint16 DN or float32 (a tensor, an
        array or a list of cubes; any H and W), model_index a host array of Q pair indices (tile q takes ``model(model_index[q])``;
        optional when there is one pair or one group: all zeros) -> (Q, T, H, W) float32 on the device with the bits of
        ``model(model_index[q]).predict_cube(s2s[q], nodata=s2_nodata)``.  One predict launch over the gathered model rows on the
        current stream; nothing synchronises with the host."""
        f = self._fit
        nb, P = f["n_in"], f["b64"].shape[0]
        (Q, nbq, H, W), sdt = _describe(s2s, "s2", 3)
        if nbq != nb or sdt not in _DTYPES:
            raise ValueError(f"predict: s2 is {sdt} with {nbq} bands, the models take {nb} bands of uint16 or float32")
        if model_index is None:
            if P != 1 and (self.pool is None or int(self.pool.max()) != 0):
                raise ValueError(f"predict: model_index is required with {P} pairs that do not share one model")
            idx = np.zeros(Q, dtype=np.int64)
        else:
            if _is_torch(model_index) and model_index.device.type != "cpu":
                raise ValueError("predict: model_index is host data; reading a device tensor would need a host sync")
            idx = np.asarray(model_index)
            if idx.dtype.kind not in "iu" or idx.shape != (Q,):
                raise ValueError(f"predict: model_index must hold {Q} integer pair indices, got {idx.dtype} of shape {idx.shape}")
            if idx.min() < 0 or idx.max() >= P:
                raise ValueError(f"predict: model_index must lie in [0, {P}), got [{idx.min()}, {idx.max()}]")
            idx = idx.astype(np.int64)
        torch = nat.require_gpu()
        lib = nat.load()
        dev = f["b64"].device
        S = _stack_dev(s2s, torch, dev)
        Xf = (S.to(torch.int32) & 0xFFFF).to(torch.float32) if sdt == "uint16" else S      # as step 6 of fuse_tile_pairs
        rows = _index_dev(idx, torch, dev)
        model = dict(W=f["W32"].index_select(0, rows), b=f["b32"].index_select(0, rows), mean=f["mean32"].index_select(0, rows),
                     inv=f["inv32"].index_select(0, rows))
        nat.check(lib.hsr_polyfeat_prepare(nb, self.degree), "hsr_polyfeat_prepare")
        T, npix = len(self.bands), H * W
        out = torch.empty((Q, T, npix), dtype=torch.float32, device=dev)
        _predict_batched(lib, _stream(torch), self.degree, model, _ptr(Xf), 1, npix, nb * npix, npix, Q, 1, True, s2_nodata, out)
        return out.view(Q, T, H, W)


# What the fit of fuse_tile_pairs (steps 1 - 5) hands to the steps that read it: fit = TilePairOutput._fit; model = the predict
# kernels' float32 operands W, b, mean, inv (tensors of fit); x (P, nb, npix) float32 S2 on the EMIT grid; y (P, T, npix) float32
# decoded targets; group (P, npix) uint8: 1 fit, 2 held out, 0 neither; degree.
_FitState = namedtuple("_FitState", "fit model x y group degree")


def fuse_tile_pairs(emits, s2s, *, bands=32, degree: int = 3, alpha: float = 1.0, factor: int = 6,
                    emit_nodata: Optional[float] = None, s2_nodata: Optional[float] = None, s2_coarse=None,
                    eps: float = 1e-4, report: bool = False, train_mask=None, validate: bool = False, pool=None) -> TilePairOutput:
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
    launches more, no host sync, and every other output keeps its bits.
    pool: None (a model per pair), ``"all"`` (one model from the training pixels of all P pairs) or P ints on the host (a list or a
    NumPy array; a device tensor is refused, reading it would need a host sync): pair i belongs to group ``pool[i]``, the ids being
    exactly 0 .. M-1.  A group is fitted on the union of its members' ``valid & train_mask`` pixels and every member's cube comes
    from that model, also a member that supplied no training pixel (``train_mask`` all False: a wholly held-out pair, status 0); a
    group without any training pixel has status 1 and all-NaN cubes.  See ``TilePairOutput`` for the outputs under pooling."""
    plan = _plan(emits, s2s, bands, degree, factor, s2_coarse, report, train_mask, validate, pool)
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
    pooled = plan.pool is not None
    M = plan.M if pooled else P                        # the systems to solve: one per group, or one per pair
    if pooled:                                         # the group's scaler for every member (Chan merge of the pairs' statistics)
        order, start, group_of = _pool_dev(plan.pool, torch, dev)
        gstats = torch.empty((M, 1 + 2 * nb), **f64)
        n_pool = torch.empty(M, dtype=torch.int64, device=dev)
        gmean = torch.empty((M, nb), **f64)
        gscale = torch.empty((M, nb), **f64)
        mean = torch.empty((P, nb), **f64)
        scale = torch.empty((P, nb), **f64)
        nat.check(lib.hsr_pool_stats(_ptr(stats), nb, P, _ptr(order), _ptr(start), M, _ptr(gstats), _ptr(n_pool), _ptr(gmean),
                                     _ptr(gscale), _ptr(mean), _ptr(scale), st), "hsr_pool_stats")
    # 3. [1 | Phi | logit(y)] rows of the training pixels, zero rows for the others; 4. their Gram
    Q = torch.empty((P, npix, ldq), **f64)
    nat.check(lib.hsr_pair_expand_f64(_ptr(x), nb * npix, _ptr(mean), _ptr(scale), nb, _ptr(y), T * npix, _ptr(mask), npix, npix,
                                      nb, int(degree), T, float(eps), _ptr(Q), ldq, npix * ldq, na, P, st), "hsr_pair_expand_f64")
    wq = lib.hsr_gram_work_bytes(na, ldq, npix) // 8
    work = torch.empty((P, wq), **f64)
    G = torch.empty((P, na, ldq), **f64)
    nat.check(lib.hsr_gram_f64_batched(_ptr(Q), ldq, na, ldq, npix, npix * ldq, _ptr(work), wq, _ptr(G), ldq, na * ldq, P, st),
              "hsr_gram_f64_batched")
    Gs, smean, sscale = G, mean, scale                 # the Gram, mean and scale of each system
    if pooled:                                         # a group's Gram = the sum of its members' (rows expanded with one scaler)
        Gs, smean, sscale = torch.empty((M, na, ldq), **f64), gmean, gscale
        nat.check(lib.hsr_pool_gram(_ptr(G), na * ldq, na * ldq, _ptr(stats), 1 + 2 * nb, P, _ptr(order), _ptr(start), M, _ptr(Gs),
                                    na * ldq, st), "hsr_pool_gram")
    # 5. centred ridge systems, M Cholesky factorisations side by side (M = P without pooling), model read-out
    fit, status, rstatus = _solve(lib, torch, st, dims, Gs, smean, sscale, nb, T, float(alpha), M)
    pool_fit = pool_status = None
    if pooled:                                         # every pair gets its group's model: the per-pair layout the later steps read
        pool_fit, pool_status = fit, status
        fit = dict(n_in=nb, nf=nf, mean=mean, scale=scale, Bp=torch.empty((P, npad, T), **f64), b64=torch.empty((P, T), **f64),
                   W32=torch.empty((P, kpad, T), **f32), b32=torch.empty((P, T), **f32), mean32=torch.empty((P, nb), **f32),
                   inv32=torch.empty((P, nb), **f32))
        status = torch.empty(P, dtype=torch.int32, device=dev)
        rstatus = torch.empty(P, dtype=torch.int32, device=dev)
        g = pool_fit
        nat.check(lib.hsr_pool_models(_ptr(g["Bp"]), npad * T, _ptr(g["b64"]), _ptr(g["W32"]), kpad * T, _ptr(g["b32"]),
                                      _ptr(g["mean32"]), _ptr(g["inv32"]), _ptr(pool_status), _ptr(n_train), _ptr(group_of), nf, npad,
                                      kpad, T, nb, _ptr(fit["Bp"]), _ptr(fit["b64"]), _ptr(fit["W32"]), _ptr(fit["b32"]),
                                      _ptr(fit["mean32"]), _ptr(fit["inv32"]), _ptr(status), _ptr(rstatus), P, M, st),
                  "hsr_pool_models")
    Bp, b64, W32, b32, mean32, inv32 = (fit[k] for k in ("Bp", "b64", "W32", "b32", "mean32", "inv32"))
    r2 = rmse = None
    if report:                                         # the notebook's cell 26 on the rows Q the fit read
        rw = lib.hsr_pair_report_work_bytes(npix, T) // 8
        rwork = torch.empty((P, rw), **f64)
        r2 = torch.empty((P, T), **f64)
        rmse = torch.empty((P, T), **f64)
        nat.check(lib.hsr_pair_report_f64(_ptr(Q), ldq, npix * ldq, na, npix, _ptr(b64), T, _ptr(Bp), T, npad * T, nf, _ptr(y),
                                          T * npix, _ptr(mask), npix, T, _ptr(rstatus), _ptr(rwork), rw, _ptr(r2), _ptr(rmse), T, P,
                                          st), "hsr_pair_report_f64")
    # 6. the 10 m prediction: predict_cube_logit's rule for unusable pixels, per pair
    if plan.s2_dtype == "uint16":                      # DN as float32 (exact), from the int16 bits
        Xf = (S.to(torch.int32) & 0xFFFF).to(torch.float32)
    else:
        Xf = S
    Xf = Xf.reshape(P, nb, npix10)
    state = _FitState(fit, dict(W=W32, b=b32, mean=mean32, inv=inv32), x, y, group, int(degree))
    cube = _predict_batched(lib, st, state.degree, state.model, _ptr(Xf), 1, npix10, nb * npix10, npix10, P, 1, True, s2_nodata,
                            torch.empty((P, T, npix10), **f32))
    validation = _validate(lib, torch, st, plan, state, cube, s2_nodata) if validate else None
    held = (group == 2) if Tm is not None else torch.zeros_like(mask, dtype=torch.bool)
    mask_b = mask.view(P, h, w).bool()
    valid_b = mask_b if Tm is None else valid.view(P, h, w).bool()
    return TilePairOutput(cube=cube.view(P, T, h * f, w * f), n_train=n_train, status=status, mask=mask_b,
                          s2_coarse=x.view(P, nb, h, w), bands=plan.bands, degree=int(degree), alpha=float(alpha), _fit=fit,
                          r2=r2, rmse=rmse, valid=valid_b, held_out=held.view(P, h, w), validation=validation,
                          pool=plan.pool, n_pool=n_pool if pooled else None, pool_status=pool_status, _pool_fit=pool_fit)


def _solve(lib, torch, st, dims, G, mean, scale, nb: int, T: int, alpha: float, M: int):
    """Step 5 for M systems: G (M, na, ldq) Grams with their float64 mean / scale (M, nb) -> (the fit arrays with a leading M
    axis, status (M,), the report's status = the same tensor): assembly, M Cholesky factorisations side by side, read-out."""
    nf, na, ldq, npad, kpad = dims.nf, dims.na, dims.ldq, dims.npad, dims.kpad
    dev = G.device
    f64 = dict(dtype=torch.float64, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    Gp = torch.empty((M, npad, npad), **f64)
    Bp = torch.empty((M, npad, T), **f64)
    info = torch.empty(M, dtype=torch.int32, device=dev)
    nat.check(lib.hsr_ridge_assemble_batched(_ptr(G), ldq, na * ldq, na, nf, T, alpha, _ptr(Gp), npad, npad * npad, _ptr(Bp),
                                             T, npad * T, _ptr(info), M, st), "hsr_ridge_assemble_batched")
    cw = lib.hsr_chol_work_bytes(npad) // 8
    cwork = torch.empty((M, cw), **f64)
    nat.check(lib.hsr_chol_solve_f64_batched(_ptr(Gp), npad, npad, npad * npad, _ptr(Bp), T, T, npad * T, _ptr(cwork), _ptr(info), M,
                                             st), "hsr_chol_solve_f64_batched")
    b64 = torch.empty((M, T), **f64)
    W32 = torch.empty((M, kpad, T), **f32)
    b32 = torch.empty((M, T), **f32)
    mean32 = torch.empty((M, nb), **f32)
    inv32 = torch.empty((M, nb), **f32)
    status = torch.empty(M, dtype=torch.int32, device=dev)
    nat.check(lib.hsr_ridge_finish_batched(_ptr(G), na * ldq, na, nf, T, _ptr(Bp), T, npad * T, _ptr(mean), _ptr(scale), nb, nb, kpad,
                                           _ptr(b64), _ptr(b32), T, _ptr(W32), kpad * T, _ptr(mean32), _ptr(inv32), nb, _ptr(info),
                                           _ptr(status), M, st), "hsr_ridge_finish_batched")
    fit = dict(n_in=nb, nf=nf, mean=mean, scale=scale, Bp=Bp, b64=b64, W32=W32, b32=b32, mean32=mean32, inv32=inv32)
    return fit, status, status


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
                   eps: float = 1e-4, report: bool = False, train_mask=None, validate: bool = False, pool=None) -> TilePairOutput:
    """One tile pair: emit (bands, h, w), s2 (nb, h f, w f) -> a TilePairOutput with P = 1 (``cube[0]`` is (T, h f, w f)).
    The same launches as ``fuse_tile_pairs``, so a pair gives the same bits alone as in any batch (``pool``: None, ``"all"`` or
    ``[0]``, which all give those bits)."""
    batch = lambda a: None if a is None else ([a] if not _is_torch(a) and not isinstance(a, np.ndarray) else a[None])
    return fuse_tile_pairs(batch(emit), batch(s2), bands=bands, degree=degree, alpha=alpha, factor=factor,
                           emit_nodata=emit_nodata, s2_nodata=s2_nodata, s2_coarse=batch(s2_coarse), eps=eps, report=report,
                           train_mask=batch(train_mask), validate=validate, pool=pool)
