"""fuse_tile_pairs at the shapes, dtypes and edges where its kernels go wrong, against float64 references.

One case table.  A row names a geometry - P, the S2 bands nb, degree, the targets T (or a band-index array), the tile h x w,
the factor (0: the caller's ``s2_coarse``), the EMIT / S2 dtypes, the nodata values, alpha, report and what each pair of the
batch is (fitted, without a training pixel, with fewer training pixels than features, with a constant S2 band, with one S2
vector on every pixel) - and the instances it must reach: the predict slot of hsr_polyfeat_predict_kernel (0 x16, 1 .. 3
slice<1 .. 3>, 4 .. 6 predict_kernel<1 / 2 / 4>), the Cholesky factor kernel (chol_factor_res_kernel for npad <= 288, else
chol_factor_kernel), whether chol_solve_kernel keeps the block inverses in LDS (400 npad + 4352 <= 160 KiB) and the block
kinds of the batched Gram's plan for (na, ldq) (gram_lds_plan: wide, diag, narrow).  Inputs come from a seeded generator with
the targets' logits inside [-3, 3] and 65535 / NaN / nodata samples scattered through them.  For every row:
  * prep: mask and n_train exactly the flatten rule on oracle_np.tile_decode_u16 / oracle_np.block_mean; s2_coarse
    bit-equal to oracle_np.block_mean where finite, NaN exactly where a block holds a bad sample (or the caller's s2_coarse);
  * fit: mean_ / scale_ within rtol 1e-12 of oracle_np.ridge_poly_fit on the same float32 training pixels and logit(y), the
    training-pixel logits of the device's float64 model within 1e-6 of the oracle's;
  * cube: oracle_np.predict_cube_logit of the device's float64 model on the 10 m input: the same NaN set, 1e-4 elsewhere;
  * report: r2 / rmse against report_reference of the oracle's model (the tolerances of test_gpu_tile_pairs_report);
  * status: 0 fitted, 1 no training pixel, 2 non-positive pivot; a pair with status != 0 has NaN intercepts, an all-NaN
    cube and NaN r2 / rmse;
  * bits: every pair of the batch carries the bits of fuse_tile_pair of that pair alone;
  * selection: hsr_polyfeat_predict_kernel names the row's slot, the Python mirrors of chol_launch / gram_lds_plan its
    Cholesky and Gram instances.
Then: the rows give the same bits again after rows of other (nb, degree) have swapped the process-wide monomial table, the
batched Gram and Cholesky run on exact data at every shape the table reaches and more, and the rows together reach every
predict slot, both factor kernels, both solve forms and all three Gram block kinds.
"""
import zlib
from dataclasses import dataclass
from functools import lru_cache
from math import comb
from typing import Optional, Tuple

import numpy as np
import pytest

from gpu_harness import torch_gpu  # noqa: F401
from oracle import oracle_np as onp
from test_tile_pairs_report_host import report_reference

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------
# shapes and the instances they reach (mirrors of the host rules in pairs.py, csrc/hsr_chol.hip, csrc/hsr_gram.hip and csrc/hsr_ridge.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def n_features(nb, degree):
    return sum(comb(nb + d - 1, d) for d in range(1, degree + 1))


def sizes(nb, degree, T):
    """(nf, na, ldq, npad) as fuse_tile_pairs forms them."""
    nf = n_features(nb, degree)
    na = (nf + 1 + 15) // 16 * 16
    return nf, na, na + (T + 15) // 16 * 16, (nf + 31) // 32 * 32


def chol_instances(npad):
    """(factor kernel, block inverses in LDS) of chol_launch."""
    return ("res" if npad <= 288 else "factor"), 400 * npad + 4352 <= 160 * 1024


def gram_kinds(na, ldq):
    """The block kinds of gram_lds_plan(na, ldq, sym = 1): 96-wide panels, a last strip of <= 32 columns as narrow blocks."""
    nbi = -(-na // 96)
    rem = ldq % 96
    strip = 0 < rem <= 32
    nbj = ldq // 96 if strip else -(-ldq // 96)
    kinds = set()
    if any(bj > bi for bi in range(nbi) for bj in range(nbj)):
        kinds.add("wide")
    if min(nbi, nbj) > 0:
        kinds.add("diag")
    if strip:
        kinds.add("narrow")
    return frozenset(kinds)


# pair kinds: ok = fitted; empty = no training pixel (status 1); few = fewer training pixels than features; const = S2 band 0
# constant (scale 1); same = every pixel carries one S2 vector (with alpha = 0: centred Gram exactly 0, status 2)
@dataclass(frozen=True)
class Row:
    id: str
    nb: int
    degree: int
    T: int
    h: int
    w: int
    factor: int                      # 0: the caller's s2_coarse (the 10 m S2 is then at factor 3)
    edt: str                         # EMIT dtype
    sdt: str                         # S2 dtype
    slot: int                        # hsr_polyfeat_predict_kernel
    gram: Tuple[str, ...]            # gram_lds_plan's block kinds
    pairs: Tuple[str, ...] = ("ok",)
    emit_nd: Optional[float] = None
    s2_nd: Optional[float] = None
    alpha: float = 1.0
    report: bool = False
    bands: Optional[Tuple[int, ...]] = None    # a band-index array instead of T evenly spaced bands
    B: int = 0                       # EMIT bands (0: 285 above 64 targets, else T + 9)
    rmse_atol: float = 0.0           # an absolute floor under the report's rmse bar (rtol 1e-5), with the row's reason

    @property
    def P(self):
        return len(self.pairs)

    @property
    def nbands(self):
        return self.B or (285 if self.T > 64 else self.T + 9)

    @property
    def f10(self):
        return self.factor or 3


R = Row
ROWS = [
    # (nb, degree) = (1, 1), (4, 1): na 16; narrow only (ldq 32), diag only (ldq 48 .. 96)
    R("n1d1_T16_u16u16_report", 1, 1, 16, 5, 7, 3, "uint16", "uint16", 4, ("narrow",), ("ok", "empty", "ok"), s2_nd=0.0,
      report=True),
    R("n4d1_T40_f32f32_nd", 4, 1, 40, 9, 4, 2, "float32", "float32", 4, ("diag",), emit_nd=-9999.0, s2_nd=-1.0),
    R("n4d1_T80_tiny1x1", 4, 1, 80, 1, 1, 6, "uint16", "float32", 5, ("diag",)),
    R("n4d1_T33_tiny2x3", 4, 1, 33, 2, 3, 2, "float32", "uint16", 4, ("diag",), s2_nd=0.0),
    # (4, 3): nf 34, na 48, npad 64
    # 6 training pixels for 34 features: rmse ~4e-3 over 6 residuals, where one float32 ulp of a sigmoid (6e-8) that the
    # oracle's and the device's models round differently moves rmse by 1e-5 relative
    R("n4d3_T33_tiny_report", 4, 3, 33, 2, 3, 6, "uint16", "uint16", 4, ("diag",), report=True, rmse_atol=1e-7),
    R("n4d3_T24_P5", 4, 3, 24, 13, 11, 2, "uint16", "float32", 4, ("diag",), ("ok", "empty", "few", "const", "ok"),
      s2_nd=-1.0, report=True),
    # (10, 2): nf 65, na 80, npad 96
    R("n10d2_T32_rect_P3", 10, 2, 32, 37, 23, 2, "uint16", "float32", 4, ("diag", "narrow"), ("ok", "few", "empty")),
    R("n10d2_T100", 10, 2, 100, 11, 13, 3, "float32", "uint16", 5, ("wide", "diag"), ("ok", "const"), emit_nd=-9999.0,
      s2_nd=0.0, report=True),
    R("n10d2_T32_many_chunks_f1", 10, 2, 32, 100, 205, 1, "uint16", "uint16", 4, ("diag", "narrow"), s2_nd=0.0),
    # (16, 2): nf 152, na 160, npad 160
    R("n16d2_T200_report", 16, 2, 200, 8, 10, 4, "float32", "float32", 6, ("wide", "diag"), ("ok", "ok"), report=True),
    R("n16d2_T285_all", 16, 2, 285, 7, 6, 5, "uint16", "uint16", 6, ("wide", "diag"), ("ok", "few"), s2_nd=0.0),
    R("n16d2_T129", 16, 2, 129, 6, 5, 2, "uint16", "float32", 6, ("wide", "diag", "narrow")),
    # (10, 3): nf 285, na 288, npad 288 - the notebook's; every MFMA predict kernel
    R("n10d3_T1_x16_big_report", 10, 3, 1, 37, 29, 6, "uint16", "uint16", 0, ("wide", "diag", "narrow"), s2_nd=0.0,
      report=True),
    R("n10d3_T16_x16_report", 10, 3, 16, 12, 17, 3, "float32", "uint16", 0, ("wide", "diag", "narrow"), ("ok", "const", "ok"),
      emit_nd=-9999.0, report=True),
    R("n10d3_T17_slice1_report", 10, 3, 17, 10, 10, 6, "uint16", "uint16", 1, ("wide", "diag", "narrow"), ("ok", "ok"),
      s2_nd=0.0, report=True),
    R("n10d3_T33_slice2_report", 10, 3, 33, 9, 14, 2, "uint16", "float32", 2, ("wide", "diag"), report=True),
    R("n10d3_T40_slice2_index_array", 10, 3, 40, 15, 9, 3, "float32", "float32", 2, ("wide", "diag"), ("ok", "ok"),
      s2_nd=-1.0, bands=tuple(int(v) for v in (np.arange(40) * 37 + 11) % 80) + (), B=80),
    R("n10d3_T70_slice3", 10, 3, 70, 11, 12, 3, "uint16", "uint16", 3, ("wide", "diag")),
    R("n10d3_T128_slice2_two", 10, 3, 128, 9, 9, 6, "uint16", "float32", 2, ("wide", "diag", "narrow"), ("ok", "ok")),
    # the "few" pair: 95 training pixels for 285 features leave rmse ~2e-3, where a float32 ulp of a sigmoid is 1e-5 of it
    R("n10d3_T285_slice3_three_report", 10, 3, 285, 12, 13, 3, "uint16", "uint16", 3, ("wide", "diag"),
      ("ok", "empty", "few"), s2_nd=0.0, report=True, rmse_atol=1e-7),
    R("n10d3_T32_coarse", 10, 3, 32, 9, 14, 0, "uint16", "float32", 1, ("wide", "diag", "narrow"), ("ok", "ok"), s2_nd=-1.0),
    # (11, 3): nf 363, na 368, npad 384 - chol_factor_kernel, block inverses in LDS
    R("n11d3_T32_report", 11, 3, 32, 21, 22, 2, "uint16", "uint16", 4, ("wide", "diag", "narrow"), ("ok", "ok"), s2_nd=0.0,
      report=True),
    # (12, 3): nf 454, na 464, npad 480 (the largest accepted) - block inverses in global memory, ragged diagonal blocks
    R("n12d3_T16", 12, 3, 16, 23, 25, 2, "float32", "uint16", 4, ("wide", "diag"), ("ok", "few")),
    R("n12d3_T96_report", 12, 3, 96, 22, 25, 2, "uint16", "float32", 5, ("wide", "diag"), s2_nd=-1.0, report=True),
    # status 2: alpha = 0 and one pair whose pixels all carry one S2 vector
    R("n4d2_T20_alpha0_status2", 4, 2, 20, 6, 9, 2, "uint16", "uint16", 4, ("diag",), ("ok", "same"), alpha=0.0, report=True),
]


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def _sig(z):
    return 1.0 / (1.0 + np.exp(-z))


@lru_cache(maxsize=None)
def make_inputs(row: Row):
    """(emits (P, B, h, w), s2s (P, nb, h f, w f), s2_coarse (P, nb, h, w) or None) of a row, from its own seed."""
    rng = np.random.default_rng(zlib.crc32(row.id.encode()))
    P, nb, h, w, f, B = row.P, row.nb, row.h, row.w, row.f10, row.nbands
    npix = h * w
    emits, s2s, coarses = [], [], []
    for kind in row.pairs:
        refl = 0.05 + 0.4 * rng.random((nb, h, w))
        if kind == "const":
            refl[0] = 0.1234
        if kind == "same":
            refl[:] = (0.05 + 0.4 * rng.random(nb))[:, None, None]
        fine = np.repeat(np.repeat(refl, f, axis=1), f, axis=2)
        dither = rng.integers(-4, 5, fine.shape) * 1e-4
        if kind in ("const", "same"):
            dither[0 if kind == "const" else slice(None)] = 0.0
        fine = fine + dither
        if row.sdt == "uint16":
            s2 = np.clip(np.round(fine * 1e4), 1, 10000).astype(np.uint16)
            s2f = s2.astype(np.float32)
        else:
            s2 = fine.astype(np.float32)
            s2f = s2
        # the targets: smooth in the coarse S2 (standardised), logits in [-3, 3]
        xc = onp.block_mean(s2f, f).astype(np.float64).reshape(nb, -1)
        z = (xc - xc.mean(axis=1, keepdims=True)) / (xc.std(axis=1, keepdims=True) + 1e-3)
        wz = rng.standard_normal((B, nb)) / np.sqrt(nb)
        lg = (0.5 + 1.5 * rng.random((B, 1))) * np.tanh(wz @ z + 0.3 * np.roll(z, 1, axis=0)[:1] * z[:1]) \
            + rng.uniform(-0.8, 0.8, (B, 1)) + 0.03 * rng.standard_normal((B, npix))
        y = _sig(np.clip(lg, -3.0, 3.0)).reshape(B, h, w)
        if row.edt == "uint16":
            emit = np.clip(np.round(y * 1e4), 1, 65534).astype(np.uint16)
        else:
            emit = y.astype(np.float32)
        bad_e = 65535 if row.edt == "uint16" else np.float32(np.nan)
        if kind == "empty":
            emit[:] = bad_e
        elif kind == "few":
            keep = rng.choice(npix, size=max(1, min(npix - 1, n_features(nb, row.degree) // 3)), replace=False)
            drop = np.ones(npix, bool)
            drop[keep] = False
            emit.reshape(B, -1)[:, drop] = bad_e
        elif npix >= 16:                             # scattered bad samples: nodata / NaN in EMIT, nodata / NaN in S2
            k = max(1, npix // 40)
            emit[rng.integers(0, B, k), rng.integers(0, h, k), rng.integers(0, w, k)] = bad_e
            if row.emit_nd is not None:
                emit[rng.integers(0, B, k), rng.integers(0, h, k), rng.integers(0, w, k)] = row.emit_nd
            kf = max(1, s2.size // (nb * 400))
            idx = (rng.integers(0, nb, kf), rng.integers(0, h * f, kf), rng.integers(0, w * f, kf))
            if row.s2_nd is not None:
                s2[idx] = row.s2_nd
            elif row.sdt == "float32":
                s2[idx] = np.nan
            if row.sdt == "float32":
                s2[rng.integers(0, nb), rng.integers(0, h * f), rng.integers(0, w * f)] = np.inf
        emits.append(emit)
        s2s.append(s2)
        if row.factor == 0:                          # the caller's S2 on the EMIT grid: a block mean with its own NaNs
            c = onp.block_mean(s2.astype(np.float32), f)
            if npix >= 16 and kind == "ok":
                c[rng.integers(0, nb, 3), rng.integers(0, h, 3), rng.integers(0, w, 3)] = np.nan
            coarses.append(c.astype(np.float32))
    return np.stack(emits), np.stack(s2s), (np.stack(coarses) if row.factor == 0 else None)


def _kwargs(row):
    bands = np.array(row.bands) if row.bands is not None else ("all" if row.T == 285 and row.nbands == 285 else row.T)
    return dict(bands=bands, degree=row.degree, alpha=row.alpha, factor=row.f10, emit_nodata=row.emit_nd, s2_nodata=row.s2_nd,
                report=row.report)


def run_row(row, torch, pairs=None):
    """fuse_tile_pairs of the row's batch (device inputs), or fuse_tile_pair of one of its pairs."""
    import s2_emit
    emits, s2s, coarse = make_inputs(row)

    def dev(a):
        if a.dtype == np.uint16:
            return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    kw = _kwargs(row)
    if pairs is None:
        return s2_emit.fuse_tile_pairs(dev(emits), dev(s2s), s2_coarse=None if coarse is None else dev(coarse), **kw)
    i = pairs
    return s2_emit.fuse_tile_pair(dev(emits[i]), dev(s2s[i]), s2_coarse=None if coarse is None else dev(coarse[i]), **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
def prep_reference(row, emit, s2, coarse, bands):
    """(X (nb, h, w) float32 on the EMIT grid, Y (T, h, w) decoded float32 targets, mask (h, w)) by the flatten rule."""
    if coarse is not None:
        X = coarse
    else:
        s2f = s2.astype(np.float32)
        f = row.f10
        X = onp.block_mean(s2f, f)
        blocks = s2f.reshape(row.nb, row.h, f, row.w, f)
        bad = ~np.isfinite(blocks).all(axis=(2, 4))
        if row.s2_nd is not None:
            bad |= (blocks == np.float32(row.s2_nd)).any(axis=(2, 4))
        X = np.where(bad, np.float32(np.nan), X)
    Y = onp.tile_decode_u16(emit) if row.edt == "uint16" else emit
    Y = Y[bands]
    mask = np.isfinite(X).all(0) & np.isfinite(Y).all(0)
    if row.s2_nd is not None:
        mask &= ~(X == np.float32(row.s2_nd)).any(0)
    if row.emit_nd is not None:
        mask &= ~(Y == np.float32(row.emit_nd)).any(0)
    return X, Y, mask


def model_dict(m, degree):
    return dict(mean=m.mean_, scale=m.scale_, coef=m.coef_, intercept=m.intercept_, degree=degree)


def _bits(t):
    import torch
    t = t.contiguous()
    width = {8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()]
    return t.view(-1).view(width).cpu().numpy()


def pair_digest(out, i):
    """The bits of everything pair i of an output carries."""
    parts = [out.cube[i], out.n_train[i:i + 1], out.status[i:i + 1], out.mask[i], out.s2_coarse[i]]
    parts += [out._fit[k][i] for k in ("mean", "scale", "b64", "W32", "b32", "mean32", "inv32")]
    if out.r2 is not None:
        parts += [out.r2[i], out.rmse[i]]
    return [_bits(p).tobytes() for p in parts]


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
def test_rows_are_distinct_and_keep_the_10m_image_small():
    assert len({r.id for r in ROWS}) == len(ROWS)
    for r in ROWS:
        assert r.h * r.w * r.f10 ** 2 <= 41_000 or r.factor == 1, r.id
        nf, na, ldq, npad = sizes(r.nb, r.degree, r.T)
        assert nf <= 512 and gram_kinds(na, ldq) == frozenset(r.gram), (r.id, sorted(gram_kinds(na, ldq)))


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_row(torch_gpu, row):
    torch = torch_gpu
    from s2_emit import _native as nat
    lib = nat.load()
    nf, na, ldq, npad = sizes(row.nb, row.degree, row.T)
    emits, s2s, coarse = make_inputs(row)
    out = run_row(row, torch)
    torch.cuda.synchronize()
    # selection: the query after the call's own prepare names the row's predict slot
    assert lib.hsr_polyfeat_predict_kernel(row.nb, row.degree, row.T, -1) == row.slot
    assert lib.hsr_polyfeat_count(row.nb, row.degree) == nf
    T, P = row.T, row.P
    bands = out.bands
    assert len(bands) == T and out.cube.shape == (P, T, row.h * row.f10, row.w * row.f10)
    expect_status = [{"empty": 1, "same": 2 if row.alpha == 0.0 else 0}.get(k, 0) for k in row.pairs]
    np.testing.assert_array_equal(out.status.cpu().numpy(), expect_status)
    n_train = out.n_train.cpu().numpy()
    mask_d = out.mask.cpu().numpy()
    xc_d = out.s2_coarse.cpu().numpy()
    cube = out.cube.cpu().numpy()
    r2 = out.r2.cpu().numpy() if row.report else None
    rmse = out.rmse.cpu().numpy() if row.report else None
    for i, kind in enumerate(row.pairs):
        X, Y, mask = prep_reference(row, emits[i], s2s[i], None if coarse is None else coarse[i], bands)
        # prep
        np.testing.assert_array_equal(mask_d[i], mask, err_msg=f"pair {i}")
        assert n_train[i] == mask.sum(), i
        np.testing.assert_array_equal(np.isnan(xc_d[i]), np.isnan(X))
        fin = ~np.isnan(X)
        np.testing.assert_array_equal(xc_d[i][fin].view(np.int32), X[fin].view(np.int32))
        if kind == "empty":
            assert n_train[i] == 0
        if kind == "few":
            assert 1 <= n_train[i] < nf
        m = out.model(i)
        Xtr = X.reshape(row.nb, -1).T[mask.reshape(-1)]
        Ytr = Y.reshape(T, -1).T[mask.reshape(-1)]
        X10 = s2s[i].astype(np.float32)
        if expect_status[i] != 0:
            assert np.isnan(m.intercept_).all() and np.isnan(cube[i]).all(), i
            if row.report:
                assert np.isnan(r2[i]).all() and np.isnan(rmse[i]).all(), i
            continue
        # fit
        ref = onp.ridge_poly_fit(Xtr, onp.logit(Ytr.astype(np.float64)), degree=row.degree, alpha=row.alpha)
        np.testing.assert_allclose(m.mean_, ref["mean"], rtol=1e-12)
        np.testing.assert_allclose(m.scale_, ref["scale"], rtol=1e-12)
        if kind == "const":
            assert m.scale_[0] == 1.0
        dm = model_dict(m, row.degree)
        np.testing.assert_allclose(onp.ridge_poly_predict(dm, Xtr), onp.ridge_poly_predict(ref, Xtr), rtol=0, atol=1e-6,
                                   err_msg=f"pair {i}")
        # cube: the device's own float64 model on the 10 m input
        cref = onp.predict_cube_logit(dm, X10, nodata=row.s2_nd)
        np.testing.assert_array_equal(np.isnan(cube[i]), np.isnan(cref), err_msg=f"pair {i}")
        ok = ~np.isnan(cref)
        assert ok.any()
        assert np.abs(cube[i][ok] - cref[ok]).max() <= 1e-4, (i, np.abs(cube[i][ok] - cref[ok]).max())
        # report: against the oracle's model
        if row.report:
            rr2, rrmse = report_reference(Xtr, Ytr, ref["mean"], ref["scale"], ref["coef"], ref["intercept"], row.degree)
            assert np.abs(r2[i] - rr2).max() <= 1e-5, np.abs(r2[i] - rr2).max()
            assert (np.abs(rmse[i] - rrmse) <= 1e-5 * np.abs(rrmse) + row.rmse_atol).all(), np.abs(rmse[i] / rrmse - 1).max()
    # bits: every pair as it comes alone
    for i in range(P):
        one = run_row(row, torch, pairs=i)
        assert pair_digest(one, 0) == pair_digest(out, i), i


def test_rows_keep_their_bits_after_other_monomial_tables(torch_gpu):
    """hsr_polyfeat_prepare swaps one process-wide monomial table: every row run after rows of other (nb, degree) - in table
    order, then in reverse - gives the bits it gave before."""
    torch = torch_gpu

    def digests(order):
        d = {}
        for row in order:
            out = run_row(row, torch)
            d[row.id] = [pair_digest(out, i) for i in range(row.P)]
        torch.cuda.synchronize()
        return d

    first = digests(ROWS)
    again = digests(ROWS[::-1])
    for row in ROWS:
        assert again[row.id] == first[row.id], row.id


def test_table_reaches_every_instance():
    """Every predict slot, both Cholesky factor kernels, both forms of the solve and every Gram block kind run batched; the
    rows hold every value the table must contain."""
    slots, chol, dinv, kinds = set(), set(), set(), set()
    for r in ROWS:
        nf, na, ldq, npad = sizes(r.nb, r.degree, r.T)
        slots.add(r.slot)
        c, d = chol_instances(npad)
        chol.add(c)
        dinv.add(d)
        kinds |= gram_kinds(na, ldq)
    assert slots == set(range(7)) and chol == {"res", "factor"} and dinv == {True, False}
    assert kinds == {"wide", "diag", "narrow"}
    shapes = {(r.nb, r.degree) for r in ROWS}
    assert {(1, 1), (4, 1), (4, 3), (10, 2), (16, 2), (10, 3), (11, 3), (12, 3)} <= shapes
    assert {r.factor for r in ROWS} >= {0, 1, 2, 3, 6}
    assert {(r.edt, r.sdt) for r in ROWS} == {(e, s) for e in ("uint16", "float32") for s in ("uint16", "float32")}
    assert {r.emit_nd is None for r in ROWS} == {True, False} and {r.s2_nd is None for r in ROWS} == {True, False}
    assert {r.P for r in ROWS} >= {1, 3, 5}
    kinds_p = {k for r in ROWS for k in r.pairs}
    assert kinds_p == {"ok", "empty", "few", "const", "same"} and any(r.alpha == 0 and "same" in r.pairs for r in ROWS)
    assert {1, 16, 17, 33, 285} <= {r.T for r in ROWS if r.report}
    report_na = {sizes(r.nb, r.degree, r.T)[1] for r in ROWS if r.report}
    assert min(report_na) < 96 < max(report_na)
    assert any(r.h != r.w and r.h * r.w > 1 for r in ROWS) and {(1, 1), (2, 3)} <= {(r.h, r.w) for r in ROWS}
    assert any(r.h * r.w > 1024 and (r.h * r.w) % 8 for r in ROWS)
    t103 = {r.T for r in ROWS if (r.nb, r.degree) == (10, 3)}
    assert {1, 16, 17, 40, 128, 70, 285} <= t103
    tgen = {r.T for r in ROWS if (r.nb, r.degree) != (10, 3)}
    assert min(tgen) <= 64 and any(64 < t <= 128 for t in tgen) and any(128 < t <= 256 for t in tgen) and 285 in tgen


# ---------------------------------------------------------------------------------------------------------------------------
# batched building blocks on exact data
# ---------------------------------------------------------------------------------------------------------------------------
def _gram_shapes():
    s = {sizes(r.nb, r.degree, r.T)[1:3] for r in ROWS}
    return sorted(s | {(16, 32), (16, 48), (16, 96), (80, 112), (288, 320), (288, 576), (464, 480)})


@pytest.mark.parametrize("na,ldq", _gram_shapes())
def test_gram_batched_exact(torch_gpu, na, ldq):
    """hsr_gram_f64_batched at every (na, ldq) of the table: small-integer data, distinct per pair, so that float64 is exact -
    C of every pair equals A[:, :na]^T A, and the rows of C between the pairs are untouched."""
    torch = torch_gpu
    from s2_emit import _native as nat
    from s2_emit._engine import _ptr, _stream
    lib = nat.load()
    rng = np.random.default_rng(na * 1000 + ldq)
    P, gap = 3, 3
    for n in sorted({1, 7, 25, 4099, 1073}):
        A = rng.integers(-3, 4, (P, n, ldq)).astype(np.float64)
        A[1] += 1.0                                                      # pairs differ in more than their noise
        Ad = torch.from_numpy(A).cuda()
        wq = lib.hsr_gram_work_bytes(na, ldq, n) // 8
        work = torch.full((P, wq), np.nan, dtype=torch.float64, device="cuda")
        Cd = torch.full((P, na + gap, ldq), -7.0, dtype=torch.float64, device="cuda")
        nat.check(lib.hsr_gram_f64_batched(_ptr(Ad), ldq, na, ldq, n, n * ldq, _ptr(work), wq, _ptr(Cd), ldq, (na + gap) * ldq, P,
                                           _stream(torch)), "hsr_gram_f64_batched")
        C = Cd.cpu().numpy()
        for p in range(P):
            np.testing.assert_array_equal(C[p, :na], A[p][:, :na].T @ A[p], err_msg=f"n={n} pair {p}")
            assert (C[p, na:] == -7.0).all(), (n, p)


CHOL_NPAD = (32, 96, 288, 320, 384, 416, 480, 512)


@pytest.mark.parametrize("npad", CHOL_NPAD)
def test_chol_solve_batched(torch_gpu, npad):
    """hsr_chol_solve_f64_batched of three systems: the SPD pairs against numpy.linalg (the tolerances of
    test_chol_solve_vs_numpy) and bit-equal to their single-system solve; pair 1 is not positive definite - its info is the
    first bad pivot (LAPACK's, 1-based), and the other pairs are unchanged.  The elements between the pairs stay untouched."""
    torch = torch_gpu
    from s2_emit import _native as nat
    from s2_emit._engine import _ptr, _stream
    lib = nat.load()
    rng = np.random.default_rng(npad)
    P, bad_pair = 3, 1
    k = {32: 5, 96: 40, 288: 287, 320: 300, 384: 33, 416: 400, 480: 129, 512: 511}[npad]   # 0-based bad pivot
    mats = []
    for p in range(P):
        M = rng.standard_normal((npad, npad + 40))
        A = M @ M.T / npad + 0.5 * np.eye(npad)
        if p == bad_pair:
            L = np.linalg.cholesky(A)
            A[k, k] -= L[k, k] ** 2 + 1.0                                 # Schur pivot k becomes -1
            np.linalg.cholesky(A[:k, :k]) if k else None
            with pytest.raises(np.linalg.LinAlgError):
                np.linalg.cholesky(A[:k + 1, :k + 1])
        mats.append(A)
    cw = lib.hsr_chol_work_bytes(npad) // 8
    for T in (1, 17, 285):
        Bs = [rng.standard_normal((npad, T)) for _ in range(P)]
        pa, pb = npad * npad + 40, npad * T + 24                          # pair strides with a guard behind each pair
        Abuf = np.full(P * pa, -3.0)
        Bbuf = np.full(P * pb, -3.0)
        for p in range(P):
            Abuf[p * pa:p * pa + npad * npad] = mats[p].reshape(-1)
            Bbuf[p * pb:p * pb + npad * T] = Bs[p].reshape(-1)
        Ad, Bd = torch.from_numpy(Abuf).cuda(), torch.from_numpy(Bbuf).cuda()
        work = torch.empty(P * cw, dtype=torch.float64, device="cuda")
        info = torch.full((P,), -5, dtype=torch.int32, device="cuda")
        nat.check(lib.hsr_chol_solve_f64_batched(_ptr(Ad), npad, npad, pa, _ptr(Bd), T, T, pb, _ptr(work), _ptr(info), P,
                                                 _stream(torch)), "hsr_chol_solve_f64_batched")
        Ag, Bg, inf = Ad.cpu().numpy(), Bd.cpu().numpy(), info.cpu().numpy()
        assert list(inf) == [k + 1 if p == bad_pair else 0 for p in range(P)], (T, list(inf))
        for p in range(P):
            assert (Ag[p * pa + npad * npad:(p + 1) * pa] == -3.0).all() and (Bg[p * pb + npad * T:(p + 1) * pb] == -3.0).all()
            if p == bad_pair:
                continue
            X = Bg[p * pb:p * pb + npad * T].reshape(npad, T)
            np.testing.assert_allclose(X, np.linalg.solve(mats[p], Bs[p]), rtol=1e-9, atol=1e-11, err_msg=f"T={T} pair {p}")
            Lg = np.tril(Ag[p * pa:p * pa + npad * npad].reshape(npad, npad))
            np.testing.assert_allclose(Lg, np.linalg.cholesky(mats[p]), rtol=1e-10, atol=1e-12)
            # the same bits as the system solved alone
            A1, B1 = torch.from_numpy(mats[p].copy()).cuda(), torch.from_numpy(Bs[p].copy()).cuda()
            w1 = torch.empty(cw, dtype=torch.float64, device="cuda")
            i1 = torch.full((1,), -5, dtype=torch.int32, device="cuda")
            nat.check(lib.hsr_chol_solve_f64(_ptr(A1), npad, npad, _ptr(B1), T, T, _ptr(w1), _ptr(i1), _stream(torch)))
            assert int(i1.item()) == 0
            assert (B1.cpu().numpy().view(np.int64) == X.view(np.int64)).all(), (T, p)
