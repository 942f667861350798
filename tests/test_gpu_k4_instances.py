"""Every kernel instance and every entry point of the polynomial-ridge family K4 (csrc/hsr_ridge.hip, csrc/hsr_gram.hip,
csrc/hsr_chol.hip) against float64 / longdouble NumPy references.

One case table per family.  The entry points are called through ctypes, so that pointers can be offset and leading
dimensions padded: every output - work buffers at exactly their *_work_bytes included - is a `Buf` of gpu_harness
(sentinel fill between two 256-byte guard zones), and every byte a call does not own (guards, pad columns, stride gaps) must
come back untouched.  After every call the launch record (hsr_k4_last_launch) must show the kernels the row names; the last test
checks that the rows together reached every name hsr_k4_instance_name enumerates.  Inputs come from seeded generators; gaps of
inputs hold NaN.  References and bars:
  * stats: integer data (every sum exact) bit-equal to the kernel's formulas in float64 NumPy; reflectance-like data at the
    project's rtol 1e-12 against longdouble; an outlier first sample against the derived bound on M2 of the shifted-data form;
  * expand: bit-equal to ((z_a z_b) z_c) in float64 (the library is built without contraction); the pair form's logit
    within 2 ulp of np.log;
  * Gram: elementwise |C - C_ref| <= 2 n 2^-53 (|A|^T |B|) with C_ref in longdouble; integers up to 2^20 bit-equal to A.T @ B
    (exact in float64, not in float32);
  * assemble / finish: the formulas of the kernels' comments in float64 NumPy, bit-equal;
  * Cholesky: the project's bars against numpy.linalg on the well-conditioned class, and LAPACK's normwise test ratios in
    longdouble <= 1 on both classes; the strict upper triangle holds NaN, and the elements include/hsr.h calls unwritten are
    compared byte for byte;
  * predict: the oracle's model (oracle_np.ridge_poly_fit) at the project's bars (logit 2e-4, reflectance 1e-4), and every
    input layout bit-equal to the aligned pixel-major call.
"""
import ctypes as C
from itertools import combinations_with_replacement

import numpy as np
import pytest

from oracle import oracle_np as onp
from conftest import load_golden
from gpu_harness import FILL, Buf, LaunchLog, bits_equal, same_bits, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from gpu_harness import lib as _lib, stream as _stream
from test_gpu_tile_pairs_shapes import ROWS, chol_instances, gram_kinds, sizes

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

LOG = LaunchLog("hsr_k4_last_launch")   # its checked calls take the record as the library joins it: "first; second"
_call = LOG.call
LD = np.longdouble
U53, U52 = 2.0 ** -53, 2.0 ** -52
WORST = {}                       # family -> largest observed error / bar (printed by the last test)


def _note(family, value):
    WORST[family] = max(WORST.get(family, 0.0), float(value))


class Mat:
    """(rows, cols) elements of `dtype` in rows of `ld`, `off` bytes past a 256-byte boundary.  An output (gap None): the gaps
    hold the sentinel and get() checks that they still do; an input: the gaps hold `gap` (NaN: a read of them poisons the result)."""

    def __init__(self, torch, rows, cols, ld, dtype, off=0, data=None, gap=None):
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, np.dtype(dtype)
        host = np.full(rows * ld * self.dtype.itemsize, FILL, np.uint8).view(self.dtype).reshape(rows, ld)
        if gap is not None:
            host[:] = gap
        if data is not None:
            host[:, :cols] = data
        self.buf = Buf(torch, host.nbytes, off, host)

    @property
    def ptr(self):
        return self.buf.ptr

    def get(self):
        h = self.buf.get(self.dtype).reshape(self.rows, self.ld)
        assert (np.ascontiguousarray(h[:, self.cols:]).view(np.uint8) == FILL).all(), "write into a stride gap"
        return h[:, :self.cols].copy()


def _vec(torch, data, off=0):
    data = np.ascontiguousarray(data)
    return Buf(torch, data.nbytes, off, data)


def _out(torch, count, dtype, off=0):
    return Buf(torch, count * np.dtype(dtype).itemsize, off)


def _x_layout(torch, X, layout):
    """(buffer, x_rs, x_cs) of the float32 rows X (n, n_in): 'rows' (padded pitch), 'bands' (band-major planes with a padded
    plane stride), 'off4' (rows, base 4 bytes past the alignment)."""
    n, n_in = X.shape
    if layout == "bands":
        m = Mat(torch, n_in, n, n + 3, np.float32, data=X.T, gap=np.nan)
        return m, 1, n + 3
    m = Mat(torch, n, n_in, n_in + 3, np.float32, off=4 if layout == "off4" else 0, data=X, gap=np.nan)
    return m, n_in + 3, 1


LAYOUTS = ("rows", "bands", "off4")


# =============================================================================================================================
# hsr_ridge_stats
# =============================================================================================================================
def _stats_run(torch, X, layout, off=0):
    lib = _lib()
    n, n_in = X.shape
    xb, rs, cs = _x_layout(torch, X, layout)
    work = _out(torch, lib.hsr_ridge_stats_work_bytes(n_in) // 8, np.float64)
    stats, mean, scale = (_out(torch, k, np.float64, off) for k in (1 + 2 * n_in, n_in, n_in))
    _call("ridge_stats_partial_kernel; ridge_stats_finish_kernel", lib.hsr_ridge_stats, xb.ptr, rs, cs, n, n_in, work.ptr,
          stats.ptr, mean.ptr, scale.ptr, _stream(torch))
    work.get(np.float64)
    return stats.get(np.float64), mean.get(np.float64), scale.get(np.float64)


STATS_N = (1, 2, 255, 1023, 1024, 1025)
STATS_BIG = ((65537, 3), (131073, 1))        # more than one pass of a thread over its block's rows (n > 65 536)


def _stats_cases():
    for n in STATS_N:
        for n_in in (1, 3, 10, 16):
            for layout in LAYOUTS:
                yield n, n_in, layout
    for i, (n, n_in) in enumerate(STATS_BIG):
        for layout in LAYOUTS:
            yield n, n_in, layout


def test_stats_exact_integers(torch_gpu):
    """Float32 integers within 1024 of the first sample: every sum is exact, so stats / mean / scale carry the bits of the
    kernel's formulas in float64 NumPy.  The last column (n_in >= 3) is constant: M2 exactly 0, scale 1."""
    rng = np.random.default_rng(41)
    for k, (n, n_in, layout) in enumerate(_stats_cases()):
        X = (3000 + rng.integers(-512, 513, (n, n_in))).astype(np.float32)
        if n_in >= 3 or (n_in == 1 and n == 255):
            X[:, -1] = 777.0
        stats, mean, scale = _stats_run(torch_gpu, X, layout, off=8 * (k % 2))
        d = X.astype(np.float64) - X[0].astype(np.float64)
        assert np.abs(d).max() <= 1024
        s1, s2 = d.sum(axis=0), (d * d).sum(axis=0)
        assert (s1 == d.astype(np.int64).sum(axis=0)).all() and (s2 == (d.astype(np.int64) ** 2).sum(axis=0)).all()
        nn = np.float64(n)
        m_ref = X[0].astype(np.float64) + s1 / nn
        m2_ref = np.maximum(s2 - s1 * s1 / nn, 0.0)
        sc_ref = np.sqrt(m2_ref / nn)
        sc_ref[sc_ref == 0.0] = 1.0
        what = f"n={n} n_in={n_in} {layout}"
        same_bits(stats, np.concatenate([[nn], m_ref, m2_ref]), what + " stats")
        same_bits(mean, m_ref, what + " mean")
        same_bits(scale, sc_ref, what + " scale")
        if n_in >= 3:
            assert stats[2 * n_in] == 0.0 and scale[-1] == 1.0


def test_stats_real_data(torch_gpu):
    """Class A: reflectance x 10 000 as in the notebook (600 .. 4600): mean and scale at the project's rtol 1e-12 against
    longdouble.  Class B: the first sample - the shift K of the kernel's sums - lies about 100 sigma from the mean: M2 within
    8 n 2^-53 (1 + (x0 - mu)^2 / sigma^2) relative (sum d^2 and (sum d)^2 / n are each ~n (sigma^2 + (x0 - mu)^2) and carry a
    relative error of a few n 2^-53 at most; their difference is n sigma^2).  A constant real column gives M2 exactly 0."""
    rng = np.random.default_rng(42)
    cases = [(n, n_in, LAYOUTS[(i + j) % 3]) for i, n in enumerate((2, 255, 1025, 5003)) for j, n_in in enumerate((1, 3, 10, 16))]
    cases += [(n, n_in, LAYOUTS[i % 3]) for i, (n, n_in) in enumerate(STATS_BIG)]
    for n, n_in, layout in cases:
        X = (600 + 4000 * rng.random((n, n_in))).astype(np.float32)
        if n_in >= 3:
            X[:, 1] = np.float32(1234.5678)
        stats, mean, scale = _stats_run(torch_gpu, X, layout)
        xl = X.astype(LD)
        mu = xl.sum(axis=0) / n
        m2 = ((xl - mu) ** 2).sum(axis=0)
        sc = np.sqrt(m2 / n)
        sc[sc == 0] = 1
        what = f"A n={n} n_in={n_in} {layout}"
        _note("stats mean (rtol 1e-12)", np.max(np.abs((mean - mu) / mu)) / 1e-12)
        _note("stats scale (rtol 1e-12)", np.max(np.abs((scale - sc) / sc)) / 1e-12)
        np.testing.assert_allclose(mean, mu.astype(np.float64), rtol=1e-12, atol=0, err_msg=what)
        np.testing.assert_allclose(scale, sc.astype(np.float64), rtol=1e-12, atol=0, err_msg=what)
        if n_in >= 3:
            assert stats[1 + n_in + 1] == 0.0 and scale[1] == 1.0 and mean[1] == np.float64(np.float32(1234.5678))
    for n, n_in, layout in [(1025, 3, "rows"), (5003, 10, "bands"), (1025, 16, "off4"), (65537, 3, "bands"), (131073, 1, "rows")]:
        X = (2600 + 50 * rng.standard_normal((n, n_in))).astype(np.float32)
        X[0] = (2600 + 5000 * (1 + 0.1 * rng.random(n_in))).astype(np.float32)
        stats, mean, scale = _stats_run(torch_gpu, X, layout)
        xl = X.astype(LD)
        mu = xl.sum(axis=0) / n
        m2 = ((xl - mu) ** 2).sum(axis=0)
        bound = 8 * n * U53 * (1 + (xl[0] - mu) ** 2 / (m2 / n))
        err = np.abs(stats[1 + n_in:].astype(LD) - m2) / m2
        print(f"stats B n={n} n_in={n_in} {layout}: M2 rel err {float(err.max()):.3e}, bound {float(bound.min()):.3e}")
        _note("stats M2, outlier shift (derived bound)", np.max(err / bound))
        assert (err <= bound).all(), (n, n_in, layout, err, bound)
        np.testing.assert_allclose(mean, mu.astype(np.float64), rtol=1e-12, atol=0)


# =============================================================================================================================
# hsr_polyfeat_expand_f64 / hsr_pair_expand_f64
# =============================================================================================================================
def _table(n_in, degree):
    """The monomial index triples in sklearn's order, index n_in = the constant 1 (hsr_ridge.hip: build_table)."""
    return np.array([list(c) + [n_in] * (3 - d) for d in range(1, degree + 1)
                     for c in combinations_with_replacement(range(n_in), d)], dtype=np.int64)


def _monomials(X, mean, scale, n_in, degree):
    z = (X.astype(np.float64) - mean) / scale
    z1 = np.concatenate([z, np.ones((z.shape[0], 1))], axis=1)
    t = _table(n_in, degree)
    return (z1[:, t[:, 0]] * z1[:, t[:, 1]]) * z1[:, t[:, 2]]


def _prepare(n_in, degree):
    lib = _lib()
    assert lib.hsr_polyfeat_prepare(n_in, degree) == 0, lib.hsr_last_error()
    nf = lib.hsr_polyfeat_count(n_in, degree)
    assert nf == len(_table(n_in, degree))
    return nf


EXPAND_SHAPES = ((1, 1), (4, 3), (10, 2), (10, 3), (16, 2))


@pytest.mark.parametrize("n_in,degree", EXPAND_SHAPES)
def test_expand(torch_gpu, n_in, degree):
    """Monomial columns bit-equal to ((z_a z_b) z_c), z = (double(x) - mean) / scale; pad columns exactly 0; the gap behind
    ncols and the rows past n untouched - for ncols = nf + 1 and na, ldp = ncols and ncols + 5, three input layouts."""
    torch, lib = torch_gpu, _lib()
    nf = _prepare(n_in, degree)
    na = (nf + 1 + 15) // 16 * 16
    rng = np.random.default_rng(100 * n_in + degree)
    k = 0
    for n in (1, 31, 32, 33, 1000):
        X = (600 + 4000 * rng.random((n, n_in))).astype(np.float32)
        mean, scale = 2600 + 100 * rng.standard_normal(n_in), 900 + 300 * rng.random(n_in)
        ref = _monomials(X, mean, scale, n_in, degree)
        md, sd = _vec(torch, mean, 8), _vec(torch, scale)
        for layout in LAYOUTS:
            xb, rs, cs = _x_layout(torch, X, layout)
            for ncols in (nf + 1, na):
                for ldp in (ncols, ncols + 5):
                    k += 1
                    P = Mat(torch, n, ncols, ldp, np.float64, off=8 * (k % 2))
                    _call("expand_f64_kernel", lib.hsr_polyfeat_expand_f64, xb.ptr, rs, cs, md.ptr, sd.ptr, n, n_in, degree, P.ptr,
                          ldp, ncols, _stream(torch))
                    got = P.get()
                    what = f"n={n} {layout} ncols={ncols} ldp={ldp}"
                    assert (got[:, 0].view(np.uint64) == np.float64(1.0).view(np.uint64)).all(), what
                    same_bits(got[:, 1:nf + 1], ref, what)
                    assert (got[:, nf + 1:].view(np.uint64) == 0).all(), what + ": pad columns"


@pytest.mark.parametrize("n_in,degree,T", [(4, 3, 5), (10, 2, 17)])
def test_pair_expand(torch_gpu, n_in, degree, T):
    """Rows [1 | monomials | 0 | logit(y) | 0] of the masked-in pixels, all-zero rows (the constant column included) of the
    others; monomials bit-equal, the logit within 2 ulp of np.log(u / (1 - u)); P = 3 carries the bits of each pair alone."""
    torch, lib = torch_gpu, _lib()
    nf = _prepare(n_in, degree)
    na = (nf + 1 + 15) // 16 * 16
    ldq, eps = na + (T + 15) // 16 * 16, 1e-4
    rng = np.random.default_rng(7 * n_in + T)
    for npix in (1, 33, 1000):
        P = 3
        X = (600 + 4000 * rng.random((P, n_in, npix))).astype(np.float32)
        Y = rng.random((P, T, npix)).astype(np.float32)
        Y[:, 0, ::3], Y[:, -1, 1::5] = 0.0, 1.0                       # both clips
        mask = (rng.random((P, npix)) < 0.7).astype(np.uint8)
        mask[:, 0] = (1, 0, 1)
        mask[mask != 0] = rng.integers(1, 256, int((mask != 0).sum()))   # any non-zero byte counts
        mean, scale = 2600 + 100 * rng.standard_normal((P, n_in)), 900 + 300 * rng.random((P, n_in))
        px, py, pm, pms, pq = n_in * npix + 3, T * npix + 5, npix + 1, n_in + 2, npix * ldq + 7
        xb = Mat(torch, P, n_in * npix, px, np.float32, data=X.reshape(P, -1), gap=np.nan)
        yb = Mat(torch, P, T * npix, py, np.float32, data=Y.reshape(P, -1), gap=np.nan)
        mb = Mat(torch, P, npix, pm, np.uint8, off=1, data=mask, gap=1)
        md = Mat(torch, P, n_in, pms, np.float64, data=mean, gap=np.nan)
        sd = Mat(torch, P, n_in, pms, np.float64, data=scale, gap=np.nan)
        Q = Mat(torch, P, npix * ldq, pq, np.float64, off=8)
        _call("pair_expand_f64_kernel", lib.hsr_pair_expand_f64, xb.ptr, px, md.ptr, sd.ptr, pms, yb.ptr, py, mb.ptr, pm, npix, n_in,
              degree, T, eps, Q.ptr, ldq, pq, na, P, _stream(torch))
        got = Q.get().reshape(P, npix, ldq)
        for p in range(P):
            ok = mask[p] != 0
            what = f"npix={npix} pair {p}"
            assert (got[p][~ok].view(np.uint64) == 0).all(), what + ": masked-out rows"
            g = got[p][ok]
            assert (g[:, 0] == 1.0).all() and (g[:, nf + 1:na].view(np.uint64) == 0).all() and (g[:, na + T:].view(np.uint64) == 0).all()
            same_bits(g[:, 1:nf + 1], _monomials(X[p].T[ok], mean[p], scale[p], n_in, degree), what)
            u = np.clip(Y[p].T[ok].astype(np.float64), eps, 1 - eps)
            ref = np.log(u / (1 - u))
            ulp = np.abs(g[:, na:na + T] - ref) / np.spacing(np.abs(ref))
            _note("pair expand logit (2 ulp)", ulp.max() / 2 if ulp.size else 0)
            assert (ulp <= 2).all(), (what, ulp.max())
            # the pair alone, from its own offset pointers
            Q1 = Mat(torch, npix, ldq, ldq, np.float64)
            off = lambda b, stride, size: C.c_void_p(b.ptr.value + p * stride * size)
            _call("pair_expand_f64_kernel", lib.hsr_pair_expand_f64, off(xb, px, 4), 0, off(md, pms, 8), off(sd, pms, 8), 0,
                  off(yb, py, 4), 0, off(mb, pm, 1), 0, npix, n_in, degree, T, eps, Q1.ptr, ldq, 0, na, 1, _stream(torch))
            same_bits(Q1.get(), got[p], what + " alone")


# =============================================================================================================================
# hsr_gram_f64 / hsr_gram_f64_batched
# =============================================================================================================================
# (na, nb) -> (block kinds of the symmetric plan, of the two-matrix plan, row counts)
GRAM_SHAPES = {
    (16, 16): ("narrow", "narrow", (1, 7, 8, 9, 47, 48, 49, 239, 240, 241, 1025, 5003, 131073)),
    (16, 32): ("narrow", "narrow", (1, 9, 241)),
    (32, 48): ("diag", "wide", (7, 49, 1025)),
    (96, 96): ("diag", "wide", (8, 240, 5003)),
    (96, 128): ("diag+narrow", "wide+narrow", (47, 239, 1025)),
    (112, 160): ("wide+diag", "wide", (48, 241, 1025)),
    (288, 320): ("wide+diag+narrow", "wide+narrow", (1, 240, 1025)),
    (288, 576): ("wide+diag", "wide", (9, 241)),
}


def _gram_data(rng, n, nb, kind):
    if kind == "int":                                       # products up to 2^40, sums below 2^52: exact in float64 only
        m = int(min(2 ** 20, np.sqrt(2.0 ** 52 / n)))
        return rng.integers(-m, m + 1, (n, nb)).astype(np.float64)
    Q = rng.standard_normal((n, nb))
    if kind == "scaled":
        Q *= 10.0 ** rng.choice([-6, 0, 6], nb)
    return Q


def _gram_call(torch, expect, A, na, B, nb, n, same, ld_extra, off, ldc_extra=3):
    """One hsr_gram_f64 call; `same`: B is A's buffer (the symmetric form).  Returns C (na, nb)."""
    lib = _lib()
    lda, ldb = A.shape[1] + ld_extra, B.shape[1] + ld_extra
    Ad = Mat(torch, n, A.shape[1], lda, np.float64, off=off, data=A, gap=np.nan)
    Bd = Ad if same else Mat(torch, n, B.shape[1], ldb, np.float64, off=off, data=B, gap=np.nan)
    work = _out(torch, lib.hsr_gram_work_bytes(na, nb, n) // 8, np.float64)
    Cd = Mat(torch, na, nb, nb + ldc_extra, np.float64, off=8)
    _call(expect, lib.hsr_gram_f64, Ad.ptr, lda, na, Bd.ptr, ldb, nb, n, work.ptr, Cd.ptr, nb + ldc_extra, _stream(torch))
    work.get(np.float64)
    return Cd.get()


@pytest.mark.parametrize("na,nb", sorted(GRAM_SHAPES))
def test_gram(torch_gpu, na, nb):
    """Four call forms - two matrices, one matrix with itself, both with bases 8 bytes past the alignment (the pointer arm of
    dma_ok: the register-operand kernel) and with odd leading dimensions (the same kernel) - on standard normal data, on
    columns scaled by 1e-6 .. 1e6 and on integers up to 2^20."""
    torch = torch_gpu
    sym_kinds, full_kinds, ns = GRAM_SHAPES[(na, nb)]
    lds_sym, lds_full = (f"gram_f64_lds_kernel {k}; gram_reduce_kernel" for k in (sym_kinds, full_kinds))
    reg_sym, reg_full = (f"gram_f64_kernel {k}; gram_reduce_kernel" for k in ("sym", "full"))
    rng = np.random.default_rng(na * 1000 + nb)
    perm = rng.permutation(nb)
    for i, n in enumerate(ns):
        for kind in (("normal", "int") if i else ("normal", "scaled", "int")):
            Q = _gram_data(rng, n, nb, kind)
            A, B = np.ascontiguousarray(Q[:, :na]), np.ascontiguousarray(Q[:, perm])       # B: Q's columns, permuted
            if kind == "int":
                ref = A.T @ Q
                assert np.abs(ref).max() < 2.0 ** 53 and np.abs(Q).max() ** 2 >= min(2.0 ** 40, 2.0 ** 52 / n) / 4
                bound = None
            else:
                ref = A.astype(LD).T @ Q.astype(LD)
                bound = 2 * n * U53 * (np.abs(A).T @ np.abs(Q))
            forms = [("sym", lds_sym, True, 0, 0), ("two", lds_full, False, 0, 0), ("sym off8", reg_sym, True, 0, 8),
                     ("two off8", reg_full, False, 0, 8), ("sym odd ld", reg_sym, True, 1, 0), ("two odd ld", reg_full, False, 1, 0)]
            for name, expect, same, ld_extra, off in forms:
                if same:
                    got, want, bnd = _gram_call(torch, expect, Q, na, Q, nb, n, True, ld_extra, off), ref, bound
                else:
                    got = _gram_call(torch, expect, A, na, B, nb, n, False, ld_extra, off)
                    want, bnd = ref[:, perm], None if bound is None else bound[:, perm]
                what = f"({na}, {nb}) n={n} {kind} {name}"
                if bnd is None:
                    same_bits(got, want, what)
                else:
                    err = np.abs(got.astype(LD) - want)
                    _note("gram (2 n 2^-53 |A|^T |B|)", np.max(err / bnd))
                    assert (err <= bnd).all(), (what, float(np.max(err / bnd)))
                if same:
                    same_bits(got[:, :na], got[:, :na].T.copy(), what + ": symmetric square part")
    # the record's capacity: truncated, NUL-terminated, and cleared all the same
    lib = _lib()
    Q = _gram_data(rng, 9, nb, "normal")
    Ad, work, Cd = Mat(torch, 9, nb, nb, np.float64, data=Q), _out(torch, lib.hsr_gram_work_bytes(na, nb, 9) // 8, np.float64), \
        Mat(torch, na, nb, nb, np.float64)
    assert lib.hsr_gram_f64(Ad.ptr, nb, na, Ad.ptr, nb, nb, 9, work.ptr, Cd.ptr, nb, _stream(torch)) == 0
    buf = C.create_string_buffer(b"\x7f" * 63, 64)
    assert lib.hsr_k4_last_launch(buf, 25) == 1 and buf.raw[:25] == lds_sym.encode()[:24] + b"\0" and buf.raw[25] == 0x7f
    assert lib.hsr_k4_last_launch(buf, 64) == 0
    Cd.get()


@pytest.mark.parametrize("na,nb", sorted(GRAM_SHAPES))
def test_gram_batched(torch_gpu, na, nb):
    """hsr_gram_f64_batched at P = 1 and 4: every pair carries the bits of hsr_gram_f64 on that pair alone; the gaps between the
    pairs' results and the pairs' work areas stay untouched."""
    torch, lib = torch_gpu, _lib()
    sym_kinds, _, ns = GRAM_SHAPES[(na, nb)]
    expect = f"gram_f64_lds_kernel {sym_kinds}; gram_reduce_kernel"
    rng = np.random.default_rng(na * 1000 + nb + 1)
    for n in ns[-2:]:
        if n > 6000:
            continue
        for P in (1, 4):
            Q = rng.standard_normal((P, n, nb))
            lda, ldc = nb + 2, nb + 3
            pa, pc, pw = n * lda + 6, na * ldc + 5, lib.hsr_gram_work_bytes(na, nb, n) // 8
            rows = np.full((P, n, lda), np.nan)
            rows[:, :, :nb] = Q
            Ad = Mat(torch, P, n * lda, pa, np.float64, data=rows.reshape(P, -1), gap=np.nan)
            work = _out(torch, P * pw, np.float64)
            Cd = Mat(torch, P, na * ldc, pc, np.float64, off=8)
            _call(expect, lib.hsr_gram_f64_batched, Ad.ptr, lda, na, nb, n, pa, work.ptr, pw, Cd.ptr, ldc, pc, P, _stream(torch))
            work.get(np.float64)
            got = Cd.get().reshape(P, na, ldc)
            assert (np.ascontiguousarray(got[:, :, nb:]).view(np.uint8) == FILL).all()
            for p in range(P):
                same_bits(got[p][:, :nb], _gram_call(torch, expect, Q[p], na, Q[p], nb, n, True, 2, 0), f"n={n} P={P} pair {p}")


@pytest.mark.parametrize("shape", sorted({(r.nb, r.degree, r.T) for r in ROWS}))
def test_selection_mirrors(torch_gpu, shape):
    """For every (nb, degree, T) of the tile-pair table: the kernels one batched Gram and one batched Cholesky call of that shape
    launch are what the mirrors gram_kinds / chol_instances of test_gpu_tile_pairs_shapes predict - so that a change of the C
    rule cannot drift together with its mirror."""
    torch, lib = torch_gpu, _lib()
    nf, na, ldq, npad = sizes(*shape)
    kinds = gram_kinds(na, ldq)
    want = "gram_f64_lds_kernel " + "+".join(k for k in ("wide", "diag", "narrow") if k in kinds) + "; gram_reduce_kernel"
    P, n = 2, 40
    rng = np.random.default_rng(nf)
    Ad = _vec(torch, rng.standard_normal((P, n, ldq)))
    pw = lib.hsr_gram_work_bytes(na, ldq, n) // 8
    work, Cd = _out(torch, P * pw, np.float64), _out(torch, P * na * ldq, np.float64)
    _call(want, lib.hsr_gram_f64_batched, Ad.ptr, ldq, na, ldq, n, n * ldq, work.ptr, pw, Cd.ptr, ldq, na * ldq, P, _stream(torch))
    work.get(np.float64), Cd.get(np.float64)
    factor, in_lds = chol_instances(npad)
    want = {"res": "chol_factor_res_kernel", "factor": "chol_factor_kernel"}[factor] + "; chol_solve_kernel " + ("lds" if in_lds else "global")
    A = np.broadcast_to(4.0 * np.eye(npad), (P, npad, npad))
    Ad, Bd = _vec(torch, A), _vec(torch, np.ones((P, npad, 3)))
    cw, info = _out(torch, P * lib.hsr_chol_work_bytes(npad) // 8, np.float64), _out(torch, P, np.int32)
    _call(want, lib.hsr_chol_solve_f64_batched, Ad.ptr, npad, npad, npad * npad, Bd.ptr, 3, 3, npad * 3, cw.ptr, info.ptr, P,
          _stream(torch))
    cw.get(np.float64)
    assert (info.get(np.int32) == 0).all()
    np.testing.assert_allclose(Bd.get(np.float64), 0.25, rtol=1e-14)


# =============================================================================================================================
# hsr_ridge_assemble / hsr_ridge_finish (+ batched)
# =============================================================================================================================
ASSEMBLE_SHAPES = [(1, 1, 1), (4, 3, 20), (10, 2, 33), (10, 3, 32), (16, 2, 200)]      # (n_in, degree, T)


def _assemble_ref(G, na, nf, T, alpha, npad):
    cnt, s = G[0, 0], G[0, 1:nf + 1]
    A = np.eye(npad)
    A[:nf, :nf] = G[1:nf + 1, 1:nf + 1] - (s[:, None] * s[None, :]) / cnt
    A[np.arange(nf), np.arange(nf)] += alpha
    B = np.zeros((npad, T))
    B[:nf] = G[1:nf + 1, na:na + T] - s[:, None] * (G[0, na:na + T] / cnt)[None, :]
    return A, B


def _finish_ref(G, na, nf, T, W, mean, scale, kpad):
    """ridge_finish_kernel: eight groups take every eighth feature, their sums are added in group order."""
    cnt = G[0, 0]
    sc = G[0, 1:nf + 1] / cnt
    part = np.zeros((8, T))
    for g in range(8):
        for f in range(g, nf, 8):
            part[g] = part[g] + sc[f] * W[f]
    a = part[0].copy()
    for g in range(1, 8):
        a = a + part[g]
    b = G[0, na:na + T] / cnt - a
    W32 = np.zeros((kpad, T), np.float32)
    W32[:nf] = W.astype(np.float32)
    return b, b.astype(np.float32), W32, mean.astype(np.float32), (1.0 / scale).astype(np.float32)


def _ridge_G(rng, na, nf, T, ldg, cnt=1000.0):
    G = rng.standard_normal((na, ldg)) * 50
    G[0, 0] = cnt
    return G


@pytest.mark.parametrize("n_in,degree,T", ASSEMBLE_SHAPES)
def test_assemble_finish(torch_gpu, n_in, degree, T):
    """ldg = na + tp + 3, ldb = T + 2, ldw = T + 1, kpad even and above nf: every element of A, B, the intercepts and the float32
    operands bit-equal to the kernels' formulas in float64 NumPy; identity block, zero rows, cleared info word; the batched forms
    carry the same bits per pair, give an empty pair the identity system, status 1 and NaN intercepts, and a pair whose
    Cholesky word is set status 2 and NaN intercepts."""
    torch, lib = torch_gpu, _lib()
    nf, na, _, npad = sizes(n_in, degree, T)
    tp = (T + 15) // 16 * 16
    ldg, ldb, ldw, kpad, alpha = na + tp + 3, T + 2, T + 1, (nf + 1) // 2 * 2 + 2, 0.75
    rng = np.random.default_rng(nf * 10 + T)
    P = 3
    Gs = [_ridge_G(rng, na, nf, T, ldg, cnt) for cnt in (1000.0, 0.0, 37.0)]
    Ws = [rng.standard_normal((nf, T)) for _ in range(P)]
    means, scales = 2600 + 100 * rng.standard_normal((P, n_in)), 900 + 300 * rng.random((P, n_in))
    st = _stream(torch)
    single = []
    for p in (0, 2):
        G = Gs[p]
        Gd = Mat(torch, na, ldg, ldg, np.float64, off=8, data=G)
        Ad, Bd, info = _out(torch, npad * npad, np.float64, 8), Mat(torch, npad, T, ldb, np.float64), _out(torch, 1, np.int32)
        _call("ridge_assemble_kernel", lib.hsr_ridge_assemble, Gd.ptr, ldg, na, nf, T, alpha, Ad.ptr, npad, Bd.ptr, ldb, info.ptr, st)
        A_ref, B_ref = _assemble_ref(G, na, nf, T, alpha, npad)
        A, B = Ad.get(np.float64).reshape(npad, npad), Bd.get()
        same_bits(A, A_ref, f"A pair {p}")
        same_bits(B, B_ref, f"B pair {p}")
        assert (A[nf:, nf:] == np.eye(npad - nf)).all() and (A[nf:, :nf] == 0).all() and (B[nf:].view(np.uint64) == 0).all()
        assert info.get(np.int32)[0] == 0
        Wd = Mat(torch, nf, T, ldw, np.float64, off=8, data=Ws[p], gap=np.nan)
        md, sd = _vec(torch, means[p], 8), _vec(torch, scales[p])
        outs = [_out(torch, T, np.float64, 8), _out(torch, T, np.float32, 4), _out(torch, kpad * T, np.float32),
                _out(torch, n_in, np.float32, 4), _out(torch, n_in, np.float32)]
        _call("ridge_finish_kernel", lib.hsr_ridge_finish, Gd.ptr, na, nf, T, Wd.ptr, ldw, md.ptr, sd.ptr, n_in, kpad,
              *[o.ptr for o in outs], st)
        got = [o.get(dt) for o, dt in zip(outs, (np.float64, np.float32, np.float32, np.float32, np.float32))]
        got[2] = got[2].reshape(kpad, T)
        ref = _finish_ref(G, na, nf, T, Ws[p], means[p], scales[p], kpad)
        for g, r, name in zip(got, ref, ("b64", "b32", "W32", "mean32", "inv32")):
            same_bits(g, r, f"{name} pair {p}")
        single.append((A, B, got))
    # batched: pair 1 has no training row; pair 2's Cholesky word is set
    pg, pa, pb = na * ldg + 4, npad * npad + 6, npad * ldb + 2
    Gd = Mat(torch, P, na * ldg, pg, np.float64, data=np.stack(Gs).reshape(P, -1), gap=np.nan)
    Ad, Bd, info = Mat(torch, P, npad * npad, pa, np.float64), Mat(torch, P, npad * ldb, pb, np.float64, off=8), _out(torch, P, np.int32)
    _call("ridge_assemble_kernel", lib.hsr_ridge_assemble_batched, Gd.ptr, ldg, pg, na, nf, T, alpha, Ad.ptr, npad, pa, Bd.ptr, ldb, pb,
          info.ptr, P, st)
    A, B = Ad.get().reshape(P, npad, npad), Bd.get().reshape(P, npad, ldb)
    assert (info.get(np.int32) == 0).all()
    assert (np.ascontiguousarray(B[:, :, T:]).view(np.uint8) == FILL).all()
    for k, p in enumerate((0, 2)):
        same_bits(A[p], single[k][0], f"batched A pair {p}")
        same_bits(B[p][:, :T], single[k][1], f"batched B pair {p}")
    assert (A[1] == np.eye(npad)).all() and (B[1][:, :T].view(np.uint64) == 0).all()
    pw, pms, pbo, pw32, pmi = nf * ldw + 2, n_in + 1, T + 3, kpad * T + 5, n_in + 2
    wrows = np.full((P, nf, ldw), np.nan)
    wrows[:, :, :T] = np.stack(Ws)
    Wd = Mat(torch, P, nf * ldw, pw, np.float64, data=wrows.reshape(P, -1), gap=np.nan)
    md, sd = Mat(torch, P, n_in, pms, np.float64, data=means, gap=np.nan), Mat(torch, P, n_in, pms, np.float64, data=scales, gap=np.nan)
    infod = _vec(torch, np.array([0, 0, 9], np.int32))
    b64, b32 = Mat(torch, P, T, pbo, np.float64), Mat(torch, P, T, pbo, np.float32)
    W32, m32, i32 = Mat(torch, P, kpad * T, pw32, np.float32), Mat(torch, P, n_in, pmi, np.float32), Mat(torch, P, n_in, pmi, np.float32)
    status = _out(torch, P, np.int32)
    _call("ridge_finish_kernel", lib.hsr_ridge_finish_batched, Gd.ptr, pg, na, nf, T, Wd.ptr, ldw, pw, md.ptr, sd.ptr, pms, n_in, kpad,
          b64.ptr, b32.ptr, pbo, W32.ptr, pw32, m32.ptr, i32.ptr, pmi, infod.ptr, status.ptr, P, st)
    assert list(status.get(np.int32)) == [0, 1, 2]
    b64h, b32h, W32h, m32h, i32h = b64.get(), b32.get(), W32.get().reshape(P, kpad, T), m32.get(), i32.get()
    for g, r, name in zip((b64h[0], b32h[0], W32h[0], m32h[0], i32h[0]), single[0][2], ("b64", "b32", "W32", "mean32", "inv32")):
        same_bits(g, r, f"batched {name} pair 0")
    for p in (1, 2):
        assert np.isnan(b64h[p]).all() and np.isnan(b32h[p]).all(), p
        same_bits(W32h[p][:nf], Ws[p].astype(np.float32), f"W32 pair {p}")
        assert (W32h[p][nf:].view(np.uint32) == 0).all()
        same_bits(m32h[p], means[p].astype(np.float32), f"mean32 pair {p}")
        same_bits(i32h[p], (1.0 / scales[p]).astype(np.float32), f"inv32 pair {p}")
    same_bits(W32h[2], single[1][2][2], "batched W32 pair 2")


# =============================================================================================================================
# hsr_chol_solve_f64 / hsr_chol_solve_f64_batched
# =============================================================================================================================
CHOL_N = tuple(range(32, 289, 32)) + (320, 384, 480, 512)
CHOL_NRHS = (1, 15, 16, 17, 285)


def _chol_names(n):
    return ("chol_factor_res_kernel" if n <= 288 else "chol_factor_kernel") + "; chol_solve_kernel " + ("lds" if n <= 384 else "global")


def _spd(rng, n, kind):
    if kind == "project":                                   # M M^T / n + 0.3 I, cond ~ 10
        M = rng.standard_normal((n, n + 40))
        return M @ M.T / n + 0.3 * np.eye(n)
    F = rng.standard_normal((400, 6)) @ rng.standard_normal((6, n)) + 1e-3 * rng.standard_normal((400, n))
    return F.T @ F + np.eye(n)                              # ridge-like: 6 latent factors + noise, cond ~ 1e6


def _unwritten_upper(n):
    """The elements above the diagonal that include/hsr.h promises a call leaves alone."""
    i, j = np.indices((n, n))
    m = j > i
    if n > 288:
        m &= ~((i // 16 == j // 16) & (i >= 32))
    return m


def _chol_run(torch, A, Bm, lda, ldb, off, expect=None):
    """One single-system call on A with NaN above the diagonal.  Returns (L, X, info) after the contract checks."""
    lib = _lib()
    n, nrhs = A.shape[0], Bm.shape[1]
    An = A.copy()
    An[np.triu_indices(n, 1)] = np.nan
    Ad = Mat(torch, n, n, lda, np.float64, off=off, data=An)
    Bd = Mat(torch, n, nrhs, ldb, np.float64, off=off, data=Bm)
    work, info = _out(torch, lib.hsr_chol_work_bytes(n) // 8, np.float64), _out(torch, 1, np.int32)
    _call(expect or _chol_names(n), lib.hsr_chol_solve_f64, Ad.ptr, lda, n, Bd.ptr, ldb, nrhs, work.ptr, info.ptr, _stream(torch))
    work.get(np.float64)
    Ag = Ad.get()
    keep = _unwritten_upper(n)
    assert (Ag[keep].view(np.uint64) == An[keep].view(np.uint64)).all(), "write above the diagonal outside the named tiles"
    return np.tril(Ag), Bd.get(), int(info.get(np.int32)[0])


@pytest.mark.parametrize("n", CHOL_N)
def test_chol(torch_gpu, n):
    """Both matrix classes at every nrhs, with lda in {n, n + 1, n + 7}, ldb in {nrhs, nrhs + 2} and bases 0 / 8 bytes past the
    alignment taking turns.  The factor does not depend on the layout (bit-equal over the calls)."""
    torch = torch_gpu
    rng = np.random.default_rng(n)
    k = n // 32
    for kind in ("project", "ridge"):
        A = _spd(rng, n, kind)
        Al = A.astype(LD)
        anorm = np.abs(Al).sum(axis=1).max()
        L0 = None
        for nrhs in CHOL_NRHS:
            k += 1
            lda, ldb, off = n + (0, 1, 7)[k % 3], nrhs + 2 * (k % 2), 8 * ((k // 2) % 2)
            Bm = rng.standard_normal((n, nrhs))
            L, X, info = _chol_run(torch, A, Bm, lda, ldb, off)
            what = f"n={n} {kind} nrhs={nrhs} lda={lda} ldb={ldb} off={off}"
            assert info == 0, what
            if L0 is None:
                L0 = L
                Ll = L.astype(LD)
                r1 = np.abs(Ll @ Ll.T - Al).sum(axis=1).max() / (n * anorm * U52)
                _note(f"chol factor ratio, {kind} (<= 1)", r1)
                assert r1 <= 1, (what, float(r1))
                if kind == "project":
                    ref = np.linalg.cholesky(A)
                    _note("chol factor vs numpy (rtol 1e-10 / atol 1e-12)", np.max(np.abs(L - ref) / (1e-12 + 1e-10 * np.abs(ref))))
                    np.testing.assert_allclose(L, ref, rtol=1e-10, atol=1e-12, err_msg=what)
            else:
                same_bits(L, L0, what + ": factor")
            Xl = X.astype(LD)
            r2 = np.abs(Al @ Xl - Bm.astype(LD)).sum(axis=0).max() / (n * anorm * np.abs(Xl).sum(axis=0).max() * U52)
            _note(f"chol solve ratio, {kind} (<= 1)", r2)
            assert r2 <= 1, (what, float(r2))
            if kind == "project":
                ref = np.linalg.solve(A, Bm)
                _note("chol solution vs numpy (rtol 1e-9 / atol 1e-11)", np.max(np.abs(X - ref) / (1e-11 + 1e-9 * np.abs(ref))))
                np.testing.assert_allclose(X, ref, rtol=1e-9, atol=1e-11, err_msg=what)


@pytest.mark.parametrize("n,pivots", [(32, (0, 17, 31)), (288, (5, 140, 287)), (320, (3, 170, 319)), (512, (31, 250, 511))])
def test_chol_bad_pivot(torch_gpu, n, pivots):
    """A non-positive pivot in the first, a middle and the last block of either factor kernel: the 1-based index in info; in a
    batch of three the other systems keep the bits of their single solve, NaN above the diagonal throughout."""
    torch, lib = torch_gpu, _lib()
    rng = np.random.default_rng(n + 1)
    good = [_spd(rng, n, "project") for _ in range(2)]
    nrhs, lda, ldb = 17, n + 1, 19
    Bs = rng.standard_normal((3, n, nrhs))
    singles = [_chol_run(torch, good[i], Bs[2 * i], lda, ldb, 0) for i in range(2)]
    for kp in pivots:
        A = _spd(rng, n, "project")
        Lr = np.linalg.cholesky(A)
        A[kp, kp] -= Lr[kp, kp] ** 2 + 1.0                               # Schur pivot kp becomes -1
        _, _, info = _chol_run(torch, A, Bs[1], lda, ldb, 8)
        assert info == kp + 1, (n, kp, info)
        mats = np.stack([good[0], A, good[1]])
        mats[:, np.triu_indices(n, 1)[0], np.triu_indices(n, 1)[1]] = np.nan
        rows = np.full((3, n, lda), np.nan)
        rows[:, :, :n] = mats
        pa, pb = n * lda + 4, n * ldb + 6
        Ad = Mat(torch, 3, n * lda, pa, np.float64, off=8, data=rows.reshape(3, -1))
        brows = np.full((3, n, ldb), np.nan)
        brows[:, :, :nrhs] = Bs
        Bd = Mat(torch, 3, n * ldb, pb, np.float64, data=brows.reshape(3, -1))
        work, infod = _out(torch, 3 * lib.hsr_chol_work_bytes(n) // 8, np.float64), _out(torch, 3, np.int32)
        _call(_chol_names(n), lib.hsr_chol_solve_f64_batched, Ad.ptr, lda, n, pa, Bd.ptr, ldb, nrhs, pb, work.ptr, infod.ptr, 3,
              _stream(torch))
        work.get(np.float64)
        assert list(infod.get(np.int32)) == [0, kp + 1, 0]
        Ag, Bg = Ad.get().reshape(3, n, lda), Bd.get().reshape(3, n, ldb)
        keep = _unwritten_upper(n)
        for p in range(3):
            assert np.isnan(Ag[p][:, n:]).all() and np.isnan(Bg[p][:, nrhs:]).all()
            assert np.isnan(Ag[p][:, :n][keep]).all()
        for i, p in enumerate((0, 2)):
            same_bits(np.tril(Ag[p][:, :n]), singles[i][0], f"n={n} bad pivot {kp}: factor of pair {p}")
            same_bits(Bg[p][:, :nrhs], singles[i][1], f"n={n} bad pivot {kp}: solution of pair {p}")


# =============================================================================================================================
# hsr_polyfeat_predict / _predict_cube / _predict_cube_batched
# =============================================================================================================================
# (n_in, degree, T) -> slot of hsr_polyfeat_predict_kernel
PREDICT_ROWS = [((10, 3, 1), 0), ((10, 3, 16), 0), ((10, 3, 17), 1), ((10, 3, 32), 1), ((10, 3, 33), 2), ((10, 3, 64), 2),
                ((10, 3, 65), 3), ((10, 3, 96), 3), ((10, 3, 97), 2), ((10, 3, 285), 3), ((4, 3, 20), 4), ((10, 2, 100), 5),
                ((16, 2, 200), 6)]
PREDICT_NPIX = (1, 31, 32, 33, 511, 513, 1517)
NODATA = 2600.0
_MODELS = {}


def _predict_name(slot, arm):
    if slot >= 4:
        return f"predict_kernel<{(1, 2, 4)[slot - 4]}>"
    return ("predict103_x16_kernel " if slot == 0 else f"predict103_slice_kernel<{slot}> ") + arm


def _inputs(rng, n, n_in):
    return (600 + 4000 * np.clip(rng.random((n, 4)) @ rng.random((4, n_in)) / 2, 0, 1)).astype(np.float32)


def _model(n_in, degree, T):
    """The oracle's fit (float64) of a seeded problem, computed once per shape."""
    key = (n_in, degree, T)
    if key not in _MODELS:
        rng = np.random.default_rng(1000 * n_in + 100 * degree + T)
        N = 2501
        base = rng.random((N, 4))
        X = (600 + 4000 * np.clip(base @ rng.random((4, n_in)) / 2 + 0.02 * rng.standard_normal((N, n_in)), 0, 1)).astype(np.float32)
        Y = onp.logit(np.clip(base @ rng.random((4, T)) / 3 + 0.01 * rng.standard_normal((N, T)), 0.001, 0.6))
        _MODELS[key] = onp.ridge_poly_fit(X.astype(np.float64), Y, degree, 1.0)
    return _MODELS[key]


def _predict_ref(model, X, act, nan_bad, use_nd):
    out = onp.ridge_poly_predict(model, np.where(np.isfinite(X), X, 0.0).astype(np.float64))
    if act:
        out = onp.sigmoid(out)
    if nan_bad:
        bad = ~np.isfinite(X).all(axis=1)
        if use_nd:
            bad |= np.isclose(X, NODATA).any(axis=1)
        out[bad] = np.nan
    return out.T                                              # (T, npix)


@pytest.mark.parametrize("shape,slot", PREDICT_ROWS)
def test_predict(torch_gpu, shape, slot):
    """ldw = T + 3, out_stride = npix + 5.  The aligned pixel-major call (five float2 loads per pixel in the MFMA kernels) against
    the oracle's float64 prediction of the oracle's model; rows of an odd pitch, rows 4 bytes past the alignment, band-major planes
    and a batch of three with an odd pair stride (pair 1 takes the other arm of pred_load10) bit-equal to it."""
    torch, lib = torch_gpu, _lib()
    n_in, degree, T = shape
    nf = _prepare(n_in, degree)
    assert lib.hsr_polyfeat_predict_kernel(n_in, degree, T, -1) == slot
    model = _model(n_in, degree, T)
    kpad, ldw = (nf + 1) // 2 * 2, T + 3
    W = np.zeros((kpad, T), np.float32)
    W[:nf] = model["coef"].T
    Wd = Mat(torch, kpad, T, ldw, np.float32, off=4, data=W, gap=np.nan)
    P = 3
    biases = np.stack([model["intercept"], model["intercept"] + 0.25, model["intercept"] - 0.5]).astype(np.float32)
    bd = Mat(torch, P, T, T + 1, np.float32, data=biases, gap=np.nan)
    md, sd = _vec(torch, model["mean"].astype(np.float32), 4), _vec(torch, (1.0 / model["scale"]).astype(np.float32))
    st = _stream(torch)
    rng = np.random.default_rng(T * 31 + n_in)
    even = n_in + (n_in & 1)
    configs = [(0, 0, 0), (1, 1, 1), (0, 1, 0), (1, 0, 0)]                       # (activation, nan_bad, use_nodata)
    for i, npix in enumerate(PREDICT_NPIX):
        for act, nan_bad, use_nd in (configs if npix in (33, 1517) else [configs[i % 4], configs[(i + 1) % 4]]):
            X = _inputs(rng, P * npix, n_in).reshape(P, npix, n_in)
            if nan_bad:                                                            # unusable samples: only where they become NaN
                specials = [np.nan, np.inf, -np.inf] + ([NODATA, NODATA + 0.01, NODATA - 0.01] if use_nd else [])
                for p in range(P):
                    for s, v in enumerate(specials):
                        X[p, (s * 7 + p) % npix, (s + p) % n_in] = v
            if use_nd:
                X[:, npix // 2, 0] = np.float32(NODATA + 0.06)                       # near, but not close to, the nodata value
            ostride = npix + 5

            def run(name, entry, x, x_ps, x_cs, p):
                out = Mat(torch, T, npix, ostride, np.float32, off=4 * (p % 2))
                bias_p = C.c_void_p(bd.ptr.value + p * (T + 1) * 4)
                if entry == "predict":
                    _call(name, lib.hsr_polyfeat_predict, x.ptr, x_ps, x_cs, md.ptr, sd.ptr, npix, n_in, degree, Wd.ptr, ldw, bias_p, T,
                          act, out.ptr, ostride, st)
                else:
                    _call(name, lib.hsr_polyfeat_predict_cube, x.ptr, x_ps, x_cs, md.ptr, sd.ptr, npix, n_in, degree, Wd.ptr, ldw, bias_p,
                          T, act, nan_bad, NODATA, use_nd, out.ptr, ostride, st)
                return out.get()

            entry = "cube" if (nan_bad or use_nd) else "predict"
            base = []
            for p in range(P):
                x = Mat(torch, npix, n_in, even, np.float32, data=X[p], gap=np.nan)
                got = run(_predict_name(slot, "x2"), entry, x, even, 1, p)
                mp = dict(model, intercept=biases[p].astype(np.float64))
                ref = _predict_ref(mp, X[p], act, nan_bad, use_nd)
                what = f"{shape} npix={npix} act={act} nan_bad={nan_bad} nodata={use_nd} pair {p}"
                assert np.array_equal(np.isnan(got), np.isnan(ref)), what + ": NaN set"
                if nan_bad:
                    assert np.isnan(ref).any() and (~np.isnan(ref)).any() or npix == 1
                bar = 1e-4 if act else 2e-4
                err = np.nanmax(np.abs(got - ref)) if (~np.isnan(ref)).any() else 0.0
                _note("predict reflectance (1e-4)" if act else "predict logit (2e-4)", err / bar)
                assert err <= bar, (what, err)
                base.append(got)
            p = i % P
            odd = Mat(torch, npix, n_in, even + 1, np.float32, data=X[p], gap=np.nan)
            bits_equal(run(_predict_name(slot, "scalar"), entry, odd, even + 1, 1, p), base[p], "odd pitch")
            off4 = Mat(torch, npix, n_in, even, np.float32, off=4, data=X[p], gap=np.nan)
            bits_equal(run(_predict_name(slot, "scalar"), entry, off4, even, 1, p), base[p], "base off by 4 bytes")
            bands = Mat(torch, n_in, npix, npix + 3, np.float32, data=X[p].T, gap=np.nan)
            bits_equal(run(_predict_name(slot, "scalar"), entry, bands, 1, npix + 3, p), base[p], "band-major")
            # batched, odd pair stride: pair 1 starts 4 bytes off an 8-byte boundary
            pair_x = npix * even + 1
            rows = np.full((P, npix, even), np.nan, np.float32)
            rows[:, :, :n_in] = X
            xb = Mat(torch, P, npix * even, pair_x, np.float32, data=rows.reshape(P, -1), gap=np.nan)
            pair_out = T * ostride + 9
            out = Mat(torch, P, T * ostride, pair_out, np.float32)
            _call(_predict_name(slot, "x2"), lib.hsr_polyfeat_predict_cube_batched, xb.ptr, even, 1, pair_x, md.ptr, sd.ptr, 0, npix, n_in,
                  degree, Wd.ptr, ldw, 0, bd.ptr, T + 1, T, act, nan_bad, NODATA, use_nd, out.ptr, ostride, pair_out, P, st)
            got = out.get().reshape(P, T, ostride)
            assert (np.ascontiguousarray(got[:, :, npix:]).view(np.uint8) == FILL).all()
            for q in range(P):
                bits_equal(got[q][:, :npix], base[q], f"batched pair {q}")


# =============================================================================================================================
# PolyRidge: the single fit reports a failed factorisation
# =============================================================================================================================
# intercept_ of the g7 fit as the code before status_ (read-out through hsr_ridge_finish) produced it on an MI355X
G7_INTERCEPT_BITS = [0xbfe2d9bc4ce7cca2, 0xbff4a25057b2d0d1, 0xbfe730e2ecb1a2bf, 0xbfd472e1ca7d335a, 0xbfddcbb542f8baa5,
                     0xbfc4638b4dd5826c]


def test_single_fit_status(torch_gpu):
    """status_ of PolyRidge: 2 for alpha = 0 with one input vector on every row (the centred Gram is exactly 0), 1 for a fit on
    zero rows, both with all-NaN predictions; 0 for the g7 fit, whose intercepts keep the bits they had when the read-out went
    through hsr_ridge_finish (literals recorded from that code on an MI355X), as do coef_ and the predictions."""
    import s2_emit
    rng = np.random.default_rng(5)
    Xq = (600 + 4000 * rng.random((50, 4))).astype(np.float32)
    X = np.repeat(Xq[:1], 300, axis=0)
    Y = rng.standard_normal((300, 3))
    m = s2_emit.PolyRidge(degree=2, alpha=0.0).fit(X, Y)
    assert m.status_ == 2 and m.status_ == 2
    assert np.isnan(m.intercept_).all() and np.isnan(m.predict(Xq)).all()
    assert np.isnan(m.predict_cube(np.ascontiguousarray(Xq[:48].T.reshape(4, 6, 8)))).all()
    m = s2_emit.PolyRidge(degree=2, alpha=1.0).fit(X[:0], Y[:0])
    assert m.status_ == 1
    assert np.isnan(m.intercept_).all() and np.isnan(m.predict(Xq)).all()
    g = load_golden("g7_ridge")
    X = g["X"].astype(np.float32)
    m = s2_emit.PolyRidge(degree=3, alpha=1.0).fit(X, g["Ylogit"])
    assert m.status_ == 0
    assert [int(v) for v in m.intercept_.view(np.uint64)] == G7_INTERCEPT_BITS
    np.testing.assert_allclose(m.intercept_, g["intercept"], rtol=1e-6, atol=1e-7)
    # the same fit read out by hsr_ridge_finish: coef_, the float32 operands and the predictions bit for bit
    lib, torch = _lib(), torch_gpu
    from s2_emit._engine import _ptr
    from s2_emit.ridge import ridge_dims
    Xd, Yd = m._to_dev(X, g["Ylogit"])
    _, mean, scale = m._stats_dev(Xd)
    G = m.local_gram(Xd, Yd, mean, scale)
    d = ridge_dims(10, 3, 6)
    Gp, Bp = torch.empty((d.npad, d.npad), dtype=torch.float64, device="cuda"), torch.empty((d.npad, 6), dtype=torch.float64, device="cuda")
    info = torch.empty(1, dtype=torch.int32, device="cuda")
    st = _stream(torch)
    assert lib.hsr_ridge_assemble(_ptr(G), G.stride(0), d.na, d.nf, 6, 1.0, _ptr(Gp), d.npad, _ptr(Bp), 6, _ptr(info), st) == 0
    cw = torch.empty(lib.hsr_chol_work_bytes(d.npad) // 8, dtype=torch.float64, device="cuda")
    assert lib.hsr_chol_solve_f64(_ptr(Gp), d.npad, d.npad, _ptr(Bp), 6, 6, _ptr(cw), _ptr(info), st) == 0
    b = torch.empty(6, dtype=torch.float64, device="cuda")
    b32, Wf = torch.empty(6, dtype=torch.float32, device="cuda"), torch.empty((d.kpad, 6), dtype=torch.float32, device="cuda")
    m32, i32 = torch.empty(10, dtype=torch.float32, device="cuda"), torch.empty(10, dtype=torch.float32, device="cuda")
    assert lib.hsr_ridge_finish(_ptr(G), d.na, d.nf, 6, _ptr(Bp), 6, _ptr(mean), _ptr(scale), 10, d.kpad, _ptr(b), _ptr(b32), _ptr(Wf),
                                _ptr(m32), _ptr(i32), st) == 0
    same_bits(m.intercept_, b.cpu().numpy(), "intercept_")
    same_bits(m.coef_, Bp[:d.nf].t().contiguous().cpu().numpy(), "coef_")
    for name, t in (("W", Wf), ("b", b32), ("mean", m32), ("inv", i32)):
        bits_equal(m._dev[name].cpu().numpy(), t.cpu().numpy(), name)
    old = s2_emit.PolyRidge(degree=3, alpha=1.0)
    old.n_in, old.n_feat, old.n_targets, old._dev = 10, d.nf, 6, dict(W=Wf, b=b32, mean=m32, inv=i32)
    Xte = g["Xtest"].reshape(-1, 10).astype(np.float32)
    bits_equal(m.predict(Xte), old.predict(Xte), "predictions")
    np.testing.assert_allclose(m.predict(Xte), g["pred_logit"], rtol=0, atol=2e-4)


# =============================================================================================================================
def test_rows_reach_every_k4_instance():
    """Runs last: the rows above reached every name the record can hold."""
    lib = _lib()
    table = {lib.hsr_k4_instance_name(i).decode() for i in range(lib.hsr_k4_instance_count())}
    assert len(table) == lib.hsr_k4_instance_count()
    for k in sorted(WORST):
        print(f"largest error / bar: {k}: {WORST[k]:.3e}")
    assert LOG.seen <= table, LOG.seen - table
    assert table <= LOG.seen, f"instances no row reached: {sorted(table - LOG.seen)}"
