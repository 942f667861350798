"""The case table of the Sinkhorn kernels (csrc/hsr_ot.hip) and their references in np.longdouble.  No GPU, no library.

Three things live here:
  * SHAPES / ROWS: which (n, m) reach which loop of which kernel, and which stop rule every row ends by.  paths(n, m) mirrors
    the few loop bounds of the kernels, so that tests/test_ot_cases_host.py can check that the table reaches what it names.
  * The references: kernel matrix, one column update, one row update, the marginal error, the barycentric projection - each
    from GIVEN float64 operands, in x87 extended precision (64-bit mantissa, 15-bit exponent: nothing here overflows where
    float64 does, so "would this update overflow float64" is a comparison with DBL_MAX), each with its error bound.
  * solve(): the whole schedule on the host, every stage rounded to float64, to know where a row stops.

The bounds are derived, not measured.  U = 2**-53 is the unit roundoff of float64, UF = 2**-1074 its denormal spacing.
A product of two float64 numbers is within U relative of the exact one, or - if it falls into the denormal range - within
UF/2 absolute.  A sum of L non-negative terms has a relative error of at most (L - 1) U whatever the order it is added in
(no cancellation); sums of denormals are exact.  One divide adds U.  Together, for s = sum_k p_k q_k with p, q >= 0 and x = c / s:
    |x_dev - x| <= ((L + 3) U + L UF / s) x                                                                   [matvec_bound]
(L + 1) U would do; the 3 leaves room for the second-order terms that the first-order count drops."""
import functools

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63 and np.finfo(LD).maxexp >= 16384, "the references need x87 extended precision"

U = 2.0 ** -53
UF = 2.0 ** -1074
DBL_MAX = LD(np.finfo(np.float64).max)
NEVER = 0x7FFFFFFF
EXP_ULP = 3            # double exp: <= 3 ulp in the OpenCL C accuracy table (no device-libs table was at hand)
K_CANCEL = 12          # see kernel_matrix_bound
MARGIN = 1e-3          # |ln(q / DBL_MAX)| that every breakdown row keeps at every iteration up to its break
STATE, K_, PARTIAL, ERRPART, U0, U1, V0, V1 = range(8)       # hsr_ot_work_region's `which`

# ---------------------------------------------------------------------------------------------------------------------------
# mirror of the loop bounds
# ---------------------------------------------------------------------------------------------------------------------------
def paths(n, m):
    """Trip counts of the kernels' loops at (n, m): what the shapes of the table are chosen by."""
    nchunks = (n + 63) // 64
    rows = [min(64, n - 64 * c) for c in range(nchunks)]
    even = m % 2 == 0
    per = (nchunks + 3) >> 2
    quarters = [max(0, min(q * per + per, nchunks) - q * per) for q in range(4)]
    m2 = m // 2
    unrolled = [len(range(lane, max(m2 - 192, 0), 256)) for lane in range(64)] if even else [0] * 64      # c + 3 * 64 < m2
    rem = [len(range(lane + 256 * unrolled[lane], m2 if even else m, 64)) for lane in range(64)]
    parts = (m + 63) // 64
    return dict(
        nchunks=nchunks, last_rows=rows[-1], col_double2=even,
        col_unrolled=sorted({r // 8 for r in rows}) if even else [0],        # trips of the 8-row loop, per chunk
        col_tail=sorted({r % 8 for r in rows}) if even else sorted(set(rows)),
        col_blocks=(m + 511) // 512, init_blocks=(m + 255) // 256,
        lone_last_column=not even,                                           # the last thread of col-partial has no column j + 1
        quarters=quarters, quarter_past_end=any(q * per > nchunks for q in range(4)),
        row_unrolled=max(unrolled), row_rem=max(rem), row_rem_partial_wave=min(rem) < max(rem),      # some lanes sit the last trip out
        err_parts=parts, err_trips=(parts + 63) // 64)


SHAPES = {                                  # (n, m): the path it is the smallest shape for
    (1, 2): "one row: one chunk, a 1-row tail",
    (63, 2): "7 unrolled trips + a 7-row tail",
    (64, 2): "exactly 8 unrolled trips, no tail",
    (65, 2): "2 chunks, the second of one row",
    (61, 66): "7 unrolled + 5 tail rows on the double2 column path",
    (257, 129): "5 chunks -> quarters 2,2,1,0 (the last starts past the end); odd m: scalar paths, lone last column",
    (520, 130): "9 chunks -> quarters 3,3,3,0; row kernel: remainder loop only, partial wave",
    (66, 512): "row kernel: exactly one unrolled trip, no remainder",
    (70, 646): "row kernel: one unrolled trip + remainder with a partial wave; second column block",
    (3, 4162): "66 error parts: second trip of ot_error_kernel's loop",
    (3, 4161): "the same with odd m",
}


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def clouds(n, m, seed):
    """The clouds of the shape and stop-rule rows: as in test_device_sinkhorn_vs_oracle."""
    rng = np.random.default_rng(seed)
    X = rng.random((n, 3))
    Y = np.clip(X[rng.integers(0, n, m)] ** 0.8 * 0.9 + 0.05 + 0.02 * rng.standard_normal((m, 3)), 0, 1)
    return X, Y


def breakdown_clouds(n, m, seed, side, t, reg):
    """Two clouds inside [0, 0.2]^3 and one point (row 0 of `side`) moved to sqrt(t reg / 3) on all three axes: its entries of K
    are about exp(-t), denormal or zero, and some iterations later 1 / (a sum of them) overflows."""
    rng = np.random.default_rng(seed)
    X, Y = rng.random((n, 3)) * 0.2, rng.random((m, 3)) * 0.2
    (X if side == "X" else Y)[0] = np.sqrt(t * reg / 3.0)
    return X, Y


def near_clouds(n, m, seed):
    """clouds() with the first 20 targets within 1e-9 of a source point: d = (a2 + b2) - 2 x.y then cancels down to its rounding
    error, of either sign - the entries that the clamp at 0 is for."""
    X, Y = clouds(n, m, seed)
    Y[:20] = X[:20] + 1e-9 * np.random.default_rng(seed + 1).standard_normal((20, 3))
    return X, Y


def device_sqdist(X, Y):
    """d as ot_init_kernel forms it BEFORE the clamp: the same float64 operations in the same order, no contraction."""
    x, y = np.asarray(X, np.float64)[:, None, :], np.asarray(Y, np.float64)[None, :, :]
    a2 = x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1] + x[..., 2] * x[..., 2]
    b2 = y[..., 0] * y[..., 0] + y[..., 1] * y[..., 1] + y[..., 2] * y[..., 2]
    return a2 + b2 - 2.0 * (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1] + x[..., 2] * y[..., 2])


def zero_column_clouds():
    """test_device_sinkhorn_breakdown_keeps_previous_iterate: exp(-7500 / 0.01) == 0, a column sum of exactly 0 at iteration 0."""
    rng = np.random.default_rng(5)
    X, Y = rng.random((200, 3)) * 0.1, rng.random((180, 3)) * 0.1
    Y[7] = 50.0
    return X, Y


def _row(n, m, reg=0.05, itmax=12, thr=0.0, seed=None, gen="clouds", stepwise=12, **expect):
    return dict(n=n, m=m, reg=reg, itmax=itmax, thr=thr, seed=n + m if seed is None else seed, gen=gen, stepwise=stepwise, expect=expect)


def _brk(n, m, seed, side, t, reg, break_iter, through, itmax=40):
    """A row that breaks down at `break_iter`: stepped one iteration at a time up to the call after the break."""
    return _row(n, m, reg, itmax, 1e-9, seed, ("breakdown", side, t), stepwise=break_iter + 2,
                break_iter=break_iter, conv_iter=None, checks=(break_iter + 9) // 10, through=through)


# expect: break_iter / conv_iter (None: never), checks = error evaluations, through = which predicate breaks ("v", "u", "zero").
# The host test holds every entry against solve().  Rows without a threshold run 12 iterations with stopThr = 0: two error
# checks (iterations 0 and 10), never converged, ended by count.
ROWS = {("shape-%dx%d" % s): _row(*s, break_iter=None, conv_iter=None, checks=2) for s in SHAPES}
ROWS.update({
    # d < 0 before the clamp in some entries: K must not exceed 1 there
    "clamp-61x66": _row(61, 66, gen="near", break_iter=None, conv_iter=None, checks=2),
    # ended by count, on even and on odd iterations_done
    "count0-61x66": _row(61, 66, itmax=0, break_iter=None, conv_iter=None, checks=0),
    "count1-61x66": _row(61, 66, itmax=1, break_iter=None, conv_iter=None, checks=1),
    "count2-257x129": _row(257, 129, itmax=2, break_iter=None, conv_iter=None, checks=1),
    "count11-70x646": _row(70, 646, itmax=11, break_iter=None, conv_iter=None, checks=2),
    "count23-257x129": _row(257, 129, itmax=23, break_iter=None, conv_iter=None, checks=3),          # stopThr 0 never converges
    # converged
    "conv0-61x66": _row(61, 66, itmax=12, thr=1e30, break_iter=None, conv_iter=0, checks=1),
    "conv0-257x129": _row(257, 129, itmax=5, thr=1e30, break_iter=None, conv_iter=0, checks=1),
    "conv10-61x66": _row(61, 66, itmax=35, thr=0.01, break_iter=None, conv_iter=10, checks=2),       # err 0.0475, 0.00213
    "conv20-70x646": _row(70, 646, itmax=35, thr=0.00041, break_iter=None, conv_iter=20, checks=3),  # err 0.0114, 0.00108, 0.000155
    # breakdowns.  Iteration 0 through a column sum of exactly 0 (the input of test_device_sinkhorn_breakdown_keeps_previous_iterate),
    # the last four found by tools/scan_ot_cases.py: the widest margin of each class among 200 seeds x 2 shapes x 2 reg x {X, Y}.
    # That scan yields no stable input that breaks at a multiple of 10 above 0 and none that breaks through u alone at an even
    # iteration (17 stable inputs in all, at iterations 1, 3, 5, 7, 12, 16, 17, 18, 27, 31): those two classes have no row.
    "break0-zero": _row(200, 180, 0.01, 50, 1e-9, 5, "zero", stepwise=2, break_iter=0, conv_iter=None, checks=0, through="zero"),
    # every entry of the moved point's column is a positive denormal (reg 1, t 739: exp(-739) .. exp(-720)): v overflows at once, and
    # K v is then inf in EVERY row, u = 0 - finite: only the column pass's own test of v sees this breakdown
    "break0-v": _brk(97, 65, 0, "Y", 739.0, 1.0, 0, "v"),
    "break5-v": _brk(97, 65, 81, "Y", 781.0, 0.05, 5, "v"),             # odd, through v;         margin 0.21
    "break12-v": _brk(130, 66, 185, "Y", 885.0, 0.01, 12, "v"),         # even and not 0;         margin 0.138
    "break1-u": _brk(97, 65, 176, "X", 876.0, 0.01, 1, "u"),            # through u alone, odd;   margin 0.287
    "break31-v": _brk(97, 65, 181, "Y", 881.0, 0.01, 31, "v"),          # odd, after 4 checks;    margin 0.192
})


def inputs(name):
    r = ROWS[name]
    if r["gen"] == "clouds":
        return clouds(r["n"], r["m"], r["seed"])
    if r["gen"] == "near":
        return near_clouds(r["n"], r["m"], r["seed"])
    if r["gen"] == "zero":
        return zero_column_clouds()
    _, side, t = r["gen"]
    return breakdown_clouds(r["n"], r["m"], r["seed"], side, t, r["reg"])


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
def f64(x):
    """Rounded to float64; what exceeds DBL_MAX becomes inf, silently."""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=LD).astype(np.float64)


def kernel_matrix(X, Y, reg):
    """K_ref = exp(-max(d, 0) / reg) with d = |x - y|^2, everything in long double from the float64 inputs."""
    x, y = np.asarray(X, np.float64).astype(LD), np.asarray(Y, np.float64).astype(LD)
    d = np.maximum(((x[:, None, :] - y[None, :, :]) ** 2).sum(-1), LD(0))
    return np.exp(-d / LD(reg))


def kernel_matrix_bound(X, Y, reg, K_ref):
    """|K_dev - K_ref| allowed.  The kernel forms d = (a2 + b2) - 2 x.y in float64: a2, b2 and x.y are sums of three products
    (3 U relative each, x.y relative to sum |x_k y_k| <= (a2 + b2) / 2), two more roundings for the sum and the difference
    (each <= U (a2 + b2) and 2 U (a2 + b2)) and one for the divide by reg (U d / reg <= 2 U (a2 + b2) / reg):
    |dt| <= (3 + 3 + 1 + 2 + 2) U (a2 + b2) / reg, K_CANCEL = 12 with the second-order terms; exp turns dt into the relative
    error expm1(|dt|).  Then EXP_ULP ulp of the device exp at K_ref, and one denormal spacing for the rounding of K_ref itself."""
    a2 = (np.asarray(X, np.float64).astype(LD) ** 2).sum(-1)[:, None]
    b2 = (np.asarray(Y, np.float64).astype(LD) ** 2).sum(-1)[None, :]
    dt = LD(K_CANCEL * U) * (a2 + b2) / LD(reg)
    return K_ref * np.expm1(dt) + LD(EXP_ULP) * np.spacing(f64(K_ref)).astype(LD) + LD(UF)


def matvec_bound(L, s):
    """Relative bound of c / s for a device sum s of L non-negative products (module docstring); inf where s is 0."""
    s = np.asarray(s, LD)
    with np.errstate(divide="ignore"):
        return LD((L + 3) * U) + LD(L * UF) / s


def col_update(K, u, m):
    """(K^T u, v' = b / K^T u) from float64 K [n][m] and u [n]; b = fl(1 / m) as the launcher forms it."""
    K, u = np.asarray(K, np.float64).astype(LD), np.asarray(u, np.float64).astype(LD)
    KtU = (K * u[:, None]).sum(0)
    with np.errstate(divide="ignore"):
        return KtU, LD(1.0 / m) / KtU


def row_update(K, v, n):
    """(K v, u' = a / K v) from float64 K and v [m]."""
    K, v = np.asarray(K, np.float64).astype(LD), np.asarray(v, np.float64).astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):       # v holds inf after a breakdown through v
        Kv = (K * v[None, :]).sum(1)
        return Kv, LD(1.0 / n) / Kv


def breakdown(KtU, v, u):
    """The three predicates of the schedule, on the values rounded to float64: which of them hold."""
    KtU, v, u = f64(KtU), f64(v), f64(u)
    return dict(zero=bool((KtU == 0).any()), v=bool(not np.isfinite(v).all()), u=bool(not np.isfinite(u).all()))


def marginal_error(K, u, v):
    """err = || v (K^T u) - b ||_2 from float64 (K, u, v), and its bound.
    r_j = v_j s_j - b with s_j = (K^T u)_j can cancel, so the bound is absolute: the device's s_j is within (n + 1) U relative
    (+ n UF absolute, products in the denormal range), the product v_j s_j and the difference add a rounding each:
        e_j = (n + 4) U (|v_j| s_j + b) + n UF |v_j|
    and | ||r_dev|| - ||r|| | <= ||e||.  Squaring, adding m terms in any order and the root are relative: (m + 4) U err; a
    square that falls into the denormal range costs sqrt(m UF) at most."""
    K, u, v = (np.asarray(a, np.float64).astype(LD) for a in (K, u, v))
    n, m = K.shape
    b = LD(1.0 / m)
    s = (K * u[:, None]).sum(0)
    r = v * s - b
    err = np.sqrt((r * r).sum())
    e = LD((n + 4) * U) * (np.abs(v) * s + b) + LD(n * UF) * np.abs(v)
    return err, np.sqrt((e * e).sum()) + LD((m + 4) * U) * err + np.sqrt(LD(m * UF))


def projection(K, u, v, Y):
    """Ybar_i = sum_j P_ij Y_j / (sum_j P_ij + 1e-32), P_ij = (u_i K_ij) v_j, from float64 operands, and its absolute bound.
    P_ij carries two roundings (2 U, or UF / 2 (|v_j| + 1) if a product is denormal); the numerator may cancel (Y of either sign):
    its error is at most (m + 3) U A_c + UFT_c with A_c = sum_j P_ij |Y_jc| and UFT_c = UF sum_j (|v_j| + 1) |Y_jc|; the
    denominator's (m + 3) U den + UF sum_j (|v_j| + 1).  With |t_c| <= A_c and one more rounding for the divide:
        |Ybar_dev - Ybar| <= (2 (m + 4) U A_c + UFT_c + UF sum_j (|v_j| + 1) A_c / den) / den."""
    K, u, v, Y = (np.asarray(a, np.float64).astype(LD) for a in (K, u, v, Y))
    m = K.shape[1]
    P = (u[:, None] * K) * v[None, :]
    den = P.sum(1) + LD(1e-32)
    ybar = (P @ Y) / den[:, None]
    A = P @ np.abs(Y)
    w = np.abs(v) + 1
    bound = (LD(2 * (m + 4) * U) * A + LD(UF) * (w @ np.abs(Y))[None, :] + LD(UF) * w.sum() * A / den[:, None]) / den[:, None]
    return ybar, bound


def final_buffer(break_iter, conv_iter, iters):
    """Which of the two (u, v) buffers the projection reads: the pair before a breakdown, else the pair after the last update."""
    if break_iter is not None and (conv_iter is None or break_iter <= conv_iter):
        return break_iter & 1
    if conv_iter is not None:
        return (conv_iter + 1) & 1
    return iters & 1


def solve(X, Y, reg, itmax, thr, K=None, upto=None):
    """The schedule of the kernels on the host: every stage in long double from float64 operands, rounded to float64.
    -> dict(break_iter, conv_iter, checks, err, errs [(ii, err, bound)], through, u, v, K, q [ln(max(v', u') / DBL_MAX) per iteration])."""
    n, m = len(X), len(Y)
    K = f64(kernel_matrix(X, Y, reg)) if K is None else K
    u, v = np.full(n, 1.0 / n), np.full(m, 1.0 / m)
    out = dict(break_iter=None, conv_iter=None, checks=0, err=np.inf, errs=[], through=None, q=[], K=K)
    for ii in range(itmax if upto is None else min(itmax, upto)):
        KtU, vn = col_update(K, u, m)
        Kv, un = row_update(K, f64(vn), n)
        with np.errstate(divide="ignore", invalid="ignore"):
            out["q"].append(float(np.log(np.nanmax(np.concatenate([vn, un])) / DBL_MAX)))
        hit = breakdown(KtU, vn, un)
        if any(hit.values()):
            out["break_iter"] = ii
            out["through"] = "zero" if hit["zero"] else ("v" if hit["v"] else "u")
            break
        u, v = f64(un), f64(vn)
        if ii % 10 == 0:
            err, bound = marginal_error(K, u, v)
            out["checks"] += 1
            out["err"] = float(err)
            out["errs"].append((ii, float(err), float(bound)))
            if f64(err) < thr:
                out["conv_iter"] = ii
                break
    out["u"], out["v"] = u, v
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """solve() of the row `name`: computed once, shared, not to be written to."""
    r = ROWS[name]
    X, Y = inputs(name)
    return solve(X, Y, r["reg"], r["itmax"], r["thr"])


def perturbed(K, how, seed=0):
    """K with every element moved by 4 float64 spacings (in the denormal range: 4 denormal spacings), not below 0:
    how = +1 / -1: all up / all down, 0: a random sign per element."""
    sign = np.random.default_rng(seed).choice([-1, 1], size=K.shape) if how == 0 else how
    bits = K.view(np.int64) + 4 * sign
    return np.maximum(bits, 0).view(np.float64)
