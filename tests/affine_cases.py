"""The case table of the affine colour kernels (csrc/hsr_color.hip, include/hsr_color.h) and their references.  No GPU; the
library only where a test hands it in.

  * MOMENT_ROWS / APPLY_ROWS / SOLVE_ROWS: which sizes, layouts, alignments, masks, stretches and inputs reach which loop bound
    and which kernel instance.  mode() / moments_instance() / apply_instance() mirror the host-side predicate of the entry
    points; slots() / slot_rows() mirror the slot geometry.  A row is named by the bound it sits at.
  * The references: the 22 moments in np.longdouble with sum |term| for the bar, np.linalg.lstsq on the same float64 rows, and
    the apply restated elementwise in float64 in the order include/hsr_color.h states.

Bars (derived, not measured):
  moments  |dev - ref| <= (n + 2) EPS sum|term|, n the counted rows: the first-order bound of ANY summation order of n terms
           plus the product roundings.  G33, the count, is exact.
  solve    the largest difference between the fitted map and np.linalg.lstsq's over the 9 x 9 x 9 grid of [0, 1]^3 is at most
           64 kappa EPS max(1, max|W|), kappa = largest / smallest KEPT eigenvalue of the row's Gram.
  apply    bit-equal to apply_ref.

Worst ratio diff / (kappa EPS max(1, max|W|)) per solve row - the bar is 64.  host: hsr_affine_solve_host on long-double moments
(tests/test_affine_host.py prints it with -s); device: hsr_affine_moments_f64 + hsr_affine_reduce_solve on an MI355X
(tests/test_gpu_color_instances.py prints it):
                    host    device                         host    device
  full-5000         0.22    0.15       count-2             0.18    0.18
  equal-channels    0.33    0.27       count-3             0.29    0.29
  gray              0.45    0.56       at-min-count        0.27    0.30
  constant         31.0    31.0        narrow              0.14    0.27
  count-1           2.0     2.0        below-min-count, count-0: the identity, exact
The 31 of the constant row is np.linalg.lstsq's own distance from the exact minimum-norm solution (W = z ybar^T / |z|^2 in long
double); the solve is 1 EPS from it.
"""
import functools

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
NMOM = 22
SLOT_PIXELS, MAX_SLOTS = 2048, 512           # HSR_AFFINE_SLOT_PIXELS, HSR_AFFINE_MAX_SLOTS
GROUP, THREADS = 4, 256                      # pixels a thread takes per pass; threads of a workgroup
PASS = GROUP * THREADS                       # pixels a workgroup takes per pass
PACKED, PADDED, PLANAR = "packed", "padded", "planar"
PLANAR_GAP = 5                               # a planar test image has band stride npix + PLANAR_GAP
PAD_IN = 7.5                                 # the fourth float of a padded INPUT row: never read into a result
TRI = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]


# ---------------------------------------------------------------------------------------------------------------------------
# mirror of the host-side predicate and the slot geometry
# ---------------------------------------------------------------------------------------------------------------------------
def slots(npix):
    return min(max((npix + SLOT_PIXELS - 1) // SLOT_PIXELS, 1), MAX_SLOTS)


def slot_rows(npix, nslots):
    per = (npix + nslots - 1) // nslots
    return (per + 3) // 4 * 4


def mode(layout, off):
    """0 dword, 1 one 16-byte access per padded row, 2 three per four packed rows; `off` = bytes past a 16-byte boundary."""
    if layout == PLANAR or off % 16:
        return 0
    return 1 if layout == PADDED else 2


def strides(layout, npix):
    """(band stride, pixel stride, floats of the buffer)"""
    if layout == PACKED:
        return 1, 3, 3 * npix
    if layout == PADDED:
        return 1, 4, 4 * npix
    return npix + PLANAR_GAP, 1, 3 * (npix + PLANAR_GAP)


def moments_instance(r):
    return f"affine_moments_kernel<{mode(r['x'][0], r['x'][1])}, {mode(r['y'][0], r['y'][1])}>"


def apply_instance(r):
    return f"affine_apply_kernel<{mode(r['x'][0], r['x'][1])}, {mode(r['out'][0], r['out'][1])}>"


def all_instances():
    return ([f"affine_moments_kernel<{a}, {b}>" for a in range(3) for b in range(3)] + ["affine_moments_f64_kernel", "affine_reduce_solve_kernel"]
            + [f"affine_apply_kernel<{a}, {b}>" for a in range(3) for b in range(3)])


def pack(rows, layout, fill=PAD_IN):
    """(npix, 3) float32 -> the flat float32 buffer of the layout; pads and gaps hold `fill`."""
    rows = np.ascontiguousarray(rows, np.float32)
    npix = rows.shape[0]
    if layout == PACKED:
        return rows.reshape(-1).copy()
    if layout == PADDED:
        out = np.full((npix, 4), fill, np.float32)
        out[:, :3] = rows
        return out.reshape(-1)
    out = np.full((3, npix + PLANAR_GAP), fill, np.float32)
    out[:, :npix] = rows.T
    return out.reshape(-1)


def unpack(flat, layout, npix):
    """The flat float32 buffer of the layout -> ((npix, 3) rows, the floats beside them: pads or gaps, or None)."""
    flat = np.asarray(flat, np.float32)
    if layout == PACKED:
        return flat.reshape(npix, 3), None
    if layout == PADDED:
        a = flat.reshape(npix, 4)
        return a[:, :3], a[:, 3]
    a = flat.reshape(3, npix + PLANAR_GAP)
    return a[:, :npix].T, a[:, npix:]


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
def stretch(v, lohi):
    """float32(clip((v - lo) / (hi - lo + 1e-12), 0, 1)) in float64, per channel (s2_emit/color.py:33); lohi (3, 2) or None."""
    v = np.asarray(v, np.float32)
    if lohi is None:
        return v
    lohi = np.asarray(lohi, np.float64)
    with np.errstate(invalid="ignore"):
        r = (v.astype(np.float64) - lohi[:, 0]) / (lohi[:, 1] - lohi[:, 0] + 1e-12)
        return np.clip(r, 0.0, 1.0).astype(np.float32)


def usable(x, y, mask):
    ok = np.isfinite(x).all(axis=1) & np.isfinite(y).all(axis=1)
    return ok if mask is None else ok & (np.asarray(mask) != 0)


def moments_ld(xs, ys):
    """The 22 moments of the float64 rows xs, ys (n, 3) summed in long double, and sum |term| per moment."""
    z = np.concatenate([np.asarray(xs, np.float64), np.ones((len(xs), 1))], axis=1).astype(LD)
    y = np.asarray(ys, np.float64).astype(LD)
    terms = [z[:, i] * z[:, j] for i, j in TRI] + [z[:, i] * y[:, c] for i in range(4) for c in range(3)]
    return (np.array([t.sum(dtype=LD) for t in terms], LD), np.array([np.abs(t).sum(dtype=LD) for t in terms], LD))


def moments_bar(n, mag):
    return (n + 2) * EPS * np.asarray(mag, np.float64)


def gram_of(mom):
    g = np.zeros((4, 4), np.asarray(mom).dtype)
    for k, (i, j) in enumerate(TRI):
        g[i, j] = g[j, i] = mom[k]
    return g


def lstsq_ref(xs, ys, min_count):
    """np.linalg.lstsq([xs 1], ys, rcond=None) -> W (4, 3): A = W[:3], t = W[3]; the identity below min_count (or without rows)."""
    xs, ys = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    if len(xs) < max(min_count, 1):
        return np.concatenate([np.eye(3), np.zeros((1, 3))])
    W, *_ = np.linalg.lstsq(np.concatenate([xs, np.ones((len(xs), 1))], axis=1), ys, rcond=None)
    return W


GRID = np.stack(np.meshgrid(*[np.linspace(0.0, 1.0, 9)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)


def grid_diff(W1, W2):
    """The largest difference of the maps x -> x A + t over the 9 x 9 x 9 grid of [0, 1]^3; W (4, 3) or At (12,)."""
    W1, W2 = np.asarray(W1, np.float64).reshape(4, 3), np.asarray(W2, np.float64).reshape(4, 3)
    return float(np.abs((GRID @ W1[:3] + W1[3]) - (GRID @ W2[:3] + W2[3])).max())


def spectrum(xs):
    """Eigenvalues of the long-double Gram of the rows (rounded to float64, as the kernels hold it), ascending."""
    mom, _ = moments_ld(xs, np.zeros((len(xs), 3)))
    return np.linalg.eigvalsh(gram_of(mom[:10].astype(np.float64)))


def kept(ev, count):
    """lstsq's cut on the eigenvalues of the Gram: above (EPS max(count, 4))^2 of the largest - floored at 4 EPS."""
    return ev[ev > max((EPS * max(count, 4)) ** 2, 4 * EPS) * ev.max()] if ev.max() > 0 else ev[:0]


def solve_bar(xs, W):
    ev = spectrum(xs)
    k = kept(ev, len(xs))
    kappa = float(k.max() / k.min()) if len(k) else 1.0
    return 64.0 * kappa * EPS * max(1.0, float(np.abs(W).max())), kappa


def apply_ref(x, At, mask, lohi, clip_mode):
    """The apply, elementwise in float64, in the order include/hsr_color.h states: o_c = ((v0 A0c + v1 A1c) + v2 A2c) + tc."""
    v = stretch(x, lohi)
    At = np.asarray(At, np.float64)
    A, t = At[:9].reshape(3, 3), At[9:]
    vd = v.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        o = np.stack([((vd[:, 0] * A[0, c] + vd[:, 1] * A[1, c]) + vd[:, 2] * A[2, c]) + t[c] for c in range(3)], axis=1)
        if clip_mode:
            o = np.clip(o, 0.0, 1.0)
        o = o.astype(np.float32)
        m = np.ones(len(v), bool) if mask is None else np.asarray(mask) != 0
        out = np.where(m[:, None], o, np.clip(v, np.float32(0), np.float32(1)) if clip_mode == 2 else v)
    return out.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def image_pair(npix, seed):
    """float32 rows with values outside [0, 1]: x, and y an affine image of x with noise."""
    rng = np.random.default_rng(seed)
    x = (rng.random((npix, 3)) * 1.3 - 0.15).astype(np.float32)
    M = np.array([[0.8, 0.1, -0.05], [0.15, 0.7, 0.1], [-0.1, 0.2, 0.9]])
    y = (x.astype(np.float64) @ M + [0.03, -0.02, 0.05] + 0.02 * rng.standard_normal((npix, 3))).astype(np.float32)
    return x, y


def poison(x, y, bad, seed):
    """Rows invalid through x only, through y only or both, by NaN, +inf and -inf; every other row stays."""
    rng = np.random.default_rng(seed + 1000)
    n = len(x)
    vals = [np.nan, np.inf, -np.inf]
    if bad in ("x", "both"):
        for k, i in enumerate(rng.choice(n, size=min(n, 5), replace=False)):
            x[i, k % 3] = vals[k % 3]
    if bad in ("y", "both"):
        for k, i in enumerate(rng.choice(n, size=min(n, 5), replace=False)):
            y[i, (k + 1) % 3] = vals[(k + 1) % 3]


def make_mask(npix, kind, seed):
    if kind == "none":
        return None
    if kind == "all":
        return np.full(npix, 255, np.uint8)
    if kind == "clear":
        return np.zeros(npix, np.uint8)
    m = (np.random.default_rng(seed + 2000).random(npix) < 0.85).astype(np.uint8)
    m[m != 0] = np.random.default_rng(seed + 2001).integers(1, 256, int(m.sum()))      # any non-zero byte counts
    return m


LOHI_PLAIN = np.array([[0.05, 0.9], [0.1, 1.05], [-0.05, 0.8]])
LOHI_Y = np.array([[0.0, 0.95], [0.08, 0.9], [0.02, 1.1]])
LOHI_FLAT = np.array([[0.05, 0.9], [0.4, 0.4], [-0.05, 0.8]])         # hi == lo in channel 1: the 1e-12 decides


def _mrow(npix, x=(PACKED, 0), y=(PADDED, 0), mask="part", bad="both", lohi_x=None, lohi_y=None):
    return dict(npix=npix, x=x, y=y, mask=mask, bad=bad, lohi_x=lohi_x, lohi_y=lohi_y)


MOMENT_ROWS = {
    "one-pixel": _mrow(1, mask="all", bad="none"),
    "group-below": _mrow(GROUP - 1), "group-exact": _mrow(GROUP), "group-above": _mrow(GROUP + 1),
    "pass-below": _mrow(PASS - 1), "pass-exact": _mrow(PASS, x=(PADDED, 0), y=(PACKED, 0)), "pass-above": _mrow(PASS + 1),
    "slot-below": _mrow(SLOT_PIXELS - 1, x=(PADDED, 0), y=(PACKED, 0)), "slot-exact": _mrow(SLOT_PIXELS),
    "slot-above": _mrow(SLOT_PIXELS + 1),
    "slots-3-ragged": _mrow(2 * SLOT_PIXELS + 1, x=(PACKED, 0), y=(PACKED, 0)),
    "slots-33-ragged": _mrow(66001, x=(PADDED, 0), y=(PADDED, 0)),
    "mask-none": _mrow(1500, mask="none"), "mask-all": _mrow(1500, mask="all"), "mask-clear": _mrow(1500, mask="clear"),
    "bad-x-only": _mrow(1500, bad="x"), "bad-y-only": _mrow(1500, bad="y"), "bad-none": _mrow(1500, bad="none"),
    "stretch-both": _mrow(2500, lohi_x=LOHI_PLAIN, lohi_y=LOHI_Y), "stretch-x-flat": _mrow(2500, lohi_x=LOHI_FLAT),
    "stretch-y": _mrow(2500, lohi_y=LOHI_Y),
}
for _lx, _x in ((1, (PADDED, 0)), (2, (PACKED, 0)), (0, (PLANAR, 0))):
    for _ly, _y in ((1, (PADDED, 0)), (2, (PACKED, 0)), (0, (PLANAR, 0))):
        MOMENT_ROWS[f"layout-{_x[0]}-{_y[0]}"] = _mrow(PASS + 7, x=_x, y=_y, lohi_x=LOHI_PLAIN)
for _l in (PADDED, PACKED, PLANAR):
    MOMENT_ROWS[f"off4-x-{_l}"] = _mrow(PASS + 7, x=(_l, 4), y=(PADDED, 0))
    MOMENT_ROWS[f"off4-y-{_l}"] = _mrow(PASS + 7, x=(PACKED, 0), y=(_l, 4))
MOMENT_ROWS["off8-both"] = _mrow(PASS + 7, x=(PACKED, 8), y=(PADDED, 8))


moment_row = _mrow                           # the pure constructor, under the name the sweeps use


@functools.lru_cache(maxsize=None)
def moment_case(name):
    return moment_case_of(MOMENT_ROWS[name], sorted(MOMENT_ROWS).index(name))


def moment_case_of(r, seed):
    """The images, the mask and the long-double moments of the moment row `r`; `seed` picks the images, the poisoned samples and
    the mask (a table row's is its place among the sorted names)."""
    x, y = image_pair(r["npix"], seed)
    poison(x, y, r["bad"], seed)
    mask = make_mask(r["npix"], r["mask"], seed)
    ok = usable(x, y, mask)
    xs, ys = stretch(x, r["lohi_x"])[ok], stretch(y, r["lohi_y"])[ok]
    ref, mag = moments_ld(xs, ys)
    return dict(x=x, y=y, mask=mask, ok=ok, xs=xs, ys=ys, ref=ref, mag=mag, n=int(ok.sum()))


# ---- apply ----------------------------------------------------------------------------------------------------------------
AT_PLAIN = np.array([0.8, 0.1, -0.05, 0.15, 0.7, 0.1, -0.1, 0.2, 0.9, 0.03, -0.02, 0.05])
AT_ZEROS = np.array([1.2, 0.0, 0.3, 0.0, 0.9, 0.0, -0.4, 0.0, 1.1, 0.0, 0.1, -0.3])    # zero entries: inf * 0 = NaN
AT_WIDE = np.array([2.5, -1.5, 0.2, -1.0, 2.0, 0.3, 0.1, 0.4, -2.0, -0.4, 0.2, 1.3])    # results below 0 and above 1


def _arow(npix, x=(PACKED, 0), out=(PACKED, 0), mask="part", clip=1, lohi=None, At=AT_PLAIN, bad=False):
    return dict(npix=npix, x=x, out=out, mask=mask, clip=clip, lohi=lohi, At=At, bad=bad)


APPLY_ROWS = {
    "one-pixel": _arow(1, mask="all"),
    "group-below": _arow(GROUP - 1), "group-exact": _arow(GROUP), "group-above": _arow(GROUP + 1),
    "pass-below": _arow(PASS - 1), "pass-exact": _arow(PASS, x=(PADDED, 0), out=(PADDED, 0)), "pass-above": _arow(PASS + 1),
    "blocks-3-ragged": _arow(2 * PASS + 3, At=AT_WIDE),
    "blocks-65": _arow(66001, x=(PADDED, 0), out=(PACKED, 0), At=AT_WIDE, bad=True),
    "mask-none-clip0": _arow(1500, mask="none", clip=0, At=AT_WIDE), "mask-none-clip1": _arow(1500, mask="none", At=AT_WIDE),
    "mask-none-clip2": _arow(1500, mask="none", clip=2, At=AT_WIDE),
    "mask-part-clip0": _arow(1500, clip=0, At=AT_WIDE, bad=True), "mask-part-clip1": _arow(1500, At=AT_WIDE, bad=True),
    "mask-part-clip2": _arow(1500, clip=2, At=AT_WIDE, bad=True),
    "mask-clear-clip2": _arow(1500, mask="clear", clip=2),
    "stretch-clip2": _arow(2500, clip=2, lohi=LOHI_PLAIN, x=(PADDED, 0), out=(PADDED, 0), bad=True),
    "stretch-flat-clip1": _arow(2500, lohi=LOHI_FLAT, bad=True),
    "zeros-vs-inf-nan": _arow(1500, mask="all", clip=1, At=AT_ZEROS, bad=True),
    "zeros-vs-inf-nan-clip0": _arow(1500, mask="all", clip=0, At=AT_ZEROS, bad=True),
}
for _li, _x in ((1, (PADDED, 0)), (2, (PACKED, 0)), (0, (PLANAR, 0))):
    for _lo, _o in ((1, (PADDED, 0)), (2, (PACKED, 0)), (0, (PLANAR, 0))):
        APPLY_ROWS[f"layout-{_x[0]}-{_o[0]}"] = _arow(PASS + 7, x=_x, out=_o, At=AT_WIDE, bad=True)
for _l in (PADDED, PACKED, PLANAR):
    APPLY_ROWS[f"off4-x-{_l}"] = _arow(PASS + 7, x=(_l, 4), out=(PADDED, 0), bad=True)
    APPLY_ROWS[f"off4-out-{_l}"] = _arow(PASS + 7, x=(PACKED, 0), out=(_l, 4), bad=True)
APPLY_ROWS["off12-both"] = _arow(PASS + 7, x=(PADDED, 12), out=(PACKED, 12), clip=2, bad=True)


apply_row = _arow


@functools.lru_cache(maxsize=None)
def apply_case(name):
    return apply_case_of(APPLY_ROWS[name], 100 + sorted(APPLY_ROWS).index(name))


def apply_case_of(r, seed):
    x, y = image_pair(r["npix"], seed)
    if r["bad"]:
        poison(x, y, "x", seed)
    mask = make_mask(r["npix"], r["mask"], seed)
    return dict(x=x, mask=mask, ref=apply_ref(x, r["At"], mask, r["lohi"], r["clip"]))


# ---- solve ----------------------------------------------------------------------------------------------------------------
MIN_COUNT = 200


def _solve_inputs(kind, n, seed):
    rng = np.random.default_rng(seed)
    x, y = image_pair(max(n, 1), seed)
    x, y = x[:n], y[:n]
    if kind == "equal-channels":
        x[:, 1] = x[:, 0]
    elif kind == "gray":
        x[:, 1] = x[:, 0]
        x[:, 2] = x[:, 0]
    elif kind == "constant":
        x[:] = np.float32([0.3, 0.55, 0.7])
    elif kind == "narrow":
        x[:] = (0.79 + 0.02 * rng.random((n, 3))).astype(np.float32)
    return x.astype(np.float64), y.astype(np.float64)


def _srow(kind, n, rank, min_count=0):
    return dict(kind=kind, n=n, rank=rank, min_count=min_count)


SOLVE_ROWS = {
    "full-5000": _srow("full", 5000, 4),
    "equal-channels": _srow("equal-channels", 3000, 3),
    "gray": _srow("gray", 3000, 2),
    "constant": _srow("constant", 3000, 1),
    "count-1": _srow("full", 1, 1), "count-2": _srow("full", 2, 2), "count-3": _srow("full", 3, 3),
    "below-min-count": _srow("full", MIN_COUNT - 1, 4, MIN_COUNT),
    "at-min-count": _srow("full", MIN_COUNT, 4, MIN_COUNT),
    "count-0": _srow("full", 0, 0, 1),
    "narrow": _srow("narrow", 4000, 4),
}


solve_row = _srow


@functools.lru_cache(maxsize=None)
def solve_case(name):
    return solve_case_of(SOLVE_ROWS[name], 300 + sorted(SOLVE_ROWS).index(name))


def solve_case_of(r, seed):
    xs, ys = _solve_inputs(r["kind"], r["n"], seed)
    W = lstsq_ref(xs, ys, r["min_count"])
    identity = r["n"] < max(r["min_count"], 1)
    bar, kappa = (0.0, 1.0) if identity else solve_bar(xs, W)
    mom, mag = moments_ld(xs, ys)
    return dict(xs=xs, ys=ys, W=W, identity=identity, bar=bar, kappa=kappa, mom=mom, mag=mag)
