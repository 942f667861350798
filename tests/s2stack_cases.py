"""The NumPy statement of include/hsr_s2stack.h and the case tables of the S2 stack kernels (csrc/hsr_s2stack.hip).  No GPU, no
library; not a test module.

Every output of the family is an integer or the float32 rounding of one float64 expression of integers, so every comparison is an
equality.  The statement (stack_ref) works on integer arrays - the taps, their weights, N and Wt are int64 - and its float64
expression is written once (f64_value).  It shares nothing with the kernels: no tiles, no staging, no separable sums.

A row of ROWS is a dict: the 10 m grid, the window (row0, col0, h, w), the bands (up, method, add_offset), dtype, rule, the nodata
convention and the content of the planes.  case(name) materialises it (planes, read-only) and ref(name) is the statement's output;
layout(name) gives the strided buffers of tests/gpu_harness.py's row protocol: every plane with a row stride of W + 5, the output
with out_rs = w + 3 and a padded band stride, everything else holding the sentinel.
Sizes follow the kernel's loop bounds (the output tile TILE_H x TILE_W, a thread's eight outputs, 16-byte segments), not the
workload: nothing is larger than (TILE_H + 1) x (TILE_W + 3)."""
import functools

import numpy as np

MAX_BANDS, NEAREST, BILINEAR, STRICT, RENORM, U16, F32 = 16, 0, 1, 0, 1, 0, 1
TILE_H, TILE_W = 16, 512                                   # HSR_S2_TILE_H, HSR_S2_TILE_W (tests/test_s2stack_host.py compares)
SENT = 0xA5                                                # gpu_harness.FILL
SENT16 = 0xA5A5
GRIDS = ((17, 21), (18, 22), (TILE_H + 1, TILE_W + 3))     # odd, even, one tile boundary crossed in each direction
DTYPES = {"u16": U16, "f32": F32}
DTYPE_NAMES = {"uint16": U16, "float32": F32}             # assemble_s2_stack's out_dtype
RULES = {"strict": STRICT, "renorm": RENORM}
NP_DTYPE = {U16: np.uint16, F32: np.float32}


def all_instances():
    return ["s2_stack_kernel<U16, STRICT>", "s2_stack_kernel<U16, RENORM>", "s2_stack_kernel<F32, STRICT>", "s2_stack_kernel<F32, RENORM>",
            "s2_expand_kernel<UP1>", "s2_expand_kernel<UP2>"]


def stack_instance(dtype, rule):
    return "s2_stack_kernel<%s, %s>" % (("U16", "F32")[dtype], ("STRICT", "RENORM")[rule])


def ceil_div(a, b):
    return -(-a // b)


# ---- the statement --------------------------------------------------------------------------------------------------------------------
def f64_value(N, Wt, off, quant):
    """THE float64 expression of the float32 output: both divisions in float64, one rounding to float32."""
    return ((N.astype(np.float64) / Wt.astype(np.float64) + np.float64(off)) / np.float64(quant)).astype(np.float32)


def taps_of(up, method, Y, X, H, W):
    """The taps of the output pixels (Y[:, None], X[None, :]): a list of (row index (h,), column index (w,), weight (h, w))."""
    one = np.ones((len(Y), len(X)), dtype=np.int64)
    if up == 1:
        return [(Y, X, one)]
    if method == NEAREST:
        return [(Y >> 1, X >> 1, one)]
    i0, j0 = (Y - 1) >> 1, (X - 1) >> 1                      # floor: -1 at 0
    w1y, w1x = np.where(Y & 1, 1, 3), np.where(X & 1, 1, 3)
    rows = ((np.clip(i0, 0, H - 1), 4 - w1y), (np.clip(i0 + 1, 0, H - 1), w1y))
    cols = ((np.clip(j0, 0, W - 1), 4 - w1x), (np.clip(j0 + 1, 0, W - 1), w1x))
    return [(i, j, wy[:, None] * wx[None, :]) for i, wy in rows for j, wx in cols]


def band_ref(plane, up, method, off, window, has_nodata, nodata_in, rule, dtype, nodata_out, fill, quant):
    """-> (the (h, w) output of one band, the number of invalid outputs)."""
    row0, col0, h, w = window
    H, W = plane.shape
    Y, X = row0 + np.arange(h, dtype=np.int64), col0 + np.arange(w, dtype=np.int64)
    p = plane.astype(np.int64)
    taps = taps_of(up, method, Y, X, H, W)
    wsum = sum(wt for _, _, wt in taps)
    assert (wsum == (16 if len(taps) == 4 else 1)).all()
    lead = 9 if len(taps) == 4 else 1
    assert (sum((wt == lead).astype(int) for _, _, wt in taps) == 1).all()      # exactly one tap has the leading weight
    N, Wt = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    every, leading = np.ones((h, w), bool), np.ones((h, w), bool)
    for i, j, wt in taps:
        dn = p[i][:, j]
        valid = ~(dn == nodata_in) if has_nodata else np.ones((h, w), bool)
        every &= valid
        leading &= np.where(wt == lead, valid, True)
        use = np.ones((h, w), bool) if rule == STRICT else valid
        N += np.where(use, wt * dn, 0)
        Wt += np.where(use, wt, 0)
    ok = every if rule == STRICT else leading
    Wt = np.where(ok, Wt, 1)
    if dtype == U16:
        q = (2 * N + Wt) // (2 * Wt)
        lo, hi = (1, 65535) if nodata_out == 0 else (0, 65534)
        out = np.where(ok, np.clip(q + off, lo, hi), nodata_out).astype(np.uint16)
    else:
        out = np.where(ok, f64_value(N, Wt, off, quant), np.float32(fill)).astype(np.float32)
    return out, int((~ok).sum())


def stack_ref(planes, bands, window, has_nodata, nodata_in, rule, dtype, nodata_out, fill, quant):
    outs = [band_ref(p, up, method, off, window, has_nodata, nodata_in, rule, dtype, nodata_out, fill, quant)
            for p, (up, method, off) in zip(planes, bands)]
    return np.stack([o for o, _ in outs]), np.array([n for _, n in outs], dtype=np.int64)


def expand_ref(plane, up, window):
    row0, col0, h, w = window
    return plane[(row0 + np.arange(h)) // up][:, (col0 + np.arange(w)) // up]


# ---- strided buffers ------------------------------------------------------------------------------------------------------------------
def strided(a, rs, fill):
    H, W = a.shape
    buf = np.full((H - 1) * rs + W, fill, dtype=a.dtype)
    for y in range(H):
        buf[y * rs: y * rs + W] = a[y]
    return buf


def unstrided3(buf, nb, h, w, bs, rs):
    """-> (the (nb, h, w) payload, every other element)."""
    mask = np.ones(buf.size, bool)
    out = np.empty((nb, h, w), dtype=buf.dtype)
    for b in range(nb):
        for y in range(h):
            at = b * bs + y * rs
            out[b, y] = buf[at: at + w]
            mask[at: at + w] = False
    return out, buf[mask]


# ---- the rows -------------------------------------------------------------------------------------------------------------------------
def windows_of(H, W):
    """name -> (row0, col0, h, w): the full grid, the interior, the four origin parities, 1 x 1 at each corner, a single row and
    a single column, and a window on each edge."""
    out = {"full": (0, 0, H, W), "interior": (1, 1, H - 2, W - 2)}
    for pr in (0, 1):
        for pc in (0, 1):
            out[f"parity{pr}{pc}"] = (2 + pr, 2 + pc, 7, 9)
    out.update({"corner-tl": (0, 0, 1, 1), "corner-tr": (0, W - 1, 1, 1), "corner-bl": (H - 1, 0, 1, 1), "corner-br": (H - 1, W - 1, 1, 1),
                "one-row": (3, 0, 1, W), "one-column": (0, 4, H, 1),
                "edge-top": (0, 3, 4, 5), "edge-bottom": (H - 4, 3, 4, 5), "edge-left": (3, 0, 4, 5), "edge-right": (3, W - 5, 4, 5)})
    return out


THREE = ((1, NEAREST, 0), (2, NEAREST, 0), (2, BILINEAR, 0))          # every kind of band
BIL = ((2, BILINEAR, 0),)


def _row(grid, window, bands=THREE, dtype=U16, rule=STRICT, content=("random", 0.1), has_nodata=1, nodata_in=0, nodata_out=0,
         fill=np.nan, quant=10000.0, seed=0, src_off=0, dst_off=0, rs_pad=5, ors_pad=3, obs_pad=7, count=True):
    return dict(grid=grid, window=window, bands=tuple(bands), dtype=dtype, rule=rule, content=content, has_nodata=has_nodata,
                nodata_in=nodata_in, nodata_out=nodata_out, fill=fill, quant=quant, seed=seed, src_off=src_off, dst_off=dst_off,
                rs_pad=rs_pad, ors_pad=ors_pad, obs_pad=obs_pad, count=count)


def _rows():
    rows = {}
    n = 0
    for grid in GRIDS:
        for wname, win in windows_of(*grid).items():
            for dname, dtype in DTYPES.items():
                for rname, rule in RULES.items():
                    n += 1
                    rows[f"win-{grid[0]}x{grid[1]}-{wname}-{dname}-{rname}"] = _row(grid, win, dtype=dtype, rule=rule, seed=n, count=n % 3 != 0,
                                                                                   src_off=2 * (n % 5), dst_off=(2 + 2 * dtype) * (n % 4))
    g = GRIDS[1]
    full = (0, 0) + g
    for dname, dtype in DTYPES.items():
        for rname, rule in RULES.items():
            tag = f"{dname}-{rname}"
            for method in (NEAREST, BILINEAR):             # both dtypes x both rules x both methods at up = 2
                rows[f"up2-method{method}-{tag}"] = _row(g, full, ((2, method, 0),), dtype, rule, seed=7 + method)
            # nodata: none; one invalid source pixel at every parity (it is every tap position of some output, and the weight-9 tap
            # alone of its own four); a 2 x 2 block (all four taps of the outputs between); every corner and an edge (the duplicate
            # taps of the clamp); a border; everything
            rows[f"nodata-none-{tag}"] = _row(g, full, BIL, dtype, rule, ("random", 0.1), has_nodata=0)
            for i, j in ((4, 5), (4, 6), (5, 5), (5, 6)):
                rows[f"nodata-one-{i}-{j}-{tag}"] = _row(g, full, BIL, dtype, rule, ("holes", ((i, j),)))
            rows[f"nodata-block-{tag}"] = _row(g, full, BIL, dtype, rule, ("holes", ((6, 6), (6, 7), (7, 6), (7, 7))))
            for i, j in ((0, 0), (0, 10), (8, 0), (8, 10), (0, 5), (4, 10)):
                rows[f"nodata-clamped-{i}-{j}-{tag}"] = _row(g, full, BIL, dtype, rule, ("holes", ((i, j),)))
            rows[f"nodata-border-{tag}"] = _row(g, full, THREE, dtype, rule, ("border", 2))
            rows[f"nodata-all-{tag}"] = _row(g, full, THREE, dtype, rule, ("constant", 0))
            rows[f"nodata-65535-{tag}"] = _row(g, full, THREE, dtype, rule, ("random", 0.1), nodata_in=65535, nodata_out=65535)
            # values
            for dn in (0, 1, 65535):
                rows[f"value-{dn}-{tag}"] = _row(g, full, THREE, dtype, rule, ("constant", dn), has_nodata=0, quant=1.0)
            for nd_out in (0, 65535):                      # the BOA offset under DN < 1000: the clamp at the low end, on either side of nodata_out
                rows[f"offset-{nd_out}-{tag}"] = _row(g, full, tuple((u, m, -1000) for u, m, _ in THREE), dtype, rule, ("small", 2000), nodata_out=nd_out)
            rows[f"offset-up-{tag}"] = _row(g, full, tuple((u, m, 1000) for u, m, _ in THREE), dtype, rule, ("large", 2000), nodata_out=65535)
            rows[f"fill-{tag}"] = _row(g, full, THREE, dtype, rule, ("random", 0.2), fill=-9999.0, quant=1.0)
        # 1, 9, 10 and 16 bands in one launch
        mixed = [(1, NEAREST, 0), (1, BILINEAR, -3), (2, BILINEAR, -1000), (2, NEAREST, 5)]
        for nb in (1, 9, 10, 16):
            rows[f"bands-{nb}-{dname}"] = _row(GRIDS[0], (1, 2, 15, 18), [mixed[(b + nb) % 4] for b in range(nb)], dtype, RENORM if nb % 2 else STRICT,
                                               seed=nb)
        # rows whose strides and bases are multiples of 16 bytes: every row takes the same 16-byte path
        rows[f"aligned-{dname}"] = _row(GRIDS[2], (0, 0) + GRIDS[2], THREE, dtype, RENORM, seed=3, rs_pad=None, ors_pad=None, obs_pad=None)
        rows[f"aligned-window-{dname}"] = _row(GRIDS[2], (1, 3, 16, 512), THREE, dtype, STRICT, seed=4, rs_pad=None, ors_pad=None, obs_pad=None)
    return rows


ROWS = _rows()


def _sweep_rows(count=24, seed=2023):
    """Seeded random rows in the same form."""
    rng = np.random.default_rng(seed)
    rows = {}
    for k in range(count):
        H, W = int(rng.integers(1, 40)), int(rng.choice([int(rng.integers(1, 40)), int(rng.integers(500, 540))]))
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        win = (int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w)
        bands = [(int(rng.integers(1, 3)), int(rng.integers(0, 2)), int(rng.choice([0, -1000, 17]))) for _ in range(int(rng.integers(1, 5)))]
        rows[f"sweep-{k}"] = _row((H, W), win, bands, int(rng.integers(0, 2)), int(rng.integers(0, 2)), ("random", float(rng.choice([0.0, 0.05, 0.5]))),
                                  has_nodata=int(rng.integers(0, 2)), nodata_out=int(rng.choice([0, 65535])), fill=float(rng.choice([np.nan, -9999.0])),
                                  quant=float(rng.choice([10000.0, 1.0, 3.0])), seed=1000 + k, src_off=2 * int(rng.integers(0, 8)),
                                  dst_off=4 * int(rng.integers(0, 4)), rs_pad=int(rng.integers(0, 9)), ors_pad=int(rng.integers(0, 9)),
                                  obs_pad=int(rng.integers(0, 9)), count=bool(k % 2))
    return rows


SWEEP_ROWS = _sweep_rows()
ALL_ROWS = dict(ROWS, **SWEEP_ROWS)


def _content(kind, arg, shape, nodata, rng):
    if kind == "random":                                    # DN over the whole range with 0, 1 and 65535 frequent, nodata sprinkled
        p = rng.integers(0, 65536, size=shape)
        p = np.where(rng.random(shape) < 0.1, rng.choice([0, 1, 65535, 65534], size=shape), p)
        p = np.where(p == nodata, (nodata + 7) % 65536, p)
        return np.where(rng.random(shape) < arg, nodata, p)
    if kind == "holes":
        p = rng.integers(1, 65535, size=shape)
        for i, j in arg:
            p[i, j] = nodata
        return p
    if kind == "border":
        p = rng.integers(1, 65535, size=shape)
        keep = np.zeros(shape, bool)
        keep[arg:shape[0] - arg, arg:shape[1] - arg] = True
        return np.where(keep, p, nodata)
    if kind == "constant":
        return np.full(shape, arg)
    if kind == "small":
        return rng.integers(1, arg, size=shape)
    if kind == "large":
        return rng.integers(65536 - arg, 65536, size=shape)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> the list of the row's planes, uint16 and read-only.  A 20 m `holes` / `border` plane is built at 20 m; the 10 m plane of a
    row gets the same content kind on its own grid."""
    r = ALL_ROWS[name]
    H10, W10 = r["grid"]
    rng = np.random.default_rng(r["seed"])
    planes = []
    for up, _, _ in r["bands"]:
        shape = (ceil_div(H10, up), ceil_div(W10, up))
        p = _content(r["content"][0], r["content"][1], shape, r["nodata_in"], rng).astype(np.uint16)
        p.setflags(write=False)
        planes.append(p)
    return planes


@functools.lru_cache(maxsize=None)
def ref(name):
    r = ALL_ROWS[name]
    out, invalid = stack_ref(case(name), r["bands"], r["window"], r["has_nodata"], r["nodata_in"], r["rule"], r["dtype"], r["nodata_out"],
                             r["fill"], r["quant"])
    out.setflags(write=False)
    return out, invalid


def strides_of(name):
    """-> ([rs of every plane], out_rs, out_bs): a pad of None rounds the stride up to a multiple of 16 bytes instead."""
    r = ALL_ROWS[name]
    H10, W10 = r["grid"]
    _, _, h, w = r["window"]
    up8 = lambda n: ceil_div(n, 8) * 8  # noqa: E731
    rs = [up8(ceil_div(W10, up)) if r["rs_pad"] is None else ceil_div(W10, up) + r["rs_pad"] for up, _, _ in r["bands"]]
    ors = up8(w) if r["ors_pad"] is None else w + r["ors_pad"]
    obs = up8((h - 1) * ors + w) if r["obs_pad"] is None else (h - 1) * ors + w + r["obs_pad"]
    return rs, ors, obs


def layout(name):
    """The flat buffers of a row: [(strided plane, byte offset)], the output's element count, byte offset and dtype."""
    r = ALL_ROWS[name]
    rs, ors, obs = strides_of(name)
    _, _, h, w = r["window"]
    nb = len(r["bands"])
    srcs = [(strided(p, s, SENT16 if r["nodata_in"] != SENT16 else 0), r["src_off"]) for p, s in zip(case(name), rs)]
    return srcs, (nb - 1) * obs + (h - 1) * ors + w, r["dst_off"], NP_DTYPE[r["dtype"]]


def band_table(S2Band, name, pointers):
    """The hsr_s2_band array of a row for planes at `pointers`."""
    r = ALL_ROWS[name]
    rs, _, _ = strides_of(name)
    table = (S2Band * len(pointers))()
    for e, ptr, s, p, (up, method, off) in zip(table, pointers, rs, case(name), r["bands"]):
        e.plane_dev, e.rs, e.H, e.W, e.up, e.method, e.add_offset, e.reserved = ptr, s, p.shape[0], p.shape[1], up, method, off, 0
    return table


def stack_args(name, table, out_ptr, invalid_ptr):
    """The arguments of hsr_s2_stack / hsr_s2_stack_host between the table and the stream."""
    import ctypes as C
    r = ALL_ROWS[name]
    _, ors, obs = strides_of(name)
    row0, col0, h, w = r["window"]
    return (table, len(r["bands"]), r["grid"][0], r["grid"][1], row0, col0, h, w, r["has_nodata"], r["nodata_in"], r["rule"], r["dtype"], out_ptr,
            obs, ors, r["nodata_out"], C.c_float(r["fill"]), C.c_double(r["quant"]), invalid_ptr)


def check_output(name, flat, invalid):
    """The row's output buffer (flat, in the output dtype) and counts (None: not asked for) against the statement."""
    r = ALL_ROWS[name]
    _, ors, obs = strides_of(name)
    _, _, h, w = r["window"]
    want, want_invalid = ref(name)
    got, gaps = unstrided3(flat, len(r["bands"]), h, w, obs, ors)
    assert (gaps.view(np.uint8) == SENT).all(), f"{name}: an element between the rows or bands was written"
    iv = np.uint16 if r["dtype"] == U16 else np.uint32
    nan = np.isnan(want) if r["dtype"] == F32 else np.zeros(want.shape, bool)
    if r["dtype"] == F32:
        assert np.array_equal(np.isnan(got), nan), f"{name}: NaN positions differ"
    bad = (got.view(iv) != want.view(iv)) & ~nan
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0]}: {got[bad][:4]} vs {want[bad][:4]}"
    if invalid is not None:
        assert np.array_equal(invalid, want_invalid), (name, invalid, want_invalid)


# ---- the byte plane under the window --------------------------------------------------------------------------------------------------
def _expand_rows():
    rows = {}
    n = 0
    for grid in GRIDS:
        for wname, win in windows_of(*grid).items():
            for up in (1, 2):
                n += 1
                rows[f"expand-{grid[0]}x{grid[1]}-{wname}-up{up}"] = dict(grid=grid, window=win, up=up, rs_pad=n % 4, ors_pad=3 * (n % 2), src_off=n % 3,
                                                                          dst_off=n % 16)
    for up in (1, 2):                                       # rows of whole 16-byte segments
        rows[f"expand-aligned-up{up}"] = dict(grid=GRIDS[2], window=(0, 0) + GRIDS[2], up=up, rs_pad=None, ors_pad=None, src_off=0, dst_off=0)
    return rows


EXPAND_ROWS = _expand_rows()


@functools.lru_cache(maxsize=None)
def expand_case(name):
    r = EXPAND_ROWS[name]
    H, W = ceil_div(r["grid"][0], r["up"]), ceil_div(r["grid"][1], r["up"])
    p = np.random.default_rng(len(name)).integers(0, 12, size=(H, W)).astype(np.uint8)
    p.setflags(write=False)
    rs = ceil_div(W, 16) * 16 if r["rs_pad"] is None else W + r["rs_pad"]
    ors = ceil_div(r["window"][3], 16) * 16 if r["ors_pad"] is None else r["window"][3] + r["ors_pad"]
    return p, rs, ors, expand_ref(p, r["up"], r["window"])
