"""The NumPy statement of include/hsr_hist.h, its key function and the case tables of the histogram-matching tests
(test_hist_host.py on the CPU; test_gpu_hist_instances.py, test_gpu_hist.py, test_gpu_hist_capture.py on the GPU).  NumPy only;
not a test module.

The statement is the header's, on values: sorted valid samples S and R, the integer ranks cs, hi, lo, one float64 expression.  It
is written on the values of the input's own dtype, so that it also runs on the float64 images of fixture g8; on float32 it is what
the library computes.  key_of is the header's key, tested against the order of the values in test_hist_host.py."""
import functools
import zlib

import numpy as np

TILE, PIVOT, SCAN_STEP, BITS, MAX_CHANNELS = 8192, 256, 4096, 8, 16
SENTINEL = np.uint32(0xFFFFFFFF)
BINS = 1 << BITS
FLT_MAX = np.finfo(np.float32).max
DENORM = np.float32(1e-45)


# ---- the key ------------------------------------------------------------------------------------------------------------------------------
def key_of(x):
    """uint32 key of float32 values: -0.0 as +0.0; sign bit set for >= 0, all bits inverted for < 0; the sentinel for non-finite."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).copy()
    u[u == 0x80000000] = 0
    k = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[~np.isfinite(x)] = SENTINEL
    return k


def value_of(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k & 0x80000000, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


# ---- the statement -------------------------------------------------------------------------------------------------------------------------
def valid_of(src, ref, mask):
    return np.asarray(mask, bool) & np.isfinite(src) & np.isfinite(ref)


def lookup_values(S, R, v):
    """The definition for the values v given the ascending valid samples S and R (both of length n >= 1): float64."""
    n = np.float64(len(S))
    Rd = R.astype(np.float64)
    cs = np.searchsorted(S, v, side="right")
    a = R[cs - 1]
    hi, lo = np.searchsorted(R, a, side="right"), np.searchsorted(R, a, side="left")
    plain = (hi == cs) | (lo == 0)
    b = Rd[np.maximum(lo, 1) - 1]
    ad = a.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        res = ((ad - b) / (hi / n - lo / n)) * (cs / n - lo / n) + b
    return np.where(plain, ad, res)


def match_channel(src, ref, mask):
    """One channel, any shape: -> (out in src's dtype, n)."""
    src, ref = np.asarray(src), np.asarray(ref)
    valid = valid_of(src, ref, mask)
    n = int(valid.sum())
    with np.errstate(invalid="ignore"):
        out = np.clip(src, 0, 1)                          # NaN stays NaN
    if n:
        S, R = np.sort(src[valid] + src.dtype.type(0)), np.sort(ref[valid] + ref.dtype.type(0))       # + 0: -0.0 becomes +0.0
        out[valid] = np.clip(lookup_values(S, R, src[valid]).astype(src.dtype), 0, 1)
    return out, n


def match_hwc(src, ref, mask, channels=3):
    """(H, W, C) images: the first `channels` matched, the others clipped -> (out, counts)."""
    with np.errstate(invalid="ignore"):
        out = np.clip(src, 0, 1)
    counts = []
    for c in range(channels):
        out[..., c], n = match_channel(src[..., c], ref[..., c], mask)
        counts.append(n)
    return out, np.array(counts, np.int64)


def match_planes(src, ref, mask):
    """(C, ...) planes under one mask -> (out, counts)."""
    outs, counts = zip(*(match_channel(s, r, mask) for s, r in zip(src, ref)))
    return np.stack(outs), np.array(counts, np.int64)


def equal_by_value(got, want, what=""):
    """The same shape and dtype, NaN at the same places, every other element equal by value (-0 == +0)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN at different places"
    bad = (got != want) & ~gn
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first {got[bad][:4]} vs {want[bad][:4]}"


# ---- the images of fixture g19 and of the end-to-end tests ----------------------------------------------------------------------------------
H, W = 36, 32


def _mask(rng, share):
    m = rng.random((H, W)) < share
    return m


def _image_case(name):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    src = rng.random((H, W, 3)).astype(np.float32)
    ref = (rng.random((H, W, 3)) ** 2).astype(np.float32)
    mask = np.ones((H, W), bool)
    if name == "continuous":
        pass
    elif name == "ref-8bit":
        ref = (rng.integers(0, 256, (H, W, 3)).astype(np.float32) / np.float32(255)).astype(np.float32)
        mask = _mask(rng, 0.85)
    elif name == "both-quantised":
        src = (np.round(src * 40) / 40).astype(np.float32)
        ref = (np.round(ref * 50) / 50).astype(np.float32)
        mask = _mask(rng, 0.85)
    elif name == "src-constant-channel":
        src[..., 1] = np.float32(0.25)
        mask = _mask(rng, 0.85)
    elif name == "ref-constant-channel":
        ref[..., 2] = np.float32(0.75)
        ref[..., 0] = (np.round(ref[..., 0] * 6) / 6).astype(np.float32)
    elif name == "outside-0-1":
        src = (src * 3 - 1).astype(np.float32)
        ref = (ref * 2.5 - 0.75).astype(np.float32)
        src[0, 0, 0], ref[0, 1, 1] = np.float32(-0.0), np.float32(-0.0)
        mask = _mask(rng, 0.85)
    elif name == "mask-5-percent":
        ref = (np.round(ref * 20) / 20).astype(np.float32)
        mask = _mask(rng, 0.05)
    elif name == "one-masked-pixel":
        mask = np.zeros((H, W), bool)
        mask[H // 2, W // 3] = True
    else:
        raise KeyError(name)
    return src, ref, mask


IMAGE_CASES = ("continuous", "ref-8bit", "both-quantised", "src-constant-channel", "ref-constant-channel", "outside-0-1", "mask-5-percent",
               "one-masked-pixel")


@functools.lru_cache(maxsize=None)
def image_case(name):
    """(src, ref (H, W, 3) float32, mask (H, W) bool) of a row of fixture g19; read-only."""
    out = _image_case(name)
    for a in out:
        a.setflags(write=False)
    return out


def input_crc(name):
    return zlib.crc32(b"".join(np.ascontiguousarray(a).tobytes() for a in image_case(name)))


# ---- rows with non-finite samples (not in g19: what np.unique does with NaN is not claimed) -----------------------------------------------
@functools.lru_cache(maxsize=None)
def nonfinite_case():
    rng = np.random.default_rng(1919)
    src = rng.random((H, W, 3)).astype(np.float32)
    ref = (np.round(rng.random((H, W, 3)) * 30) / 30).astype(np.float32)
    mask = rng.random((H, W)) < 0.7
    src[1, 2, 0], src[3, 4, 1], src[5, 6, 2], src[7, 7, 0] = np.nan, np.inf, -np.inf, np.nan
    ref[2, 2, 0], ref[3, 5, 1], ref[5, 7, 2] = np.nan, -np.inf, np.inf
    mask[1, 2] = mask[3, 4] = mask[5, 6] = mask[2, 2] = mask[3, 5] = True
    mask[7, 7] = mask[5, 7] = False
    for a in (src, ref, mask):
        a.setflags(write=False)
    return src, ref, mask


# ---- the sort's tables ----------------------------------------------------------------------------------------------------------------------
SCAN_SECOND_STEP = (SCAN_STEP // BINS) * TILE + 1        # the smallest npix with 256 * tiles > 4096 counters: 17 tiles
SORT_NPIX = (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, SCAN_SECOND_STEP)
SORT_PATTERNS = ("equal", "two-alternating", "ascending", "descending", "digit-0", "digit-1", "digit-2", "digit-3", "random-finite", "specials")
SENTINEL_SHARES = ("none", "half", "all-but-one", "all")


def sort_keys(pattern, npix, plane, share):
    """(npix,) uint32 keys of one plane."""
    rng = np.random.default_rng(zlib.crc32(f"{pattern}/{npix}/{plane}/{share}".encode()))
    i = np.arange(npix, dtype=np.uint64)
    if pattern == "equal":
        k = np.full(npix, 0xBF000000 + plane, np.uint32)
    elif pattern == "two-alternating":
        k = np.where(i % 2 == 0, np.uint32(0xC0000001), np.uint32(0x3FFFFF00 + plane)).astype(np.uint32)
    elif pattern == "ascending":
        k = (np.uint64(0x00800000) + i * np.uint64(max(1, (0xFF000000 - 0x00800000) // max(npix, 1)))).astype(np.uint32)
    elif pattern == "descending":
        k = (np.uint64(0xFF000000) - i * np.uint64(max(1, (0xFF000000 - 0x00800000) // max(npix, 1)))).astype(np.uint32)
    elif pattern.startswith("digit-"):
        d = int(pattern[-1])
        k = (np.uint32(0x81818181) & ~np.uint32(0xFF << (8 * d))) | (rng.integers(0, 255 if d == 3 else 256, npix).astype(np.uint32) << np.uint32(8 * d))
        k = k.astype(np.uint32)
    elif pattern == "random-finite":
        k = key_of(rng.integers(0, 1 << 32, npix, dtype=np.uint64).astype(np.uint32).view(np.float32))
        k[k == SENTINEL] = np.uint32(0x80000000)         # a non-finite pattern: zero instead
    elif pattern == "specials":
        vals = np.array([0.0, -0.0, DENORM, -DENORM, FLT_MAX, -FLT_MAX, 1.0, -1.0, np.float32(1.17549435e-38)], np.float32)
        k = key_of(vals[rng.integers(0, len(vals), npix)])
    else:
        raise KeyError(pattern)
    k = k.copy()
    if share == "half":
        k[rng.random(npix) < 0.5] = SENTINEL
    elif share == "all-but-one":
        keep = int(rng.integers(0, npix))
        one = k[keep]
        k[:] = SENTINEL
        k[keep] = one
    elif share == "all":
        k[:] = SENTINEL
    return k


# ---- the lookup's tables: one channel, (src values, ref values) of the n valid pixels; the test adds invalid pixels round them --------------
LOOKUP_N = (0, 1, 2, PIVOT - 1, PIVOT, PIVOT + 1)


def lookup_case(name, n):
    """(src, ref) float32 (n,) of the valid pixels, in pixel order."""
    rng = np.random.default_rng(zlib.crc32(f"{name}/{n}".encode()))
    cont = lambda: rng.random(n).astype(np.float32)  # noqa: E731
    quant = lambda q: (rng.integers(0, q + 1, n).astype(np.float32) / np.float32(q)).astype(np.float32)  # noqa: E731
    if name == "no-ties":
        return cont(), (cont() ** 2).astype(np.float32)
    if name == "ties-in-S":
        return quant(7), cont()
    if name == "ties-in-R":
        return cont(), quant(5)
    if name == "ties-in-both":
        return quant(9), quant(4)
    if name == "S-constant":
        return np.full(n, 0.5, np.float32), quant(6)
    if name == "R-constant":
        return cont(), np.full(n, 0.625, np.float32)
    if name == "left-clamp":                               # the least reference value is a long run: lo == 0 for the least sources
        r = quant(3)
        r[: max(1, n // 2)] = 0.0
        return cont(), rng.permutation(r)
    if name == "run-end-hit":                              # S and R quantised alike: cs lands on the ends of R's runs (hi == cs)
        q = quant(6)
        return q, rng.permutation(q)
    if name == "last-run":                                 # the greatest reference value is a long run
        r = quant(3)
        r[: max(1, n // 2)] = 1.0
        return cont(), rng.permutation(r)
    if name == "outside-0-1":
        return (cont() * 4 - 2).astype(np.float32), (quant(8) * 3 - 1).astype(np.float32)
    raise KeyError(name)


LOOKUP_CASES = ("no-ties", "ties-in-S", "ties-in-R", "ties-in-both", "S-constant", "R-constant", "left-clamp", "run-end-hit", "last-run",
                "outside-0-1")


def pivot_run_case(n, runs):
    """A reference whose equal runs are given as (start, length) pairs over ascending ramps, a continuous source: runs that cross one
    pivot or span several.  -> (src, ref) float32 (n,), shuffled."""
    rng = np.random.default_rng(n + 7 * len(runs))
    r = np.linspace(0.05, 0.95, n).astype(np.float32)
    for start, length in runs:
        r[start: start + length] = r[start]
    return rng.random(n).astype(np.float32), rng.permutation(r)


def all_instances():
    return (["hist_keys_kernel<PIXMAJOR>", "hist_keys_kernel<PLANAR>"] + [f"hist_count_kernel<{p}>" for p in range(4)] + ["hist_scan_kernel"]
            + [f"hist_scatter_kernel<{p}>" for p in range(4)] + ["hist_pivots_kernel", "hist_lookup_kernel<PIXMAJOR>", "hist_lookup_kernel<PLANAR>"])


def sort_record():
    return [n for p in range(4) for n in (f"hist_count_kernel<{p}>", "hist_scan_kernel", f"hist_scatter_kernel<{p}>")]


def layout_name(planar):
    return "PLANAR" if planar else "PIXMAJOR"
