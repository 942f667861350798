"""Every kernel instance of the operators around K1 - K3 - the exact percentile select (csrc/hsr_select.hip), the resamplers and
the upsample + histogram producer (csrc/hsr_resample.hip), the uint16 tile codec and the ENVI transposer (csrc/hsr_tile.hip) -
and the Sinkhorn kernels (csrc/hsr_ot.hip) against NumPy references.

One case table per family.  A row names a geometry, the data class and the instance(s) the library's launch record
(hsr_aux_last_launch) must show; the entry points are called through ctypes so that pointers can be offset, strides padded and
outputs pre-filled: every output lies between two guard zones inside a buffer filled with a sentinel byte, and every byte the
call does not own (guards, pad columns, stride gaps) must come back untouched.  References:
  * select: np.percentile(vals[mask], [pmin, pmax]) of the float32 values per channel (values equal, NaN in the same places;
    NaN for an empty mask, where NumPy has no answer), the pass-1 region against np.bincount(key >> 21) (+ the masked NaN count
    in word 2048), the regions of passes 2 and 3 against the bincount of the samples under each query's prefix, and the per-pass
    calls bit-identical to hsr_percentile_limits;
  * block mean: integers bit for bit against oracle_np.block_mean x float32(scale); float32 bit for bit against a float64 sum in
    the kernel's (dy, dx) order and, on multiples of 2^-12 (sums exact in any order), against oracle_np.block_mean;
  * bilinear: bit-equal to oracle_np.bilinear_upsample; the producer's mask, pass-1 region and limits against NumPy on its output;
  * codec: oracle_np.tile_encode_u16 / tile_decode_u16, bit-equal;  transposer: np.transpose + cast, exact;
  * Sinkhorn: oracle_np.ot_barycentric_targets at the bars of test_gpu_parity.test_device_sinkhorn_vs_oracle.
The last test checks that the rows reached every name hsr_aux_instance_name enumerates.
"""
import ctypes as C
import math
import warnings

import numpy as np
import pytest

from gpu_harness import SENT32, Buf, LaunchLog, bits_equal, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from gpu_harness import lib as _lib, stream as _stream
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu

LOG = LaunchLog("hsr_aux_last_launch")
_call = LOG.call


def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


NAN_POS, NAN_NEG = _f32([0x7fc00000])[0], _f32([0xffc00000])[0]


# =============================================================================================================================
# select
# =============================================================================================================================
def _key(v):
    """The select's monotone uint32 image of float32 values, restated: ~u for negatives, u | 0x80000000 otherwise."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _ranks(n, pmin, pmax):
    """(prev, next) of both percentiles, as np.percentile's 'linear' method indexes the sorted samples."""
    out = []
    for p in (pmin, pmax):
        vi = (n - 1) * (p / 100.0)
        prev = int(math.floor(vi))
        out += [prev, min(prev + 1, n - 1)]
    return out


def _pattern(vals, pmin, pmax, bits):
    """Pattern of equal / distinct radix prefixes (top `bits` key bits) of the four ranks, e.g. 'AABC'."""
    k = np.sort(_key(vals))
    pre = [int(k[r]) >> (32 - bits) for r in _ranks(len(k), pmin, pmax)]
    names = {}
    return "".join(names.setdefault(p, "ABCD"[len(names)]) for p in pre)


# geometry id -> (layout, npix, nb, stride, x offset in bytes, mask: None / "a" aligned / "o" off by one byte, hist family)
#   layout "p": band-major planes, stride = plane stride in floats;  "r": band-last rows, stride = row length in floats
#   family M1 / M0: select_hist_kernel<PASS, 1 / 0>, R4: select_hist_rows4_kernel<PASS>
MEGA, CAP = (1 << 20) + 1, 4194304 + 1          # smallest sizes above the two-iteration rule / above the 16-byte path's grid cap
SELECT_GEOMS = {
    # MODE 1: contiguous, the three tails behind a padded stride, mask present / absent
    "m1_contig":      ("p", 40000, 3, 40000, 0, "a", "M1"),
    "m1_contig_nomask": ("p", 33000, 2, 33000, 0, None, "M1"),
    "m1_tail1":       ("p", 40001, 3, 40004, 0, "a", "M1"),
    "m1_tail2":       ("p", 33002, 2, 33004, 0, "a", "M1"),
    "m1_tail3":       ("p", 40003, 3, 40008, 0, "a", "M1"),
    "m1_tail1_nomask": ("p", 33001, 2, 33004, 0, None, "M1"),
    "m1_tail3_nomask": ("p", 33003, 1, 33004, 0, None, "M1"),
    "m1_nb16":        ("p", 33002, 16, 33004, 0, "a", "M1"),
    "m1_mega_tail":   ("p", MEGA, 1, MEGA + 3, 0, "a", "M1"),
    "m1_cap_tail":    ("p", CAP, 1, CAP + 3, 0, "a", "M1"),
    # MODE 0 through each of its causes
    "m0_stride":      ("p", 40001, 3, 40001, 0, "a", "M0"),           # x_bs % 4 != 0
    "m0_xoff":        ("p", 40000, 3, 40000, 4, "a", "M0"),           # plane pointer off by 4 bytes
    "m0_maskoff":     ("p", 40000, 3, 40000, 0, "o", "M0"),           # mask pointer off by 1 byte
    "m0_rows8_nb5":   ("r", 33000, 5, 8, 0, "a", "M0"),
    "m0_rows8_nb8":   ("r", 33000, 8, 8, 0, "a", "M0"),
    "m0_rows4_off":   ("r", 40000, 3, 4, 4, "a", "M0"),               # rows of 4 off by 4 bytes
    "m0_mega":        ("p", MEGA, 1, MEGA, 0, "a", "M0"),
    "m0_nb16":        ("p", 32769, 16, 32769, 0, "a", "M0"),
    # rows of 4
    "r4_nb1":         ("r", 33000, 1, 4, 0, "a", "R4"),
    "r4_nb2":         ("r", 32769, 2, 4, 0, "a", "R4"),
    "r4_nb3":         ("r", 40001, 3, 4, 0, "a", "R4"),
    "r4_nb4":         ("r", 40003, 4, 4, 0, "a", "R4"),
    "r4_nb3_nomask":  ("r", 33001, 3, 4, 0, None, "R4"),
    "r4_maskoff":     ("r", 33001, 3, 4, 0, "o", "R4"),
    "r4_mega":        ("r", MEGA, 3, 4, 0, "a", "R4"),
}
# select_tiny_kernel: one launch up to 32768 pixels, in all three layouts (the per-pass calls still reach the hist kernels)
for _n in (1, 2, 1023, 1024, 1025, 32768):
    SELECT_GEOMS[f"tiny_p_{_n}"] = ("p", _n, 3, (_n + 3) // 4 * 4, 0, "a", "M1")
    SELECT_GEOMS[f"tiny_r4_{_n}"] = ("r", _n, 3, 4, 0, "a", "R4")
    SELECT_GEOMS[f"tiny_r8_{_n}"] = ("r", _n, 5, 8, 0, "a", "M0")
TINY_MAX = 32768


# ---- data classes: fn(rng, npix, masked indices) -> float32 plane; what matters is what the masked samples hold ------------------
def _d_noise(rng, n, m):
    return rng.uniform(-0.2, 1.2, n).astype(np.float32)


def _d_neg(rng, n, m):
    return (-rng.uniform(0.1, 5.0, n)).astype(np.float32)


def _split(k, q=0.5):
    """How many of k sorted samples lie at or below the prev rank of quantile q."""
    return min(k, int(math.floor((k - 1) * q)) + 1) if k else 0


def _d_straddle(rng, n, m):
    """Mixed sign; the prev / next ranks of the 50th percentile are the largest negative and the smallest positive sample."""
    v = rng.uniform(0.001, 3.0, n).astype(np.float32)
    lo = _split(len(m))
    v[rng.permutation(m)[:lo]] *= np.float32(-1.0)
    return v


def _d_zeros(rng, n, m):
    v = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    few = rng.choice(n, max(1, n // 50), replace=False)
    v[few] = rng.uniform(-1e-3, 1e-3, len(few)).astype(np.float32)
    return v


def _d_denorm(rng, n, m):
    u = rng.integers(1, 0x800000, n, dtype=np.uint32) | (rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31))
    return u.view(np.float32).copy()


def _d_inf(rng, n, m):
    v = _d_noise(rng, n, m)
    if len(m) >= 2:
        v[m[0]], v[m[-1]] = np.inf, -np.inf
    if len(m) > 4:
        v[m[len(m) // 2]] = np.inf
    return v


def _with_nan(nan, inside):
    def fn(rng, n, m):
        v = _d_noise(rng, n, m)
        out = np.setdiff1d(np.arange(n), m)
        where = m if inside else out
        if len(where):
            v.view(np.uint32)[where[len(where) // 3]] = nan.view(np.uint32)
        if inside and len(out):                       # and decoys of both signs outside the mask all the same
            v.view(np.uint32)[out[0]] = NAN_NEG.view(np.uint32)
        return v
    return fn


def _d_const(rng, n, m):
    return np.full(n, np.float32(0.37), np.float32)


def _d_two(rng, n, m):
    """Two values; the prev / next ranks of the 50th percentile straddle the step."""
    v = np.full(n, np.float32(0.75), np.float32)
    v[rng.permutation(m)[:_split(len(m))]] = np.float32(0.25)
    return v


DATA = {"noise": _d_noise, "neg": _d_neg, "straddle": _d_straddle, "zeros": _d_zeros, "denorm": _d_denorm, "inf": _d_inf,
        "nan+in": _with_nan(NAN_POS, True), "nan-in": _with_nan(NAN_NEG, True), "nan+out": _with_nan(NAN_POS, False),
        "nan-out": _with_nan(NAN_NEG, False), "const": _d_const, "two": _d_two}


# ---- mask classes: fn(rng, npix) -> uint8 bytes (used only where the geometry has a mask) ----------------------------------------
def _mask_sparse(k):
    def fn(rng, n):
        m = np.zeros(n, np.uint8)
        kk = min(k, n)
        if kk:
            m[rng.choice(n - 1, kk - 1, replace=False)] = 1
            m[n - 1] = 1                                    # the last pixel (the 16-byte path's tail) is always in
        return m
    return fn


MASKS = {"half": lambda rng, n: (rng.random(n) < 0.6).astype(np.uint8),
         "bytes": lambda rng, n: rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), n),
         "n101": _mask_sparse(101), "s0": _mask_sparse(0), "s1": _mask_sparse(1), "s2": _mask_sparse(2), "s3": _mask_sparse(3),
         "s4": _mask_sparse(4), "s50": _mask_sparse(50)}

P_STD = (2.0, 98.0)
# (id, geometry, data, mask, (pmin, pmax))
SELECT_ROWS = []


def _row(geom, data="noise", mask="half", pair=P_STD):
    SELECT_ROWS.append((f"{geom}-{data}-{mask}-{pair[0]:g}_{pair[1]:g}", geom, data, mask, pair))


for _g in SELECT_GEOMS:                                       # every geometry once on plain data
    _row(_g, "noise", "bytes" if _g.startswith("tiny") else "half")
_FAM = {"M1": ["m1_tail1", "m1_tail3", "m1_contig", "m1_tail2", "tiny_p_1025"],
        "M0": ["m0_stride", "m0_xoff", "m0_maskoff", "m0_rows8_nb5", "m0_rows4_off", "tiny_r8_1025"],
        "R4": ["r4_nb3", "r4_nb4", "r4_nb2", "r4_maskoff", "tiny_r4_1025"]}
_i = 0
for _d, _pair in (("neg", P_STD), ("straddle", (50.0, 75.0)), ("zeros", P_STD), ("denorm", P_STD), ("inf", P_STD), ("inf", (0.0, 100.0)),
                  ("nan+in", P_STD), ("nan-in", P_STD), ("nan+out", P_STD), ("nan-out", P_STD), ("const", P_STD), ("two", (50.0, 50.0))):
    for _f in ("M1", "M0", "R4"):                             # each data class meets each hist family
        _row(_FAM[_f][_i % len(_FAM[_f])], _d, "half", _pair)
    _i += 1
for _m in ("s0", "s1", "s2", "s3", "s4", "s50", "bytes"):     # sparse masks and mask bytes other than 0 / 1
    for _f in ("M1", "M0", "R4"):
        _row(_FAM[_f][_i % len(_FAM[_f])], "noise", _m, P_STD)
    _i += 1
# percentile pairs; with exactly 101 masked samples (n - 1) q is 25 and 75 (exact integers) for (25, 75), and 25.3 / 75.7 (the
# fractional part on either side of 0.5) for (25.3, 75.7)
for _pair in ((0.0, 100.0), (0.0, 0.0), (100.0, 100.0), (50.0, 50.0), (98.0, 2.0), (25.0, 75.0), (25.3, 75.7)):
    for _f in ("M1", "M0", "R4"):
        _row(_FAM[_f][_i % len(_FAM[_f])], "noise", "n101" if _pair[0] in (25.0, 25.3) else "half", _pair)
    _i += 1
assert len({r[0] for r in SELECT_ROWS}) == len(SELECT_ROWS)


def _select_run(torch, geom, planes, mask, pair, claim=None):
    """planes (nb, npix) float32, mask (npix,) uint8 or None -> runs the one-call and the per-pass select in the geometry, checks
    records, pass-1 region, per-pass == one-call bits and the limits against np.percentile."""
    lib, st = _lib(), _stream(torch)
    layout, npix, nb, stride, xoff, mk, fam = SELECT_GEOMS[geom]
    assert planes.shape == (nb, npix) and planes.dtype == np.float32
    rng = np.random.default_rng(7)
    if layout == "p":
        img = rng.uniform(-9, 9, (nb, stride)).astype(np.float32)          # stride gap: decoys
        img[:, npix:] = np.nan
        img[:, :npix] = planes
        if nb == 1 and stride > npix:
            img = img[:, :npix]                                              # a single plane needs no gap behind it
        x_bs, x_ps = stride, 1
    else:
        img = np.full((npix, stride), np.nan, np.float32)                   # pad columns: NaN decoys
        img[:, :nb] = planes.T
        x_bs, x_ps = 1, stride
    xb = Buf(torch, img.nbytes, xoff, img)
    mb = None
    if mk is not None:
        assert mask is not None
        mb = Buf(torch, npix, 1 if mk == "o" else 0, mask)
    else:
        mask = None
    mptr = mb.ptr if mb is not None else None
    hist = {"M1": "select_hist_kernel<%d, 1>", "M0": "select_hist_kernel<%d, 0>", "R4": "select_hist_rows4_kernel<%d>"}[fam]
    # reference
    ref = np.empty((nb, 2))
    sel = np.ones(npix, bool) if mask is None else mask != 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for c in range(nb):
            vals = planes[c][sel]
            ref[c] = np.percentile(vals, list(pair)) if len(vals) else np.nan
            if claim is not None:
                got_claim = (_pattern(vals, *pair, 11), _pattern(vals, *pair, 22))
                assert got_claim == claim[c], (c, got_claim, claim[c])
    wbytes = lib.hsr_percentile_work_bytes(nb)
    # one call
    w1, l1 = Buf(torch, wbytes), Buf(torch, nb * 16)
    _call("select_tiny_kernel" if npix <= TINY_MAX else "select_scan_kernel<3>", lib.hsr_percentile_limits, xb.ptr, x_bs, x_ps, mptr,
          npix, nb, pair[0], pair[1], w1.ptr, l1.ptr, st)
    one = l1.get(np.float64).reshape(nb, 2)
    w1.get(np.uint8)
    # per pass, with a look at the region (and nothing else) in between
    w2, l2 = Buf(torch, wbytes), Buf(torch, nb * 16)
    assert lib.hsr_percentile_begin(w2.ptr, nb, st) == 0
    for p in (1, 2, 3):
        _call(hist % p, lib.hsr_percentile_hist, p, xb.ptr, x_bs, x_ps, mptr, npix, nb, w2.ptr, st)
        off, cnt = C.c_int64(0), C.c_int64(0)
        assert lib.hsr_percentile_hist_region(p, nb, C.byref(off), C.byref(cnt)) == 0
        region = w2.get(np.uint8)[off.value: off.value + 4 * cnt.value].view(np.uint32)
        if p == 1:
            assert cnt.value == nb * 2052
            region = region.reshape(nb, 2052)
            for c in range(nb):
                vals = planes[c][sel]
                want = np.bincount(_key(vals) >> np.uint32(21), minlength=2048)
                assert np.array_equal(region[c, :2048], want), f"pass-1 histogram of channel {c}"
                assert region[c, 2048] == int(np.isnan(vals).sum()) and not region[c, 2049:].any()
        else:
            # passes 2 / 3: per rank query the histogram of the next 11 / 10 key bits over the masked samples that share the query's
            # prefix; a query whose prefix equals its predecessor's is not histogrammed a second time (its slot stays zero)
            top, nbins = (21, 2048) if p == 2 else (10, 1024)
            region = region.reshape(nb, 4, nbins)
            for c in range(nb):
                keys = np.sort(_key(planes[c][sel]))
                want = np.zeros((4, nbins), np.int64)
                if len(keys):
                    pre = [int(keys[r]) >> top for r in _ranks(len(keys), *pair)]
                    for q in range(4):
                        if q == 0 or pre[q] != pre[q - 1]:
                            hit = keys[(keys >> np.uint32(top)) == pre[q]]
                            want[q] = np.bincount((hit >> np.uint32(top - (11 if p == 2 else 10))) & np.uint32(nbins - 1), minlength=nbins)
                assert np.array_equal(region[c], want), f"pass-{p} histograms of channel {c}"
        _call(f"select_scan_kernel<{p}>", lib.hsr_percentile_scan, p, nb, pair[0], pair[1], w2.ptr, l2.ptr, st)
    per = l2.get(np.float64).reshape(nb, 2)
    assert np.array_equal(per.view(np.int64), one.view(np.int64)), (per, one)
    np.testing.assert_array_equal(one, ref)
    xb.get(np.uint8)
    return one


@pytest.mark.parametrize("rid,geom,data,mask,pair", SELECT_ROWS, ids=[r[0] for r in SELECT_ROWS])
def test_select_rows(torch_gpu, rid, geom, data, mask, pair):
    _, npix, nb, _, _, mk, _ = SELECT_GEOMS[geom]
    rng = np.random.default_rng(sum(map(ord, rid)))
    m = MASKS[mask](rng, npix) if mk is not None else None
    idx = np.flatnonzero(m) if m is not None else np.arange(npix)
    planes = np.stack([DATA[data](rng, npix, idx) for _ in range(nb)])
    if data == "straddle" and len(idx) >= 2:
        s = np.sort(planes[0][idx])
        prev = int(math.floor((len(s) - 1) * 0.5))
        assert s[prev] < 0 < s[prev + 1]
    if data == "two" and len(idx) >= 2:
        s = np.sort(planes[0][idx])
        prev = int(math.floor((len(s) - 1) * 0.5))
        assert s[prev] == np.float32(0.25) and s[prev + 1] == np.float32(0.75)
    if mask == "n101" and m is not None:
        assert len(idx) == 101
    _select_run(torch_gpu, geom, planes, m, pair)


# ---- prefix-slot rows: four masked samples at percentiles (10, 90) are the four ranks; their radix prefixes (top 11 key bits in
# pass 2, top 22 in pass 3) form the stated pattern.  second / more of the kernels: AAAA 0 / off, AAAB 3 / off, AABB 2 / off,
# ABBB 1 / off, AABC 2 / on, ABBC and ABCC 1 / on, ABCD 1 / on.  (sample set, pass-2 pattern, pass-3 pattern)
E = 2.0 ** -23
PREFIX_SETS = {
    # positive data
    "pos_AAAA_ABCD": ([1, 1.001, 1.002, 1.003], "AAAA", "ABCD"),
    "pos_AAAA_AAAA": ([1, 1 + E, 1 + 2 * E, 1 + 4 * E], "AAAA", "AAAA"),
    "pos_AAAA_AABC": ([1, 1 + E, 1.001, 1.002], "AAAA", "AABC"),
    "pos_AAAA_ABBC": ([1, 1.001, 1.001 + E, 1.002], "AAAA", "ABBC"),
    "pos_AAAB": ([1, 1 + E, 1 + 2 * E, 9], "AAAB", "AAAB"),
    "pos_AABB": ([1, 1 + E, 9, 9 + 8 * E], "AABB", "AABB"),
    "pos_ABBB": ([1, 9, 9 + 8 * E, 9 + 16 * E], "ABBB", "ABBB"),
    "pos_AABC": ([5, 5.0000005, 300, 7000], "AABC", "AABC"),
    "pos_ABBC": ([1, 9, 9 + 8 * E, 700], "ABBC", "ABBC"),
    "pos_ABCC": ([0.01, 0.3, 5, 5.0000005], "ABCC", "ABCC"),
    "pos_ABCD": ([0.01, 0.3, 5, 700], "ABCD", "ABCD"),
    # across the sign boundary (AAAA cannot straddle it - the sign is the prefix's top bit - and is all negative instead)
    "neg_AAAA_ABCD": ([-1.003, -1.002, -1.001, -1], "AAAA", "ABCD"),
    "neg_AAAA_AAAA": ([-1 - 4 * E, -1 - 2 * E, -1 - E, -1], "AAAA", "AAAA"),
    "sgn_AAAB": ([-1 - 2 * E, -1 - E, -1, 9], "AAAB", "AAAB"),
    "sgn_AABB": ([-1 - E, -1, 9, 9 + 8 * E], "AABB", "AABB"),
    "sgn_ABBB": ([-1, 9, 9 + 8 * E, 9 + 16 * E], "ABBB", "ABBB"),
    "sgn_AABC": ([-5.0000005, -5, 300, 7000], "AABC", "AABC"),
    "sgn_AABC_neg2": ([-5.0000005, -5, -0.3, 7], "AABC", "AABC"),
    "sgn_ABBC": ([-9, -1 - E, -1, 700], "ABBC", "ABBC"),
    "sgn_ABBC_pos2": ([-1, 9, 9 + 8 * E, 700], "ABBC", "ABBC"),
    "sgn_ABCC": ([-3, -0.3, 5, 5.0000005], "ABCC", "ABCC"),
    "sgn_ABCD": ([-3, -0.001, 0.002, 40], "ABCD", "ABCD"),
    "sgn_ABCD_neg3": ([-300, -3, -0.001, 0.5], "ABCD", "ABCD"),
    "neg_ABCD": ([-700, -5, -0.3, -0.01], "ABCD", "ABCD"),
}
_PK = list(PREFIX_SETS)
# (geometry, the sets of its channels)
PREFIX_ROWS = [("m1_nb16", _PK[:16]), ("m1_nb16", _PK[8:]), ("m0_nb16", _PK[:16]), ("m0_nb16", _PK[8:]),
               ("m1_tail1", _PK[9:12]), ("m0_maskoff", _PK[19:22])]
PREFIX_ROWS += [("r4_nb4", _PK[i:i + 4]) for i in range(0, 24, 4)] + [("r4_nb3", ["sgn_ABBC", "pos_AAAA_ABCD", "sgn_ABCD"])]
PREFIX_ROWS += [("tiny_p_1025", _PK[i:i + 3]) for i in (0, 8, 15, 21)] + [("tiny_r4_1025", _PK[i:i + 3]) for i in (4, 12, 18)]
PREFIX_ROWS += [("tiny_r8_1025", _PK[i:i + 5]) for i in (3, 11, 19)] + [("m0_rows8_nb8", _PK[5:13])]


@pytest.mark.parametrize("geom,sets", PREFIX_ROWS, ids=[f"{g}-{s[0]}..{s[-1]}" for g, s in PREFIX_ROWS])
def test_select_prefix_slots(torch_gpu, geom, sets):
    _, npix, nb, _, _, mk, _ = SELECT_GEOMS[geom]
    assert len(sets) == nb and mk is not None
    rng = np.random.default_rng(len(geom) + nb)
    pos = np.array([0, npix // 3, (2 * npix) // 3 + 1, npix - 1])         # first and last pixel (the tail) among the four
    mask = np.zeros(npix, np.uint8)
    mask[pos] = 1
    planes = np.empty((nb, npix), np.float32)
    for c, name in enumerate(sets):
        vals = np.array(PREFIX_SETS[name][0], np.float32)
        decoy = np.concatenate([vals, -vals, _f32([0x7fc00000, 0xffc00000, 0x7f800000, 0xff800000, 0, 0x80000000])])
        planes[c] = rng.choice(decoy, npix)                                # masked-out samples share every prefix
        planes[c][pos] = rng.permutation(vals)
    _select_run(torch_gpu, geom, planes, mask, (10.0, 90.0), claim=[PREFIX_SETS[s][1:] for s in sets])


def test_select_prefix_patterns_cover_every_slot_combination():
    """The sets above build all eight patterns in both passes, with positive data and across (or below) the sign boundary."""
    allp = {"AAAA", "AAAB", "AABB", "ABBB", "AABC", "ABBC", "ABCC", "ABCD"}
    for pre in ("pos", ("neg", "sgn")):
        names = [k for k in PREFIX_SETS if k.startswith(pre)]
        assert {PREFIX_SETS[k][1] for k in names} == allp and {PREFIX_SETS[k][2] for k in names} == allp
    used = {s for _, sets in PREFIX_ROWS for s in sets}
    assert used == set(PREFIX_SETS)
    for fam in ("M1", "M0", "R4"):                                         # every set meets every hist family
        assert {s for g, sets in PREFIX_ROWS if SELECT_GEOMS[g][6] == fam for s in sets} == set(PREFIX_SETS), fam


# =============================================================================================================================
# block mean
# =============================================================================================================================
NP_T = {"float": np.float32, "uint8_t": np.uint8, "uint16_t": np.uint16}
DT_CODE = {"float": 0, "uint8_t": 1, "uint16_t": 2}
# (dtype, in layout, out layout, nb, Hc, Wc, f, staged?, why)  in layout: planar / packed (band-last rows of nb) / padded (rows of 4,
# nb = 3) / planar+1 (input pointer off by one element) / planar^1 (plane stride one element longer)
# staged needs: 16-byte aligned pointer, row bytes and plane stride, and f * 64 * f * interleave * sizeof(T) <= 48 KB:
#   float planes f <= 13, uint16 planes f <= 19, uint8 planes f <= 27, uint8 rows of 3 f <= 16, uint16 rows of 3 f <= 11
BM_ROWS = [
    ("float", "planar", "planar", 2, 5, 64, 1, True, "f=1"),
    ("float", "planar", "pixmajor", 3, 5, 64, 2, True, "f=2"),
    ("float", "planar", "planar", 1, 1, 64, 3, True, "f=3 Hc=1"),
    ("float", "planar", "planar", 2, 5, 129, 4, True, "Wc=129: three segments, the last of one column"),
    ("float", "planar", "pixmajor", 2, 5, 63, 4, True, "Wc=63"),
    ("float", "planar", "planar", 2, 1, 65, 4, True, "Wc=65"),
    ("float", "planar", "planar", 2, 5, 1, 4, True, "Wc=1"),
    ("float", "planar", "planar", 2, 5, 64, 6, True, "f=6"),
    ("float", "planar", "planar", 2, 5, 64, 13, True, "f=13: 43264 B of LDS"),
    ("float", "planar", "planar", 2, 5, 64, 14, False, "f=14: 50176 B of LDS"),
    ("float", "planar", "planar", 1, 1, 5, 64, False, "f=64"),
    ("float", "planar", "planar", 2, 5, 65, 6, False, "row bytes 1560"),
    ("float", "planar", "planar", 2, 5, 1, 1, False, "row bytes 4"),
    ("float", "planar+1", "planar", 2, 5, 64, 2, False, "pointer off by one element"),
    ("float", "planar^1", "pixmajor", 2, 5, 64, 2, False, "plane stride % 16 B"),
    ("float", "packed", "planar", 4, 5, 63, 3, True, "rows of 4 floats, packed"),
    ("float", "packed", "pixmajor", 3, 5, 64, 2, True, "rows of 3 floats, packed"),
    ("float", "padded", "pixmajor", 3, 5, 64, 2, False, "padded rows"),
    ("uint8_t", "planar", "planar", 2, 5, 65, 16, True, "Wc=65"),
    ("uint8_t", "planar", "planar", 2, 1, 63, 16, True, "Wc=63 Hc=1"),
    ("uint8_t", "planar", "planar", 1, 5, 16, 27, True, "f=27: 46656 B"),
    ("uint8_t", "planar", "planar", 1, 5, 16, 28, False, "f=28: 50176 B"),
    ("uint8_t", "planar", "planar", 1, 1, 3, 64, False, "f=64"),
    ("uint8_t", "planar+1", "planar", 2, 5, 64, 2, False, "pointer off by one element"),
    ("uint8_t", "planar^1", "planar", 2, 5, 64, 2, False, "plane stride % 16 B"),
    ("uint8_t", "planar", "planar", 2, 5, 13, 6, False, "row bytes 78"),
    ("uint8_t", "packed", "pixmajor", 3, 5, 129, 16, True, "RGB f=16: 49152 B, Wc=129"),
    ("uint8_t", "packed", "pixmajor", 3, 5, 32, 6, True, "RGB f=6"),
    ("uint8_t", "packed", "planar", 3, 5, 16, 17, False, "RGB f=17: 55488 B"),
    ("uint8_t", "padded", "pixmajor", 3, 5, 64, 6, False, "padded rows"),
    ("uint16_t", "planar", "planar", 2, 5, 64, 1, True, "f=1"),
    ("uint16_t", "planar", "pixmajor", 2, 5, 8, 19, True, "f=19: 46208 B"),
    ("uint16_t", "planar", "planar", 2, 5, 8, 20, False, "f=20: 51200 B"),
    ("uint16_t", "planar", "planar", 2, 1, 65, 8, True, "Wc=65 Hc=1"),
    ("uint16_t", "planar", "planar", 2, 5, 63, 13, False, "row bytes 1638"),
    ("uint16_t", "planar", "planar", 2, 5, 64, 14, True, "f=14"),
    ("uint16_t", "planar+1", "planar", 2, 5, 64, 2, False, "pointer off by one element"),
    ("uint16_t", "planar^1", "planar", 2, 5, 64, 2, False, "plane stride % 16 B"),
    ("uint16_t", "packed", "pixmajor", 3, 5, 64, 11, True, "rows of 3, f=11: 46464 B"),
    ("uint16_t", "packed", "pixmajor", 3, 5, 64, 12, False, "rows of 3, f=12: 55296 B"),
    ("uint16_t", "padded", "planar", 3, 1, 64, 3, False, "padded rows"),
    ("uint16_t", "planar", "planar", 1, 1, 2, 64, False, "f=64"),
]


def _bm_ref_f32(x, f, scale):
    """float64 sum in the kernel's (dy, dx) order, /(f f) in float64, float32, x float32(scale)."""
    s = np.zeros((x.shape[0], x.shape[1] // f, x.shape[2] // f))
    for dy in range(f):
        for dx in range(f):
            s = s + x[:, dy::f, dx::f].astype(np.float64)
    return (s / float(f * f)).astype(np.float32) * np.float32(scale)


@pytest.mark.parametrize("row", BM_ROWS, ids=[f"{r[0]}-{r[1]}-{r[2]}-nb{r[3]}-{r[4]}x{r[5]}-f{r[6]}" for r in BM_ROWS])
def test_block_mean_rows(torch_gpu, row):
    torch, lib = torch_gpu, _lib()
    tname, lay, olay, nb, Hc, Wc, f, staged, _why = row
    T = NP_T[tname]
    isz = np.dtype(T).itemsize
    Hf, Wf = Hc * f, Wc * f
    rng = np.random.default_rng(Hc * 1000 + Wc * 10 + f)
    datas = ([("q12", (rng.integers(0, 4096, (nb, Hf, Wf)) / 4096.0).astype(np.float32), 1.0),
              ("mixed", (rng.standard_normal((nb, Hf, Wf)) * 10.0 ** rng.integers(-6, 6, (nb, Hf, Wf))).astype(np.float32), 0.37)]
             if T is np.float32 else
             [("full", rng.integers(0, np.iinfo(T).max + 1, (nb, Hf, Wf)).astype(T), 1.0 / 255.0 if T is np.uint8 else 1e-4)])
    # the derivation of the LDS threshold, restated
    il = nb if lay == "packed" else 1
    lds = f * 64 * f * il * isz
    assert staged == (lay in ("planar", "packed") and lds <= 48 * 1024 and (Wf * il * isz) % 16 == 0), (lds, Wf * il * isz)
    for dname, x, scale in datas:
        npf = Hf * Wf
        off = 0
        if lay.startswith("planar"):
            bs = npf + (1 if lay == "planar^1" else 0)
            if lay == "planar" and nb > 1:
                bs = (npf * isz + 15) // 16 * 16 // isz                      # planes start 16-byte aligned
                assert (bs * isz) % 16 == 0
            img = np.zeros((nb, bs), T)
            img[:, :npf] = x.reshape(nb, npf)
            ibs, ips = bs, 1
            off = isz if lay == "planar+1" else 0
        else:
            rowlen = nb if lay == "packed" else 4
            img = np.full((npf, rowlen), 77, T)
            img[:, :nb] = x.reshape(nb, npf).T
            ibs, ips = 1, rowlen
        xb = Buf(torch, img.nbytes, off, img)
        npc = Hc * Wc
        if olay == "planar":
            obs, ops, ofl = npc + 3, 1, nb * (npc + 3)
        else:
            obs, ops, ofl = 1, (nb + 3) // 4 * 4, npc * ((nb + 3) // 4 * 4)
        ob = Buf(torch, ofl * 4)
        kern = ("block_mean_tile_kernel<%s>" if staged else "block_mean_kernel<%s>") % tname
        _call(kern, lib.hsr_block_mean, xb.ptr, DT_CODE[tname], ibs, ips, nb, Hc, Wc, f, scale, ob.ptr, obs, ops, _stream(torch))
        raw = ob.get(np.uint32)
        if olay == "planar":
            raw = raw.reshape(nb, npc + 3)
            assert (raw[:, npc:] == SENT32).all(), "stride gap written"
            got = raw[:, :npc].view(np.float32).reshape(nb, Hc, Wc)
        else:
            raw = raw.reshape(npc, ops)
            assert (raw[:, nb:] == SENT32).all(), "pad columns written"
            got = np.ascontiguousarray(raw[:, :nb].T).view(np.float32).reshape(nb, Hc, Wc)
        if T is np.float32:
            bits_equal(got, _bm_ref_f32(x, f, scale), f"{dname} vs ordered float64 sum")
            if dname == "q12":
                bits_equal(got, onp.block_mean(x, f) * np.float32(scale), "q12 vs oracle")
        else:
            bits_equal(got, onp.block_mean(x, f) * np.float32(scale), "vs oracle")


# =============================================================================================================================
# bilinear upsampling and the producer
# =============================================================================================================================
# (in layout, out layout, nb, Hc, Wc, f, instance)   layouts: planar, rows4, rows8, rows4+4 (rows of 4, pointer off by 4 bytes)
UP_FF, UP_TF, UP_TT = "bilinear_up_kernel<false, false>", "bilinear_up_kernel<true, false>", "bilinear_up_kernel<true, true>"
UP_ROWS = [
    ("planar", "planar", 2, 1, 1, 1, UP_FF), ("planar", "planar", 2, 1, 5, 7, UP_FF), ("planar", "planar", 1, 5, 1, 3, UP_FF),
    ("planar", "planar", 2, 2, 2, 64, UP_FF), ("planar", "planar", 1, 3, 85, 3, UP_FF), ("planar", "planar", 1, 4, 128, 2, UP_FF),
    ("planar", "planar", 1, 9, 257, 1, UP_FF), ("planar", "planar", 3, 31, 3, 1, UP_FF), ("planar", "planar", 1, 11, 2, 3, UP_FF),
    ("rows8", "rows8", 5, 4, 5, 2, UP_FF), ("rows4", "planar", 3, 3, 4, 6, UP_FF), ("planar", "rows4+4", 3, 3, 4, 2, UP_FF),
    ("planar", "rows4", 1, 1, 1, 1, UP_TF), ("planar", "rows4", 2, 1, 4, 7, UP_TF), ("planar", "rows4", 3, 2, 2, 64, UP_TF),
    ("planar", "rows4", 4, 16, 128, 2, UP_TF), ("planar", "rows4", 3, 3, 85, 3, UP_TF), ("planar", "rows4", 3, 33, 257, 1, UP_TF),
    ("rows4+4", "rows4", 3, 5, 3, 6, UP_TF), ("rows8", "rows4", 3, 5, 1, 6, UP_TF),
    ("rows4", "rows4", 1, 1, 1, 1, UP_TT), ("rows4", "rows4", 2, 1, 4, 7, UP_TT), ("rows4", "rows4", 3, 4, 1, 2, UP_TT),
    ("rows4", "rows4", 4, 2, 2, 64, UP_TT), ("rows4", "rows4", 3, 3, 85, 3, UP_TT), ("rows4", "rows4", 3, 4, 128, 2, UP_TT),
    ("rows4", "rows4", 3, 7, 257, 1, UP_TT), ("rows4", "rows4", 3, 32, 2, 1, UP_TT), ("rows4", "rows4", 3, 11, 5, 3, UP_TT),
    ("rows4", "rows4", 3, 5, 7, 6, UP_TT),
]
HIST_T, HIST_F = "bilinear_up_hist_kernel<true>", "bilinear_up_hist_kernel<false>"
UPH_ROWS = [
    ("rows4", 1, 1, 1, 1, HIST_T), ("rows4", 3, 1, 4, 7, HIST_T), ("rows4", 3, 31, 3, 1, HIST_T), ("rows4", 4, 16, 128, 2, HIST_T),
    ("rows4", 3, 11, 85, 3, HIST_T), ("rows4", 2, 2, 2, 64, HIST_T), ("rows4", 3, 6, 257, 1, HIST_T), ("rows4", 3, 6, 5, 6, HIST_T),
    ("planar", 1, 1, 1, 1, HIST_F), ("planar", 3, 1, 4, 7, HIST_F), ("planar", 3, 33, 3, 1, HIST_F), ("planar", 4, 16, 128, 2, HIST_F),
    ("planar", 3, 11, 85, 3, HIST_F), ("planar", 2, 2, 2, 64, HIST_F), ("planar", 3, 9, 257, 1, HIST_F), ("rows4+4", 3, 6, 5, 6, HIST_F),
    ("rows8", 4, 8, 3, 4, HIST_F),
]


def _coarse(rng, nb, Hc, Wc, special=True):
    """Coarse planes with a NaN / +Inf / -Inf pixel in the interior and on each edge where the image has room."""
    x = rng.uniform(-0.3, 1.3, (nb, Hc, Wc)).astype(np.float32)
    if special and Hc * Wc >= 12:
        sp = [np.nan, np.inf, -np.inf]
        spots = [(0, Wc // 2), (Hc - 1, Wc // 2), (Hc // 2, 0), (Hc // 2, Wc - 1), (Hc // 2, Wc // 2), (0, 0), (Hc - 1, Wc - 1)]
        for i, (r, c) in enumerate(spots):
            x[i % nb, r, c] = sp[i % 3]
    return x


def _layout_in(torch, x, lay):
    """planes (nb, H, W) -> (Buf, band stride, pixel stride)"""
    nb, npix = x.shape[0], x.shape[1] * x.shape[2]
    if lay == "planar":
        return Buf(torch, x.nbytes, 0, x), npix, 1
    rowlen = 8 if lay == "rows8" else 4
    img = np.full((npix, rowlen), np.float32(123.0), np.float32)
    img[:, :nb] = x.reshape(nb, npix).T
    return Buf(torch, img.nbytes, 4 if lay.endswith("+4") else 0, img), 1, rowlen


def _check_rows_out(raw, nb, ref, rowlen, pad_zero, what):
    """raw uint32 (npix, rowlen): bands bit-equal to ref (nb, npix); pad floats 0.0 (16-byte stores) or untouched."""
    raw = raw.reshape(-1, rowlen)
    bits_equal(np.ascontiguousarray(raw[:, :nb].T).view(np.float32), ref, what)
    assert (raw[:, nb:] == (0 if pad_zero else SENT32)).all(), f"{what}: pad columns"


@pytest.mark.parametrize("row", UP_ROWS, ids=[f"{r[0]}-{r[1]}-nb{r[2]}-{r[3]}x{r[4]}-f{r[5]}" for r in UP_ROWS])
def test_bilinear_rows(torch_gpu, row):
    torch, lib = torch_gpu, _lib()
    ilay, olay, nb, Hc, Wc, f, inst = row
    rng = np.random.default_rng(Hc * 100 + Wc + f)
    x = _coarse(rng, nb, Hc, Wc)
    with np.errstate(invalid="ignore"):
        ref = onp.bilinear_upsample(x, f).reshape(nb, -1)
    npf = Hc * f * Wc * f
    xb, ibs, ips = _layout_in(torch, x, ilay)
    if olay == "planar":
        obs, ops, ob = npf + 5, 1, Buf(torch, nb * (npf + 5) * 4)
    else:
        rowlen = 8 if olay == "rows8" else 4
        obs, ops, ob = 1, rowlen, Buf(torch, npf * rowlen * 4, 4 if olay.endswith("+4") else 0)
    _call(inst, lib.hsr_bilinear_upsample, xb.ptr, ibs, ips, nb, Hc, Wc, f, ob.ptr, obs, ops, _stream(torch))
    raw = ob.get(np.uint32)
    if olay == "planar":
        raw = raw.reshape(nb, npf + 5)
        assert (raw[:, npf:] == SENT32).all(), "stride gap written"
        bits_equal(raw[:, :npf].view(np.float32), ref, "planar")
    else:
        _check_rows_out(raw, nb, ref, ops, inst != UP_FF, olay)
    xb.get(np.uint8)


@pytest.mark.parametrize("row", UPH_ROWS, ids=[f"{r[0]}-nb{r[1]}-{r[2]}x{r[3]}-f{r[4]}" for r in UPH_ROWS])
def test_bilinear_producer_rows(torch_gpu, row):
    """hsr_bilinear_upsample_mask_hist, then the select's scans and passes 2 and 3 on its output (the chain of the driver)."""
    torch, lib = torch_gpu, _lib()
    st = _stream(torch)
    ilay, nb, Hc, Wc, f, inst = row
    rng = np.random.default_rng(Hc * 100 + Wc + f + 1)
    x = _coarse(rng, nb, Hc, Wc)
    x[0] -= np.float32(0.8)                                               # a band of mostly negative values
    with np.errstate(invalid="ignore"):
        ref = onp.bilinear_upsample(x, f).reshape(nb, -1)
    npf = ref.shape[1]
    xb, ibs, ips = _layout_in(torch, x, ilay)
    ob, mb, wb, lb = Buf(torch, npf * 16), Buf(torch, npf), Buf(torch, lib.hsr_percentile_work_bytes(nb)), Buf(torch, nb * 16)
    assert lib.hsr_percentile_begin(wb.ptr, nb, st) == 0
    _call(inst, lib.hsr_bilinear_upsample_mask_hist, xb.ptr, ibs, ips, nb, Hc, Wc, f, ob.ptr, mb.ptr, wb.ptr, st)
    _check_rows_out(ob.get(np.uint32), nb, ref, 4, True, "producer output")
    mask = mb.get(np.uint8)
    want_mask = np.isfinite(ref).all(axis=0)
    assert np.array_equal(mask, want_mask.astype(np.uint8))
    off, cnt = C.c_int64(0), C.c_int64(0)
    assert lib.hsr_percentile_hist_region(1, nb, C.byref(off), C.byref(cnt)) == 0
    region = wb.get(np.uint8)[off.value: off.value + 4 * cnt.value].view(np.uint32).reshape(nb, 2052)
    for c in range(nb):
        assert np.array_equal(region[c, :2048], np.bincount(_key(ref[c][want_mask]) >> np.uint32(21), minlength=2048)), c
        assert not region[c, 2048:].any()
    _call("select_scan_kernel<1>", lib.hsr_percentile_scan, 1, nb, 2.0, 98.0, wb.ptr, lb.ptr, st)
    for p in (2, 3):
        _call(f"select_hist_rows4_kernel<{p}>", lib.hsr_percentile_hist, p, ob.ptr, 1, 4, mb.ptr, npf, nb, wb.ptr, st)
        _call(f"select_scan_kernel<{p}>", lib.hsr_percentile_scan, p, nb, 2.0, 98.0, wb.ptr, lb.ptr, st)
    lohi = lb.get(np.float64).reshape(nb, 2)
    want = np.array([np.percentile(ref[c][want_mask], [2.0, 98.0]) if want_mask.any() else [np.nan, np.nan] for c in range(nb)])
    np.testing.assert_array_equal(lohi, want)


# =============================================================================================================================
# uint16 tile codec
# =============================================================================================================================
BIG_N = 4200003            # odd, n / 4 above 4096 workgroups x 256 threads: the grid-stride loops wrap


def _codec_values(rng, n):
    """Every float32 binade in both signs, half-way ties of x * scale for scale 1 / 2 / 4, -0.0, values beyond the int32 range,
    +-Inf, NaN of both signs, the source nodata value; filled up with reflectance-like noise."""
    binades = _f32([(e << 23) | m for e in range(0, 255) for m in (0, 1, 0x400000, 0x7fffff)])
    ties = np.concatenate([np.arange(0, 70000, 7) + 0.5, (np.arange(0, 3000) + 0.5) / 2, (np.arange(0, 3000) + 0.5) / 4]).astype(np.float32)
    special = np.array([-0.0, 0.0, 3e9, -3e9, 2147483648.0, -2147483648.0, 2147483520.0, 1e20, -1e20, 3.4e38, -3.4e38, np.inf, -np.inf,
                        np.nan, -9999.0, 6.5534, 6.5535, 6.5536, 65534.5, 65535.5, -0.00004, 0.00005, 0.00015], np.float32)
    pool = np.concatenate([binades, -binades, ties, -ties[:50], special, _f32([0xffc00000])])
    if n <= 1100:
        return rng.choice(pool, n).astype(np.float32) if n else np.zeros(0, np.float32)
    out = rng.uniform(-0.1, 7.0, n).astype(np.float32)
    k = min(len(pool), n)
    out[rng.choice(n, k, replace=False)] = pool[:k]
    return out


# (n, input offset bytes, output offset bytes, path, scale, src nodata, nodata_u16)
ENC_ROWS = [(n, 0, 0, "vec", 1e4, None, 65535) for n in (0, 1, 3, 4, 5, 1027)]
ENC_ROWS += [(n, 4, 0, "scalar", 1e4, None, 65535) for n in (1, 4, 1027)] + [(n, 0, 2, "scalar", 1e4, -9999.0, 65535) for n in (0, 3, 5, 1027)]
ENC_ROWS += [(1027, 8, 4, "scalar", 1.0, None, 65535), (1027, 0, 4, "scalar", 2.0, -9999.0, 1000), (1027, 16, 8, "vec", 1.0, -9999.0, 65535),
             (40003, 0, 0, "vec", 1.0, None, 65535), (40003, 0, 0, "vec", 2.0, None, 65535), (40003, 0, 0, "vec", 4.0, -9999.0, 1),
             (40003, 0, 0, "vec", 1e4, -9999.0, 1000), (40003, 0, 2, "scalar", 1.0, -9999.0, 65535),
             (BIG_N, 0, 0, "vec", 1e4, -9999.0, 65535), (BIG_N, 4, 2, "scalar", 1e4, None, 65535)]


@pytest.mark.parametrize("row", ENC_ROWS, ids=[f"n{r[0]}-in{r[1]}-out{r[2]}-{r[3]}-s{r[4]:g}-nd{r[5]}-{r[6]}" for r in ENC_ROWS])
def test_tile_encode_rows(torch_gpu, row):
    torch, lib = torch_gpu, _lib()
    n, ioff, ooff, path, scale, src_nd, nd16 = row
    assert (path == "vec") == (ioff % 16 == 0 and ooff % 8 == 0)
    x = _codec_values(np.random.default_rng(n + ioff + ooff), n)
    xb, ob = Buf(torch, max(n, 1) * 4, ioff, x), Buf(torch, n * 2, ooff)
    _call(f"tile_encode_kernel {path}" if n else None, lib.hsr_tile_encode_u16, xb.ptr, n, scale, 1 if src_nd is not None else 0,
          src_nd if src_nd is not None else 0.0, nd16, ob.ptr, _stream(torch))
    got = ob.get(np.uint16)
    want = onp.tile_encode_u16(x, src_nd, scale, nd16)
    assert np.array_equal(got, want), (np.flatnonzero(got != want)[:5], x[got != want][:5], got[got != want][:5], want[got != want][:5])


# (n, input offset bytes, output offset bytes, path, scale (None = the default 1e-4), nodata (None = none))
DEC_ROWS = [(n, 0, 0, "vec", None, 65535) for n in (0, 1, 3, 4, 5, 1027, 65536)]
DEC_ROWS += [(n, 2, 0, "scalar", None, 65535) for n in (1, 4, 1027)] + [(n, 0, 4, "scalar", None, None) for n in (0, 3, 5, 65536)]
DEC_ROWS += [(65536, 0, 0, "vec", None, None), (65536, 8, 16, "vec", 0.5, 0), (65536, 4, 8, "scalar", 2.5e-5, 1234), (65536, 6, 12, "scalar", None, 65535),
             (BIG_N, 0, 0, "vec", None, 65535), (BIG_N, 2, 4, "scalar", 2.5e-5, None)]


@pytest.mark.parametrize("row", DEC_ROWS, ids=[f"n{r[0]}-in{r[1]}-out{r[2]}-{r[3]}-s{r[4]}-nd{r[5]}" for r in DEC_ROWS])
def test_tile_decode_rows(torch_gpu, row):
    torch, lib = torch_gpu, _lib()
    n, ioff, ooff, path, scale, nd = row
    assert (path == "vec") == (ioff % 8 == 0 and ooff % 16 == 0)
    rng = np.random.default_rng(n + ioff)
    u = rng.permutation(np.arange(65536, dtype=np.uint16)) if n == 65536 else rng.integers(0, 65536, n).astype(np.uint16)   # all codes
    if n > 8 and n != 65536:
        u[-3:] = [65535, 0, 1234]                                              # the tail samples hold the special codes too
    ub, ob = Buf(torch, max(n, 1) * 2, ioff, u), Buf(torch, n * 4, ooff)
    _call(f"tile_decode_kernel {path}" if n else None, lib.hsr_tile_decode_u16, ub.ptr, n, 1e-4 if scale is None else scale,
          -1 if nd is None else nd, ob.ptr, _stream(torch))
    bits_equal(ob.get(np.float32), onp.tile_decode_u16(u, scale, nd), "decode")


# =============================================================================================================================
# ENVI transposer
# =============================================================================================================================
TR_T = {0: (np.float32, "float"), 2: (np.uint16, "uint16_t"), 3: (np.int16, "int16_t")}
# (in dtype, out dtype, interleave 1 BIL / 2 BSQ, lines, samples, bands)
TR_ROWS = [(0, 0, 1, 3, 63, 64), (0, 0, 2, 2, 65, 63), (2, 2, 1, 2, 130, 65), (2, 2, 2, 3, 1, 285), (2, 0, 1, 2, 65, 285), (2, 0, 2, 2, 63, 1),
           (3, 0, 1, 3, 1, 63), (3, 0, 2, 2, 130, 64), (0, 0, 1, 2, 130, 1), (3, 0, 1, 2, 63, 65), (2, 0, 2, 5, 65, 65), (0, 0, 2, 2, 32, 64),
           (2, 2, 1, 65537, 1, 2)]                                                 # BIL lines above 65535: folded into a second launch


@pytest.mark.parametrize("row", TR_ROWS, ids=[f"{TR_T[r[0]][1]}-{TR_T[r[1]][1]}-{'BIL' if r[2] == 1 else 'BSQ'}-{r[3]}x{r[4]}x{r[5]}" for r in TR_ROWS])
def test_interleave_to_bip_rows(torch_gpu, row):
    torch, lib = torch_gpu, _lib()
    idt, odt, il, lines, samples, bands = row
    TI, TO = TR_T[idt][0], TR_T[odt][0]
    rng = np.random.default_rng(lines + samples + bands)
    shape = (lines, bands, samples) if il == 1 else (bands, lines, samples)
    if TI is np.float32:
        x = rng.standard_normal(shape).astype(np.float32)
        x.reshape(-1)[:: 97] = np.nan
    else:
        x = rng.integers(np.iinfo(TI).min, np.iinfo(TI).max + 1, shape).astype(TI)
    want = np.ascontiguousarray(np.transpose(x, (0, 2, 1) if il == 1 else (1, 2, 0))).astype(TO)
    xb, ob = Buf(torch, x.nbytes, 0, x), Buf(torch, want.nbytes)
    _call(f"transpose_rc_kernel<{TR_T[idt][1]}, {TR_T[odt][1]}>", lib.hsr_interleave_to_bip, xb.ptr, idt, il, lines, samples, bands,
          ob.ptr, odt, _stream(torch))
    got = ob.get(TO).reshape(want.shape)
    if TO is np.float32:
        bits_equal(got, want, "transpose")
    else:
        assert np.array_equal(got, want)


# =============================================================================================================================
# Sinkhorn (no launch record: these kernels are not chosen by geometry)
# =============================================================================================================================
@pytest.mark.parametrize("ns,nt", [(1, 1), (1, 5), (5, 1), (63, 65), (65, 64), (130, 3), (257, 2)])
def test_sinkhorn_small_shapes(torch_gpu, ns, nt):
    """The checks and bars of test_gpu_parity.test_device_sinkhorn_vs_oracle at n or m of 1, fewer rows than a 64-row chunk, fewer
    chunks than the four quarters of the column sum, odd m below 64."""
    torch = torch_gpu
    from s2_emit import _ot
    reg, itmax, thr = 0.05, 300, 1e-6
    rng = np.random.default_rng(ns + nt)
    X = rng.random((ns, 3))
    Y = np.clip(X[rng.integers(0, ns, nt)] ** 0.8 * 0.9 + 0.05 + 0.02 * rng.standard_normal((nt, 3)), 0, 1)
    want = onp.ot_barycentric_targets(X, Y, reg, itmax, thr)
    got, info = _ot.barycentric_targets_device(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), reg, itmax, thr, return_info=True)
    got = got.cpu().numpy()
    a, b = np.full(ns, 1 / ns), np.full(nt, 1 / nt)
    K = np.exp(onp.sqeuclidean_cost(X, Y) / -reg)
    u, v, stop, checks = a.copy(), b.copy(), None, 0
    for ii in range(itmax):
        v = b / (K.T @ u)
        u = a / (K @ v)
        if ii % 10 == 0:
            checks += 1
            if np.linalg.norm(v * (K.T @ u) - b) < thr:
                stop = ii
                break
    assert info["break_iter"] is None and info["conv_iter"] == stop and info["checks"] == checks
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)
    assert (got.min(0) >= Y.min(0) - 1e-12).all() and (got.max(0) <= Y.max(0) + 1e-12).all()
    again = _ot.barycentric_targets_device(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), reg, itmax, thr)
    assert np.array_equal(again.cpu().numpy().view(np.int64), got.view(np.int64))
    for k in (7, 50):
        polled, pinfo = _ot.barycentric_targets_device(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), reg, itmax, thr,
                                                       return_info=True, poll_every=k)
        assert np.array_equal(polled.cpu().numpy().view(np.int64), got.view(np.int64))
        assert pinfo["conv_iter"] == info["conv_iter"] and pinfo["checks"] == info["checks"]


# =============================================================================================================================
# the guarded buffer itself
# =============================================================================================================================
def test_buf_get_notices_a_byte_written_on_either_side_of_the_payload(torch_gpu):
    payload = np.arange(64, dtype=np.uint8)
    buf = Buf(torch_gpu, 64, 4, payload)
    assert np.array_equal(buf.get(np.uint8), payload)
    for at in (buf.lo - 1, buf.lo + buf.nbytes):
        buf = Buf(torch_gpu, 64, 4, payload)
        buf.t[at] = 0
        with pytest.raises(AssertionError, match="write outside the buffer"):
            buf.get(np.uint8)


# =============================================================================================================================
# completeness
# =============================================================================================================================
def test_rows_reach_every_instance(torch_gpu):
    lib = _lib()
    table = {lib.hsr_aux_instance_name(i).decode() for i in range(lib.hsr_aux_instance_count())}
    assert len(table) == lib.hsr_aux_instance_count()
    assert LOG.seen == table, (sorted(table - LOG.seen), sorted(LOG.seen - table))
