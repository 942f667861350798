"""The case table of the swath -> scene gather (csrc/hsr_ortho.hip, hsr_ortho_glt) and the NumPy reference it is compared with.

Shared by tests/test_gpu_ortho_instances.py (every row on the GPU, with the library's launch record hsr_ortho_last_launch),
tests/test_gpu_ortho.py and tests/test_ortho_host.py (what the table claims, and fixture g16, on the reference alone).  Not a test
module itself; everything here is NumPy.

Mirrors of the kernel's constants: a workgroup owns PX = 64 consecutive pixels of an output row, a wave PX_WAVE = 16 of them,
AHEAD = 4 at a time (bsq: eight waves, PX_WAVE_BSQ = 8 pixels each, all 8 at a time); MAX_BANDS = 512.  Mirror of the instance selection of hsr_ortho_glt:
    layout 0   ortho_bip_kernel<kMask, kVec>: kMask = a quality or a band mask is given; kVec = bands % 4 == 0 and the swath and
               the output both start on 16 bytes (16-byte aligned float4; else dword-aligned float4 and a tail of bands % 4);
    layout 1   ortho_bsq_kernel<kMask>.
Pointer alignments are byte offsets from a 256-byte boundary, which is where the tests' buffers start.

The reference (ortho_ref) restates the operator's semantics as include/hsr.h gives them - no data, out of bounds = fill and
dropped, the value copy with `== 1` and np.unpackbits' bit order - on uint32 bit patterns, so that NaN payloads compare.
"""
import functools

import numpy as np

PX, PX_WAVE, AHEAD, PX_WAVE_BSQ, MAX_BANDS = 64, 16, 4, 8, 512
INSTANCE_COUNT = 6
I32_MAX, I32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min
BIP, BSQ = 0, 1


def _b(flag):
    return "true" if flag else "false"


def bip_vec(bands, swath_off, out_off):
    return bands % 4 == 0 and swath_off % 16 == 0 and out_off % 16 == 0


def instance(layout, bands, mask, swath_off=0, out_off=0):
    if layout == BIP:
        return f"ortho_bip_kernel<{_b(mask)}, {_b(bip_vec(bands, swath_off, out_off))}>"
    return f"ortho_bsq_kernel<{_b(mask)}>"


def all_instances():
    return [instance(BIP, b, m) for m in (False, True) for b in (3, 4)] + [instance(BSQ, 3, m) for m in (False, True)]


# =============================================================================================================================
# the reference
# =============================================================================================================================
def f32_bits(v):
    return np.float32(v).view(np.uint32)


def ortho_ref(swath, glt, window=None, qmask=None, bmask=None, fill=-9999.0, masked=-9999.0, nodata=0, layout=BIP):
    """-> (the output as uint32 bits, bip (h, w, bands) or bsq (bands, h, w); dropped)."""
    rows, cols, bands = swath.shape
    r0, c0, h, w = window if window is not None else (0, 0, glt.shape[0], glt.shape[1])
    g = glt[r0:r0 + h, c0:c0 + w].astype(np.int64)
    valid = (g[..., 0] != nodata) & (g[..., 1] != nodata)
    sx, sy = g[..., 0] - 1, g[..., 1] - 1
    inside = (sx >= 0) & (sx < cols) & (sy >= 0) & (sy < rows)
    take = valid & inside
    src = np.ascontiguousarray(swath, np.float32).view(np.uint32).copy()
    if qmask is not None:
        src[qmask == 1] = f32_bits(masked)
    if bmask is not None:
        src[np.unpackbits(bmask, axis=-1)[:, :, :bands] == 1] = f32_bits(masked)
    out = np.full((h, w, bands), f32_bits(fill), np.uint32)
    out[take] = src[sy[take], sx[take]]
    if layout == BSQ:
        out = np.ascontiguousarray(out.transpose(2, 0, 1))
    return out, int((valid & ~inside).sum())


# =============================================================================================================================
# inputs
# =============================================================================================================================
SPECIAL_BITS = [0x7fc00000, 0x7fc12345, 0xffc00001, 0x7f800001, 0x7f800000, 0xff800000, 0x80000000, 0, 1, 0x80000001, 0x007fffff]


@functools.lru_cache(maxsize=None)
def swath_of(rows, cols, bands):
    """Random bit patterns - NaN with payloads, infinities, denormals - with the special ones in band 0 of the first pixels."""
    rng = np.random.default_rng(1000 * rows + 10 * cols + bands)
    bits = rng.integers(0, 1 << 32, (rows, cols, bands), dtype=np.uint64).astype(np.uint32)
    flat = bits.reshape(-1, bands)
    n = min(len(flat), len(SPECIAL_BITS))
    flat[:n, 0] = SPECIAL_BITS[:n]
    out = bits.view(np.float32)
    out.setflags(write=False)
    return out


DROP_ENTRIES = ("one past the swath", -1, -7, I32_MAX, I32_MIN)


@functools.lru_cache(maxsize=None)
def glt_of(kind, gh, gw, rows, cols, nodata=0):
    """mixed: about 15 % no data (x only, y only, both), 15 % out of bounds (one past the swath, negatives, INT32_MAX, INT32_MIN,
    and - when no data is not 0 - the entry 0), the rest valid with repeats; valid / nodata / dropped: every cell of that kind."""
    rng = np.random.default_rng(7 * gh + 13 * gw + rows + cols + len(kind))
    g = np.stack([rng.integers(1, cols + 1, (gh, gw)), rng.integers(1, rows + 1, (gh, gw))], axis=-1).astype(np.int64)
    g[g == nodata] = 1 if nodata != 1 else 2
    common = [e for e in DROP_ENTRIES if not isinstance(e, str)] + ([0] if nodata != 0 else [])
    bad = np.array([[cols + 1] + common, [rows + 1] + common], np.int64)          # per axis: one past the swath, then the rest
    if kind == "nodata":
        which = rng.integers(0, 3, (gh, gw))
        g[..., 0][which != 1] = nodata
        g[..., 1][which != 0] = nodata
    elif kind == "dropped":
        pick, axis = rng.integers(0, bad.shape[1], (gh, gw)), rng.integers(0, 2, (gh, gw))
        g[..., 0][axis == 0] = bad[0][pick][axis == 0]
        g[..., 1][axis == 1] = bad[1][pick][axis == 1]
    elif kind == "mixed":
        u = rng.random((gh, gw))
        which = rng.integers(0, 3, (gh, gw))
        nd = u < 0.15
        g[..., 0][nd & (which != 1)] = nodata
        g[..., 1][nd & (which != 0)] = nodata
        dr = (u >= 0.15) & (u < 0.30)
        pick, axis = rng.integers(0, bad.shape[1], (gh, gw)), rng.integers(0, 2, (gh, gw))
        g[..., 0][dr & (axis == 0)] = bad[0][pick][dr & (axis == 0)]
        g[..., 1][dr & (axis == 1)] = bad[1][pick][dr & (axis == 1)]
    else:
        assert kind == "valid", kind
    out = g.astype(np.int32)
    out.setflags(write=False)
    return out


def glt_drawn(key, gh, gw, rows, cols, nodata=0):
    """Every entry on its own: a uniformly random cell of the swath (55 %: neighbours scatter over the swath's rows), a copy of its
    left neighbour (20 %), no data in x, y or both (12 %), or one of DROP_ENTRIES on one axis (13 %)."""
    rng = np.random.default_rng(list(key) + [gh, gw])
    g = np.stack([rng.integers(1, cols + 1, (gh, gw)), rng.integers(1, rows + 1, (gh, gw))], axis=-1).astype(np.int64)
    common = [e for e in DROP_ENTRIES if not isinstance(e, str)] + ([0] if nodata != 0 else [])
    bad = np.array([[cols + 1] + common, [rows + 1] + common], np.int64)
    u, which = rng.random((gh, gw)), rng.integers(0, 3, (gh, gw))
    pick, axis = rng.integers(0, bad.shape[1], (gh, gw)), rng.integers(0, 2, (gh, gw))
    nd = (u >= 0.75) & (u < 0.87)
    g[..., 0][nd & (which != 1)] = nodata
    g[..., 1][nd & (which != 0)] = nodata
    dr = u >= 0.87
    g[..., 0][dr & (axis == 0)] = bad[0][pick][dr & (axis == 0)]
    g[..., 1][dr & (axis == 1)] = bad[1][pick][dr & (axis == 1)]
    for j in range(1, gw):
        same = (u[:, j] >= 0.55) & (u[:, j] < 0.75)
        g[same, j] = g[same, j - 1]
    out = g.astype(np.int32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def qmask_of(rows, cols):
    rng = np.random.default_rng(rows * 31 + cols)
    q = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=(rows, cols), p=[0.4, 0.3, 0.15, 0.15])
    q.reshape(-1)[:4] = [0, 1, 2, 255][:q.size]
    return q


@functools.lru_cache(maxsize=None)
def bmask_of(rows, cols, bands, nbytes):
    """Random bits, the pad bits past `bands` (and the bytes past ceil(bands / 8)) set on most pixels; pixel 0 has none of the
    band bits set, the last pixel all of them."""
    rng = np.random.default_rng(rows * 17 + cols * 3 + bands + nbytes)
    un = (rng.random((rows, cols, nbytes * 8)) < 0.3).astype(np.uint8)
    un[:, :, bands:] = rng.random((rows, cols, nbytes * 8 - bands)) < 0.8
    un[0, 0, :bands] = 0
    un[-1, -1, :] = 1
    for b in (0, 7, 8, 15, bands - 2, bands - 1):
        if 0 <= b < bands:
            un[(b + 1) % rows, b % cols, b] = 1
    return np.packbits(un, axis=-1)


# =============================================================================================================================
# the case table
# =============================================================================================================================
# name -> dict(bands, rows, cols, grid, gh, gw, window, q, bbytes (0: no band mask), layout, swath_off, out_off, fill, masked,
#              nodata, count (False: dropped_dev = NULL))
ROWS = {}
BANDS = (1, 3, 4, 63, 64, 65, 285)
WIDTHS = (1, 3, PX - 1, PX, PX + 1, 2 * PX + 2)
MASKS = ((False, 0), (True, 0), (False, 1), (True, 1))                # (quality mask, band mask: 0 none, 1 given)


def make_row(bands, layout, width, height, *, rows=4, cols=5, grid="mixed", q=False, bm=0, extra_bytes=0, window=None, gh=None,
             gw=None, swath_off=0, out_off=0, fill=-9999.0, masked=-7777.5, nodata=0, count=True):
    """The row itself, registered nowhere.  grid: one of glt_of's kinds, or ("drawn", seed, index): the table of glt_drawn."""
    gh, gw = gh or height, gw or width
    return dict(bands=bands, rows=rows, cols=cols, grid=grid, gh=gh, gw=gw, window=window or (0, 0, height, width), q=q,
                bbytes=((bands + 7) // 8 + extra_bytes) if bm else 0, layout=layout, swath_off=swath_off, out_off=out_off,
                fill=fill, masked=masked, nodata=nodata, count=count)


def _row(name, *args, **kw):
    assert name not in ROWS, name
    ROWS[name] = make_row(*args, **kw)


# every band count x layout x width; heights 1 and 3, the mask combinations and the base offsets rotate through the rows
_k = 0
for _bands in BANDS:
    for _layout in (BIP, BSQ):
        for _wi, _w in enumerate(WIDTHS):
            _q, _bm = MASKS[_k % 4]
            _so, _oo = ((0, 0), (4, 8), (16, 0), (12, 4), (0, 32), (8, 12))[(_k // 4) % 6] if _k % 3 else (0, 0)
            _row(f"b{_bands}-{'bip' if _layout == BIP else 'bsq'}-w{_w}", _bands, _layout, _w, 3 if _wi % 2 else 1, q=_q, bm=_bm,
                 extra_bytes=_k % 2, swath_off=_so, out_off=_oo)
            _k += 1
# every pair of base offsets for the float4 path and its fallback (bands % 4 == 0), and the offsets for shapes that never take it
for _so in (0, 4, 8, 12):
    for _oo in (0, 4, 8, 12):
        _row(f"align-b4-bip-s{_so}-o{_oo}", 4, BIP, PX + 1, 3, swath_off=_so, out_off=_oo, q=_so == 8, bm=int(_oo == 8))
    _row(f"align-b64-bip-s{_so}", 64, BIP, 5, 1, swath_off=_so, out_off=(16 - _so) % 16)
    _row(f"align-b285-bip-s{_so}", 285, BIP, 5, 1, swath_off=_so, out_off=_so)
    _row(f"align-b3-bsq-s{_so}", 3, BSQ, PX + 1, 3, swath_off=_so, out_off=(_so + 4) % 16)
_row("align-b64-bip-16-on", 64, BIP, 5, 1, swath_off=16, out_off=48, q=True)
# grids of one kind
for _grid in ("nodata", "valid", "dropped"):
    for _layout in (BIP, BSQ):
        for _bands in (3, 285):
            _row(f"{_grid}-b{_bands}-{'bip' if _layout == BIP else 'bsq'}", _bands, _layout, PX + 1, 3, grid=_grid, q=True, bm=1)
# every mask combination per layout, a byte pitch larger than needed (EMIT: 36 for 285 bands), pad bits set
for _q, _bm in MASKS:
    for _layout in (BIP, BSQ):
        for _bands, _extra in ((3, 2), (64, 1), (285, 0)):
            _row(f"mask-q{int(_q)}-b{_bm}-b{_bands}-{'bip' if _layout == BIP else 'bsq'}", _bands, _layout, PX + 3, 3, q=_q, bm=_bm,
                 extra_bytes=_extra, rows=6, cols=7)
# windows of a larger grid at offsets that are no multiple of PX, and a 1 x 1 window
for _layout in (BIP, BSQ):
    _n = "bip" if _layout == BIP else "bsq"
    _row(f"window-b5-{_n}", 5, _layout, 70, 3, gh=6, gw=150, window=(1, 7, 3, 70), q=True)
    _row(f"window-b285-{_n}", 285, _layout, PX, 2, gh=5, gw=150, window=(3, 65, 2, PX), bm=1, extra_bytes=0)
    _row(f"window-1x1-{_n}", 7, _layout, 1, 1, gh=5, gw=150, window=(2, 65, 1, 1))
    _row(f"window-1x1-dropped-{_n}", 7, _layout, 1, 1, gh=5, gw=150, window=(4, 149, 1, 1), grid="dropped")
    # no counter; a NaN fill; a no-data value other than 0, under which the entry 0 points outside the swath
    _row(f"no-counter-{_n}", 65, _layout, PX + 1, 3, count=False, q=True, bm=1)
    _row(f"nan-fill-{_n}", 3, _layout, PX + 1, 3, fill=float("nan"), masked=float("inf"), q=True)
    _row(f"nodata-7-{_n}", 4, _layout, PX + 1, 3, nodata=7, rows=9, cols=9)
    _row(f"max-bands-{_n}", MAX_BANDS, _layout, PX + 1, 1, bm=1)


def instance_of(r):
    return instance(r["layout"], r["bands"], r["q"] or r["bbytes"] > 0, r["swath_off"], r["out_off"])


def row_instance(name):
    return instance_of(ROWS[name])


@functools.lru_cache(maxsize=None)
def case(name):
    return case_of(ROWS[name])


def case_of(r):
    """-> dict(swath, glt, qmask, bmask, ref (uint32 bits in the row's layout), ref_bip, dropped): the row's inputs and reference."""
    swath = swath_of(r["rows"], r["cols"], r["bands"])
    if isinstance(r["grid"], tuple):
        glt = glt_drawn(r["grid"][1:], r["gh"], r["gw"], r["rows"], r["cols"], r["nodata"])
    else:
        glt = glt_of(r["grid"], r["gh"], r["gw"], r["rows"], r["cols"], r["nodata"])
    qmask = qmask_of(r["rows"], r["cols"]) if r["q"] else None
    bmask = bmask_of(r["rows"], r["cols"], r["bands"], r["bbytes"]) if r["bbytes"] else None
    kw = dict(window=r["window"], qmask=qmask, bmask=bmask, fill=r["fill"], masked=r["masked"], nodata=r["nodata"])
    ref, dropped = ortho_ref(swath, glt, layout=r["layout"], **kw)
    ref_bip, _ = ortho_ref(swath, glt, layout=BIP, **kw)
    return dict(swath=swath, glt=glt, qmask=qmask, bmask=bmask, ref=ref, ref_bip=ref_bip, dropped=dropped)
