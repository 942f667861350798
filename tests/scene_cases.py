"""The case tables of the scene kernels (csrc/hsr_scene.hip) and the references they are compared with.

Shared by tests/test_gpu_scene_instances.py (every row on the GPU, with the library's launch record hsr_scene_last_launch) and
tests/test_scene_instances_host.py (what the tables claim about every row, on the references alone).  Not a test module itself;
everything here is NumPy.

Every row carries the instance it must reach.  The name comes from a mirror of the selection rules of the four entry points:
  scan     scene_black_kernel<T>: the scene's dtype;
  gather   scene_gather_kernel<TI, TO, kEncode, kVec>: kVec = tw % 4 == 0 and the output on a 4-sample boundary (16 bytes for
           float32, 8 for uint16);
  mosaic   scene_mosaic_kernel<kVec>: kVec = W % 4 == 0 and tw % 4 == 0 and both bases on 16 bytes;
  blend    scene_blend_kernel<kVec, KMAX>: kVec as the mosaic and sx % 4 == 0; KMAX = K = (th / sy)(tw / sx) rounded up to 1, 2, 4,
           8 or 16.
Pointer alignments are byte offsets from a 256-byte boundary, which is where the tests' buffers start.  The loop mirrors
(scan_rows_per_wave, gather_trips, row_trips) restate the grid arithmetic, so that a row can claim a second trip of a loop.

References:
  scan     black_mask_np: the contract of the reference's is_black_mask - np.isclose(arr, v, atol=nodata_atol),
           np.abs(arr) < zero_atol, .all(axis=0) and the three-way OR on the array in its own dtype, so NumPy decides every edge -
           then window_counts;
  gather   NumPy slicing for bits, oracle_np.tile_encode_u16 for the encoding form;
  mosaic   assemble (the NumPy assembly test_gpu_scene_tiles.py uses too);
  blend    blend_ref64 / check_blend of test_scene_blend_host.py, unchanged.
"""
import functools

import numpy as np

from oracle import oracle_np as onp
from test_gpu_scene_blend import make_case
from test_scene_blend_host import blend_ref64
from test_scene_tiles_host import window_counts

F32, U16 = np.dtype(np.float32), np.dtype(np.uint16)
DT_CODE = {F32: 0, U16: 2}                      # the dtype codes of the C entry points
INSTANCE_COUNT = 20


# =============================================================================================================================
# the selection rules, mirrored
# =============================================================================================================================
def _t(dtype):
    return {F32: "float", U16: "uint16_t"}[np.dtype(dtype)]


def _b(flag):
    return "true" if flag else "false"


def scan_instance(dtype):
    return f"scene_black_kernel<{_t(dtype)}>"


def gather_vec(out_dtype, tw, out_off):
    return tw % 4 == 0 and out_off % (4 * np.dtype(out_dtype).itemsize) == 0


def gather_instance(dtype, encode, tw, out_off):
    out = U16 if encode else np.dtype(dtype)
    return f"scene_gather_kernel<{_t(dtype)}, {_t(out)}, {_b(encode)}, {_b(gather_vec(out, tw, out_off))}>"


def mosaic_vec(W, tw, out_off, cubes_off):
    return W % 4 == 0 and tw % 4 == 0 and out_off % 16 == 0 and cubes_off % 16 == 0


def mosaic_instance(W, tw, out_off=0, cubes_off=0):
    return f"scene_mosaic_kernel<{_b(mosaic_vec(W, tw, out_off, cubes_off))}>"


def blend_vec(W, tw, sx, out_off, cubes_off):
    return W % 4 == 0 and tw % 4 == 0 and sx % 4 == 0 and out_off % 16 == 0 and cubes_off % 16 == 0


def blend_kmax(K):
    return next(k for k in (1, 2, 4, 8, 16) if K <= k)


def blend_instance(W, th, tw, sy, sx, out_off=0, cubes_off=0):
    return f"scene_blend_kernel<{_b(blend_vec(W, tw, sx, out_off, cubes_off))}, {blend_kmax((th // sy) * (tw // sx))}>"


def all_instances():
    names = [scan_instance(d) for d in (F32, U16)]
    names += [gather_instance(d, e, tw, 0) for d, e in ((F32, False), (U16, False), (F32, True)) for tw in (7, 8)]
    names += [mosaic_instance(W, 8) for W in (31, 36)]
    names += [blend_instance(W, k, sx, 1, sx) for W, sx in ((31, 3), (36, 4)) for k in (1, 2, 4, 8, 16)]
    return names


def scan_rows_per_wave(H, W, th, tw):
    """Rows a wave of hsr_scene_black_counts walks: as many as leave about 16 Ki waves, at most 64, enough for the grid's y."""
    ny, nx = H // th, W // tw
    waves = (nx * tw + 63) // 64 * (ny * th)
    rows = min(max(waves // 16384, 1), 64)
    while (ny * th + rows - 1) // rows > 65535:
        rows *= 2
    return rows


def gather_trips(th, tw, vec):
    """Trips of the gather's chunk loop: grid x is capped at 1024 workgroups of 256 threads."""
    n = th * tw // 4 if vec else th * tw
    grid = min((n + 255) // 256, 1024)
    return -(-n // (grid * 256))


def row_trips(T, H, W, vec):
    """(gridDim.y, trips of the row loop) of the mosaic and the blend: about 64 Ki workgroups, rows strided over them."""
    gx = ((W // 4 if vec else W) + 255) // 256
    gy = min(max(65536 // (gx * T), 1), H)
    return gy, -(-H // gy)


# =============================================================================================================================
# scan
# =============================================================================================================================
def black_mask_np(arr, nodata=None, masked_val=-0.01, nodata_atol=1e-3, zero_atol=1e-6):
    """The contract: is_black_mask's statements on ``arr`` in its own dtype; the values are Python floats, as its caller passes
    them.  A non-finite ``nodata`` makes NumPy subtract infinities: the warnings are silenced, the result is NumPy's."""
    with np.errstate(invalid="ignore"):
        masked = np.isclose(arr, masked_val, atol=nodata_atol).all(axis=0)
        zero = (np.abs(arr) < zero_atol).all(axis=0)
        if nodata is None:
            return masked | zero
        return np.isclose(arr, nodata, atol=nodata_atol).all(axis=0) | masked | zero


def scan_ref(scene, th, tw, **kw):
    return window_counts(black_mask_np(scene, **kw), th, tw)


def scan_row(dtype, bands, H, W, th, tw, nodata=None, masked_val=-0.01, nodata_atol=1e-3, zero_atol=1e-6, passed=0.0, key=0, density=0.3):
    """One scan call on a scene of its own (planted_scene): the shape, the window, the settings of the call - nodata None: the
    criterion is off and `passed` goes to the entry point instead - and what picks the scene."""
    return dict(dtype=np.dtype(dtype), bands=bands, H=H, W=W, th=th, tw=tw, nodata=nodata, masked_val=masked_val, nodata_atol=nodata_atol,
                zero_atol=zero_atol, passed=passed, key=key, density=density)


def scan_settings(r):
    return {k: r[k] for k in ("nodata", "masked_val", "nodata_atol", "zero_atol")}


@functools.lru_cache(maxsize=64)
def planted_scene(dtype, bands, H, W, key, density=0.3):
    """Valid noise with black pixels planted at random: about `density` of the pixels hold one black value of BLACK_VALUES in
    every band, and half of those are broken in one random band - by a valid sample or by a sample beside a tolerance edge
    (f32_edge_values() / U16_SAMPLES) - so that the band which decides a pixel, and ends a wave's band loop, is random."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng([key, bands, H, W, dtype.itemsize])
    if dtype == F32:
        scene, near = rng.uniform(0.05, 0.6, (bands, H, W)).astype(np.float32), f32_edge_values()
    else:
        scene, near = rng.integers(1, 4000, (bands, H, W)).astype(np.uint16), np.array(U16_SAMPLES, np.uint16)
    values = np.array(list(BLACK_VALUES[dtype].values()), dtype)
    black = rng.random((H, W)) < density
    scene[:, black] = values[rng.integers(0, len(values), int(black.sum()))]
    ys, xs = np.nonzero(black & (rng.random((H, W)) < 0.5))
    b = rng.integers(0, bands, len(ys))
    scene[b, ys, xs] = np.where(rng.random(len(ys)) < 0.5, near[rng.integers(0, len(near), len(ys))], scene[b, (ys + 1) % H, xs])
    scene.setflags(write=False)
    return scene


def scan_case_of(r):
    scene = planted_scene(r["dtype"], r["bands"], r["H"], r["W"], r["key"], r["density"])
    return dict(scene=scene, ref=scan_ref(scene, r["th"], r["tw"], **scan_settings(r)))


def scan_tilings(H, W):
    """(1, 1): a wave meets 64 windows in a row; one window; (5, 3); a new window row on every row; window edges on and off the
    wave boundaries."""
    return [(1, 1), (H, W), (5, 3), (1, W), (3, 64), (3, 65)]


# ---- the deciding band --------------------------------------------------------------------------------------------------------
DECIDING_BANDS = (1, 2, 8, 9, 10, 17)
DECIDING_HW = (5, 150)                          # three waves a row, the third of 22 lanes
BLACK_VALUES = {F32: {"nodata": -9999.0, "masked": -0.01, "zero": 0.0}, U16: {"nodata": 65535, "zero": 0}}
# (settings of the call, the kinds of black value that count under them).  uint16: -0.01 is no sample, so the masked predicate is
# reached through nodata_atol = 0.02, which brings 0 within reach of -0.01, with the zero predicate switched off (zero_atol = 0).
DECIDING_SETTINGS = {
    F32: [(dict(nodata=-9999.0), ("nodata", "masked", "zero")), (dict(nodata=None), ("masked", "zero"))],
    U16: [(dict(nodata=65535.0), ("nodata", "zero")), (dict(nodata=65535.0, nodata_atol=0.02, zero_atol=0.0), ("nodata", "zero")),
          (dict(nodata=None), ("zero",))],
}


@functools.lru_cache(maxsize=None)
def deciding_scene(dtype, bands):
    """-> (scene (bands, 5, 150), cls (5, 150): index into specs or -1 for a valid background pixel, specs).  A spec is
    (kind, variant, k): ``all`` holds the kind's black value in every band; ``broken`` in every band but k, which is valid;
    ``band0_valid`` in every band but 0; ``mixed`` holds a black value in every band, of alternating kinds.  Only ``all`` counts.
    Row 0 is valid (waves without a live lane after band 0), row 1 holds two lone pixels (waves with a single live lane), rows 2
    and 3 hold every spec in runs of 2 and of 1 at different phases of the wave, row 4 a full black wave and a part of one."""
    dtype = np.dtype(dtype)
    H, W = DECIDING_HW
    rng = np.random.default_rng(100 + bands + dtype.itemsize)
    if dtype == F32:
        scene = rng.uniform(0.05, 0.6, (bands, H, W)).astype(np.float32)
    else:
        scene = rng.integers(1, 4000, (bands, H, W)).astype(np.uint16)
    values = BLACK_VALUES[dtype]
    kinds = list(values)
    ks = sorted({k for k in (0, 1, 8, 9, bands - 1) if k < bands})
    specs = []
    for kind in kinds:
        specs.append((kind, "all", None))
        specs += [(kind, "broken", k) for k in ks]
        if bands > 1:
            specs.append((kind, "band0_valid", None))
    if bands > 1:
        specs.append(("mixed", "mixed", None))
    cls = np.full((H, W), -1, np.int64)

    def put(y, x, s):
        kind, variant, k = specs[s]
        keep = scene[:, y, x].copy()
        if variant == "mixed":
            scene[:, y, x] = [values[kinds[b % len(kinds)]] for b in range(bands)]
        else:
            scene[:, y, x] = values[kind]
            if variant == "broken":
                scene[k, y, x] = keep[k]
            elif variant == "band0_valid":
                scene[0, y, x] = keep[0]
        cls[y, x] = s

    last_broken = max(s for s, sp in enumerate(specs) if sp[1] == "broken")
    zero_all = next(s for s, sp in enumerate(specs) if sp[:2] == ("zero", "all"))      # zero counts under every setting
    put(1, 70, zero_all)
    put(1, 140, last_broken)
    for s in range(len(specs)):
        for x in (1 + 5 * s, 2 + 5 * s):
            put(2, x, s)
        put(3, 3 + 6 * (len(specs) - 1 - s), s)
    for x in range(0, 64):
        put(4, x, zero_all)
    for x in range(64, 101):
        put(4, x, 0)
    for x in range(101, W, 2):
        put(4, x, last_broken)
    return scene, cls, tuple(specs)


def intended_black(spec, enabled):
    return spec[1] == "all" and spec[0] in enabled


# ---- float32 samples on the edges of the tolerances -------------------------------------------------------------------------------
MASKED_VAL, ZERO_ATOL = -0.01, 1e-6
F32_EDGE_SETS = [(-9999.0, 1e-3), (0.3, 1e-3), (-0.01, 1e-6), (7.0, 0.0)]          # (nodata, nodata_atol)
# every call on the edge scene: the finite sets, a non-finite nodata that is in use, and a NaN that is passed but not in use
F32_EDGE_CALLS = [dict(nodata=nd, nodata_atol=atol) for nd, atol in F32_EDGE_SETS]
F32_EDGE_CALLS += [dict(nodata=float("inf")), dict(nodata=float("-inf")), dict(nodata=float("nan")),
                   dict(nodata=None, passed=float("nan"))]
F32_EDGE_CENTERS = (-9999.0, 0.3, -0.01, 7.0, 0.0)


def around(x, n=3):
    """float32(x) and its n neighbours on either side."""
    c = np.float32(x)
    lo, hi, out = c, c, [c]
    for _ in range(n):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return out


def f32_edge_points(nodata, nodata_atol):
    """The two edges of np.isclose's interval round ``nodata`` and round the masked value, as float64."""
    out = []
    for c in (nodata, MASKED_VAL):
        tol = nodata_atol + 1e-5 * abs(c)
        out += [c - tol, c + tol]
    return out


@functools.lru_cache(maxsize=None)
def f32_edge_values():
    vals = []
    for nd, atol in F32_EDGE_SETS:
        for e in f32_edge_points(nd, atol) + [nd, MASKED_VAL]:
            vals += around(e)
    vals += around(ZERO_ATOL) + around(-ZERO_ATOL)
    vals += [np.float32(v) for v in (-0.0, 0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.17549435e-38, np.inf, -np.inf, np.nan)]
    bits = np.array(vals, np.float32).view(np.uint32).tolist() + [0x7fc12345, 0xffc00000]
    return np.array(sorted(set(bits)), np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def f32_edge_scene():
    """-> (scene (3, H, 150), vals).  Flat pixel i (1 + C) holds value i in all three bands; pixel i (1 + C) + 1 + j holds it in
    band 1 between two samples that are exactly centre j of F32_EDGE_CENTERS, so band 1 decides; the rest is valid."""
    vals = f32_edge_values()
    C = len(F32_EDGE_CENTERS)
    n = len(vals) * (1 + C)
    W = 150
    H = -(-n // W)
    flat = np.full((3, H * W), np.float32(0.25), np.float32)
    for i, v in enumerate(vals.view(np.uint32)):
        p = i * (1 + C)
        flat.view(np.uint32)[:, p] = v
        for j, c in enumerate(F32_EDGE_CENTERS):
            flat[:, p + 1 + j] = np.float32(c)
            flat.view(np.uint32)[1, p + 1 + j] = v
    return flat.reshape(3, H, W), vals


def ref_kwargs(call):
    """A call's settings as the reference takes them (``passed`` is what goes to the C entry point when nodata is not in use)."""
    return {k: v for k, v in call.items() if k != "passed"}


# ---- uint16 samples ------------------------------------------------------------------------------------------------------------------
U16_SAMPLES = (0, 1, 2, 100, 101, 65534, 65535)
U16_EDGE_CALLS = [dict(nodata=nd, nodata_atol=atol, zero_atol=z) for z in (1e-6, 1.5, 0.0)
                  for nd, atol in ((65535.0, 1e-3), (65535.0, 1.0), (100.5, 0.5))]
U16_EDGE_CALLS += [dict(nodata=None, nodata_atol=0.02), dict(nodata=65535.0, nodata_atol=0.02)]


@functools.lru_cache(maxsize=None)
def u16_edge_scene():
    """(3, 2, 70): pixel p holds sample p % 7 in bands 0 and 2 and sample (p // 7) % 7 in band 1: every pair, twice and more."""
    p = np.arange(140)
    s = np.array(U16_SAMPLES, np.uint16)
    a, b = s[p % 7], s[(p // 7) % 7]
    return np.stack([a, b, a]).reshape(3, 2, 70)


# ---- window indexing -------------------------------------------------------------------------------------------------------------------
STRIP_TILE = (4, 48)                            # 2 x 2 windows on (11, 140): a strip of 44 columns right of them, of 3 rows below


@functools.lru_cache(maxsize=None)
def strip_scenes(dtype):
    """-> (scene whose remainder strips are black, the same scene with valid strips); about half of the window pixels are black."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(31 + dtype.itemsize)
    H, W = 11, 140
    th, tw = STRIP_TILE
    valid = rng.uniform(0.05, 0.6, (2, H, W)).astype(np.float32) if dtype == F32 else rng.integers(1, 4000, (2, H, W)).astype(np.uint16)
    inner = valid.copy()
    density = np.full((H, W), 0.5)
    for wy in range(H // th):
        for wx in range(W // tw):                           # a density of its own for every window: four different counts
            density[wy * th:(wy + 1) * th, wx * tw:(wx + 1) * tw] = 0.2 + 0.2 * (wy * (W // tw) + wx)
    inner[:, rng.random((H, W)) < density] = 0
    inner[:, H // th * th:, :] = valid[:, H // th * th:, :]
    inner[:, :, W // tw * tw:] = valid[:, :, W // tw * tw:]
    black = inner.copy()
    black[:, H // th * th:, :] = 0
    black[:, :, W // tw * tw:] = 0
    return black, inner


# ---- float32, several rows per wave --------------------------------------------------------------------------------------------------
LARGE_HW = (2100, 1024)
LARGE_TILINGS = [(1, 1024), (3, 5), (7, 64), (2100, 1024)]       # second window on every row; evictions; both; one window


@functools.lru_cache(maxsize=None)
def large_f32_scene():
    """(1, 2100, 1024) float32, about half black: noise plus blocks, black samples of all three kinds (one band: each decides)."""
    rng = np.random.default_rng(77)
    H, W = LARGE_HW
    scene = rng.uniform(0.05, 0.6, (1, H, W)).astype(np.float32)
    black = rng.random((H, W)) < 0.4
    black[300:900, 100:500] = True
    black[1500:1600, :] = True
    black[1000:1400, 600:1000] = False
    kind = rng.integers(0, 3, (H, W))
    scene[0][black] = np.array([-9999.0, -0.01, 0.0], np.float32)[kind[black]]
    return scene


# =============================================================================================================================
# gather
# =============================================================================================================================
GATHER_SHAPE = (3, 21, 27)
ENC_ND, ENC_PLAIN, ENC_SMALL = (10000.0, 1, -9999.0, 65535), (10000.0, 0, 0.0, 65535), (2000.0, 0, 0.0, 4000)
F32_SPECIAL_BITS = [0x7fc00000, 0x7fc12345, 0xffc00001, 0x7f800000, 0xff800000, 0x80000000]
F32_SPECIAL_VALUES = [-9999.0, 3e6, -3e6, 1e5, 214748.36, 214748.38, 6.5535, 6.55345, 0.39995, 0.00005, 0.00015, -0.00004, 1.99975, 2.0]


@functools.lru_cache(maxsize=None)
def gather_scene(dtype, shape=GATHER_SHAPE):
    """float32: noise with NaN (a payload among them), +-Inf, -0.0, the source nodata, values whose product with the scale
    overflows int32 (3e6 x 1e4, which the writer's cast turns into INT32_MIN and the clip into 0), is clipped from above (1e5 x 1e4)
    or ties (x.5), one in every 7 samples; uint16: every code is as good as any other."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(5 + dtype.itemsize + shape[1])
    if dtype == U16:
        return rng.integers(0, 65536, shape).astype(np.uint16)
    x = (rng.standard_normal(shape) * 0.3).astype(np.float32)
    pool = np.concatenate([np.array(F32_SPECIAL_BITS, np.uint32), np.array(F32_SPECIAL_VALUES, np.float32).view(np.uint32)])
    where = np.flatnonzero(rng.random(x.size) < 1 / 7)
    x.reshape(-1).view(np.uint32)[where] = pool[np.arange(len(where)) % len(pool)]
    return x


def gather_origins(th, tw, H=GATHER_SHAPE[1], W=GATHER_SHAPE[2]):
    """Columns of every residue mod 4, the last row and the last column, a duplicate - and, between them, four windows that leave
    the scene (a negative origin, an origin one past the last valid one): their slices stay as they were."""
    valid = [(0, 0), (1, 1), (2, 2), (3, 3), (H - th, W - tw), (H - th, 0), (0, W - tw), (1, 1)]
    bad = [(-1, 0), (0, -1), (H - th + 1, 0), (0, W - tw + 1)]
    out = []
    for i, v in enumerate(valid):
        out.append(v)
        if i % 2 == 1:
            out.append(bad[i // 2])
    return np.array(out, np.int32)


def origin_inside(r, c, th, tw, H, W):
    return 0 <= r <= H - th and 0 <= c <= W - tw


def gather_ref(scene, origins, th, tw, encode):
    """-> (want (P, bands, th, tw) in the output dtype - zeros in the slices of windows outside the scene - and inside (P,))."""
    bands, H, W = scene.shape
    out = np.zeros((len(origins), bands, th, tw), np.uint16 if encode else scene.dtype)
    inside = np.array([origin_inside(r, c, th, tw, H, W) for r, c in origins])
    for p, (r, c) in enumerate(origins):
        if inside[p]:
            tile = scene[:, r:r + th, c:c + tw]
            out[p] = onp.tile_encode_u16(tile, encode[2] if encode[1] else None, encode[0], encode[3]) if encode else tile
    return out, inside


# name -> (dtype, encode, scene shape, origins, th, tw, output offset in bytes)
GATHER_ROWS = {}


def gather_row(dtype, encode, th, tw, off, shape=GATHER_SHAPE, origins=None):
    """The row itself, registered nowhere."""
    org = gather_origins(th, tw, shape[1], shape[2]) if origins is None else np.array(origins, np.int32).reshape(-1, 2)
    return (np.dtype(dtype), encode, tuple(shape), org, th, tw, off)


def _gather_row(name, *args, **kw):
    GATHER_ROWS[name] = gather_row(*args, **kw)


def gather_case_of(row):
    """-> dict(scene, want, inside): the row's scene (gather_scene of its dtype and shape) and gather_ref on it."""
    dtype, encode, shape, org, th, tw, _ = row
    scene = gather_scene(dtype, shape)
    want, inside = gather_ref(scene, org, th, tw, encode)
    return dict(scene=scene, want=want, inside=inside)


def gather_instance_of(row):
    dtype, encode, _, _, _, tw, off = row
    return gather_instance(dtype, encode is not None, tw, off)


for _d, _n, _e, _sz in ((F32, "f32", None, 4), (U16, "u16", None, 2), (F32, "enc_nd", ENC_ND, 2), (F32, "enc_plain", ENC_PLAIN, 2),
                        (F32, "enc_small", ENC_SMALL, 2)):
    _gather_row(f"{_n}-6x8-aligned", _d, _e, 6, 8, 0)                    # vector
    _gather_row(f"{_n}-6x8-one-sample-off", _d, _e, 6, 8, _sz)           # the same shape one sample past the boundary: scalar
    _gather_row(f"{_n}-6x8-next-boundary", _d, _e, 6, 8, 4 * _sz)        # 16 (8) bytes on: vector again
    _gather_row(f"{_n}-3x4-aligned", _d, _e, 3, 4, 0)
    _gather_row(f"{_n}-5x7", _d, _e, 5, 7, 0)
    _gather_row(f"{_n}-4x1", _d, _e, 4, 1, _sz)
# the chunk loop: more samples (quads) in one tile plane than 1024 workgroups x 256 threads
CHUNK_SCALAR, CHUNK_VEC = (1, 517, 520), (1, 1030, 1028)
_gather_row("chunk-scalar-u16", U16, None, 515, 513, 0, CHUNK_SCALAR, [(2, 7)])
_gather_row("chunk-scalar-enc", F32, ENC_ND, 515, 513, 0, CHUNK_SCALAR, [(2, 7)])
_gather_row("chunk-vec-f32", F32, None, 1028, 1024, 0, CHUNK_VEC, [(2, 3), (2, 4)])    # an odd and an aligned source column
GATHER_CHUNK_ROWS = ("chunk-scalar-u16", "chunk-scalar-enc", "chunk-vec-f32")


def gather_row_instance(name):
    return gather_instance_of(GATHER_ROWS[name])


# =============================================================================================================================
# mosaic
# =============================================================================================================================
def assemble(cubes, slot, out, th, tw, fill, fill_rest):
    """hsr_scene_mosaic in NumPy, on a copy of the prefilled output."""
    out = out.copy()
    ny, nx = slot.shape
    if fill_rest:
        out[:, ny * th:, :] = fill
        out[:, :, nx * tw:] = fill
    for wy in range(ny):
        for wx in range(nx):
            s, win = slot[wy, wx], (slice(None), slice(wy * th, (wy + 1) * th), slice(wx * tw, (wx + 1) * tw))
            if 0 <= s < len(cubes):
                out[win] = cubes[s]
            elif s == -1:
                out[win] = fill
    return out


# name -> (T, H, W, th, tw, P, output offset, stack offset, [(fill, fill_rest)])
NAN32 = np.float32(np.nan)
BOTH = ((NAN32, True), (np.float32(7.25), False))
MOSAIC_ROWS = {
    "vec-36-8": (3, 23, 36, 6, 8, 4, 0, 0, BOTH),                   # 3 x 4 windows, a 5-row strip below and a strip right of them
    "scalar-31-8": (3, 23, 31, 6, 8, 4, 0, 0, BOTH),
    "scalar-36-6": (3, 23, 36, 6, 6, 4, 0, 0, BOTH),
    "scalar-30-7": (3, 23, 30, 6, 7, 4, 0, 0, BOTH),
    "stack-4-bytes-off": (3, 23, 36, 6, 8, 4, 0, 4, BOTH),          # the vector shape: scalar
    "output-4-bytes-off": (3, 23, 36, 6, 8, 4, 4, 0, BOTH),
    "both-16-bytes-on": (3, 23, 36, 6, 8, 4, 16, 16, BOTH),         # vector
    "no-cubes": (3, 23, 36, 6, 8, 0, 0, 0, BOTH),                   # P = 0, a NULL stack: fill only
    "row-loop-vec": (2048, 70, 12, 6, 4, 5, 0, 0, BOTH[:1]),        # gridDim.y = 32: rows y, y + 32, y + 64
    "row-loop-scalar": (2048, 70, 13, 6, 4, 5, 0, 0, BOTH[1:]),
    "z-limit": (65535, 3, 4, 1, 4, 2, 0, 0, BOTH[:1]),              # gridDim.y = 1: one workgroup walks all three rows
}
MOSAIC_ROW_LOOP = {"row-loop-vec": 32, "row-loop-scalar": 32, "z-limit": 1}         # the gridDim.y a row claims


@functools.lru_cache(maxsize=None)
def mosaic_case(name):
    return mosaic_case_of(MOSAIC_ROWS[name], sum(map(ord, name)))


def mosaic_case_of(row, seed, drawn_slots=False):
    """-> (cubes (P, T, th, tw) with a NaN and a NaN payload, slot (H // th, W // tw)): cubes used once, twice and not at all,
    -1 (fill), -2 (leave alone) and an index past the stack (leave alone) - in the table's fixed pattern, or (drawn_slots) every
    slot drawn on its own from -2 .. P + 2."""
    T, H, W, th, tw, P, *_ = row
    rng = np.random.default_rng(seed)
    cubes = rng.standard_normal((P, T, th, tw)).astype(np.float32)
    if P:                                                  # both in cube 0, which every slot grid uses
        cubes[0, 0, th // 2, tw - 1] = np.nan
        cubes.view(np.uint32)[0, T - 1, 0, 0] = 0x7fc12345
    ny, nx = H // th, W // tw
    slot = np.full(ny * nx, -1, np.int32)
    pattern = [0, 3, -2, 1, 2, 0, 9, -2, -1, 4]
    slot[:] = rng.integers(-2, P + 3, ny * nx) if drawn_slots else [pattern[i % len(pattern)] for i in range(ny * nx)]
    slot[-1] = -1
    return cubes, slot.reshape(ny, nx)


def mosaic_instance_of(row):
    _, _, W, _, tw, P, out_off, cubes_off, _ = row
    return mosaic_instance(W, tw, out_off, cubes_off if P else 0)


def mosaic_row_instance(name):
    return mosaic_instance_of(MOSAIC_ROWS[name])


# =============================================================================================================================
# blend
# =============================================================================================================================
LATTICES = [(1, 1), (2, 1), (1, 2), (3, 1), (2, 2), (1, 4), (4, 1), (5, 1), (2, 4), (3, 3), (3, 4), (4, 4)]    # ky x kx


def blend_geometry(ky, kx, vec):
    """(th, tw, sy, sx, H, W): four lattice steps of room in both directions and a remainder row; the vector geometry has tw, sx
    and W multiples of 4, the scalar one a pitch of 3 columns and a remainder column."""
    sy, sx = (3 if ky <= 2 else 2), (4 if vec else 3)
    th, tw = sy * ky, sx * kx
    return th, tw, sy, sx, th + 4 * sy + 1, tw + 4 * sx + (0 if vec else 1)


# name -> dict(th, tw, sy, sx, H, W, T, out_off, cubes_off, kind)
BLEND_ROWS = {}
for _ky, _kx in LATTICES:
    for _vec in (True, False):
        _th, _tw, _sy, _sx, _H, _W = blend_geometry(_ky, _kx, _vec)
        BLEND_ROWS[f"{_ky}x{_kx}-{'vec' if _vec else 'scalar'}"] = dict(th=_th, tw=_tw, sy=_sy, sx=_sx, H=_H, W=_W, T=3, kind="lattice")
BLEND_ROWS["short-table"] = dict(th=6, tw=8, sy=3, sx=4, H=19, W=24, T=3, kind="short")        # 2 x 2, fewer rows / columns of cells
BLEND_ROWS["tile-taller-than-output"] = dict(th=8, tw=8, sy=4, sx=4, H=5, W=36, T=3, kind="nofit")
BLEND_ROWS["tile-wider-than-output"] = dict(th=8, tw=8, sy=4, sx=4, H=23, W=4, T=3, kind="nofit")
BLEND_ROWS["row-loop"] = dict(th=8, tw=8, sy=4, sx=4, H=70, W=12, T=2048, kind="rowloop")      # K = 4, vector, gridDim.y = 32
BLEND_ROWS["output-4-bytes-off"] = dict(th=6, tw=8, sy=3, sx=4, H=19, W=24, T=3, kind="lattice", out_off=4)
BLEND_ROWS["stack-4-bytes-off"] = dict(th=6, tw=8, sy=3, sx=4, H=19, W=24, T=3, kind="lattice", cubes_off=4)
for _r in BLEND_ROWS.values():
    _r.setdefault("out_off", 0)
    _r.setdefault("cubes_off", 0)


def blend_row(th, tw, sy, sx, H, W, T=3, kind="lattice", out_off=0, cubes_off=0):
    """The row itself, registered nowhere."""
    return dict(th=th, tw=tw, sy=sy, sx=sx, H=H, W=W, T=T, kind=kind, out_off=out_off, cubes_off=cubes_off)


def blend_instance_of(r):
    return blend_instance(r["W"], r["th"], r["tw"], r["sy"], r["sx"], r["out_off"], r["cubes_off"])


def blend_row_instance(name):
    return blend_instance_of(BLEND_ROWS[name])


@functools.lru_cache(maxsize=None)
def blend_case(name):
    return blend_case_of(BLEND_ROWS[name], sum(map(ord, name)))


def blend_case_of(r, seed):
    """-> dict(cubes, start, K, ref): make_case of test_gpu_scene_blend.py for the row's geometry (holes, bad and spare entries, NaN,
    a payload, an all-NaN pixel), with a start table cut short, or whose tile does not fit, or more or fewer planes, where the row
    says so; ref is blend_ref64 of exactly what the kernel is given."""
    th, tw, sy, sx, H, W, T = (r[k] for k in ("th", "tw", "sy", "sx", "H", "W", "T"))
    if r["kind"] == "nofit":                               # make_case needs room for a window: build the table by hand
        rng = np.random.default_rng(seed)
        cubes = rng.random((2, T, th, tw), dtype=np.float32)
        start, K = np.array([[0, 1, -1], [1, 0, 5]], np.int32), (th // sy) * (tw // sx)
    else:
        cubes, start, K = make_case(th, tw, sy, sx, H, W, seed)
        if r["kind"] == "short":
            start = np.ascontiguousarray(start[:start.shape[0] - 3, :start.shape[1] - 2])
        if T < cubes.shape[1]:
            cubes = np.ascontiguousarray(cubes[:, :T])
        if T > cubes.shape[1]:                             # more planes: the first three keep what make_case planted
            rng = np.random.default_rng(seed + 1)
            more = rng.random((cubes.shape[0], T, th, tw), dtype=np.float32) * 0.98 + 0.01
            more[rng.random(more.shape) < 0.05] = np.nan
            more[:, :cubes.shape[1]] = cubes
            cubes = more
    return dict(cubes=cubes, start=start, K=K, ref=blend_ref64(cubes, start, sy, sx, H, W))


@functools.lru_cache(maxsize=None)
def blend_const_case(name):
    """The row's table over cubes that are 0.5 everywhere: sums of w / 2 and of w are exact, so every covered pixel is 0.5."""
    r, case = BLEND_ROWS[name], blend_case(name)
    cubes = np.full(case["cubes"].shape, np.float32(0.5), np.float32)
    return dict(cubes=cubes, start=case["start"], K=case["K"], ref=blend_ref64(cubes, case["start"], r["sy"], r["sx"], r["H"], r["W"]))
