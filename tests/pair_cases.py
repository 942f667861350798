"""The case tables of the tile-pair kernels (csrc/hsr_pairs.hip) and the references they are compared with.

Shared by tests/test_gpu_pair_instances.py (every row on the GPU, with the library's launch record hsr_pairs_last_launch) and
tests/test_pair_instances_host.py (what the tables claim about every row, on the references alone).  Not a test module itself;
everything here is NumPy.

Every row names the sequence of instances its call must record (None: the entry point must refuse the call and launch nothing).
Two entry points choose between instances, and their predicates are mirrored here:
  score      pair_score_partial_kernel<kVec>: kVec = npix, pair_pred, pair_y, pair_group and pair_map all multiples of 4, pred, y and
             sam_map on 16-byte boundaries, group on a 4-byte one (score_vec, nine terms);
  pool gram  pool_gram_kernel<kVec>: kVec = n_elems, pair_g and group_out even, both bases on 16 bytes (pool_gram_vec, five terms).
Pointer alignments are byte offsets from a 256-byte boundary, which is where the tests' buffers start.  The chunk plans
(report_chunks, report_panels, score_chunks, score_finish_trips, pool_gram_blocks, pool_models_blocks) restate the grid
arithmetic, so that a row can claim a second trip of a loop.

References:
  prep         oracle_np.block_mean (NaN where a block holds a non-finite or nodata sample), oracle_np.tile_decode_u16, and the
               float32 closeness rule close32 for the mask;
  stats        np.longdouble two-pass statistics; on the dyadic rows the exact integer sum;
  report       report_reference of test_tile_pairs_report_host at degree 1 (phi(Z) = Z), on exact dyadic logits;
  score        validation_reference of test_tile_pairs_validate_host on dyadic data;
  pool stats   np.longdouble two-pass statistics of the concatenated members (as pool_reference of test_tile_pairs_pool_host
               concatenates them: in pair order, empty members left out);
  pool gram    integer sums; pool models: the copies themselves.
"""
import dataclasses
import functools

import numpy as np

from oracle import oracle_np as onp
from test_tile_pairs_report_host import report_reference
from test_tile_pairs_validate_host import validation_reference

NAMES = ("pair_prep_kernel", "pair_stats_kernel", "pair_report_partial_kernel", "pair_report_finish_kernel", "pair_holdout_kernel",
         "pair_score_partial_kernel<false>", "pair_score_partial_kernel<true>", "pair_score_finish_kernel", "pool_stats_kernel",
         "pool_gram_kernel<false>", "pool_gram_kernel<true>", "pool_models_kernel")
INSTANCE_COUNT = 12
FILL = 0xA5                      # the sentinel byte of the GPU tests' buffers (gpu_harness.Buf)
P = 3                            # pairs of a batch
DT_CODE = {"float32": 0, "uint16": 2}
NP_DT = {"float32": np.float32, "uint16": np.uint16}

# the constants of csrc/hsr_pairs.hip the plans depend on
REP_ROWS, REP_KC, SCORE_PIX, SCORE_AHEAD, SCORE_FINISH_THREADS = 256, 96, 512, 4, 512
STATS_THREADS, POOL_AHEAD, POOL_GRAM_ELEMS, POOL_MODEL_ELEMS, POOL_MODEL_BLOCKS, PAIR_MAX_IN = 1024, 4, 2 * 256, 1024, 64, 16

PREP_SEQ = ["pair_prep_kernel"]
STATS_SEQ = ["pair_stats_kernel"]
REPORT_SEQ = ["pair_report_partial_kernel", "pair_report_finish_kernel"]
HOLDOUT_SEQ = ["pair_holdout_kernel"]
POOL_STATS_SEQ = ["pool_stats_kernel"]
POOL_MODELS_SEQ = ["pool_models_kernel"]


# =============================================================================================================================
# the selection rules and the chunk plans, mirrored
# =============================================================================================================================
def _b(flag):
    return "true" if flag else "false"


def score_vec(npix, pair_pred, pair_y, pair_group, pair_map, off_pred=0, off_y=0, off_group=0, off_map=0):
    return (npix % 4 == 0 and pair_pred % 4 == 0 and pair_y % 4 == 0 and pair_group % 4 == 0 and pair_map % 4 == 0 and
            off_pred % 16 == 0 and off_y % 16 == 0 and off_group % 4 == 0 and off_map % 16 == 0)


def score_sequence(*args, **kw):
    return [f"pair_score_partial_kernel<{_b(score_vec(*args, **kw))}>", "pair_score_finish_kernel"]


def pool_gram_vec(n_elems, pair_g, group_out, off_g=0, off_out=0):
    return n_elems % 2 == 0 and pair_g % 2 == 0 and group_out % 2 == 0 and off_g % 16 == 0 and off_out % 16 == 0


def pool_gram_sequence(*args, **kw):
    return [f"pool_gram_kernel<{_b(pool_gram_vec(*args, **kw))}>"]


def _ceil(a, b):
    return -(-a // b)


def report_chunks(npix):
    return _ceil(npix, REP_ROWS)


def report_panels(na):
    return _ceil(na, REP_KC)


def score_chunks(npix):
    return _ceil(npix, SCORE_PIX)


def score_finish_trips(npix):
    return _ceil(score_chunks(npix), SCORE_AHEAD)


def pool_gram_blocks(n_elems):
    return _ceil(n_elems, POOL_GRAM_ELEMS)


def pool_models_total(npad, kpad, T, nb):
    return npad * T + kpad * T + 2 * T + 2 * nb


def pool_models_blocks(npad, kpad, T, nb):
    return min(_ceil(pool_models_total(npad, kpad, T, nb), POOL_MODEL_ELEMS), POOL_MODEL_BLOCKS)


# =============================================================================================================================
# buffers with gaps
# =============================================================================================================================
def sentinel(dtype, n):
    return np.frombuffer(bytes([FILL]) * (int(n) * np.dtype(dtype).itemsize), dtype).copy()


def pack(parts, stride):
    """Equal-length 1-D arrays, part i at element i * stride of one array whose gaps hold the sentinel byte."""
    parts = [np.ascontiguousarray(p).reshape(-1) for p in parts]
    n = parts[0].size
    assert all(p.size == n and p.dtype == parts[0].dtype for p in parts) and (len(parts) == 1 or stride >= n)
    out = sentinel(parts[0].dtype, (len(parts) - 1) * stride + n)
    for i, p in enumerate(parts):
        out[i * stride: i * stride + n] = p
    return out


def unpack(flat, count, stride, n):
    """The inverse for an output: (count, n), after checking that every byte of the gaps still holds the sentinel."""
    flat = np.ascontiguousarray(flat).reshape(-1)
    assert flat.size == (count - 1) * stride + n, (flat.size, count, stride, n)
    own = np.zeros(flat.size, bool)
    for i in range(count):
        own[i * stride: i * stride + n] = True
    gaps = flat[~own]
    assert (gaps.view(np.uint8) == FILL).all(), "write into a gap between two pairs"
    return np.stack([flat[i * stride: i * stride + n] for i in range(count)])


def span(count, stride, n):
    return (count - 1) * stride + n


# =============================================================================================================================
# prep
# =============================================================================================================================
def close32(x, nd):
    """pair_close of the kernel: x == nd or |x - nd| <= 1e-8f + 1e-5f |nd|, every operation in float32."""
    x, nd = np.asarray(x, np.float32), np.float32(nd)
    with np.errstate(invalid="ignore", over="ignore"):
        return (x == nd) | (np.abs(x - nd) <= np.float32(1e-8) + np.float32(1e-5) * np.abs(nd))


def closeness_edge(nd):
    """(inside, outside) above nd and (inside, outside) below it: the last float32 value that is close to nd and its neighbour."""
    nd = np.float32(nd)
    out = []
    for way in (np.float32(np.inf), np.float32(-np.inf)):
        v = nd
        for _ in range(100000):
            nxt = np.nextafter(v, way)
            if not close32(nxt, nd):
                break
            v = nxt
        out += [v, np.nextafter(v, way)]
    return tuple(out)


@dataclasses.dataclass(frozen=True)
class PrepRow:
    name: str
    H: int
    W: int
    f: int                       # 0: the float32 coarse image
    nb: int
    B: int                       # emit_bands
    bands: tuple
    edt: str
    sdt: str
    end: float = None            # emit_nodata
    snd: float = None            # s2_nodata
    pad: int = 0                 # elements added to both dense pair strides
    plant: tuple = ()            # "nonfinite", "edge", "mean"

    @property
    def npix(self):
        return self.H * self.W

    @property
    def T(self):
        return len(self.bands)

    @property
    def s2_shape(self):
        k = max(self.f, 1)
        return (self.nb, self.H * k, self.W * k)

    @property
    def pair_emit(self):
        return self.B * self.npix + self.pad

    @property
    def pair_s2(self):
        return int(np.prod(self.s2_shape)) + self.pad


MIXED = (0, 19, 7, 7, 3)         # unsorted, a repeat, band 0 and band emit_bands - 1
PREP_ROWS = (
    PrepRow("1x1 f2 u16/u16 T=1", 1, 1, 2, 1, 4, (2,), "uint16", "uint16", snd=0.0),
    PrepRow("15x17 f6 nb=10 u16/u16 mixed bands", 15, 17, 6, 10, 20, MIXED, "uint16", "uint16", snd=0.0),
    PrepRow("16x16 f1 nb=16 f32/f32 T=emit_bands", 16, 16, 1, 16, 6, tuple(range(6)), "float32", "float32", end=-9999.0,
            plant=("nonfinite",)),
    PrepRow("257x1 f7 nb=1 u16/f32", 257, 1, 7, 1, 3, (1,), "uint16", "float32", plant=("nonfinite",)),
    PrepRow("7x37 f2 nb=10 f32/u16", 7, 37, 2, 10, 20, MIXED, "float32", "uint16", end=-9999.0, snd=0.0, plant=("nonfinite",)),
    PrepRow("2x3 f64 nb=1 u16/u16", 2, 3, 64, 1, 2, (1, 0), "uint16", "uint16"),
    PrepRow("7x37 coarse nb=10 f32", 7, 37, 0, 10, 20, MIXED, "float32", "float32", end=1000.0, snd=1000.0,
            plant=("nonfinite", "edge")),
    PrepRow("16x16 f1 nd=1000 edge f32/f32", 16, 16, 1, 1, 5, (4, 0), "float32", "float32", end=1000.0, snd=1000.0, plant=("edge",)),
    PrepRow("15x17 f2 mean == nd", 15, 17, 2, 10, 4, (1,), "float32", "float32", snd=1000.0, plant=("mean",)),
    PrepRow("7x37 f2 padded u16/u16", 7, 37, 2, 16, 20, MIXED, "uint16", "uint16", snd=0.0, pad=3),
    PrepRow("15x17 f6 padded f32/f32 no nodata", 15, 17, 6, 1, 20, MIXED, "float32", "float32", pad=5, plant=("nonfinite",)),
)
# (name, overrides of the call of PREP_REFUSED_BASE): the entry point must return an error and launch nothing
PREP_REFUSED_BASE = PREP_ROWS[4]
PREP_REFUSED = (("T > emit_bands", dict(T=21)), ("nb = 17", dict(nb=17)), ("factor = 65", dict(f=65)),
                ("uint16 coarse image", dict(f=0, sdt="uint16")), ("overlapping emit stride", dict(pair_emit=20 * 7 * 37 - 1)),
                ("overlapping s2 stride", dict(pair_s2=10 * 7 * 37 * 4 - 1)), ("P = 0", dict(P=0)))


class _Picker:
    """Distinct pixels in a seeded order (it wraps round on a tile with fewer pixels than plants)."""

    def __init__(self, rng, npix):
        self.order, self.i = rng.permutation(npix), 0

    def __call__(self):
        p = int(self.order[self.i % len(self.order)])
        self.i += 1
        return p


@functools.lru_cache(maxsize=None)
def prep_inputs(row):
    """-> (emit (P, B, H, W), s2 (P,) + row.s2_shape).  Float32 samples are dyadic (EMIT k / 4096, S2 k / 4), so every block sum
    is exact in float64 in any order.  Pair 0 is clean; pairs 1 and 2 carry the planted samples: a nodata value on each side that
    has one, 65535 in a uint16 tile (EMIT: NaN, in a selected band and in one that is not selected; S2: an ordinary value), and
    what row.plant names.  S2 plants sit on the LAST sample of their block (dy = dx = f - 1)."""
    r = row
    rng = np.random.default_rng(sum(map(ord, r.name)))
    k = max(r.f, 1)
    if r.edt == "uint16":
        emit = rng.integers(1, 60000, (P, r.B, r.H, r.W)).astype(np.uint16)
    else:
        emit = (rng.integers(1, 4096, (P, r.B, r.H, r.W)) / 4096.0).astype(np.float32)
    if r.sdt == "uint16":
        s2 = rng.integers(1, 10000, (P,) + r.s2_shape).astype(np.uint16)
    else:
        s2 = (rng.integers(4, 3200, (P,) + r.s2_shape) / 4.0).astype(np.float32)     # below 800: never close to 1000
    unselected = [b for b in range(r.B) if b not in r.bands]
    for p in (1, 2):
        pick = _Picker(rng, r.npix)

        def s2_at(c, pix, v, dy=k - 1, dx=k - 1):
            s2[p, c, (pix // r.W) * k + dy, (pix % r.W) * k + dx] = v

        def emit_at(b, pix, v):
            emit[p, b, pix // r.W, pix % r.W] = v
        if r.snd is not None:
            s2_at(int(rng.integers(r.nb)), pick(), r.snd, dy=k - 1, dx=0)
        if r.end is not None:
            emit_at(r.bands[-1], pick(), r.end)
        if r.edt == "uint16":
            emit_at(r.bands[-1], pick(), 65535)
            if unselected:
                emit_at(unselected[0], pick(), 65535)
        if r.sdt == "uint16":
            s2_at(r.nb - 1, pick(), 65535)
        if "nonfinite" in r.plant:
            for v in (np.nan, np.inf, -np.inf):
                if r.sdt == "float32":
                    s2_at(int(rng.integers(r.nb)), pick(), v)
                if r.edt == "float32":
                    emit_at(r.bands[0], pick(), v)
            if r.sdt == "float32" and k > 1:                 # +Inf and -Inf in one block: the sum is NaN
                pix = pick()
                s2_at(0, pix, np.inf, dy=0, dx=0)
                s2_at(0, pix, -np.inf)
        if "edge" in r.plant:
            for v in closeness_edge(1000.0) + (np.float32(1000.0),):
                s2_at(r.nb - 1, pick(), v)
                emit_at(r.bands[0], pick(), v)
        if "mean" in r.plant:                                # four samples nd +- 1: the mean is nd, no sample is close
            pix = pick()
            for dy in range(2):
                for dx in range(2):
                    s2_at(3, pix, np.float32(r.snd + (1 if (dy + dx) % 2 else -1)), dy=dy, dx=dx)
    emit.setflags(write=False)
    s2.setflags(write=False)
    return emit, s2


def prep_reference(row, emit, s2):
    """One pair: emit (B, H, W), s2 row.s2_shape -> x (nb, npix) float32, y (T, npix) float32, mask (npix,) uint8."""
    r = row
    if r.f == 0:
        x = np.array(s2, np.float32)
    else:
        v = s2.astype(np.float32)                            # uint16 -> float32 is exact
        with np.errstate(invalid="ignore", over="ignore"):
            x = onp.block_mean(v, r.f)
        bad = ~np.isfinite(v)
        if r.snd is not None:
            bad |= close32(v, r.snd)
        x[bad.reshape(r.nb, r.H, r.f, r.W, r.f).any(axis=(2, 4))] = np.nan
    sel = emit[list(r.bands)]
    y = onp.tile_decode_u16(sel) if r.edt == "uint16" else np.array(sel, np.float32)
    x, y = x.reshape(r.nb, -1), y.reshape(r.T, -1)
    ok = np.isfinite(x).all(axis=0) & np.isfinite(y).all(axis=0)
    if r.snd is not None:
        ok &= ~close32(x, r.snd).any(axis=0)
    if r.end is not None:
        ok &= ~close32(y, r.end).any(axis=0)
    return x, y, ok.astype(np.uint8)


# =============================================================================================================================
# stats
# =============================================================================================================================
@dataclasses.dataclass(frozen=True)
class StatsRow:
    npix: int
    nb: int
    kind: str                    # "dyadic": 4096 + k / 64 (band 0 of nb = 16 constant); "random"

    @property
    def name(self):
        return f"npix={self.npix} nb={self.nb} {self.kind}"


STATS_NPIX = (1, 63, 64, 1023, 1024, 1025, 4097)
STATS_ROWS = tuple(StatsRow(n, 1, "dyadic") for n in STATS_NPIX) + tuple(StatsRow(n, 16, "dyadic") for n in (1, 1023, 1025, 4097)) + \
    tuple(StatsRow(n, nb, "random") for n, nb in ((63, 16), (1024, 1), (1025, 16), (4097, 1)))
STATS_MASKS = ("empty", "one", "most")      # the three pairs of a batch
STATS_CONST_BAND = 0


@functools.lru_cache(maxsize=None)
def stats_inputs(row):
    """-> x (P, nb, npix) float32, mask (P, npix) uint8: pair 0 all zero, pair 1 exactly one pixel, pair 2 about 70 % set with the
    bytes 1, 2 and 255; NaN samples under mask 0 in every pair."""
    rng = np.random.default_rng(row.npix * 31 + row.nb)
    if row.kind == "dyadic":
        x = (4096.0 + rng.integers(0, 64, (P, row.nb, row.npix)) / 64.0).astype(np.float32)
        if row.nb > 1:
            x[:, STATS_CONST_BAND] = np.float32(4096.5)
    else:
        x = (1000 + 300 * rng.standard_normal((P, row.nb, row.npix))).astype(np.float32)
    mask = np.zeros((P, row.npix), np.uint8)
    mask[1, int(rng.integers(row.npix))] = 2
    most = rng.random(row.npix) < 0.7
    most[-1] = True                                          # the last pixel counts: a dropped tail shows
    mask[2, most] = rng.choice(np.array([1, 2, 255], np.uint8), int(most.sum()))
    for p in range(P):
        off = np.flatnonzero(mask[p] == 0)
        x[p][:, off[::3]] = np.nan
    x.setflags(write=False)
    mask.setflags(write=False)
    return x, mask


def stats_reference(x, mask):
    """One pair: x (nb, npix), mask (npix,) -> n, mean (nb,), m2 (nb,), scale (nb,) by two passes in np.longdouble."""
    sel = np.asarray(x)[:, np.asarray(mask) != 0].astype(np.longdouble)
    n = sel.shape[1]
    if n == 0:
        z = np.zeros(len(x))
        return 0, z, z.copy(), np.ones(len(x))
    mean = sel.sum(axis=1) / n
    m2 = ((sel - mean[:, None]) ** 2).sum(axis=1)
    scale = np.sqrt(m2 / n)
    scale = np.where(m2 == 0, 1.0, scale)
    return n, mean.astype(np.float64), m2.astype(np.float64), scale.astype(np.float64)


def dyadic_mean(x, mask):
    """The dyadic rows: float64(exact sum) / n, the sum taken in integers (x is a multiple of 1 / 64 below 2^13)."""
    sel = np.asarray(x)[:, np.asarray(mask) != 0].astype(np.float64)
    k = np.rint(sel * 64).astype(np.int64)
    assert (k / 64.0 == sel).all()
    total = k.sum(axis=1)
    assert (np.abs(total) < 2 ** 53).all()
    return (total.astype(np.float64) / 64.0) / np.float64(sel.shape[1])


def one_pass_m2(x, mask):
    """What a one-pass kernel would give (sum x^2 - n mean^2 in float64): used on the CPU to show that the M2 bar separates."""
    sel = np.asarray(x)[:, np.asarray(mask) != 0].astype(np.float64)
    n = sel.shape[1]
    mean = sel.sum(axis=1) / n
    return (sel * sel).sum(axis=1) - n * mean * mean


# =============================================================================================================================
# report
# =============================================================================================================================
@dataclasses.dataclass(frozen=True)
class ReportRow:
    na: int
    nf: int
    T: int
    npix: int
    padded: bool = False
    flags: tuple = ()            # "clip", "status" (pair 1: status 2), "empty" (pair 2: all-zero mask, status 1)

    @property
    def name(self):
        return f"na={self.na} nf={self.nf} T={self.T} npix={self.npix}{' padded' if self.padded else ''} {' '.join(self.flags)}".strip()

    @property
    def rows_bp(self):
        return self.nf + 4                                   # rows nf .. nf + 3 hold NaN

    @property
    def work(self):
        return report_chunks(self.npix) * self.T * 4

    def strides(self):
        a = 1 if self.padded else 0
        ldq = self.na + 16 + 2 * a
        ldbp = self.T + 3 * a
        return dict(ldq=ldq, pair_q=self.npix * ldq + 6 * a, pair_b=self.T + a, ldbp=ldbp, pair_bp=self.rows_bp * ldbp + 5 * a,
                    pair_y=self.T * self.npix + 3 * a, pair_m=self.npix + 5 * a, pair_work=self.work + 2 * a, pair_out=self.T + 3 * a)


REPORT_NA, REPORT_T, REPORT_NPIX = (16, 48, 96, 112, 192, 288), (1, 15, 16, 17, 32, 33, 285), (1, 15, 16, 17, 255, 256, 257, 1037)
REPORT_ROWS = (
    ReportRow(16, 3, 17, 1),
    ReportRow(48, 35, 15, 15, flags=("status",)),
    ReportRow(96, 95, 16, 16, padded=True),
    ReportRow(112, 99, 17, 17, flags=("clip",)),
    ReportRow(192, 191, 1, 255, flags=("empty",)),
    ReportRow(288, 275, 33, 256, padded=True, flags=("clip", "status")),
    ReportRow(16, 15, 285, 257),
    ReportRow(112, 111, 32, 1037, padded=True, flags=("empty",)),
    ReportRow(288, 287, 17, 257),
    ReportRow(96, 83, 33, 255, flags=("clip",)),
    ReportRow(192, 179, 16, 1037, padded=True, flags=("status", "empty")),
    ReportRow(48, 47, 32, 256),
)


@functools.lru_cache(maxsize=None)
def report_inputs(row):
    """The exact-integer construction of test_report_kernel_on_exact_integer_data: Q in quarters, Bp in eighths, b64 in halves, so
    every logit is exact in float64 in any order and exact in float32.  Q columns >= na, Bp rows >= nf and Bp columns >= T hold
    NaN (never read); the targets of masked-out pixels are NaN (never used).  With npix == 1 a statistic is one pixel and M2 = 0
    (r2 = 1 - d^2 / 1e-8), so b64 is chosen there to make every logit 0 or 64: sigmoid = 0.5 or 1 exactly under any expf."""
    r = row
    s = r.strides()
    rng = np.random.default_rng(r.na * 1000 + r.T * 7 + r.npix)
    mask = (rng.random((P, r.npix)) < 0.8).astype(np.uint8)
    mask[:, -1] = 1                                          # the last pixel counts
    if r.npix >= 15:
        mask[:, 2] = 0
    Q = np.full((P, r.npix, s["ldq"]), np.nan)
    Q[:, :, :r.na] = 0.0
    Q[:, :, 0] = 1.0
    Q[:, :, 1:r.nf + 1] = rng.integers(-2, 3, (P, r.npix, r.nf)) * 0.25
    Q[mask == 0, :r.na] = 0.0                                # an untrained pixel is a zero row
    Bp = np.full((P, r.rows_bp, s["ldbp"]), np.nan)
    Bp[:, :r.nf, :r.T] = rng.integers(-2, 3, (P, r.nf, r.T)) * 0.125
    b64 = rng.integers(-4, 5, (P, r.T)) * 0.5
    if "clip" in r.flags:
        b64[:, ::3] = 80.0
        b64[:, 1::3] = -80.0
    if r.npix == 1:
        z = np.einsum("pk,pkt->pt", Q[:, 0, 1:r.nf + 1], Bp[:, :r.nf, :r.T])
        b64 = np.where(np.arange(r.T) % 2 == 0, 0.0, 64.0) - z
    y = (rng.integers(0, 65, (P, r.T, r.npix)) / 64.0).astype(np.float32)
    y[np.broadcast_to((mask == 0)[:, None], y.shape)] = np.nan
    status = np.zeros(P, np.int32)
    if "status" in r.flags:
        status[1] = 2
    if "empty" in r.flags:
        mask[2] = 0
        Q[2, :, :r.na] = 0.0
        y[2] = np.nan
        status[2] = 1
    out = dict(Q=Q, Bp=Bp, b64=b64, y=y, mask=mask, status=status)
    for v in out.values():
        v.setflags(write=False)
    return out


def report_expected(row, d, p):
    """(r2, rmse) (T,) of pair p: NaN under a non-zero status, else report_reference at degree 1 on the masked rows."""
    if d["status"][p] != 0:
        return np.full(row.T, np.nan), np.full(row.T, np.nan)
    m = d["mask"][p] != 0
    X = d["Q"][p][m][:, 1:row.nf + 1]
    return report_reference(X, d["y"][p].T[m], np.zeros(row.nf), np.ones(row.nf), d["Bp"][p, :row.nf, :row.T].T, d["b64"][p], 1)


def report_direct(row, d, p):
    """The same numbers as the existing exact-integer test writes them (a matrix product on Q's own columns)."""
    m = d["mask"][p] != 0
    z = (d["Q"][p][m][:, :row.nf + 1] @ np.concatenate([d["b64"][p][None], d["Bp"][p, :row.nf, :row.T]])).astype(np.float32)
    yp = np.float32(1) / (np.float32(1) + np.exp(-np.clip(z, np.float32(-50), np.float32(50))))
    yt = d["y"][p].T[m]
    dd = (yt - yp).astype(np.float64)
    ss_res = (dd * dd).sum(0)
    ss_tot = ((yt - yt.astype(np.float64).mean(0)) ** 2).sum(0) + 1e-8
    return 1 - ss_res / ss_tot, np.sqrt(ss_res / m.sum()), z


# =============================================================================================================================
# holdout
# =============================================================================================================================
HOLDOUT_ROWS = ((1, 0), (255, 0), (256, 0), (257, 0), (255, 3), (257, 7))      # (npix, elements added to pair_train)


@functools.lru_cache(maxsize=None)
def holdout_inputs(npix):
    rng = np.random.default_rng(npix)
    valid = rng.choice(np.array([0, 1, 1, 7], np.uint8), (P, npix))
    train = rng.choice(np.array([0, 100, 200, 255], np.uint8), (P, npix))
    return valid, train


def holdout_reference(valid, train):
    return ((valid != 0) & (train != 0)).astype(np.uint8), np.where(valid == 0, 0, np.where(train != 0, 1, 2)).astype(np.uint8)


# =============================================================================================================================
# score
# =============================================================================================================================
@dataclasses.dataclass(frozen=True)
class ScoreRow:
    T: int
    npix: int
    groups: tuple = ("mix", "ones", "twos")      # the three pairs: "mix", "ones", "twos", "zeros", "lastlane"
    flip: str = ""               # the predicate term flipped alone ("" none): pair_pred, pair_y, pair_group, pair_map (stride + 1),
    #                              pred, y, group, sam_map (base moved by 4 bytes; group: by 1)

    @property
    def name(self):
        return f"T={self.T} npix={self.npix} {'/'.join(self.groups)} {('flip ' + self.flip) if self.flip else ''}".strip()

    def layout(self):
        """Strides (elements) and base offsets (bytes): aligned and padded unless flipped."""
        up4 = lambda n: (n + 3) // 4 * 4 + 4
        lay = dict(pair_pred=up4(self.T * self.npix), pair_y=up4(self.T * self.npix) + 4, pair_group=up4(self.npix),
                   pair_map=up4(self.npix) + 8, off_pred=0, off_y=0, off_group=0, off_map=0)
        if self.flip in ("pair_pred", "pair_y", "pair_group", "pair_map"):
            lay[self.flip] += 1
        elif self.flip in ("pred", "y", "sam_map"):
            lay["off_" + {"sam_map": "map"}.get(self.flip, self.flip)] = 4
        elif self.flip == "group":
            lay["off_group"] = 1
        else:
            assert self.flip in ("", "npix")
        return lay

    @property
    def vec(self):
        return score_vec(self.npix, **self.layout())

    @property
    def expect(self):
        return score_sequence(self.npix, **self.layout())

    @property
    def work(self):
        return score_chunks(self.npix) * (self.T * 8 + 4)


SCORE_T, SCORE_NPIX = (1, 2, 3, 4, 5, 7, 8, 285, 513), (1, 4, 7, 8, 9, 511, 512, 513, 2564, 4096)
SCORE_FLIPS = ("pair_pred", "pair_y", "pair_group", "pair_map", "pred", "y", "group", "sam_map")
SCORE_PRED_SHAPE = (5, 516)      # the predicate rows: two chunks, npix % 4 == 0
SCORE_ROWS = (
    ScoreRow(1, 1), ScoreRow(2, 4), ScoreRow(3, 7), ScoreRow(4, 8, ("zeros", "mix", "ones")), ScoreRow(5, 9),
    ScoreRow(7, 511), ScoreRow(8, 512, ("lastlane", "mix", "twos")), ScoreRow(285, 513), ScoreRow(513, 9, ("mix", "zeros", "twos")),
    ScoreRow(5, 2564, ("lastlane", "mix", "ones")), ScoreRow(3, 4096), ScoreRow(4, 4096, ("lastlane", "zeros", "mix")),
    ScoreRow(5, 517, flip="npix"),
)
SCORE_BASE = ScoreRow(*SCORE_PRED_SHAPE)
SCORE_FLIP_ROWS = tuple(ScoreRow(*SCORE_PRED_SHAPE, flip=f) for f in SCORE_FLIPS)
LASTLANE_PIXEL = SCORE_PIX - 1   # lane 63, second vector, last element: 256 + 4 * 63 + 3


@functools.lru_cache(maxsize=None)
def score_inputs(T, npix, groups):
    """The dyadic construction of test_score_kernel_on_exact_data: targets k / 64 in (0, 1], errors k / 64 in [-1/8, 1/8], one
    constant band, NaNs in single bands of pred, a zero spectrum; group codes per pair as `groups` names them - "mix" draws from
    0, 1, 2, 3 and 255 (the last two count as 0), "lastlane" is all 1 but the last pixel of every full chunk, which is 2."""
    rng = np.random.default_rng(T * 10007 + npix)
    y = (rng.integers(1, 65, (P, T, npix)) / 64.0).astype(np.float32)
    y[:, min(3, T - 1)] = np.float32(0.375)
    pred = (y + rng.integers(-8, 9, (P, T, npix)) / 64.0).astype(np.float32)
    if npix >= 16:
        pred[rng.random((P, T, npix)) < 0.002] = np.nan
        pred[1, :, 5] = 0.0
        pred[0, T - 1, npix - 1] = np.nan                    # the last band of the last pixel
    group = np.zeros((P, npix), np.uint8)
    for p, kind in enumerate(groups):
        if kind == "mix":
            group[p] = rng.choice(np.array([0, 1, 1, 2, 2, 3, 255], np.uint8), npix)
            group[p, -1] = 1 + p % 2
        elif kind == "lastlane":
            group[p] = 1
            group[p, LASTLANE_PIXEL::SCORE_PIX] = 2
        else:
            group[p] = {"ones": 1, "twos": 2, "zeros": 0}[kind]
    for a in (pred, y, group):
        a.setflags(write=False)
    return pred, y, group


def score_reference(pred, y, group, factor=6):
    """validation_reference with the bytes that are neither 1 nor 2 read as 0, as the kernel reads them."""
    g = np.where((group == 1) | (group == 2), group, 0)
    return validation_reference(pred, y, g, factor)


# =============================================================================================================================
# pooling
# =============================================================================================================================
POOL_SIZES = (1, 3, 4, 5, 8, 9, 3)               # group sizes; the last group has empty members only
POOL_M = len(POOL_SIZES)
POOL_P = sum(POOL_SIZES)
POOL_EMPTY_AT = {3: (0,), 4: (3,), 5: (8,), 6: (0, 1, 2)}    # group -> positions (in pair order) of its members without pixels


@functools.lru_cache(maxsize=None)
def pool_ids():
    """Group ids of the POOL_P pairs, interleaved (dealt round robin while a group still wants members), so that the members of
    a group are far apart and `order` is no identity."""
    left = list(POOL_SIZES)
    ids = []
    while any(left):
        for g in range(POOL_M - 1, -1, -1):
            if left[g]:
                ids.append(g)
                left[g] -= 1
    return tuple(ids)


def pool_members(ids=None):
    ids = pool_ids() if ids is None else ids
    return [[p for p, g in enumerate(ids) if g == grp] for grp in range(max(ids) + 1)]


def pool_empty_pairs():
    mem = pool_members()
    return sorted(mem[g][k] for g, ks in POOL_EMPTY_AT.items() for k in ks)


def pool_layout(ids):
    """s2_emit.pairs.pool_layout restated (the GPU test uses the package's own and compares)."""
    ids = np.asarray(ids, np.int64)
    order = np.argsort(ids, kind="stable").astype(np.int32)
    start = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=int(ids.max()) + 1))]).astype(np.int32)
    return order, start


@functools.lru_cache(maxsize=None)
def pool_stats_inputs(nb):
    """-> samples (list over pairs of (nb, n_p) float32; n_p = 0 for an empty pair), stats (POOL_P, 1 + 2 nb) float64: each
    pair's [n, mean.., M2..] by two passes in np.longdouble, what hsr_pair_stats hands over."""
    rng = np.random.default_rng(100 + nb)
    empty = set(pool_empty_pairs())
    samples, stats = [], np.zeros((POOL_P, 1 + 2 * nb))
    for p in range(POOL_P):
        n = 0 if p in empty else int(rng.integers(1, 400))
        x = (1000 + 300 * rng.standard_normal((nb, n)) + 50 * p).astype(np.float32)
        samples.append(x)
        if n:
            _, mean, m2, _ = stats_reference(x, np.ones(n, np.uint8))
            stats[p] = np.concatenate([[n], mean, m2])
    stats.setflags(write=False)
    return samples, stats


def pool_stats_reference(samples, members, nb):
    """A group: the two-pass longdouble statistics of its members' samples, concatenated in pair order."""
    cat = np.concatenate([samples[p] for p in members], axis=1) if members else np.zeros((nb, 0), np.float32)
    return stats_reference(cat, np.ones(cat.shape[1], np.uint8))


# order / start with entries no kernel may follow: (name, edit(order, start) -> (the members every group still walks, the pairs
# no group reaches any more))
def _skip_order(order, start):
    mem = pool_members()
    out = [mem[5][0], mem[5][4], mem[4][7], mem[2][1]]
    for p, bad in zip(out, (-1, POOL_P, 2 ** 31 - 1, -(2 ** 31))):
        order[list(order).index(p)] = bad
    return [[p for p in m if p not in out] for m in mem], sorted(out)


def _skip_start(order, start):
    """start[0] below 0 and start[M] past P (both clamped: nothing changes for the first group and nothing past P is read), and
    the last group's slice turned round, [P + 7, P + 3): it is empty after the clamp, and the group before it, whose slice now
    ends at the clamped P, walks the last group's members (all empty) behind its own."""
    start[0] = -5
    start[POOL_M - 1], start[POOL_M] = POOL_P + 7, POOL_P + 3
    mem = pool_members()
    return mem[:POOL_M - 2] + [mem[POOL_M - 2] + mem[POOL_M - 1], []], []


POOL_SKIPS = (("order entries outside [0, P)", _skip_order), ("start slices outside [0, P]", _skip_start))


def pool_skip_layout(edit):
    """-> order, start (edited, int32), members (list over groups of the pairs still walked), the pairs no group reaches."""
    order, start = pool_layout(pool_ids())
    order, start = order.astype(np.int64), start.astype(np.int64)
    members, untouched = edit(order, start)
    return order.astype(np.int32), start.astype(np.int32), members, untouched


@dataclasses.dataclass(frozen=True)
class GramRow:
    n_elems: int
    flip: str = ""               # "", "n_elems", "pair_g", "group_out", "g", "out"

    @property
    def name(self):
        return f"n_elems={self.n_elems} {('flip ' + self.flip) if self.flip else ''}".strip()

    def layout(self):
        n = self.n_elems
        lay = dict(pair_g=n + 6 + n % 2, group_out=n + 4 + n % 2, off_g=0, off_out=0)
        if self.flip in ("pair_g", "group_out"):
            lay[self.flip] += 1
        elif self.flip in ("g", "out"):
            lay["off_" + self.flip] = 8
        else:
            assert self.flip in ("", "n_elems")
        return lay

    @property
    def expect(self):
        return pool_gram_sequence(self.n_elems, **self.layout())


GRAM_BASE = GramRow(600)                         # two blocks of 512 elements
GRAM_FLIP_ROWS = tuple(GramRow(600, f) for f in ("pair_g", "group_out", "g", "out")) + (GramRow(601, "n_elems"),)
GRAM_ROWS = (GramRow(1, "n_elems"), GramRow(2), GramRow(511, "n_elems"), GramRow(512), GramRow(513, "n_elems"), GramRow(1026), GRAM_BASE)
GRAM_PAIR_COUNT = 3


@functools.lru_cache(maxsize=None)
def gram_inputs(n_elems):
    """-> src (POOL_P, n_elems) float64 small integers (every sum exact), cnt (POOL_P,) float64: 0 for the empty pairs.  Element 0
    of the singleton group's pair is -0.0: a copy keeps the sign, a sum with 0.0 loses it."""
    rng = np.random.default_rng(n_elems)
    src = rng.integers(-1000, 1000, (POOL_P, n_elems)).astype(np.float64)
    src[pool_members()[0][0], 0] = -0.0
    cnt = rng.integers(1, 50, POOL_P).astype(np.float64)
    cnt[pool_empty_pairs()] = 0.0
    src.setflags(write=False)
    cnt.setflags(write=False)
    return src, cnt


def gram_reference(src, cnt, members):
    """(groups, n_elems): the members with cnt != 0 added in pair order; the first one copied; zeros for a group without one."""
    out = np.zeros((len(members), src.shape[1]))
    for g, mem in enumerate(members):
        live = [p for p in mem if cnt[p] != 0]
        if live:
            out[g] = src[live[0]]
            for p in live[1:]:
                out[g] = out[g] + src[p]
    return out


@dataclasses.dataclass(frozen=True)
class ModelsRow:
    nf: int
    npad: int
    kpad: int
    T: int
    nb: int
    padded: bool = False

    @property
    def name(self):
        return f"nf={self.nf} npad={self.npad} kpad={self.kpad} T={self.T} nb={self.nb}{' padded' if self.padded else ''}"

    @property
    def group_bp(self):
        return (self.nf + 2) * self.T + (7 if self.padded else 0)      # two NaN rows behind the nf the kernel may read

    @property
    def group_w32(self):
        return self.kpad * self.T + (5 if self.padded else 0)


MODELS_P, MODELS_M = 5, 2
MODELS_GROUP_OF = (0, -1, 1, MODELS_M, 0)        # pairs 1 and 3 are outside [0, M): all their outputs keep the sentinel
MODELS_POOL_STATUS = (0, 3)
MODELS_N_TRAIN = (0, 5, 6, 0, 7)                 # pair 0: status 0 but no training pixel -> report_status 1
MODELS_ROWS = (ModelsRow(5, 16, 8, 3, 2), ModelsRow(5, 16, 8, 3, 2, padded=True), ModelsRow(14, 16, 16, 37, 4, padded=True),
               ModelsRow(275, 288, 288, 285, 16), ModelsRow(275, 288, 280, 285, 16, padded=True))
MODELS_FIELDS = ("bp", "b64", "w32", "b32", "mean32", "inv32")


@functools.lru_cache(maxsize=None)
def models_inputs(row):
    """The group models: g_bp (M, nf + 2, T) with NaN in the two rows behind nf, the rest random bits of their types."""
    r = row
    rng = np.random.default_rng(r.npad * 3 + r.T)
    g = dict(bp=np.full((MODELS_M, r.nf + 2, r.T), np.nan), b64=rng.standard_normal((MODELS_M, r.T)),
             w32=rng.standard_normal((MODELS_M, r.kpad, r.T)).astype(np.float32), b32=rng.standard_normal((MODELS_M, r.T)).astype(np.float32),
             mean32=rng.standard_normal((MODELS_M, r.nb)).astype(np.float32), inv32=rng.standard_normal((MODELS_M, r.nb)).astype(np.float32))
    g["bp"][:, :r.nf] = rng.standard_normal((MODELS_M, r.nf, r.T))
    for v in g.values():
        v.setflags(write=False)
    return g


def models_expected(row, g, grp):
    """What a pair of group grp receives: its group's arrays, Bp with zero rows nf .. npad."""
    bp = np.zeros((row.npad, row.T))
    bp[:row.nf] = g["bp"][grp, :row.nf]
    return dict(bp=bp, b64=g["b64"][grp], w32=g["w32"][grp], b32=g["b32"][grp], mean32=g["mean32"][grp], inv32=g["inv32"][grp])


def models_status(grp, n_train):
    s = MODELS_POOL_STATUS[grp]
    return s, (s if s != 0 else (1 if n_train == 0 else 0))


# =============================================================================================================================
# the driver: what fuse_tile_pairs records on the `small` geometry of test_gpu_tile_pairs_pool.py (9 x 11 pixels: npix = 99, so the
# score takes the plain instance; the pooled Gram is (na, ldq) doubles with even sizes in fresh allocations: the 16-byte instance)
# =============================================================================================================================
_SCORE_PLAIN = ["pair_score_partial_kernel<false>", "pair_score_finish_kernel"]
DRIVER_RECORDS = {
    "plain": ["pair_prep_kernel", "pair_stats_kernel"],
    "report": ["pair_prep_kernel", "pair_stats_kernel", "pair_report_partial_kernel", "pair_report_finish_kernel"],
    "train_mask+validate": ["pair_prep_kernel", "pair_holdout_kernel", "pair_stats_kernel"] + _SCORE_PLAIN + _SCORE_PLAIN,
    "pool": ["pair_prep_kernel", "pair_stats_kernel", "pool_stats_kernel", "pool_gram_kernel<true>", "pool_models_kernel"],
    "s2_coarse": ["pair_prep_kernel", "pair_stats_kernel"],
}


def all_expected_names():
    """Every name some row of the tables says it records."""
    seen = set(PREP_SEQ + STATS_SEQ + REPORT_SEQ + HOLDOUT_SEQ + POOL_STATS_SEQ + POOL_MODELS_SEQ)
    for r in SCORE_ROWS + SCORE_FLIP_ROWS + (SCORE_BASE,):
        seen |= set(r.expect)
    for r in GRAM_ROWS + GRAM_FLIP_ROWS:
        seen |= set(r.expect)
    return seen
