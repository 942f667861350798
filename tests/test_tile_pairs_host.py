"""fuse_tile_pairs on the host side: fixture g12 rebuilds from its stored factors, and the argument checks that need no GPU."""
import numpy as np
import pytest

from conftest import load_golden

P, B, C, h, f = 3, 285, 10, 100, 6


def g12_inputs(g):
    """(emit (P, 285, 100, 100) uint16, s2 (P, 10, 600, 600) uint16) from the stored factors of g12 (tests/golden/gen_g12.py
    builds them with the same statements)."""
    ab = g["abund"].astype(np.float64) / 255.0                                          # (P, 3, h, h)
    bb, ii, jj = np.meshgrid(np.arange(B), np.arange(h), np.arange(h), indexing="ij")
    emit = np.empty((P, B, h, h), np.uint16)
    for p in range(P):
        refl = np.einsum("kij,kb->bij", ab[p], g["spectra"])
        dn = np.round(1e4 * refl) + ((7 * ii + 13 * jj + 5 * bb + 11 * p) % 17 - 8)
        emit[p] = np.clip(dn, 1, 9000).astype(np.uint16)
    for p, b_, i_, j_ in g["emit_nd"]:                       # b_ == -1: every band
        if b_ < 0:
            emit[p, :, i_, j_] = 65535
        else:
            emit[p, b_, i_, j_] = 65535
    i2, j2 = np.meshgrid(np.arange(h), np.arange(h), indexing="ij")
    bad2 = (3 * i2 + 7 * j2) % 5 < 2                         # pair 2: 40 % of the pixels lose one selected band
    sel = g["bands"]
    emit[2, sel[(i2 + j2) % len(sel)][bad2], i2[bad2], j2[bad2]] = 65535
    cc, fi, fj = np.meshgrid(np.arange(C), np.arange(h * f), np.arange(h * f), indexing="ij")
    s2 = np.empty((P, C, h * f, h * f), np.uint16)
    for p in range(P):
        coarse = np.einsum("kij,kc->cij", ab[p], g["s2_resp"])
        fine = np.repeat(np.repeat(coarse, f, axis=1), f, axis=2) + ((3 * fi + 5 * fj + 7 * cc + p) % 11 - 5)
        s2[p] = np.clip(np.round(fine), 1, 10000).astype(np.uint16)
    for p, c_, i_, j_ in g["s2_zero"]:
        s2[p, c_, i_, j_] = 0
    return emit, s2


def block_mean_rule(s2, nodata=None, factor=f):
    """S2 (C, H f, W f) -> (C, H, W) float32 on the host: float64 sum / f^2, NaN where a sample is non-finite or nodata."""
    Cn, Hf, Wf = s2.shape
    v = s2.astype(np.float64).reshape(Cn, Hf // factor, factor, Wf // factor, factor)
    m = (v.sum(axis=(2, 4)) / (factor * factor)).astype(np.float32)
    bad = ~np.isfinite(v).all(axis=(2, 4))
    if nodata is not None:
        bad |= np.isclose(v, nodata).any(axis=(2, 4))
    m[bad] = np.nan
    return m


def decode_u16(e):
    return np.where(e == 65535, np.float32(np.nan), e.astype(np.float32) * np.float32(1e-4))


def test_g12_inputs_rebuild_and_training_counts():
    import s2_emit
    g = load_golden("g12_tile_pairs")
    emit, s2 = g12_inputs(g)
    assert emit.shape == (P, B, h, h) and s2.shape == (P, C, h * f, h * f)
    np.testing.assert_array_equal(g["bands"], s2_emit.subsample_bands_evenly(B, 32))
    # the cases the fixture must hold: a pixel 65535 in every band, one in a selected band, one only in an unselected band
    assert (emit[0, :, 5, 7] == 65535).all() and emit[0, g["bands"][3], 10, 20] == 65535 and emit[0, 1, 30, 40] == 65535
    assert 1 not in g["bands"]
    for p in range(P):
        X = block_mean_rule(s2[p], nodata=0.0)
        Y = decode_u16(emit[p])[g["bands"]]
        Xtr, Ytr = s2_emit.flatten_pixels(X, Y, x_nodata=0.0)
        assert len(Xtr) == g["n_train"][p], p
        mask = np.isfinite(X).all(0) & np.isfinite(Y).all(0) & ~np.isclose(X, 0.0).any(0)
        np.testing.assert_array_equal(np.packbits(mask.reshape(-1)), g["mask_packed"][p])
    assert g["n_train"][0] == h * h - 3 and bool(np.unpackbits(g["mask_packed"][0])[30 * h + 40])   # unselected band kept
    assert abs(g["n_train"][2] / (h * h) - 0.6) < 0.01                                              # ~40 % invalid
    assert g["pred_nan_count"][1] > 0                                                                 # S2 zero DN -> NaN at 10 m


def test_g12_fixture_within_the_size_limit():
    """A committed file stays under 1 MiB: the 10 m predictions are stored as a strided sample, one row and checksums."""
    import os
    from conftest import GOLDEN
    assert os.path.getsize(os.path.join(GOLDEN, "g12_tile_pairs.npz")) <= 1 << 20


def test_argument_validation_before_gpu_work():
    """Bad arguments raise ValueError from the host checks, before the GPU is asked for (no GPU here)."""
    from s2_emit import fuse_tile_pair, fuse_tile_pairs
    emit = np.zeros((285, 4, 5), np.uint16)
    s2 = np.zeros((10, 24, 30), np.uint16)
    bad = [
        (dict(emit=emit, s2=np.zeros((10, 24, 31), np.uint16)), "needs 24 x 30"),                 # shape mismatch
        (dict(emit=emit, s2=s2, factor=6.0), "integer"),                                          # non-integer factor
        (dict(emit=emit, s2=s2, factor=2.5), "integer"),
        (dict(emit=emit, s2=s2, factor=0), ">= 1"),
        (dict(emit=emit, s2=s2, bands=0), "between 1 and 285"),
        (dict(emit=emit, s2=s2, bands=286), "between 1 and 285"),
        (dict(emit=emit, s2=s2, bands="some"), "'all'"),
        (dict(emit=emit, s2=s2, bands=np.array([0, 285])), r"\[0, 285\)"),
        (dict(emit=emit, s2=s2, bands=np.array([0.5, 2.0])), "integer index array"),
        (dict(emit=emit, s2=s2, bands=True), "bool"),
        (dict(emit=emit.astype(np.int32), s2=s2), "uint16 or float32"),
        (dict(emit=emit, s2=s2, degree=4), "degree"),
        (dict(emit=emit[0], s2=s2), "expected"),
        (dict(emit=emit, s2=np.zeros((17, 24, 30), np.uint16)), "bands: 1 .. 16"),
        (dict(emit=emit, s2=s2, s2_coarse=np.zeros((10, 4, 5), np.float64)), "s2_coarse"),
        (dict(emit=emit, s2=np.zeros((13, 24, 30), np.uint16)), "nf=559 .* at most 512"),              # Sentinel-2's 13 bands
        (dict(emit=emit, s2=np.zeros((16, 24, 30), np.uint16), degree=3), "nf=968 .* at most 512"),
        (dict(emit=emit[:, :1, :1], s2=np.zeros((10, 65, 65), np.uint16), factor=65), "factor=65: .* at most 64"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            fuse_tile_pair(kw.pop("emit"), kw.pop("s2"), **kw)
    with pytest.raises(ValueError, match="2 EMIT tiles but 1 S2"):
        fuse_tile_pairs(np.stack([emit, emit]), s2[None])
    with pytest.raises(ValueError, match="share one shape"):
        fuse_tile_pairs([emit, emit[:, :3]], [s2, s2])


def test_largest_accepted_shapes_pass_the_host_checks(monkeypatch):
    """The bounds are inclusive: 12 S2 bands at degree 3 (nf 454), 16 at degree 2 (152) and factor 64 get past every host check
    to the GPU request (a stand-in that raises), while 13 bands at degree 3 / factor 65 never reach it."""
    import s2_emit
    from s2_emit import _native as nat

    class Asked(Exception):
        pass

    def gpu():
        raise Asked

    monkeypatch.setattr(nat, "require_gpu", gpu)
    emit = np.zeros((285, 2, 3), np.uint16)
    for nb, deg, fac in ((12, 3, 1), (16, 2, 1), (10, 3, 64), (1, 1, 64)):
        with pytest.raises(Asked):
            s2_emit.fuse_tile_pair(emit, np.zeros((nb, 2 * fac, 3 * fac), np.uint16), degree=deg, factor=fac)
    for nb, deg, fac in ((13, 3, 1), (10, 3, 65)):
        with pytest.raises(ValueError):
            s2_emit.fuse_tile_pair(emit, np.zeros((nb, 2 * fac, 3 * fac), np.uint16), degree=deg, factor=fac)
