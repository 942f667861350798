"""fuse_tile_pairs(report=True) on an MI355X: per-band R^2 and RMSE of every pair's fit on its training pixels (the notebook's
cell 26) against fixture g13, against a NumPy restatement from the device's own outputs (T = 32 and all 285 bands), the report
kernel alone on exact integer data, batch bits == single-pair bits, no effect on the other outputs, a non-default stream and
float32 inputs."""
import numpy as np
import pytest

from conftest import load_golden
from gpu_harness import torch_gpu  # noqa: F401
from test_tile_pairs_host import decode_u16, g12_inputs
from test_tile_pairs_report_host import report_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g12():
    g = load_golden("g12_tile_pairs")
    emit, s2 = g12_inputs(g)
    return g, emit, s2


def _same_bits(a, b):
    import torch
    assert a.shape == b.shape and a.dtype == b.dtype
    width = {torch.float64: torch.int64, torch.int64: torch.int64}.get(a.dtype)
    if width is None:
        width = torch.int32 if a.element_size() == 4 else torch.uint8
    return bool((a.contiguous().view(-1).view(width) == b.contiguous().view(-1).view(width)).all())


def _check_close(r2, rmse, r2_ref, rmse_ref):
    r2, rmse = np.asarray(r2), np.asarray(rmse)
    assert np.abs(r2 - r2_ref).max() <= 1e-5, np.abs(r2 - r2_ref).max()
    assert (np.abs(rmse - rmse_ref) <= 1e-5 * np.abs(rmse_ref)).all(), np.abs(rmse / rmse_ref - 1).max()


def _restate(out, i, Y_bhw):
    """The report of pair i restated from the device's outputs: its mask, S2 on the EMIT grid and float64 model."""
    m = out.model(i)
    mask = out.mask[i].cpu().numpy().reshape(-1)
    X = out.s2_coarse[i].cpu().numpy().reshape(m.n_in, -1).T[mask]
    Y = Y_bhw.reshape(Y_bhw.shape[0], -1).T[mask]
    return report_reference(X, Y, m.mean_, m.scale_, m.coef_, m.intercept_, out.degree)


def test_g13_batch_against_notebook(torch_gpu, g12):
    import s2_emit
    g, emit, s2 = g12
    g13 = load_golden("g13_tile_pairs_report")
    out = s2_emit.fuse_tile_pairs(emit, s2, bands=32, s2_nodata=0.0, report=True)
    assert out.r2.shape == (3, 32) and out.rmse.shape == (3, 32) and out.r2.dtype == torch_gpu.float64
    np.testing.assert_array_equal(out.n_train.cpu().numpy(), g13["n_train"])
    _check_close(out.r2.cpu().numpy(), out.rmse.cpu().numpy(), g13["r2"], g13["rmse"])


@pytest.mark.parametrize("bands", [32, "all"])
def test_against_restatement_from_device_outputs(torch_gpu, g12, bands):
    """T = 32 (the three pairs) and T = 285 (pair 0: 18 band tiles of 16, the last one padded; 9 band groups of 32)."""
    import s2_emit
    g, emit, s2 = g12
    pairs = [0, 1, 2] if bands == 32 else [0]
    out = s2_emit.fuse_tile_pairs(emit[pairs], s2[pairs], bands=bands, s2_nodata=0.0, report=True)
    T = len(out.bands)
    assert out.r2.shape == (len(pairs), T)
    for i, p in enumerate(pairs):
        r2, rmse = _restate(out, i, decode_u16(emit[p])[out.bands])
        _check_close(out.r2[i].cpu().numpy(), out.rmse[i].cpu().numpy(), r2, rmse)


def test_report_kernel_on_exact_integer_data(torch_gpu):
    """hsr_pair_report_f64 alone on small dyadic integers (every logit exact in float64 and float32), npix not a multiple of 16
    or of the 256-row chunk, T = 40 (a partial band group): catches a wrong MFMA row / column map or a dropped tail."""
    from s2_emit import _native as nat
    from s2_emit._engine import _ptr
    torch = torch_gpu
    lib = nat.load()
    rng = np.random.default_rng(13)
    P, npix, nf, T = 2, 1000 + 37, 35, 40
    na, npad = 48, 64
    ldq = na + 48
    mask = (rng.random((P, npix)) < 0.8).astype(np.uint8)
    Q = np.zeros((P, npix, ldq))
    Q[:, :, 0] = 1.0
    Q[:, :, 1:nf + 1] = rng.integers(-2, 3, (P, npix, nf)) * 0.25
    Q[:, :, na:] = 7.0                                   # the target columns: never read
    Q[mask == 0] = 0.0
    Bp = np.full((P, npad, T), 3.0)                      # rows past nf: never read
    Bp[:, :nf] = rng.integers(-2, 3, (P, nf, T)) * 0.125
    b64 = rng.integers(-4, 5, (P, T)) * 0.5
    y = rng.random((P, T, npix)).astype(np.float32)
    status = np.array([0, 0], np.int32)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Qd, Bd, bd, yd, md, sd = d(Q), d(Bp), d(b64), d(y), d(mask), d(status)
    rw = lib.hsr_pair_report_work_bytes(npix, T) // 8
    work = torch.empty((P, rw), dtype=torch.float64, device="cuda")
    r2 = torch.empty((P, T), dtype=torch.float64, device="cuda")
    rmse = torch.empty_like(r2)
    nat.check(lib.hsr_pair_report_f64(_ptr(Qd), ldq, npix * ldq, na, npix, _ptr(bd), T, _ptr(Bd), T, npad * T, nf, _ptr(yd), T * npix,
                                      _ptr(md), npix, T, _ptr(sd), _ptr(work), rw, _ptr(r2), _ptr(rmse), T, P, None),
              "hsr_pair_report_f64")
    for p in range(P):
        m = mask[p] == 1
        z = (Q[p][m][:, :nf + 1] @ np.concatenate([b64[p][None], Bp[p, :nf]])).astype(np.float32)
        yp = np.float32(1) / (np.float32(1) + np.exp(-np.clip(z, np.float32(-50), np.float32(50))))
        yt = y[p].T[m]
        dd = (yt - yp).astype(np.float64)
        ss_res = (dd * dd).sum(0)
        ss_tot = ((yt - yt.astype(np.float64).mean(0)) ** 2).sum(0) + 1e-8
        np.testing.assert_allclose(r2[p].cpu().numpy(), 1 - ss_res / ss_tot, rtol=1e-12, atol=1e-6)
        np.testing.assert_allclose(rmse[p].cpu().numpy(), np.sqrt(ss_res / m.sum()), rtol=1e-6)


def test_batch_bits_equal_single_pairs_any_order(torch_gpu, g12):
    """A pair's r2 / rmse carry the same float64 bits alone and in any position of a batch; a pair without training pixels
    (status 1) is NaN and leaves the others untouched."""
    import s2_emit
    torch = torch_gpu
    g, emit, s2 = g12
    emit4 = np.concatenate([emit, np.full((1,) + emit.shape[1:], 65535, np.uint16)])
    s24 = np.concatenate([s2, s2[:1]])
    E = torch.from_numpy(emit4.view(np.int16)).cuda().view(torch.uint16)
    S = torch.from_numpy(s24.view(np.int16)).cuda().view(torch.uint16)
    batch = s2_emit.fuse_tile_pairs(E, S, s2_nodata=0.0, report=True)
    perm = [3, 2, 0, 1]
    permuted = s2_emit.fuse_tile_pairs([E[i] for i in perm], [S[i] for i in perm], s2_nodata=0.0, report=True)
    singles = [s2_emit.fuse_tile_pair(E[i], S[i], s2_nodata=0.0, report=True) for i in range(4)]
    np.testing.assert_array_equal(batch.status.cpu().numpy(), [0, 0, 0, 1])
    assert bool(torch.isnan(batch.r2[3]).all()) and bool(torch.isnan(batch.rmse[3]).all())
    assert bool(torch.isfinite(batch.r2[:3]).all()) and bool(torch.isfinite(batch.rmse[:3]).all())
    for i in range(4):
        for k in ("r2", "rmse"):
            one = getattr(singles[i], k)[0]
            assert _same_bits(getattr(batch, k)[i], one), (i, k)
            assert _same_bits(getattr(permuted, k)[perm.index(i)], one), (i, k)


def test_report_leaves_every_other_output_unchanged(torch_gpu, g12):
    import s2_emit
    g, emit, s2 = g12
    off = s2_emit.fuse_tile_pairs(emit, s2, s2_nodata=0.0)
    on = s2_emit.fuse_tile_pairs(emit, s2, s2_nodata=0.0, report=True)
    assert off.r2 is None and off.rmse is None
    for k in ("cube", "status", "n_train", "mask", "s2_coarse"):
        assert _same_bits(getattr(on, k), getattr(off, k)), k
    for k in ("mean", "scale", "Bp", "b64", "W32", "b32", "mean32", "inv32"):
        assert _same_bits(on._fit[k], off._fit[k]), k


def test_non_default_stream_and_float32_inputs(torch_gpu, g12):
    """The same bits on a side stream; float32 EMIT / S2 with NaNs and nodata values against the restatement."""
    import s2_emit
    torch = torch_gpu
    g, emit, s2 = g12
    E = torch.from_numpy(emit[:2].view(np.int16)).cuda().view(torch.uint16)
    S = torch.from_numpy(s2[:2].view(np.int16)).cuda().view(torch.uint16)
    ref = s2_emit.fuse_tile_pairs(E, S, s2_nodata=0.0, report=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = s2_emit.fuse_tile_pairs(E, S, s2_nodata=0.0, report=True)
    side.synchronize()
    assert _same_bits(got.r2, ref.r2) and _same_bits(got.rmse, ref.rmse)

    ef = decode_u16(emit[0])
    sf = s2[0].astype(np.float32)
    sel = g["bands"]
    ef[sel[5], 40, 41] = np.nan
    ef[sel[7], 50, 51] = -9999.0
    sf[3, 120, 130] = np.nan
    sf[6, 240, 250] = -1.0
    out = s2_emit.fuse_tile_pair(ef, sf, emit_nodata=-9999.0, s2_nodata=-1.0, report=True)
    assert int(out.status[0]) == 0
    r2, rmse = _restate(out, 0, ef[out.bands])
    _check_close(out.r2[0].cpu().numpy(), out.rmse[0].cpu().numpy(), r2, rmse)
