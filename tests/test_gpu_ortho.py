"""s2_emit.ortho on an MI355X: the public functions against fixture g16 (the reference's apply_glt) for NumPy and tensor input,
out= reuse, repeatability, byte offsets past 2^32 on the swath side and on the output side (checked on the device: one boolean
crosses to the host), and the scene it makes going straight into find_valid_paired_tiles."""
import numpy as np
import pytest

import ortho_cases as oc
import s2_emit
from conftest import load_golden
from gpu_harness import torch_gpu  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _host(t):
    return t.cpu().numpy()


def test_apply_glt_against_g16(torch_gpu):
    torch = torch_gpu
    g = load_golden("g16_ortho")
    s285, s3, mixed = g["swath285"], g["swath3"], g["glt_mixed"]
    got = s2_emit.apply_glt(s285, mixed)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (9, 11, 285)
    np.testing.assert_array_equal(_bits(got), _bits(g["out285_plain"]))
    got = s2_emit.apply_glt(torch.from_numpy(s285).cuda(), torch.from_numpy(mixed).cuda())
    assert got.is_cuda and got.dtype == torch.float32
    np.testing.assert_array_equal(_bits(_host(got)), _bits(g["out285_plain"]))
    np.testing.assert_array_equal(_bits(s2_emit.apply_glt(s3, mixed.astype(np.int64))), _bits(g["out3_plain"]))
    np.testing.assert_array_equal(_bits(s2_emit.apply_glt(s285, g["glt_nodata"])), _bits(g["out285_nodata"]))
    np.testing.assert_array_equal(_bits(s2_emit.apply_glt(s285, g["glt_valid"].astype(np.uint16))), _bits(g["out285_valid"]))
    np.testing.assert_array_equal(_bits(s2_emit.apply_glt(s285, g["glt_drop"])), _bits(g["out285_drop"]))
    # a 2-d input is one band; a float64 input is cast as NumPy's assignment casts it; fill_value and the no-data value are used
    one = s2_emit.apply_glt(s3[:, :, 1], mixed)
    np.testing.assert_array_equal(_bits(one), _bits(g["out3_plain"][:, :, 1:2]))
    f64 = np.linspace(-1.0, 1.0, 6 * 5 * 3).reshape(6, 5, 3) / 3.0
    ref, _ = oc.ortho_ref(f64.astype(np.float32), mixed, fill=7.5)
    np.testing.assert_array_equal(_bits(s2_emit.apply_glt(f64, mixed, fill_value=7.5)), ref)
    other = np.where(mixed == 0, -3, mixed).astype(np.int32)
    np.testing.assert_array_equal(_bits(s2_emit.apply_glt(s3, other, GLT_NODATA_VALUE=-3)), _bits(g["out3_plain"]))


def test_ortho_scene_against_g16(torch_gpu):
    torch = torch_gpu
    g = load_golden("g16_ortho")
    s285, s3, mixed, q, b = g["swath285"], g["swath3"], g["glt_mixed"], g["qmask"], g["bmask"]
    dev = lambda a: torch.from_numpy(a).cuda()                                            # noqa: E731
    for as_tensor in (False, True):
        conv = dev if as_tensor else (lambda a: a)
        for tag, qm, bm in (("plain", None, None), ("q", q, None), ("b", None, b), ("qb", q, b)):
            for layout in ("bip", "bsq"):
                out = s2_emit.ortho_scene(conv(s285), conv(mixed), qmask=None if qm is None else conv(qm),
                                          band_mask=None if bm is None else conv(bm), layout=layout)
                assert out.scene.is_cuda and out.dropped.is_cuda and out.dropped.dtype == torch.int64 and out.dropped.shape == ()
                assert out.window == (0, 0, 9, 11)
                got = _host(out.scene)
                np.testing.assert_array_equal(_bits(got if layout == "bip" else got.transpose(1, 2, 0)), _bits(g[f"out285_{tag}"]))
                assert int(out.dropped) == 0
        out = s2_emit.ortho_scene(conv(s3), conv(mixed), qmask=conv(q.astype(np.float64)), layout="bip")   # a float mask: == 1
        np.testing.assert_array_equal(_bits(_host(out.scene)), _bits(g["out3_q"]))
        out = s2_emit.ortho_scene(conv(s285), conv(g["glt_drop"]), layout="bip")
        np.testing.assert_array_equal(_bits(_host(out.scene)), _bits(g["out285_drop"]))
        assert int(out.dropped) == int(g["dropped_drop"])
        for k, win in enumerate(g["windows"]):
            win = tuple(int(v) for v in win)
            out = s2_emit.ortho_scene(conv(s285), conv(g["glt_drop"]), qmask=conv(q), band_mask=conv(b), window=win, layout="bsq")
            assert out.window == win and tuple(out.scene.shape) == (285, win[2], win[3])
            np.testing.assert_array_equal(_bits(_host(out.scene).transpose(1, 2, 0)), _bits(g[f"out285_win{k}"]))
            assert int(out.dropped) == int(g[f"dropped_win{k}"])
        # entries outside int32 are out of bounds: dropped, whatever they would wrap to
        wide = g["glt_mixed"].astype(np.int64)
        wide[4, 4], wide[5, 5] = ((1 << 32) + 2, 3), (2, -(1 << 40))
        ref, dropped = oc.ortho_ref(s3, np.where(np.abs(wide) > (1 << 31), -1, wide).astype(np.int32))
        out = s2_emit.ortho_scene(conv(s3), conv(wide), layout="bip")
        np.testing.assert_array_equal(_bits(_host(out.scene)), ref)
        assert int(out.dropped) == dropped == 2
    # masked_value is a parameter of its own
    out = s2_emit.ortho_scene(s3, mixed, qmask=q, layout="bip", fill_value=1.5, masked_value=-2.5)
    ref, _ = oc.ortho_ref(s3, mixed, qmask=q, fill=1.5, masked=-2.5)
    np.testing.assert_array_equal(_bits(_host(out.scene)), ref)


def test_out_reuse_and_repeatability(torch_gpu):
    torch = torch_gpu
    g = load_golden("g16_ortho")
    S, G = torch.from_numpy(g["swath285"]).cuda(), torch.from_numpy(g["glt_drop"]).cuda()
    Q, B = torch.from_numpy(g["qmask"]).cuda(), torch.from_numpy(g["bmask"]).cuda()
    for layout in ("bip", "bsq"):
        first = s2_emit.ortho_scene(S, G, qmask=Q, band_mask=B, layout=layout)
        buf = torch.full_like(first.scene, 123.0)
        again = s2_emit.ortho_scene(S, G, qmask=Q, band_mask=B, layout=layout, out=buf)
        assert again.scene.data_ptr() == buf.data_ptr()
        assert torch.equal(first.scene.view(torch.int32), buf.view(torch.int32)) and int(first.dropped) == int(again.dropped) == 10
        third = s2_emit.ortho_scene(S, G, qmask=Q, band_mask=B, layout=layout, out=buf)             # over its own result
        assert torch.equal(first.scene.view(torch.int32), third.scene.view(torch.int32))
        with pytest.raises(ValueError):
            s2_emit.ortho_scene(S, G, layout=layout, out=buf.reshape(-1))


def test_swath_byte_offsets_past_2_to_32(torch_gpu):
    """A (1, N, 285) swath just over 2^32 bytes holding (flat index mod 2^24) and a small table that points at its first and last
    pixels and at the pixels on either side of the 2^31- and 2^32-byte marks."""
    torch = torch_gpu
    bands, N = 285, 3767600
    assert N * bands * 4 > 1 << 32 and (N - 100) * bands * 4 < 1 << 32
    S = torch.arange(N * bands, dtype=torch.int32, device="cuda").bitwise_and_(0xFFFFFF).to(torch.float32).view(1, N, bands)
    half, full = (1 << 31) // (bands * 4), (1 << 32) // (bands * 4)
    cols = [1, N, half, half + 1, half + 2, full, full + 1, full + 2, N - 1, 2, N + 1, 0]          # one-based; the last two: fill
    G = torch.tensor([[c, 1] for c in cols], dtype=torch.int32, device="cuda").view(3, 4, 2)
    idx = (G[..., 0].to(torch.int64) - 1)[..., None] * bands + torch.arange(bands, device="cuda")
    want = idx.bitwise_and(0xFFFFFF).to(torch.float32)
    want[2, 2:] = -9999.0
    for layout in ("bip", "bsq"):
        out = s2_emit.ortho_scene(S, G, layout=layout)
        got = out.scene if layout == "bip" else out.scene.permute(1, 2, 0).contiguous()
        assert bool(torch.equal(got.view(torch.int32), want.view(torch.int32))), layout
        assert int(out.dropped) == 1
    del S


def test_bsq_output_byte_offsets_past_2_to_32(torch_gpu):
    """A band-sequential output just over 2^32 bytes from a tiny swath, against the torch indexing expression."""
    torch = torch_gpu
    bands, side = 285, 1942
    assert side * side * bands * 4 > 1 << 32
    gen = torch.Generator(device="cuda").manual_seed(5)
    S = torch.randint(-(1 << 31), (1 << 31) - 1, (6, 5, bands), dtype=torch.int64, device="cuda", generator=gen).to(torch.int32).view(torch.float32)
    gx = torch.randint(0, 6, (side, side), device="cuda", generator=gen)                  # 0: no data, 1 .. 5 valid
    gy = torch.randint(1, 7, (side, side), device="cuda", generator=gen)
    G = torch.stack([gx, gy], dim=-1).to(torch.int32)
    out = s2_emit.ortho_scene(S, G, layout="bsq")
    Si = S.view(torch.int32)
    want = Si[gy - 1, (gx - 1).clamp(min=0)]                                              # (side, side, bands)
    want[gx == 0] = torch.tensor(-9999.0).view(torch.int32).item()
    want = want.permute(2, 0, 1).contiguous()
    assert bool(torch.equal(out.scene.view(torch.int32), want))
    assert int(out.dropped) == 0 and tuple(out.scene.shape) == (bands, side, side)


def test_scene_goes_into_find_valid_paired_tiles(torch_gpu):
    """ortho_scene(layout="bsq") of a strictly positive swath is a scene for find_valid_paired_tiles(emit_nodata=-9999): the black
    pixels of a window are its fill pixels - the cells without data or outside the swath, counted from the table on the host."""
    torch = torch_gpu
    rows, cols, bands, tile = 7, 9, 5, 10
    rng = np.random.default_rng(3)
    swath = rng.uniform(0.05, 0.6, (rows, cols, bands)).astype(np.float32)
    glt = oc.glt_of("mixed", 40, 60, rows, cols)
    out = s2_emit.ortho_scene(swath, glt, layout="bsq")
    s2 = torch.ones((1, 40, 60), dtype=torch.float32, device="cuda")
    tiles = s2_emit.find_valid_paired_tiles(out.scene, s2, tile, 1, 1.0, emit_nodata=-9999.0)
    assert len(tiles) == 4 * 6
    g = glt.astype(np.int64)
    valid = (g != 0).all(axis=-1) & (g[..., 0] >= 1) & (g[..., 0] <= cols) & (g[..., 1] >= 1) & (g[..., 1] <= rows)
    total = 0
    for t in tiles:
        w = t["emit_window"]
        fill = int((~valid[w.row_off:w.row_off + tile, w.col_off:w.col_off + tile]).sum())
        assert t["emit_black_frac"] == fill / (tile * tile) and t["s2_black_frac"] == 0.0
        total += fill
    assert 0 < total < 40 * 60 and int(out.dropped) == int(((g != 0).all(axis=-1) & ~valid).sum())
