"""resample_area, resample_to_grid and resize_s2_rgb_to on device tensors, on an MI355X: the NumPy statement of
tests/resize_cases.py on planar, pixel-major, padded and sliced tensors; identity; aligned integer factors against hsr_block_mean;
a window of a resample against the same cells of the full one; the resident chain of the demonstration cell.  Every comparison is
an equality."""
import numpy as np
import pytest

import resize_cases as rc
from gpu_harness import lib, stream, torch_gpu  # noqa: F401  (torch_gpu: the fixture)

pytestmark = pytest.mark.gpu


def _img(dtype, shape, seed):
    rng = np.random.default_rng(seed)
    if dtype == "float32":
        return rng.uniform(0.0, 1.0, size=shape).astype(np.float32)
    return rng.integers(0, np.iinfo(dtype).max + 1, size=shape).astype(dtype)


def _dev(torch, a):
    return torch.from_numpy(a.copy()).cuda()


def _host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "float32"])
def test_resample_area_planar_and_pixel_major(torch_gpu, dtype):
    import s2_emit
    torch = torch_gpu
    a = _img(dtype, (3, 45, 83), 1)
    kw = dict(origin=(0.25, -0.5), scale=(2.5, 3.25), rule="renorm", min_valid_frac=0.5)
    want, winv = rc.area_ref(a, (17, 26), kw["origin"], kw["scale"], None, "renorm", 0.5)
    r = s2_emit.resample_area(_dev(torch, a), (17, 26), channel_axis=0, **kw)
    assert isinstance(r, s2_emit.AreaResampleOutput) and r.image.is_cuda and r.invalid.is_cuda and r.image.shape == (3, 17, 26)
    rc.same(_host(r.image), want, "planar")
    assert np.array_equal(_host(r.invalid), winv)
    r = s2_emit.resample_area(_dev(torch, np.moveaxis(a, 0, -1)), (17, 26), channel_axis=-1, **kw)
    assert r.image.shape == (17, 26, 3) and r.image.is_contiguous()
    rc.same(_host(r.image), np.ascontiguousarray(np.moveaxis(want, 0, -1)), "pixel-major")
    # a channel slice of a wider image with padded rows, into a slice of a wider output, as float32
    wide_np = _img(dtype, (45, 90, 4), 2)
    view = _dev(torch, wide_np)[:, 3:86, 1:4]
    out = torch.full((17, 30, 5), -7.0, dtype=torch.float32, device="cuda")
    r = s2_emit.resample_area(view, (17, 26), channel_axis=-1, out_dtype="float32", post_scale=0.5, out=out[:, 2:28, 1:4], **kw)
    want, _ = rc.area_ref(np.moveaxis(wide_np[:, 3:86, 1:4], -1, 0), (17, 26), kw["origin"], kw["scale"], None, "renorm", 0.5, "float32", 0.5)
    rc.same(_host(out[:, 2:28, 1:4]), np.ascontiguousarray(np.moveaxis(want, 0, -1)), "slice")
    rest = _host(out).copy()
    rest[:, 2:28, 1:4] = -7.0
    assert (rest == -7.0).all()
    # a plane
    r = s2_emit.resample_area(_dev(torch, a[0]), (9, 9), nodata=float(a[0, 0, 0]), rule="strict", nodata_out=3, fill=-1.0)
    want, winv = rc.area_ref(a[:1], (9, 9), nodata=float(a[0, 0, 0]), rule="strict", nodata_out=3, fill=-1.0)
    rc.same(_host(r.image), want[0], "plane")
    assert np.array_equal(_host(r.invalid), winv) and winv[0] >= 1


def test_resample_to_grid(torch_gpu):
    import s2_emit
    torch = torch_gpu
    a = _img("uint16", (10, 120, 150), 3)
    src_gt, dst_gt = (600000.0, 10.0, 0.0, 4100040.0, 0.0, -10.0), (600002.5, 60.0, 0.0, 4100044.0, 0.0, -60.0)
    r = s2_emit.resample_to_grid(_dev(torch, a), src_gt, dst_gt, (22, 26), channel_axis=0, out_dtype="float32", post_scale=1e-4)
    want, winv = rc.area_ref(a, (22, 26), (-0.4, 0.25), (6.0, 6.0), out_dtype="float32", post=1e-4)
    rc.same(_host(r.image), want, "grid")
    assert np.array_equal(_host(r.invalid), winv) and winv[0] == 22 + 26 - 1       # the row below the source and the column past it
    with pytest.raises(ValueError, match="origin and scale"):
        s2_emit.resample_to_grid(_dev(torch, a), src_gt, dst_gt, (22, 26), channel_axis=0, scale=(6.0, 6.0))


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "float32"])
def test_resize_s2_rgb_to(torch_gpu, dtype):
    import s2_emit
    torch = torch_gpu
    a = _img(dtype, (3, 149, 211), 4)
    out = s2_emit.resize_s2_rgb_to(_dev(torch, np.moveaxis(a, 0, -1)), (24, 35))
    assert out.is_cuda and out.shape == (24, 35, 3) and str(out.dtype) == "torch." + dtype
    rc.same(_host(out), np.ascontiguousarray(np.moveaxis(rc.area_ref(a, (24, 35))[0], 0, -1)), "rgb")
    plane = s2_emit.resize_s2_rgb_to(_dev(torch, a[1]), (149, 35))
    rc.same(_host(plane), rc.area_ref(a[1:2], (149, 35))[0][0], "plane")
    for bad in ((150, 35), (24, 212)):
        with pytest.raises(ValueError, match="hsr_bilinear_upsample"):
            s2_emit.resize_s2_rgb_to(_dev(torch, a[1]), bad)


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "float32"])
def test_identity_equals_the_input(torch_gpu, dtype):
    import s2_emit
    a = _img(dtype, (37, 65, 3), 5)
    if dtype == "float32":
        a = (a - np.float32(0.5)) * np.float32(1e6)
    out = s2_emit.resize_s2_rgb_to(_dev(torch_gpu, a), (37, 65))
    assert np.array_equal(_host(out).view(np.uint8), a.view(np.uint8))


@pytest.mark.parametrize("dtype,f,pixmajor", [("uint8", 2, False), ("uint8", 6, True), ("uint16", 6, False), ("uint16", 3, True),
                                              ("uint8", 12, False)])
def test_aligned_factor_equals_block_mean(torch_gpu, dtype, f, pixmajor):
    """hsr_block_mean(scale = 1) on the same buffers, bit for bit; f = 12 takes the gather instance."""
    import s2_emit
    torch = torch_gpu
    nb, Hc, Wc = 3, 21, 40                                  # rows of Wc f elements are multiples of 16 bytes: the staged block mean
    a = _img(dtype, (Hc * f, Wc * f, nb) if pixmajor else (nb, Hc * f, Wc * f), 6)
    src = _dev(torch, a)
    r = s2_emit.resample_area(src, (Hc, Wc), channel_axis=-1 if pixmajor else 0, out_dtype="float32")
    ref = torch.full((Hc, Wc, nb) if pixmajor else (nb, Hc, Wc), -1.0, dtype=torch.float32, device="cuda")
    in_bs, in_ps, out_bs, out_ps = (1, nb, 1, nb) if pixmajor else (Hc * f * Wc * f, 1, Hc * Wc, 1)
    assert lib().hsr_block_mean(src.data_ptr(), rc.CODES[dtype], in_bs, in_ps, nb, Hc, Wc, f, 1.0, ref.data_ptr(), out_bs, out_ps,
                                stream(torch)) == 0, lib().hsr_last_error()
    assert np.array_equal(_host(r.image).view(np.uint32), _host(ref).view(np.uint32))
    assert not _host(r.invalid).any()


def test_window_equals_the_cells_of_the_full_resample(torch_gpu):
    """The origin moved by whole destination cells.  Scale and origin are dyadic, so origin + Y0 * scale is exact and the window's
    cell edges are the full resample's, bit for bit: that case only."""
    import s2_emit
    a = _img("float32", (2, 150, 170), 7)
    a[0, 40:44, 60:70] = np.nan
    src = _dev(torch_gpu, a)
    origin, scale = (0.25, -1.5), (2.5, 3.25)
    full = s2_emit.resample_area(src, (58, 50), channel_axis=0, origin=origin, scale=scale, rule="strict")
    for Y0, X0, hh, ww in ((0, 0, 58, 50), (9, 7, 20, 33), (40, 17, 18, 33), (57, 49, 1, 1)):
        win = s2_emit.resample_area(src, (hh, ww), channel_axis=0, origin=(origin[0] + Y0 * scale[0], origin[1] + X0 * scale[1]), scale=scale,
                                    rule="strict")
        rc.same(_host(win.image), _host(full.image)[:, Y0:Y0 + hh, X0:X0 + ww], f"window {(Y0, X0, hh, ww)}")
    assert _host(full.invalid)[0] > 0


def test_resident_chain_of_the_demonstration_cell(torch_gpu):
    """pseudo_s2_rgb -> resize_s2_rgb_to -> apply_shared_percentile_stretch -> histogram_match_rgb with every image on the device:
    the resized S2 RGB equals the statement, and the chain's result equals the chain fed with the statement's image."""
    import s2_emit
    torch = torch_gpu
    H, W = 40, 52
    rng = np.random.default_rng(8)
    bands = {b: _dev(torch, rng.uniform(0.02, 0.4, size=(H, W)).astype(np.float32)) for b in ("B4", "B3", "B2")}
    s2 = _img("uint8", (3, 247, 319), 9)
    mask = torch.ones((H, W), dtype=torch.bool, device="cuda")
    mask[:3, :] = False
    pseudo = s2_emit.pseudo_s2_rgb(bands)
    small = s2_emit.resize_s2_rgb_to(_dev(torch, np.moveaxis(s2, 0, -1)), pseudo.shape[:2])
    assert small.is_cuda and small.dtype == torch.uint8 and tuple(small.shape) == (H, W, 3)
    want = np.ascontiguousarray(np.moveaxis(rc.area_ref(s2, (H, W))[0], 0, -1))
    assert np.array_equal(_host(small), want)
    a, b = s2_emit.apply_shared_percentile_stretch(pseudo, mask), s2_emit.apply_shared_percentile_stretch(small, mask)
    matched = s2_emit.histogram_match_rgb(a, b, mask)
    assert matched.is_cuda and matched.dtype == torch.float32 and tuple(matched.shape) == (H, W, 3)
    b_ref = s2_emit.apply_shared_percentile_stretch(_dev(torch, want), mask)
    ref = s2_emit.histogram_match_rgb(a, b_ref, mask)
    assert np.array_equal(_host(matched).view(np.uint32), _host(ref).view(np.uint32))
    assert np.isfinite(_host(matched)).all()
