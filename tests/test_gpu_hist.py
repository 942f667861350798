"""Histogram matching end to end on an MI355X: hsr_hist_match and the two Python functions against the reference's outputs (fixture
g19) and the statement of tests/hist_cases.py by value, against the host twin bit for bit, twice with the same bits; what comes back
(a new float32 tensor on the device, inputs untouched); more than three channels, non-contiguous input, masks of other dtypes,
out == src; the dtype refusal.  Before this family existed a GPU tensor died in src_rgb.copy()."""
import numpy as np
import pytest

import hist_cases as hc
from conftest import load_golden
from gpu_harness import Buf, LaunchLog, lib, stream, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from test_hist_host import host_match

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
LOG = LaunchLog("hsr_hist_last_launch", joined=True)


def _chain(planar):
    lay = hc.layout_name(planar)
    return [f"hist_keys_kernel<{lay}>"] + hc.sort_record() + ["hist_pivots_kernel", f"hist_lookup_kernel<{lay}>"]


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    gn = np.isnan(got)
    assert got.shape == want.shape and np.array_equal(gn, np.isnan(want)), what
    assert np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~gn]), f"{what}: bits differ"


def _match(torch, src, ref, mask, planar, in_place=False):
    """hsr_hist_match on (C, npix) planes or (npix, C) rows in guarded buffers -> (out, counts)."""
    L = lib()
    Cn, npix = src.shape if planar else src.shape[::-1]
    cs, ps = (npix, 1) if planar else (1, Cn)
    m = np.ascontiguousarray(mask, np.uint8).reshape(-1)
    bs, br, bm = Buf(torch, src.nbytes, 0, src), Buf(torch, ref.nbytes, 4, ref), Buf(torch, npix, 1, m)
    bo = bs if in_place else Buf(torch, src.nbytes, 4)
    need = L.hsr_hist_scratch_bytes(npix, Cn)
    bw, bn = Buf(torch, need), Buf(torch, 8 * Cn, 8)
    LOG.call(_chain(planar), L.hsr_hist_match, bs.ptr, cs, ps, br.ptr, cs, ps, bm.ptr, npix, Cn, bo.ptr, cs, ps, bn.ptr, bw.ptr, need,
             stream(torch))
    out = bo.get(np.float32).reshape(src.shape)
    bw.get(np.uint8)
    if not in_place:
        assert np.array_equal(bs.get(np.uint32), np.ascontiguousarray(src).reshape(-1).view(np.uint32)), "src was written to"
    assert np.array_equal(br.get(np.uint32), np.ascontiguousarray(ref).reshape(-1).view(np.uint32)) and np.array_equal(bm.get(np.uint8), m)
    return out, bn.get(np.int64)


@pytest.mark.parametrize("name", hc.IMAGE_CASES)
@pytest.mark.parametrize("planar", (False, True))
def test_match_equals_g19_the_statement_and_the_host_twin(torch_gpu, name, planar):
    src, ref, mask = hc.image_case(name)
    want, counts = hc.match_hwc(src, ref, mask)
    s, r = src.reshape(-1, 3), ref.reshape(-1, 3)
    if planar:
        s, r = np.ascontiguousarray(s.T), np.ascontiguousarray(r.T)
    got, n = _match(torch_gpu, s, r, mask, planar)
    again, n2 = _match(torch_gpu, s, r, mask, planar)
    _same_bits(again, got, "two runs")
    twin, nt = host_match(s, r, mask, planar)
    _same_bits(got, twin, "device against the host twin")
    img = (got.T if planar else got).reshape(src.shape)
    hc.equal_by_value(img, want, name)
    hc.equal_by_value(img, load_golden("g19_histmatch_f32")["out/" + name], name + " vs g19")
    assert np.array_equal(n, counts) and np.array_equal(n2, counts) and np.array_equal(nt, counts)


def test_match_nonfinite_many_tiles_and_in_place(torch_gpu):
    """Three tiles and more, non-finite samples inside the mask, a channel without a valid pixel; then the same call with out == src."""
    rng = np.random.default_rng(11)
    npix, Cn = 2 * hc.TILE + 77, 4
    src = (rng.random((npix, Cn)) * 1.5 - 0.25).astype(np.float32)
    ref = (np.round(rng.random((npix, Cn)) * 300) / 300).astype(np.float32)
    mask = rng.random(npix) < 0.6
    src[::97, 0], ref[5::89, 1], ref[:, 3] = np.nan, np.inf, np.nan
    want, counts = hc.match_planes(src.T, ref.T, mask)
    got, n = _match(torch_gpu, src, ref, mask, False)
    hc.equal_by_value(got, np.ascontiguousarray(want.T), "many tiles")
    assert np.array_equal(n, counts) and counts[3] == 0 and counts[0] < mask.sum()
    _same_bits(got, host_match(src, ref, mask, False)[0], "device against the host twin")
    inp, n = _match(torch_gpu, src, ref, mask, False, in_place=True)
    _same_bits(inp, got, "out == src")


# ---- the Python functions ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hc.IMAGE_CASES)
def test_histogram_match_rgb_on_gpu_tensors(torch_gpu, name):
    import s2_emit
    torch = torch_gpu
    src, ref, mask = hc.image_case(name)
    ts, tr, tm = torch.from_numpy(src.copy()).cuda(), torch.from_numpy(ref.copy()).cuda(), torch.from_numpy(mask.copy()).cuda()
    out = s2_emit.histogram_match_rgb(ts, tr, tm)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == src.shape
    assert out.data_ptr() != ts.data_ptr() and torch.equal(ts.cpu(), torch.from_numpy(src.copy())) and torch.equal(tr.cpu(), torch.from_numpy(ref.copy()))
    got = out.cpu().numpy()
    hc.equal_by_value(got, load_golden("g19_histmatch_f32")["out/" + name], name + " vs g19")
    hc.equal_by_value(got, s2_emit.histogram_match_rgb(src, ref, mask), name + " vs the NumPy path")
    planes, n = s2_emit.histogram_match_planes(ts.permute(2, 0, 1), tr.permute(2, 0, 1), tm)          # non-contiguous views
    assert planes.is_cuda and planes.dtype == torch.float32 and n.is_cuda and n.dtype == torch.int64 and tuple(planes.shape) == (3,) + src.shape[:2]
    _same_bits(planes.permute(1, 2, 0).cpu().numpy(), got, "planes against rgb")
    assert np.array_equal(n.cpu().numpy(), hc.match_hwc(src, ref, mask)[1])


def test_more_channels_noncontiguous_and_masks(torch_gpu):
    import s2_emit
    torch = torch_gpu
    rng = np.random.default_rng(23)
    H, W = 70, 131                                          # 9170 pixels: two tiles
    src = (rng.random((H, W, 5)) * 1.4 - 0.2).astype(np.float32)
    ref = (rng.integers(0, 256, (H, W, 5)) / 255).astype(np.float32)
    src[3, 4, 4], src[0, 0, 3] = np.nan, 7.0
    mask = rng.random((H, W)) < 0.6
    want, _ = hc.match_hwc(src, ref, mask)
    ts, tr = torch.from_numpy(src).cuda(), torch.from_numpy(ref).cuda()
    for tm in (torch.from_numpy(mask).cuda(), torch.from_numpy(mask.astype(np.uint8) * 3).cuda(), mask, torch.from_numpy(mask.astype(np.float32)).cuda()):
        out = s2_emit.histogram_match_rgb(ts, tr, tm)
        hc.equal_by_value(out.cpu().numpy(), want, "C = 5")
    assert np.isnan(out[3, 4, 4].item()) and out[0, 0, 3].item() == 1.0                                 # the other channels: clipped
    # non-contiguous: a transposed view and a channel slice of a wider image
    wide_s, wide_r = torch.from_numpy(np.concatenate([src, src], axis=2)).cuda(), torch.from_numpy(np.concatenate([ref, ref], axis=2)).cuda()
    out = s2_emit.histogram_match_rgb(wide_s[..., 5:], wide_r[..., 5:], torch.from_numpy(mask).cuda())
    hc.equal_by_value(out.cpu().numpy(), want, "a channel slice")
    out = s2_emit.histogram_match_rgb(ts.transpose(0, 1), tr.transpose(0, 1), torch.from_numpy(mask.T.copy()).cuda())
    hc.equal_by_value(out.cpu().numpy(), np.ascontiguousarray(want.transpose(1, 0, 2)), "a transposed view")
    assert np.array_equal(ts.cpu().numpy().view(np.uint32), src.view(np.uint32)) and np.array_equal(tr.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    # 16 planes, and the counts
    p_s, p_r = (rng.random((16, 40, 50)) * 2 - 0.5).astype(np.float32), rng.random((16, 40, 50)).astype(np.float32)
    p_r[7] = np.nan
    pm = rng.random((40, 50)) < 0.5
    out, n = s2_emit.histogram_match_planes(torch.from_numpy(p_s).cuda(), torch.from_numpy(p_r).cuda(), torch.from_numpy(pm).cuda())
    want, counts = hc.match_planes(p_s, p_r, pm)
    hc.equal_by_value(out.cpu().numpy(), want, "16 planes")
    assert np.array_equal(n.cpu().numpy(), counts) and counts[7] == 0


def test_refusals_of_the_python_functions(torch_gpu):
    import s2_emit
    torch = torch_gpu
    s, m = torch.rand(6, 7, 3, device="cuda"), torch.ones(6, 7, dtype=torch.bool, device="cuda")
    LOG.clear()
    for dt in (torch.float64, torch.float16, torch.bfloat16, torch.uint8):
        with pytest.raises(ValueError, match="float32"):
            s2_emit.histogram_match_rgb(s.to(dt), s, m)
        with pytest.raises(ValueError, match="float32"):
            s2_emit.histogram_match_rgb(s, s.to(dt), m)
        with pytest.raises(ValueError, match="float32"):
            s2_emit.histogram_match_planes(s.to(dt), s, torch.ones(7, 3, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError, match="GPU tensor"):
        s2_emit.histogram_match_rgb(s, s.cpu().numpy(), m)
    with pytest.raises(ValueError, match="GPU tensor"):
        s2_emit.histogram_match_rgb(s.cpu(), s, m)
    with pytest.raises(ValueError, match="differ"):
        s2_emit.histogram_match_rgb(s, s[:5], m)
    with pytest.raises(IndexError, match="mask"):
        s2_emit.histogram_match_rgb(s, s, m[:5])
    with pytest.raises(IndexError, match="out of bounds"):
        s2_emit.histogram_match_rgb(s[..., :2], s[..., :2], m)
    with pytest.raises(ValueError, match="planes outside"):
        s2_emit.histogram_match_planes(torch.rand(17, 4, 4, device="cuda"), torch.rand(17, 4, 4, device="cuda"), torch.ones(4, 4, dtype=torch.bool, device="cuda"))
    assert LOG.read() is None                               # a refusal in Python launches nothing
