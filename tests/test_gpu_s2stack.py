"""assemble_s2_stack, the driver of the S2 stack family (s2_emit/s2stack.py), on an MI355X: a window's result is that window of the
full-granule result for every parity of its origin; the device's bits are the host twin's; a clean 20 m band equals
hsr_bilinear_upsample(factor=2) of the float-converted plane bit for bit; `scl=` gives a plane that cloud_mask takes at up = 1;
`invalid` equals the statement's counts.  Every comparison is an equality."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

import s2_emit
import s2stack_cases as sc
import scl_cases as scl
from gpu_harness import torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from s2_emit.scenes import Window

pytestmark = pytest.mark.gpu

H10, W10 = sc.TILE_H + 5, sc.TILE_W + 7                    # 21 x 519: odd, and a tile boundary in each direction
KEYS = [k for _, k, _ in s2_emit.S2_STACK_BANDS]
OFFSETS = {"blue": -1000, "rededge2": -1000, "swir22": 3}
CONFIGS = [("uint16", "strict"), ("uint16", "renorm"), ("float32", "strict"), ("float32", "renorm")]
PARITY_WINDOWS = [Window(2 + pc, 2 + pr, sc.TILE_W + 1, sc.TILE_H + 1) for pr in (0, 1) for pc in (0, 1)]


@functools.lru_cache(maxsize=None)
def granule():
    """The ten band planes of a 21 x 519 granule: DN over the whole range, 5 % nodata, a nodata border on the left."""
    rng = np.random.default_rng(23)
    bands = {}
    for _, key, method in s2_emit.S2_STACK_BANDS:
        up = 1 if method == "nearest" else 2
        p = rng.integers(1, 65536, size=(sc.ceil_div(H10, up), sc.ceil_div(W10, up)))
        p = np.where(rng.random(p.shape) < 0.05, 0, p)
        p[:, :3 // up + 1] = 0
        bands[key] = p.astype(np.uint16)
        bands[key].setflags(write=False)
    return bands


@functools.lru_cache(maxsize=None)
def statement(out_dtype, rule, window):
    b = granule()
    spec = [(1 if m == "nearest" else 2, sc.NEAREST if m == "nearest" else sc.BILINEAR, OFFSETS.get(k, 0)) for _, k, m in s2_emit.S2_STACK_BANDS]
    return sc.stack_ref([b[k] for k in KEYS], spec, (window.row_off, window.col_off, window.height, window.width), 1, 0, sc.RULES[rule],
                        sc.DTYPE_NAMES[out_dtype], 0, np.nan, 10000.0)


def _bits(t):
    """The tensor's bits on the host, as unsigned integers of its width."""
    import torch
    raw = t.view(torch.int16 if t.dtype == torch.uint16 else torch.int32).contiguous().cpu().numpy()
    return raw.view(np.uint16 if raw.dtype == np.int16 else np.uint32)


@pytest.fixture(scope="module")
def full(torch_gpu):
    return {cfg: s2_emit.assemble_s2_stack(granule(), out_dtype=cfg[0], rule=cfg[1], add_offset=OFFSETS, count_invalid=True) for cfg in CONFIGS}


@pytest.mark.parametrize("cfg", CONFIGS)
def test_full_granule_equals_the_statement_with_counts(torch_gpu, full, cfg):
    out = full[cfg]
    want, invalid = statement(cfg[0], cfg[1], Window(0, 0, W10, H10))
    assert out.names == [d for d, _, _ in s2_emit.S2_STACK_BANDS] and out.window == Window(0, 0, W10, H10) and out.scl is None
    assert out.stack.is_contiguous() and tuple(out.stack.shape) == (10, H10, W10) and out.invalid.is_cuda
    assert np.array_equal(_bits(out.stack), want.view(np.uint32) if cfg[0] == "float32" else want)
    assert np.array_equal(out.invalid.cpu().numpy(), invalid) and invalid.min() > 0
    if cfg[1] == "renorm":                                  # the footprint of a 20 m band's nodata is exactly its own pixels
        assert invalid[4] < statement(cfg[0], "strict", Window(0, 0, W10, H10))[1][4]


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("win", PARITY_WINDOWS)
def test_window_is_the_slice_of_the_full_granule(torch_gpu, full, cfg, win):
    torch = torch_gpu
    got = s2_emit.assemble_s2_stack(granule(), window=win, out_dtype=cfg[0], rule=cfg[1], add_offset=OFFSETS, count_invalid=True)
    want = full[cfg].stack[:, win.row_off:win.row_off + win.height, win.col_off:win.col_off + win.width]
    assert got.window == win and got.stack.is_contiguous()
    assert np.array_equal(_bits(got.stack), _bits(want))
    assert np.array_equal(got.invalid.cpu().numpy(), statement(cfg[0], cfg[1], win)[1])
    # into a view with strides of its own: the same bits, and nothing around them
    raw = torch.full((10, win.height + 2, win.width + 5), 7, dtype=torch.int16 if cfg[0] == "uint16" else torch.int32, device="cuda")
    view = raw.view(got.stack.dtype)[:, 1:-1, 2:-3]
    res = s2_emit.assemble_s2_stack(granule(), window=win, out_dtype=cfg[0], rule=cfg[1], add_offset=OFFSETS, out=view)
    assert res.stack is view and res.invalid is None and np.array_equal(_bits(view), _bits(got.stack))
    raw[:, 1:-1, 2:-3] = 7
    assert bool((raw == 7).all())


@pytest.mark.parametrize("cfg", CONFIGS)
def test_device_bits_are_the_host_twins(torch_gpu, full, cfg):
    from s2_emit import _native as nat
    lib, b = nat.load(), granule()
    win = PARITY_WINDOWS[3]
    table = (nat.S2Band * 10)()
    for e, (_, key, method) in zip(table, s2_emit.S2_STACK_BANDS):
        p = b[key]
        e.plane_dev, e.rs, e.H, e.W, e.up = p.ctypes.data, p.shape[1], p.shape[0], p.shape[1], 1 if method == "nearest" else 2
        e.method, e.add_offset = sc.NEAREST if method == "nearest" else sc.BILINEAR, OFFSETS.get(key, 0)
    host = np.zeros((10, win.height, win.width), dtype=cfg[0])
    counts = np.zeros(10, dtype=np.int64)
    rc = lib.hsr_s2_stack_host(table, 10, H10, W10, win.row_off, win.col_off, win.height, win.width, 1, 0, sc.RULES[cfg[1]],
                               sc.DTYPE_NAMES[cfg[0]], C.c_void_p(host.ctypes.data), win.height * win.width, win.width, 0,
                               C.c_float(np.nan), C.c_double(10000.0), C.c_void_p(counts.ctypes.data))
    assert rc == 0, lib.hsr_last_error()
    got = s2_emit.assemble_s2_stack(b, window=win, out_dtype=cfg[0], rule=cfg[1], add_offset=OFFSETS, count_invalid=True)
    assert np.array_equal(_bits(got.stack), host.view(np.uint32) if cfg[0] == "float32" else host)
    assert np.array_equal(got.invalid.cpu().numpy(), counts)


def test_clean_20m_band_equals_bilinear_upsample(torch_gpu):
    """Offset 0, quantification 1, float32, no nodata: both are exact - every value is a multiple of 1 / 16 below 2^20."""
    torch = torch_gpu
    from s2_emit import _engine as eng
    Hc, Wc = 13, 261                                        # the fine grid 26 x 522 crosses a tile boundary in each direction
    rng = np.random.default_rng(5)
    half = rng.integers(0, 65536, size=(Hc, Wc)).astype(np.uint16)
    full10 = rng.integers(0, 65536, size=(2 * Hc, 2 * Wc)).astype(np.uint16)
    bands = {k: (full10 if m == "nearest" else half) for _, k, m in s2_emit.S2_STACK_BANDS}
    out = s2_emit.assemble_s2_stack(bands, out_dtype="float32", nodata=None, quantification=1.0)
    coarse = torch.from_numpy(half.astype(np.float32)).cuda().reshape(1, Hc * Wc)
    want = eng.bilinear_upsample(coarse, Hc, Wc, 2).reshape(2 * Hc, 2 * Wc)
    for b in range(4, 10):
        assert torch.equal(out.stack[b].view(torch.int32), want.view(torch.int32)), out.names[b]
    for b in range(4):
        assert torch.equal(out.stack[b], torch.from_numpy(full10.astype(np.float32)).cuda())


@pytest.mark.parametrize("up", [1, 2])
@pytest.mark.parametrize("win", PARITY_WINDOWS)
def test_scl_under_the_window_is_a_plane_cloud_mask_takes(torch_gpu, up, win):
    from s2_emit import clouds
    plane = np.random.default_rng(up).integers(0, 12, size=(sc.ceil_div(H10, up), sc.ceil_div(W10, up))).astype(np.uint8)
    got = s2_emit.assemble_s2_stack(granule(), window=win, scl=plane)
    want = sc.expand_ref(plane, up, (win.row_off, win.col_off, win.height, win.width))
    assert got.scl.dtype == torch_gpu.uint8 and np.array_equal(got.scl.cpu().numpy(), want)
    assert clouds._up((win.height, win.width), tuple(got.scl.shape), "scl") == 1 == clouds._up(tuple(got.stack.shape[1:]), tuple(got.scl.shape), "scl")
    mask = s2_emit.cloud_mask(got.scl, buffer=1)
    assert np.array_equal(mask.cpu().numpy(), scl.dilate_ref(want, scl.GROW, scl.FLAT, 1, scl.DISC))


def test_nine_bands_with_a_warning(torch_gpu):
    b = {k: v for k, v in granule().items() if k != "nir08"}
    with pytest.warns(UserWarning, match="9 bands"):
        out = s2_emit.assemble_s2_stack(b, window=Window(1, 1, 9, 7))
    assert tuple(out.stack.shape) == (9, 7, 9) and out.names == [d for d, k, _ in s2_emit.S2_STACK_BANDS if k != "nir08"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ten = s2_emit.assemble_s2_stack(granule(), window=Window(1, 1, 9, 7))
    keep = [i for i, k in enumerate(KEYS) if k != "nir08"]
    assert np.array_equal(out.stack.cpu().numpy(), ten.stack.cpu().numpy()[keep])
