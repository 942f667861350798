"""The scene kernels' case tables (tests/scene_cases.py) and launch record on the host side: every claim a row makes holds on the
reference alone - counted and uncounted pixels of every intended class, samples on both sides of every tolerance edge, second
trips of the loops a row is there for, windows outside the scene, the conditions of the blend cases - the mirrored instance
names cover all 20 instances, the np.isclose statement of the scan's contract agrees with the float32 / float64 restatement
black_rule on every scan row and on fixture g15, and the three new exports are declared, registered and empty without a
launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scene_cases as sc
from conftest import load_golden
from test_scene_tiles_host import black_rule, g15_mask, window_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("hsr_scene_last_launch", "hsr_scene_instance_count", "hsr_scene_instance_name")
F32, U16 = sc.F32, sc.U16


def _lib():
    from s2_emit import _native as nat
    return nat.load()


# ---- the mirror -------------------------------------------------------------------------------------------------------------------
def test_expected_names_cover_every_instance():
    """The names the rows expect are the 20 of the library's table, none missing and none unknown."""
    lib = _lib()
    table = [lib.hsr_scene_instance_name(i).decode() for i in range(lib.hsr_scene_instance_count())]
    assert lib.hsr_scene_instance_count() == sc.INSTANCE_COUNT == 20 and len(set(table)) == 20
    assert sorted(sc.all_instances()) == sorted(table)
    expected = {sc.scan_instance(d) for d in (F32, U16)}
    expected |= {sc.gather_row_instance(n) for n in sc.GATHER_ROWS}
    expected |= {sc.mosaic_row_instance(n) for n in sc.MOSAIC_ROWS}
    expected |= {sc.blend_row_instance(n) for n in sc.BLEND_ROWS}
    assert expected == set(table), (sorted(set(table) - expected), sorted(expected - set(table)))
    # the blend lattices alone reach all ten blend instances, K below KMAX at 3, 5, 9 and 12
    lattice = {sc.blend_row_instance(n) for n, r in sc.BLEND_ROWS.items() if r["kind"] == "lattice"}
    assert lattice == {t for t in table if t.startswith("scene_blend")}
    ks = sorted({ky * kx for ky, kx in sc.LATTICES})
    assert ks == [1, 2, 3, 4, 5, 8, 9, 12, 16] and [sc.blend_kmax(k) for k in (3, 5, 9, 12)] == [4, 8, 16, 16]
    assert (2, 1) in sc.LATTICES and (1, 2) in sc.LATTICES and (4, 1) in sc.LATTICES and (1, 4) in sc.LATTICES


# ---- scan ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, U16], ids=["float32", "uint16"])
@pytest.mark.parametrize("bands", sc.DECIDING_BANDS)
def test_deciding_band_scenes(dtype, bands):
    scene, cls, specs = sc.deciding_scene(dtype, bands)
    assert scene.shape == (bands,) + sc.DECIDING_HW and scene.dtype == dtype
    ks = {sp[2] for sp in specs if sp[1] == "broken"}
    assert ks == {k for k in (0, 1, 8, 9, bands - 1) if k < bands}
    assert {s for s in np.unique(cls) if s >= 0} == set(range(len(specs)))          # every spec is in the scene
    for kw, enabled in sc.DECIDING_SETTINGS[dtype]:
        mask = sc.black_mask_np(scene, **kw)
        np.testing.assert_array_equal(mask, black_rule(scene, **kw))
        assert not mask[cls < 0].any()                                               # the background is valid
        for s, spec in enumerate(specs):
            want = sc.intended_black(spec, enabled)
            assert (mask[cls == s] == want).all(), (spec, kw)
        counted = {specs[s][0] for s in np.unique(cls[mask])}
        assert counted == set(enabled)
        assert {specs[s][1] for s in np.unique(cls[~mask & (cls >= 0)])} >= {sp[1] for sp in specs if sp[1] != "all"}
        # waves (64 consecutive columns of a row) that hold no black pixel, a single one, and 64
        per_wave = [int(mask[y, x:x + 64].sum()) for y in range(mask.shape[0]) for x in (0, 64, 128)]
        assert 0 in per_wave and 1 in per_wave and 64 in per_wave
        for th, tw in sc.scan_tilings(*sc.DECIDING_HW):
            counts = window_counts(mask, th, tw)
            assert counts.sum() > 0 and sc.scan_rows_per_wave(*sc.DECIDING_HW, th, tw) == 1
            if th == 1:                                                   # windows with nothing to count: an untouched zero
                assert (counts == 0).any()


def test_f32_edge_scene():
    scene, vals = sc.f32_edge_scene()
    C1 = 1 + len(sc.F32_EDGE_CENTERS)
    assert scene.dtype == np.float32 and scene.shape[0] == 3 and len(vals) > 100
    bits = set(vals.view(np.uint32).tolist())
    assert {0x80000000, 0, 1, 0x80000001, 0x7f800000, 0xff800000, 0x7fc00000, 0x7fc12345} <= bits       # -0.0, denormals, Inf, NaN
    flat_index = {int(b): i * C1 for i, b in enumerate(vals.view(np.uint32))}

    def uniform(mask, values):
        """The mask at the pixels that hold ``values`` in all three bands."""
        return [bool(mask.reshape(-1)[flat_index[int(np.float32(v).view(np.uint32))]]) for v in values]

    for call in sc.F32_EDGE_CALLS:
        kw = sc.ref_kwargs(call)
        mask = sc.black_mask_np(scene, **kw)
        np.testing.assert_array_equal(mask, black_rule(scene, **kw))
        assert mask.any() and not mask.all()
        zero = uniform(mask, sc.around(sc.ZERO_ATOL))                       # strict <: the edge itself is out
        assert True in zero and False in zero and not uniform(mask, [np.float32(sc.ZERO_ATOL)])[0]
        assert uniform(mask, [-0.0, 1e-45, -1e-39]) == [True] * 3
        assert uniform(mask, [np.nan, np.inf, -np.inf]) == [call.get("nodata") == np.inf and i == 1 or
                                                             call.get("nodata") == -np.inf and i == 2 for i in range(3)]
    for nd, atol in sc.F32_EDGE_SETS:                                        # both sides of all four edges, in this very scene
        mask = sc.black_mask_np(scene, nodata=nd, nodata_atol=atol)
        for e in sc.f32_edge_points(nd, atol):
            side = uniform(mask, sc.around(e))
            assert True in side and False in side, (nd, atol, e)
    # a NaN nodata in use equals nothing; not in use it is not looked at: the same mask
    np.testing.assert_array_equal(sc.black_mask_np(scene, nodata=float("nan")), sc.black_mask_np(scene, nodata=None))
    # pixels that a centre brackets are decided by band 1 alone
    m = sc.black_mask_np(scene, nodata=-9999.0).reshape(-1)
    i = flat_index[int(np.float32(-9999.0).view(np.uint32))]
    assert m[i] and m[i + 1] and not m[i + 2]                               # (-9999, -9999, -9999) yes; (0.3, -9999, 0.3) no


def test_u16_edge_scene():
    scene = sc.u16_edge_scene()
    pairs = {(int(a), int(b)) for a, b in zip(scene[0].reshape(-1), scene[1].reshape(-1))}
    assert len(pairs) == 49 and (scene[0] == scene[2]).all()
    sums = []
    for call in sc.U16_EDGE_CALLS:
        mask = sc.black_mask_np(scene, **call)
        np.testing.assert_array_equal(mask, black_rule(scene, **call))
        sums.append(int(mask.sum()))
    assert len(set(sums)) >= 5                                        # the settings tell the samples apart
    uni = {int(scene[0, y, x]): (y, x) for y in range(2) for x in range(70) if scene[0, y, x] == scene[1, y, x]}

    def black(v, **kw):
        return bool(sc.black_mask_np(scene, **kw)[uni[v]])

    assert black(0) and not black(1) and black(1, zero_atol=1.5) and not black(2, zero_atol=1.5) and not black(0, zero_atol=0.0)
    assert black(65535, nodata=65535.0) and not black(65534, nodata=65535.0) and black(65534, nodata=65535.0, nodata_atol=1.0)
    assert black(100, nodata=100.5, nodata_atol=0.5) and black(101, nodata=100.5, nodata_atol=0.5)
    assert not black(2, nodata=100.5, nodata_atol=0.5)
    assert black(0, nodata_atol=0.02, zero_atol=0.0) and not black(1, nodata_atol=0.02, zero_atol=0.0)     # 0 is close to -0.01


@pytest.mark.parametrize("dtype", [F32, U16], ids=["float32", "uint16"])
def test_strip_scenes(dtype):
    black, valid = sc.strip_scenes(dtype)
    th, tw = sc.STRIP_TILE
    mb, mv = sc.black_mask_np(black), sc.black_mask_np(valid)
    np.testing.assert_array_equal(mb, black_rule(black))
    assert mb[8:, :].all() and mb[:, 96:].all() and not mv[8:, :].any() and not mv[:, 96:].any()
    np.testing.assert_array_equal(window_counts(mb, th, tw), window_counts(mv, th, tw))
    counts = window_counts(mb, th, tw)
    assert counts.shape == (2, 2) and (counts > 0).all() and (counts < th * tw).all() and len(set(counts.reshape(-1).tolist())) == 4


def test_large_float32_scene_walks_two_rows_a_wave():
    scene = sc.large_f32_scene()
    H, W = sc.LARGE_HW
    assert scene.shape == (1, H, W) and (W + 63) // 64 * H == 33600
    mask = sc.black_mask_np(scene, nodata=-9999.0)
    np.testing.assert_array_equal(mask, black_rule(scene, -9999.0))
    assert 0.4 < mask.mean() < 0.6
    for v in (-9999.0, -0.01, 0.0):
        assert (scene[0][mask] == np.float32(v)).sum() > 1000
    for th, tw in sc.LARGE_TILINGS:
        assert sc.scan_rows_per_wave(H, W, th, tw) == 2, (th, tw)
    assert sc.scan_rows_per_wave(4300, 1100, 301, 500) == 4                 # the uint16 case of test_gpu_scene_tiles.py
    assert sc.scan_rows_per_wave(200, 200, 100, 100) == 1


def test_np_isclose_statement_against_g15():
    g = load_golden("g15_scene_tiles")
    nd = float(g["nodata"])
    for key, arr, nodata in (("mask_emit", g["emit"], nd), ("mask_emit_none", g["emit"], None), ("mask_u16", g["u16"], 65535.0),
                             ("mask_u16_none", g["u16"], None), ("mask_s2_full", g["s2"], None)):
        want = g15_mask(g, key, arr.shape[1:])
        np.testing.assert_array_equal(sc.black_mask_np(arr, nodata), want, err_msg=key)
        np.testing.assert_array_equal(sc.black_mask_np(arr, nodata), black_rule(arr, nodata), err_msg=key)


# ---- gather -------------------------------------------------------------------------------------------------------------------------
def test_gather_rows():
    seen = set()
    for name, (dtype, encode, shape, org, th, tw, off) in sc.GATHER_ROWS.items():
        scene = sc.gather_scene(dtype, shape)
        assert scene.shape == shape and scene.dtype == dtype
        want, inside = sc.gather_ref(scene, org, th, tw, encode)
        out = U16 if encode else dtype
        vec = sc.gather_vec(out, tw, off)
        seen.add((dtype == U16, encode is not None, vec))
        assert inside.any() and want.dtype == out
        if name in sc.GATHER_CHUNK_ROWS:
            assert sc.gather_trips(th, tw, vec) == 2 and (th * tw // (4 if vec else 1)) > 1024 * 256
            assert any(r == shape[1] - th and c == shape[2] - tw for r, c in org)           # the last row and column
            continue
        assert sc.gather_trips(th, tw, vec) == 1
        assert (~inside).sum() == 4 and {int(c) % 4 for (r, c), ok in zip(org, inside) if ok} == {0, 1, 2, 3}
        assert any(r == shape[1] - th and c == shape[2] - tw for r, c in org)
        if tw < 7:                                          # the small tiles need not hold every special sample
            continue
        if dtype == F32:
            tiles = np.stack([scene[:, r:r + th, c:c + tw] for (r, c), ok in zip(org, inside) if ok]).view(np.uint32)
            for b in sc.F32_SPECIAL_BITS + [int(np.float32(-9999.0).view(np.uint32)), int(np.float32(3e6).view(np.uint32))]:
                assert (tiles == b).any(), (name, hex(b))
        if encode:
            tiles = np.stack([scene[:, r:r + th, c:c + tw] for (r, c), ok in zip(org, inside) if ok])
            codes = want[inside]
            assert (codes == encode[3]).any() and (codes == encode[3] - 1).any() and (codes == 0).any()   # nodata, the clamp, negatives
            assert (codes[tiles == np.float32(1e5)] == encode[3] - 1).all() and (tiles == np.float32(1e5)).any()
            assert (codes[np.abs(tiles) == np.float32(3e6)] == 0).all()                     # beyond int32: INT32_MIN, clipped to 0
            assert (codes[tiles == np.float32(-9999.0)] == (encode[3] if encode[1] else 0)).all()
    assert len(seen) == 6
    vec_names = [n for n in sc.GATHER_ROWS if n.endswith("aligned") or n.endswith("next-boundary")]
    assert all(sc.gather_row_instance(n).endswith("true>") for n in vec_names)
    assert all(sc.gather_row_instance(n).endswith("false>") for n in sc.GATHER_ROWS if n.endswith("one-sample-off"))
    assert {sc.GATHER_ROWS[n][5] for n in sc.GATHER_ROWS} >= {1, 7}


# ---- mosaic -------------------------------------------------------------------------------------------------------------------------
def test_mosaic_rows():
    for name, (T, H, W, th, tw, P, out_off, cubes_off, fills) in sc.MOSAIC_ROWS.items():
        cubes, slot = sc.mosaic_case(name)
        assert cubes.shape == (P, T, th, tw) and slot.shape == (H // th, W // tw)
        vec = sc.mosaic_vec(W, tw, out_off, cubes_off if P else 0)
        gy, trips = sc.row_trips(T, H, W, vec)
        if name in sc.MOSAIC_ROW_LOOP:
            assert gy == sc.MOSAIC_ROW_LOOP[name] and trips == 3 and H // th >= 3 and T <= 65535
        else:
            assert gy == H and trips == 1
        assert (slot == -1).any() and ((slot >= 0) & (slot < max(P, 1))).any()
        if P:
            pre = np.full((T, H, W), np.float32(-123.5), np.float32)
            for fill, fill_rest in fills:
                want = sc.assemble(cubes, slot, pre, th, tw, fill, fill_rest)
                bits = want.view(np.uint32)
                assert (bits == 0x7fc12345).any() and np.isnan(cubes).sum() >= 2
                if name != "z-limit":
                    assert (slot == -2).any() and (slot >= P).any() and (want == -123.5).any()
                if fill_rest and (H % th or W % tw):
                    assert (bits[:, H // th * th:, :] == fill.view(np.uint32)).all()
    assert sc.mosaic_row_instance("stack-4-bytes-off") == sc.mosaic_row_instance("output-4-bytes-off") == "scene_mosaic_kernel<false>"
    assert sc.mosaic_row_instance("both-16-bytes-on") == sc.mosaic_row_instance("no-cubes") == "scene_mosaic_kernel<true>"
    assert sc.mosaic_row_instance("row-loop-vec") == sc.mosaic_row_instance("z-limit") == "scene_mosaic_kernel<true>"
    assert sc.mosaic_row_instance("row-loop-scalar") == "scene_mosaic_kernel<false>"


# ---- blend --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.BLEND_ROWS))
def test_blend_rows(name):
    r, case = sc.BLEND_ROWS[name], sc.blend_case(name)
    cubes, start, K, ref = case["cubes"], case["start"], case["K"], case["ref"]
    n, cover = ref["n"], ref["cover"]
    th, tw, sy, sx, H, W, T = (r[k] for k in ("th", "tw", "sy", "sx", "H", "W", "T"))
    assert K == (th // sy) * (tw // sx) and cubes.shape[1:] == (T, th, tw) and n.shape == (T, H, W)
    vec = sc.blend_vec(W, tw, sx, r["out_off"], r["cubes_off"])
    gy, trips = sc.row_trips(T, H, W, vec)
    if r["kind"] == "nofit":
        assert (th > H or tw > W) and not cover.any() and (start >= 0).any()
        return
    if r["kind"] == "short":
        ny, nx = (H - th) // sy + 1, (W - tw) // sx + 1                     # the cells a window can start at
        assert start.shape[0] < ny and start.shape[1] < nx
        assert (cover[:, (start.shape[0] - 1) * sy + th:, :] == 0).all() and (cover[:, :, (start.shape[1] - 1) * sx + tw:] == 0).all()
        assert (cover == K).any() and (cover == 0).any()
        return
    if r["kind"] == "rowloop":
        assert (gy, trips, K, vec) == (32, 3, 4, True) and H // sy > 3 * 2
    else:
        assert gy == H and trips == 1
    # what make_case is there for: holes, single and full coverage, the bad and the spare entries, the payload
    assert (cover == 0).any() and (cover == 1).any() and (cover == K).any() and (n == 1).any()
    assert (start >= len(cubes)).sum() == 1 and (start[-1] >= 0).any() and (start[:, -1] >= 0).any()
    assert ref["one"][1, 0, 0] == 0x7fc12345 and cover[1, 0, 0] == 1
    assert ((cover > 0) & (n == 0)).any()
    if K >= 2:                                                              # an all-NaN pixel under several windows
        assert (n >= 2).any() and cover[0, sy, sx] >= 2 and n[0, sy, sx] == 0
    if r["kind"] == "lattice" and not r["out_off"] and not r["cubes_off"]:
        const = sc.blend_const_case(name)["ref"]
        assert (const["mean"][const["cover"] > 0] == 0.5).all() and (const["n"] == const["cover"]).all()
        assert {int(c) for c in np.unique(const["cover"])} >= {0, 1, K}


# ---- the record and its exports ---------------------------------------------------------------------------------------------------
def test_exports_declared_and_registered():
    from s2_emit import _native as nat
    lib = nat.load()
    text = open(os.path.join(ROOT, "include", "hsr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    for name in EXPORTS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/hsr.h"
        assert name in nat.SIGNATURES, f"{name} has no ctypes signature"
        assert name in comments, f"{name} is not documented in include/hsr.h"
    assert nat.SIGNATURES["hsr_scene_last_launch"] == nat.SIGNATURES["hsr_aux_last_launch"]
    assert nat.SIGNATURES["hsr_scene_instance_name"] == nat.SIGNATURES["hsr_aux_instance_name"]
    # a table of its own: the ABI version and the other records are what they were
    assert lib.hsr_abi_version() == 5 == nat.HSR_ABI_VERSION
    assert lib.hsr_aux_instance_count() == 32 and lib.hsr_k4_instance_count() == 31 and lib.hsr_scene_instance_count() == 20


def test_record_without_a_launch():
    """Empty at the start, untouched by calls their argument checks refuse, capacity handling; names outside the table are NULL
    with an error text."""
    lib = _lib()
    lib.hsr_scene_last_launch(None, 0)                                       # whatever an earlier test left
    buf = C.create_string_buffer(64)
    buf.value = b"junk"
    assert lib.hsr_scene_last_launch(buf, 64) == 0 and buf.value == b""
    buf.value = b"junk"
    assert lib.hsr_scene_last_launch(buf, 0) == 0 and buf.value == b"junk"  # capacity < 1: the buffer is not touched
    assert lib.hsr_scene_last_launch(buf, 1) == 0 and buf.raw[0] == 0
    p, st = C.c_void_p(64), C.c_void_p(0)
    assert lib.hsr_scene_black_counts(p, 3, 3, 10, 10, 2, 2, 0, 0.0, -0.01, 1e-3, 1e-6, p, st) == 2
    assert lib.hsr_scene_gather_tiles(p, 0, 3, 10, 10, p, 1, 11, 2, 0, 1e4, 0, 0.0, 65535, p, st) == 1
    assert lib.hsr_scene_mosaic(p, 1, 3, 4, 4, p, 10, 10, p, 3, 2, 0.0, 1, st) == 1
    assert lib.hsr_scene_mosaic_blend(p, 4, 3, 8, 8, 3, 4, p, 4, 8, p, 23, 36, 0.0, st) == 1
    assert lib.hsr_scene_last_launch(buf, 64) == 0 and buf.value == b""
    assert lib.hsr_scene_last_launch(None, 0) == 0
    names = [lib.hsr_scene_instance_name(i) for i in range(20)]
    assert all(names) and len(set(names)) == 20 and names == [lib.hsr_scene_instance_name(i) for i in range(20)]
    for bad in (-1, 20):
        assert lib.hsr_scene_instance_name(bad) is None
        assert b"hsr_scene_instance_name" in lib.hsr_last_error() and str(bad).encode() in lib.hsr_last_error()


def test_plane_count_limit_of_mosaic_and_blend():
    """T = 65535 passes the argument checks of both, 65536 passes neither.  The blend checks T before the lattice size, so a
    lattice that is refused shows which check spoke.  The mosaic has one shape check and nothing after it but the launch, so its
    acceptance shows as a launch - which only a machine without a GPU can be asked for with pointers that lead nowhere; with a
    GPU the row z-limit of test_gpu_scene_instances.py makes that call on real buffers."""
    import torch
    lib = _lib()
    p, st = C.c_void_p(64), C.c_void_p(0)

    def blend(T):
        rc = lib.hsr_scene_mosaic_blend(p, 4, T, 8, 8, 4, 4, p, 1 << 16, 1 << 15, p, 23, 36, 0.0, st)
        return rc, lib.hsr_last_error().decode()

    rc, text = blend(65535)
    assert rc == 2 and "lattice cells" in text and "T=" not in text
    rc, text = blend(65536)
    assert rc == 2 and "T=65536" in text

    def mosaic(T):
        rc = lib.hsr_scene_mosaic(p, 1, T, 1, 4, p, 3, 4, p, 3, 1, 0.0, 1, st)
        return rc, lib.hsr_last_error().decode()

    rc, text = mosaic(65536)
    assert rc == 1 and "bad shape" in text and "T=65536" in text
    if not torch.cuda.is_available():
        lib.hsr_scene_last_launch(None, 0)
        rc, text = mosaic(65535)
        assert rc == 3 and "scene_mosaic_kernel launch" in text, (rc, text)          # HSR_ERR_HIP: the checks let it through
        assert lib.hsr_scene_last_launch(None, 0) == 0                               # and a failed launch leaves no record
