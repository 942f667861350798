"""merge_scenes, ortho_merge, merge_emit and merge_grid through the package, on an MI355X.

On every row of tests/merge_cases.py that hsr_ortho_merge takes, ortho_merge - ONE launch - must give the bits of the chain it
replaces: ortho_scene per source (fill_value = nodata), then merge_scenes; and both must give the bits of the NumPy statement.  One
source at offset (0, 0) is ortho_scene itself, the dropped count included.  Device tensors and arrays go in alike; `out=` is filled in
place; the grid of merge_grid places the sources and its geotransform comes back for reproject_scene.  Every comparison is an
equality on uint32 bits."""
import numpy as np
import pytest

import merge_cases as mc
import s2_emit
from gpu_harness import torch_gpu  # noqa: F401  (torch_gpu: the fixture)

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _inputs(torch, name, device=True):
    r, c = mc.ROWS[name], mc.case(name)
    put = (lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()) if device else (lambda a: a)
    kw = dict(layout="bip" if r["layout"] == mc.BIP else "bsq", nodata=r["nodata"], masked_value=r["masked"])
    return r, c, [put(a) for a in c["swaths"]], [put(a) for a in c["glts"]], [put(a) for a in c["qmasks"]], [put(a) for a in c["bmasks"]], kw


@pytest.mark.parametrize("name", mc.ORTHO_ROWS)
def test_ortho_merge_is_the_chain(torch_gpu, name):
    r, c, swaths, glts, qmasks, bmasks, kw = _inputs(torch_gpu, name)
    shape = (r["H"], r["W"])
    fused = s2_emit.ortho_merge(swaths, glts, offsets=c["offsets"], qmasks=qmasks, band_masks=bmasks, shape=shape, source=True, **kw)
    scenes, dropped = [], []
    for k in range(len(swaths)):
        one = s2_emit.ortho_scene(swaths[k], glts[k], qmask=qmasks[k], band_mask=bmasks[k], layout=kw["layout"], fill_value=r["nodata"],
                                  masked_value=r["masked"])
        scenes.append(one.scene)
    chain = s2_emit.merge_scenes(scenes, c["offsets"], layout=kw["layout"], nodata=r["nodata"], shape=shape, source=True)
    np.testing.assert_array_equal(_bits(fused.scene), _bits(chain.scene))
    np.testing.assert_array_equal(fused.source.cpu().numpy(), chain.source.cpu().numpy())
    np.testing.assert_array_equal(_bits(fused.scene), c["ref"])
    np.testing.assert_array_equal(fused.source.cpu().numpy(), c["source"])
    assert fused.dropped.cpu().tolist() == c["dropped"] and fused.geotransform is None
    assert fused.scene.dtype == torch_gpu.float32 and fused.dropped.dtype == torch_gpu.int64 and fused.source.dtype == torch_gpu.uint8


@pytest.mark.parametrize("name", [n for n in mc.ROWS if n.startswith("n1-")])
def test_one_source_is_ortho_scene(torch_gpu, name):
    r, c, swaths, glts, qmasks, bmasks, kw = _inputs(torch_gpu, name)
    fused = s2_emit.ortho_merge(swaths, glts, qmasks=qmasks, band_masks=bmasks, **kw)          # no offsets, no shape: the GLT's grid
    one = s2_emit.ortho_scene(swaths[0], glts[0], qmask=qmasks[0], band_mask=bmasks[0], layout=kw["layout"], fill_value=r["nodata"],
                              masked_value=r["masked"])
    assert fused.scene.shape == one.scene.shape and fused.source is None
    np.testing.assert_array_equal(_bits(fused.scene), _bits(one.scene))
    assert fused.dropped.cpu().tolist() == [int(one.dropped)]


@pytest.mark.parametrize("name", ["nan-falls-bip", "nan-falls-bsq"])
def test_nan_wins_unless_asked(torch_gpu, name):
    torch, r, c = torch_gpu, mc.ROWS[name], mc.case(name)
    layout = "bip" if r["layout"] == mc.BIP else "bsq"
    scenes = [torch.from_numpy(mc.in_layout(s, r["layout"])).cuda() for s in c["scenes"]]
    on = s2_emit.merge_scenes(scenes, c["offsets"], layout=layout, shape=(r["H"], r["W"]), nan_is_nodata=True)
    off = s2_emit.merge_scenes(scenes, c["offsets"], layout=layout, shape=(r["H"], r["W"]))
    np.testing.assert_array_equal(_bits(on.scene), c["ref"])
    ref_off, _ = mc.merge_ref(c["scenes"], c["offsets"], (r["H"], r["W"]), r["nodata"], False)
    np.testing.assert_array_equal(_bits(off.scene), mc.in_layout(ref_off, r["layout"]))
    assert on.source is None and (_bits(on.scene) != _bits(off.scene)).any()


def test_arrays_out_and_the_grid(torch_gpu):
    """NumPy in (copied once), a preallocated output, and the placement from merge_grid: source 1 starts 25 cells east."""
    torch = torch_gpu
    r, c, swaths, glts, qmasks, bmasks, kw = _inputs(torch, "b5-bsq", device=False)
    gt0 = (600000.0, 60.0, 0.0, 4100040.0, 0.0, -60.0)
    gts = [gt0, (600000.0 + 25 * 60.0, 60.0, 0.0, 4100040.0, 0.0, -60.0)]
    grid = s2_emit.merge_grid(gts, [(s["gh"], s["gw"]) for s in r["sources"]])
    assert grid.offsets == tuple(c["offsets"]) and grid.shape == (r["H"], r["W"]) and grid.geotransform == gt0
    out = torch.full((r["bands"], r["H"], r["W"]), 7.0, dtype=torch.float32, device="cuda")
    fused = s2_emit.ortho_merge(swaths, glts, grid=grid, qmasks=qmasks, band_masks=bmasks, out=out, **kw)
    assert fused.scene is out and fused.geotransform == gt0 and fused.source is None
    np.testing.assert_array_equal(_bits(out), c["ref"])
    assert fused.dropped.cpu().tolist() == c["dropped"]
    scenes = [mc.in_layout(s, mc.BSQ) for s in c["scenes"]]
    merged, g2 = s2_emit.merge_emit(scenes, gts, source=True)
    assert g2 == grid
    np.testing.assert_array_equal(_bits(merged.scene), c["ref"])
    np.testing.assert_array_equal(merged.source.cpu().numpy(), c["source"])
    # bounds cut a window out of the union: two cells in from the west, one row down
    b = (gt0[0] + 120.0, gt0[3] - 60.0 * r["H"], gt0[0] + 60.0 * 40, gt0[3] - 60.0)
    cut, g3 = s2_emit.merge_emit(scenes, gts, bounds=b)
    assert g3.shape == (r["H"] - 1, 38) and g3.offsets == ((-1, -2), (-1, 23))
    np.testing.assert_array_equal(_bits(cut.scene), c["ref"][:, 1:, 2:40])
    # the geotransform goes to reproject_scene's planner as it is
    from s2_emit import reproject
    assert len(fused.geotransform) == 6 and hasattr(reproject, "reproject_scene")
