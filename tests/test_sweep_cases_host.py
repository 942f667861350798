"""The drawn rows of tests/sweep_cases.py on the references alone: what tests/test_gpu_family_sweeps.py relies on when it runs the
same rows (seeds 1 and 2, 24 each) on the GPU.  Rows are reproducible; every row passes the Python mirror of its entry point's
documented argument rules; at most 10 % of a sweep's rows fail their table's admission condition; per seed the rows reach every
instance the family's mirror can name for a valid call; per size parameter they hold at least three values no table row has; and
the planted slips - a wrong reading of the row, applied to the reference - leave the bar (or change the answer, where the bar is
bit equality) on at least one drawn row of each seed, so a kernel with that slip would fail the GPU sweep."""
import numpy as np
import pytest

import affine_cases as ac
import coreg_cases as cc
import ortho_cases as oc
import scene_cases as sc
import sweep_cases as sw

CASES = [(s, seed) for s in sw.SWEEPS for seed in sw.SEEDS]
_cache = {}


def rows_of(sweep, seed):
    """[(index, row, case, admitted)] of one GPU test, built once."""
    if (sweep, seed) not in _cache:
        out = []
        for k in range(sw.ROWS_PER_SEED):
            r = sw.draw(sweep, seed, k)
            c = sw.case(sweep, r)
            out.append((k, r, c, sw.SWEEPS[sweep].admitted(r, c)))
        _cache[sweep, seed] = out
    return _cache[sweep, seed]


def admitted_rows(sweep, seed):
    return [(k, r, c) for k, r, c, ok in rows_of(sweep, seed) if ok]


@pytest.mark.parametrize("sweep, seed", CASES)
def test_rows_are_reproducible_and_in_contract(sweep, seed):
    S = sw.SWEEPS[sweep]
    for k, r, _, _ in rows_of(sweep, seed):
        assert sw.rows_equal(r, sw.draw(sweep, seed, k)), (sweep, seed, k)
        assert S.valid(r), (sweep, seed, k, r)
    assert not sw.rows_equal(sw.draw(sweep, seed, 0), sw.draw(sweep, seed, 1))
    assert not sw.rows_equal(sw.draw(sweep, 1, 0), sw.draw(sweep, 2, 0))


def test_the_mirrors_refuse_an_out_of_contract_row():
    """One field pushed outside the documented range: the mirror of every sweep says so."""
    bad = {"scene-scan": [dict(th=0), dict(tw=10 ** 6), dict(bands=0), dict(dtype=np.dtype(np.int16))],
           "scene-gather": [(4, 0), (5, 10 ** 6), (3, np.array([[-1, 0]], np.int32)), (6, 1)],
           "scene-mosaic": [(0, 0), (3, 10 ** 6), (5, -1), (6, 2)],
           "scene-blend": [dict(sy=0), dict(sx=10 ** 6), dict(T=65536), dict(out_off=2)],
           "ortho": [dict(bands=oc.MAX_BANDS + 1), dict(window=(0, 0, 1, 10 ** 6)), dict(layout=2), dict(swath_off=2), dict(rows=0)],
           "color-moments": [dict(npix=-1), dict(x=("packed", 2)), dict(rs=(2, 3)), dict(mask="some")],
           "color-solve": [dict(nslots=0), dict(nslots=ac.MAX_SLOTS + 1), dict(min_count=-1)],
           "color-apply": [dict(npix=-1), dict(clip=3), dict(out=("rows", 0)), dict(At=np.zeros(9))],
           "coreg-surface": [dict(w=3), dict(w=65), dict(f=9), dict(f=0), dict(R=25), dict(min_valid=0), dict(pads=(0, -1, 0))],
           "coreg-peaks": [dict(w=3), dict(f=9), dict(R=0)],
           "coreg-model": [dict(kind=2), dict(min_points=-1), dict(reject_px=0.0), dict(hs=0)],
           "coreg-warp": [dict(h=0), dict(bound=(-1.0, 0.0)), dict(extra=-1), dict(off=1)]}
    assert set(bad) == set(sw.SWEEPS)
    for sweep, edits in bad.items():
        r = sw.draw(sweep, 1, 0)
        assert sw.SWEEPS[sweep].valid(r)
        for e in edits:
            if isinstance(r, tuple):                           # a tuple row: (position, value)
                edited = r[:e[0]] + (e[1],) + r[e[0] + 1:]
            else:
                assert set(e) <= set(r)
                edited = dict(r, **e)
            assert not sw.SWEEPS[sweep].valid(edited), (sweep, e)


@pytest.mark.parametrize("sweep", list(sw.SWEEPS))
def test_skipped_share(sweep):
    for seed in sw.SEEDS:
        skipped = sum(not ok for _, _, _, ok in rows_of(sweep, seed))
        print(f"{sweep} seed {seed}: {skipped} of {sw.ROWS_PER_SEED} rows skipped")
        assert skipped <= sw.MAX_SKIPPED * sw.ROWS_PER_SEED, (sweep, seed, skipped)


_COLOR = ac.all_instances()
_SCENE = sc.all_instances()
INSTANCES = {"scene-scan": set(_SCENE[:2]), "scene-gather": set(_SCENE[2:8]), "scene-mosaic": set(_SCENE[8:10]), "scene-blend": set(_SCENE[10:]),
             "ortho": set(oc.all_instances()), "color-moments": set(_COLOR[:11]), "color-solve": {_COLOR[10]}, "color-apply": set(_COLOR[11:]),
             "coreg-surface": set(cc.all_instances()[:2]), "coreg-peaks": {cc.all_instances()[2]},
             "coreg-model": {cc.all_instances()[3]}, "coreg-warp": set(cc.all_instances()[4:])}


@pytest.mark.parametrize("sweep, seed", CASES)
def test_rows_reach_every_instance(sweep, seed):
    seen = {n for _, r, _ in admitted_rows(sweep, seed) for n in sw.SWEEPS[sweep].instances(r)}
    assert seen == INSTANCES[sweep], (sorted(INSTANCES[sweep] - seen), sorted(seen - INSTANCES[sweep]))


def test_the_sweeps_name_every_instance_of_their_families():
    for family, names in (("scene", sc.all_instances()), ("ortho", oc.all_instances()), ("color", ac.all_instances()), ("coreg", cc.all_instances())):
        assert set().union(*(INSTANCES[s] for s in sw.SWEEPS if sw.SWEEPS[s].family == family)) == set(names)


@pytest.mark.parametrize("sweep", list(sw.SWEEPS))
def test_rows_hold_sizes_the_table_has_not(sweep):
    S = sw.SWEEPS[sweep]
    table = [S.sizes(r) for r in S.table]
    drawn = [S.sizes(r) for seed in sw.SEEDS for _, r, _ in admitted_rows(sweep, seed)]
    for name in drawn[0]:
        new = {d[name] for d in drawn} - {t[name] for t in table}
        assert len(new) >= 3, (sweep, name, sorted(new))


# ---- planted slips -------------------------------------------------------------------------------------------------------------------
def _ortho_slip(kind, r, c):
    """The ortho reference under a wrong reading of the row -> (bits in the row's layout, dropped)."""
    swath, glt, win, bmask, layout = c["swath"], c["glt"], r["window"], c["bmask"], r["layout"]
    rows, cols, bands = swath.shape
    kw = dict(qmask=c["qmask"], fill=r["fill"], masked=r["masked"], nodata=r["nodata"])
    if kind == "extents transposed":                          # the inside test with rows and cols exchanged
        g = glt.astype(np.int64).copy()
        sx, sy = g[..., 0] - 1, g[..., 1] - 1
        flip = ((sx >= 0) & (sx < rows) & (sy >= 0) & (sy < cols)) != ((sx >= 0) & (sx < cols) & (sy >= 0) & (sy < rows))
        valid = (g[..., 0] != r["nodata"]) & (g[..., 1] != r["nodata"])
        inside = (sx >= 0) & (sx < cols) & (sy >= 0) & (sy < rows)
        g[flip & valid & inside] = oc.I32_MAX                 # read as outside
        g[flip & valid & ~inside] = 1 if r["nodata"] != 1 else 2        # read as inside: some cell
        glt = g
    if kind == "window origin off by one":
        r0, c0, h, w = win
        win = (r0, c0 + 1 if c0 + w < r["gw"] else max(c0 - 1, 0), h, w)
    if kind == "a row stride taken from another operand" and bmask is not None:      # the band mask's pitch: the minimum, not its own
        nb = (bands + 7) // 8
        bmask = bmask.reshape(-1)[:rows * cols * nb].reshape(rows, cols, nb)
    out, dropped = oc.ortho_ref(swath, glt, window=win, bmask=bmask, layout=oc.BIP, **kw)
    if kind == "ragged tail dropped":                         # the pixels past the last whole PX of an output row stay fill
        out[:, win[3] - win[3] % oc.PX:, :] = oc.f32_bits(r["fill"])
    if kind == "band tail dropped":                           # the bands % 4 behind the float4 stay fill
        out[:, :, bands - bands % 4:] = oc.f32_bits(r["fill"])
    if layout == oc.BSQ:
        out = out.reshape(bands, win[2], win[3]) if kind == "bip/bsq permutation wrong" else np.ascontiguousarray(out.transpose(2, 0, 1))
    elif kind == "bip/bsq permutation wrong":
        out = np.ascontiguousarray(out.transpose(2, 0, 1)).reshape(win[2], win[3], bands)
    return out, dropped


@pytest.mark.parametrize("seed", sw.SEEDS)
@pytest.mark.parametrize("kind", ["none", "extents transposed", "window origin off by one", "a row stride taken from another operand",
                                  "ragged tail dropped", "band tail dropped", "bip/bsq permutation wrong"])
def test_ortho_rows_see_the_slip(kind, seed):
    hits = []
    for k, r, c in admitted_rows("ortho", seed):
        out, dropped = _ortho_slip(kind, r, c)
        if not np.array_equal(out, c["ref"]) or (r["count"] and dropped != c["dropped"]):
            hits.append(k)
    print(f"ortho seed {seed}: '{kind}' changes rows {hits}")
    assert (hits == []) if kind == "none" else hits


def _restrided(back, rs, shape, sentinel):
    """The (h, w) plane that a reader with row stride `rs` sees at the base of `back` (past its end: `sentinel`)."""
    flat = back.reshape(-1)
    need = (shape[0] - 1) * rs + shape[1]
    if need > flat.size:
        flat = np.concatenate([flat, np.full(need - flat.size, sentinel, flat.dtype)])
    return np.lib.stride_tricks.as_strided(flat, shape, (rs * flat.itemsize, flat.itemsize), writeable=False)


def _surface_slip(kind, r, c):
    emit, s2, mask, origins = c["emit"], c["s2"], c["mask"], c["origins"]
    w, f, R = r["w"], r["f"], r["R"]
    if kind == "extents transposed" or kind == "f used where R belongs":
        # the region test alone, as the kernel evaluates it before it reads anything
        if kind == "extents transposed":
            inside = [cc.region_inside(i, j, w, f, R, r["we"], r["he"], c["ws"], c["hs"]) for i, j in origins]
        else:
            inside = [cc.region_inside(i, j, w, f, f, r["he"], r["we"], c["hs"], c["ws"]) for i, j in origins]
        return None if inside == r["inside"] else "differs"
    if kind == "a row stride taken from another operand":
        if mask is None:
            return None
        mask = _restrided(c["mask_back"], c["emit_rs"], emit.shape, np.uint8(1))
    if kind == "window origin off by one":
        origins = origins + np.array([0, 1], np.int32)
    return cc.surface_ref(emit, mask, s2, c["nodata"], origins, w, f, R, c["min_valid"])[0]


@pytest.mark.parametrize("seed", sw.SEEDS)
@pytest.mark.parametrize("kind", ["none", "extents transposed", "f used where R belongs", "a row stride taken from another operand",
                                  "window origin off by one"])
def test_surface_rows_see_the_slip(kind, seed):
    hits = []
    for k, r, c in admitted_rows("coreg-surface", seed):
        got = _surface_slip(kind, r, c)
        if got is None:
            continue
        fin = np.isfinite(c["ref"])
        if isinstance(got, str) or not np.array_equal(np.isfinite(got), fin) or (np.abs(got[fin] - c["ref"][fin]) > c["bar"][fin]).any():
            hits.append(k)
    print(f"coreg-surface seed {seed}: '{kind}' changes rows {hits}")
    assert (hits == []) if kind == "none" else hits


@pytest.mark.parametrize("seed", sw.SEEDS)
@pytest.mark.parametrize("kind", ["none", "extents transposed", "a row stride taken from another operand", "ragged tail dropped"])
def test_warp_rows_see_the_slip(kind, seed):
    """The warp's answer read under a wrong output row stride, its ragged tile column left at fill, and the reference of the
    transposed scene transposed back (the model's axes exchanged with it would be the same warp: they are not)."""
    hits = []
    for k, r, c in admitted_rows("coreg-warp", seed):
        ref = c["ref"]
        got = ref
        if kind == "extents transposed":
            got = cc.warp_ref(np.ascontiguousarray(c["scene"].transpose(0, 2, 1)), c["model"], c["nodata"], c["fill"])[0].transpose(0, 2, 1)
        if kind == "a row stride taken from another operand":
            back = cc.pack_scene(ref, r["out_extra"], ref.dtype.type(3), r["out_gap"])
            flat = np.concatenate([back, np.full((back.shape[0], r["h"] * 8), 3, back.dtype)], axis=1)
            got = cc.unpack_scene(flat, r["h"], r["w"], r["extra"])[0]
        if kind == "ragged tail dropped":
            got = ref.copy()
            got[:, :, r["w"] - r["w"] % cc.TILE_W:] = cc.warp_ref(c["scene"][:, :1, :1], cc.make_model(1, 1, dy0=5.0), c["nodata"], c["fill"])[0][0, 0, 0]
        if got.tobytes() != ref.tobytes():
            hits.append(k)
    print(f"coreg-warp seed {seed}: '{kind}' changes rows {hits}")
    assert (hits == []) if kind == "none" else hits


@pytest.mark.parametrize("seed", sw.SEEDS)
def test_peak_and_model_rows_cover_their_classes(seed):
    """The peaks sweep meets every status, the border ring and exact ties; the model sweep both kinds, the fallback, a rejected
    record, the zero model and min_points on both sides of the OK count."""
    status, kinds = set(), set()
    for _, r, c in admitted_rows("coreg-peaks", seed):
        status |= set(c["ref"][:, 7].astype(int))
        kinds |= set(c["kinds"])
        assert r["he"] != r["we"]
    assert status == {cc.OK, cc.OUTSIDE, cc.NO_SCORE, cc.BORDER, cc.LOW_SCORE} and kinds == set(sw.PEAK_KINDS)
    used, sides, rejected = set(), set(), 0
    for _, r, c in admitted_rows("coreg-model", seed):
        n_ok = int((np.asarray(r["table"])[:, 7] == cc.OK).sum())
        used.add((r["kind"], int(c["model"][9])))
        sides.add(int(np.sign(r["min_points"] - n_ok)))
        rejected += int((c["table"][:, 7] == cc.OUTLIER).any())
    assert used >= {(0, 0), (1, 1), (1, 0), (1, -1)} or used >= {(0, 0), (1, 1), (0, -1)}, used
    assert sides == {-1, 0, 1} and rejected >= 3


# ---- colour ----------------------------------------------------------------------------------------------------------------------------
def _restride_rows(rows, own, other, npix):
    """The (npix, 3) rows a reader finds in the buffer of layout `own` when it walks it with the strides of layout `other`."""
    flat = ac.pack(rows, own)
    bs, ps, _ = ac.strides(other, npix)
    idx = np.minimum(np.arange(npix)[:, None] * ps + np.arange(3)[None, :] * bs, flat.size - 1)
    return flat[idx]


def _moments_slip(kind, r, c):
    """The 22 long-double moments of an image row under a wrong reading of it, or None where the slip does not apply."""
    if r["entry"] != "image":
        return None
    x, y, mask, npix = c["x"], c["y"], c["mask"], r["npix"]
    ok = ac.usable(x, y, mask)
    if kind == "a row stride taken from another operand":
        if r["x"][0] == r["y"][0]:
            return None
        y = _restride_rows(y, r["y"][0], r["x"][0], npix)
        ok = ac.usable(x, y, mask)
    xs, ys = ac.stretch(x, r["lohi_x"]), ac.stretch(y, r["lohi_y"])
    if kind == "a mask applied before instead of after the stretch":      # validity judged on the stretched values: the clip hides +-inf
        ok = ac.usable(xs, ys, mask)
    if kind == "ragged tail dropped":
        ok = ok & (np.arange(npix) < npix // ac.GROUP * ac.GROUP)
    return ac.moments_ld(xs[ok], ys[ok])[0]


@pytest.mark.parametrize("seed", sw.SEEDS)
@pytest.mark.parametrize("kind", ["none", "a row stride taken from another operand", "a mask applied before instead of after the stretch",
                                  "ragged tail dropped"])
def test_moment_rows_see_the_slip(kind, seed):
    hits = []
    for k, r, c in admitted_rows("color-moments", seed):
        got = _moments_slip(kind, r, c)
        if got is not None and (np.abs(got - c["ref"]).astype(np.float64) > ac.moments_bar(c["n"], c["mag"])).any():
            hits.append(k)
    print(f"color-moments seed {seed}: '{kind}' changes rows {hits}")
    assert (hits == []) if kind == "none" else hits


@pytest.mark.parametrize("seed", sw.SEEDS)
@pytest.mark.parametrize("kind", ["none", "a row stride taken from another operand", "a mask applied before instead of after the stretch",
                                  "ragged tail dropped"])
def test_apply_rows_see_the_slip(kind, seed):
    hits = []
    for k, r, c in admitted_rows("color-apply", seed):
        x, mask, npix = c["x"], c["mask"], r["npix"]
        got = c["ref"]
        if kind == "a row stride taken from another operand" and r["x"][0] != r["out"][0]:
            got = ac.apply_ref(_restride_rows(x, r["x"][0], r["out"][0], npix), r["At"], mask, r["lohi"], r["clip"])
        if kind == "a mask applied before instead of after the stretch" and mask is not None:     # a masked-out pixel passes through raw
            raw = np.clip(x, np.float32(0), np.float32(1)) if r["clip"] == 2 else x
            got = np.where((mask != 0)[:, None], got, raw)
        if kind == "ragged tail dropped":
            got = got.copy()
            got[npix // ac.GROUP * ac.GROUP:] = np.float32(-3.0)
        if got.tobytes() != c["ref"].tobytes():
            hits.append(k)
    print(f"color-apply seed {seed}: '{kind}' changes rows {hits}")
    assert (hits == []) if kind == "none" else hits


@pytest.mark.parametrize("seed", sw.SEEDS)
def test_colour_rows_cover_their_classes(seed):
    """Moments: both entry points, slots on both sides of 64 and at the cap, every mask kind, each stretch on and off, the flat
    channel.  Apply: the three clip modes, each table matrix and a drawn one.  Solve: every rank class, the identity on both
    grounds, slot counts of one, below and above 64."""
    M = [r for _, r, _ in admitted_rows("color-moments", seed)]
    assert {r["entry"] for r in M} == {"image", "f64"} and {r["mask"] for r in M} == {"none", "all", "clear", "part"}
    assert {ac.slots(r["npix"]) > 64 for r in M} == {False, True} and {ac.slots(r["npix"]) for r in M} >= {1, 2, 3}
    assert {r["lohi_x"] is None for r in M} == {False, True} == {r["lohi_y"] is None for r in M}
    A = [r for _, r, _ in admitted_rows("color-apply", seed)]
    assert {r["clip"] for r in A} == {0, 1, 2} and {r["lohi"] is None for r in A} == {False, True}
    assert {r["mask"] for r in A} == {"none", "all", "clear", "part"}
    S = [(r, c) for _, r, c in admitted_rows("color-solve", seed)]
    assert {r["rank"] for r, _ in S if not c_identity(r)} >= {1, 2, 3, 4} and {c["identity"] for _, c in S} == {False, True}
    assert {(r["nslots"] > 64) for r, _ in S} == {False, True}


def c_identity(r):
    return r["n"] < max(r["min_count"], 1)


# ---- scene -----------------------------------------------------------------------------------------------------------------------------
SCENE_SLIPS = ["none", "extents transposed", "window origin off by one", "ragged tail dropped"]


def _scene_slip(sweep, kind, r, c):
    """True when the row's reference changes under the slip."""
    if sweep == "scene-scan":
        mask = sc.black_mask_np(c["scene"], **sc.scan_settings(r))
        th, tw = r["th"], r["tw"]
        if kind == "extents transposed":
            th, tw = tw, th
        if kind == "window origin off by one":
            mask = np.roll(mask, 1, axis=1)
        if kind == "ragged tail dropped":                     # the lanes of a row's last, partial wave
            mask = mask.copy()
            mask[:, r["W"] - r["W"] % 64:] = False
        if th > r["H"] or tw > r["W"]:
            return True
        got = sc.window_counts(mask, th, tw)
        return got.shape != c["ref"].shape or not np.array_equal(got, c["ref"])
    if sweep == "scene-gather":
        dtype, encode, (bands, H, W), org, th, tw, _ = r
        if kind == "extents transposed":
            org = org[:, ::-1]
        if kind == "window origin off by one":
            org = np.minimum(org + np.array([0, 1], np.int32), np.array([H - th, W - tw], np.int32))
        want, inside = sc.gather_ref(c["scene"], org, th, tw, encode)
        if kind == "ragged tail dropped":
            want[..., tw - tw % 4:] = 0
        return not np.array_equal(inside, c["inside"]) or want.tobytes() != c["want"].tobytes()
    if sweep == "scene-mosaic":
        T, H, W, th, tw, P, _, _, fills, _ = r
        cubes, slot = c
        pre = np.zeros((T, H, W), np.float32)
        fill, rest = fills[0]
        want = sc.assemble(cubes, slot, pre, th, tw, fill, rest)
        if kind == "extents transposed":
            slot = slot.reshape(-1).reshape(slot.shape[::-1]).T
        if kind == "window origin off by one":
            slot = np.roll(slot, 1, axis=1)
        got = sc.assemble(cubes, slot, pre, th, tw, fill, False if kind == "ragged tail dropped" else rest)
        return got.tobytes() != want.tobytes()
    start, sy, sx = c["start"], r["sy"], r["sx"]
    if kind == "extents transposed":
        start = np.ascontiguousarray(start.reshape(-1).reshape(start.shape[::-1]).T)
    if kind == "window origin off by one":
        start = np.roll(start, 1, axis=1)
    if kind == "ragged tail dropped":                         # the windows of the last lattice column that still fits are left out
        start = start.copy()
        start[:, (r["W"] - r["tw"]) // sx] = -1
    got = sc.blend_ref64(c["cubes"], start, sy, sx, r["H"], r["W"])
    return not all(np.array_equal(got[k], c["ref"][k], equal_nan=k in ("mean", "absmean")) for k in ("cover", "n", "one", "mean"))


@pytest.mark.parametrize("seed", sw.SEEDS)
@pytest.mark.parametrize("kind", SCENE_SLIPS)
@pytest.mark.parametrize("sweep", ["scene-scan", "scene-gather", "scene-mosaic", "scene-blend"])
def test_scene_rows_see_the_slip(sweep, kind, seed):
    hits = [k for k, r, c in admitted_rows(sweep, seed) if _scene_slip(sweep, kind, r, c)]
    print(f"{sweep} seed {seed}: '{kind}' changes rows {hits}")
    assert (hits == []) if kind == "none" else hits


@pytest.mark.parametrize("seed", sw.SEEDS)
def test_scene_rows_cover_their_classes(seed):
    """Scan: nodata in use and not, the zero test on and off, pixels that count and pixels broken in one band.  Gather: the three
    encodings, origins on an edge and repeated.  Mosaic: an empty stack, both fill_rest settings, every kind of slot entry.  Blend:
    every lattice of sc.LATTICES' K classes, T of one plane and of more than 32."""
    S = [(r, c) for _, r, c in admitted_rows("scene-scan", seed)]
    assert {r["nodata"] is None for r, _ in S} == {False, True} and {r["zero_atol"] == 0 for r, _ in S} == {False, True}
    assert any(c["ref"].sum() > 0 for _, c in S) and {r["dtype"] for r, _ in S} == {sc.F32, sc.U16}
    G = [r for _, r, _ in admitted_rows("scene-gather", seed)]
    assert {None if r[1] is None else r[1][1] for r in G} == {None, 0, 1}
    assert any(len(r[3]) > len({tuple(o) for o in r[3]}) for r in G) and any((r[3] == 0).any() for r in G)
    M = [(r, c) for _, r, c in admitted_rows("scene-mosaic", seed)]
    assert any(r[5] == 0 for r, _ in M) and {bool(f[1]) for r, _ in M for f in r[8]} == {False, True}
    assert any((c[1] == -2).any() for _, c in M) and any((c[1] >= max(r[5], 1)).any() for r, c in M)
    B = [r for _, r, _ in admitted_rows("scene-blend", seed)]
    assert {r["T"] for r in B} >= {1, 33} and {sc.blend_kmax((r["th"] // r["sy"]) * (r["tw"] // r["sx"])) for r in B} == {1, 2, 4, 8, 16}
