"""tests/capture_cases.py holds what it says (CPU): every entry point of the C ABI is placed, every exclusion carries its reason, the
three input sets of every row differ and flip, in the reference, the device-side branch they are meant to flip, and the work
buffers are sized by the library's own helpers (the library loads without a GPU)."""
import numpy as np
import pytest

import capture_cases as cc
import ot_cases as otc
from s2_emit import _native as nat

ROWS = list(cc.ROWS)


def test_every_entry_point_is_placed_exactly_once():
    """A new entry point must be given a row, a reason or a place among the host-only calls before the suite passes."""
    lists = {"covers": cc.covered(), "NOT_LAUNCH_PATH": cc.NOT_LAUNCH_PATH, "EXCLUDED": list(cc.EXCLUDED)}
    for what, names in lists.items():
        assert len(names) == len(set(names)), (what, sorted(n for n in names if list(names).count(n) > 1))
    placed = [n for names in lists.values() for n in names]
    twice = sorted({n for n in placed if placed.count(n) > 1})
    assert not twice, twice
    assert sorted(placed) == sorted(nat.SIGNATURES), (sorted(set(nat.SIGNATURES) - set(placed)), sorted(set(placed) - set(nat.SIGNATURES)))


def test_exclusions_carry_reasons():
    assert all(isinstance(r, str) and len(r.strip()) > 40 for r in list(cc.EXCLUDED.values()) + list(cc.EXCLUDED_FORMS.values()))
    assert set(vars(cc)) & {"PENDING", "TODO"} == set()                         # three lists, no waiting list
    assert all(form.split()[0] in cc.covered() for form in cc.EXCLUDED_FORMS)  # a form is excluded of an entry that has a row
    lib = nat.load()
    for name in cc.covered() + list(cc.EXCLUDED):                # what the table names exists in the library
        assert hasattr(lib, name), name
    for name in cc.NOT_LAUNCH_PATH:                                           # none of them takes a stream: nothing to capture
        assert name in nat.SIGNATURES
    for name in cc.covered():
        assert nat.SIGNATURES[name][1][-1] is nat._vp, name                   # the stream is the last argument of a launch-path entry


@pytest.mark.parametrize("name", ROWS)
def test_rows_are_well_formed(name):
    row = cc.ROWS[name]
    assert row.covers and set(row.shapes) == {"small", "big"} and row.shapes["small"] != row.shapes["big"]
    assert type(row.shapes["small"]) is type(row.shapes["big"])
    assert (row.__doc__ or "").count("tests/test_gpu_"), "the row cites the module its bar comes from"
    for shape in row.shapes.values():
        sets = [row.inputs(shape, k) for k in cc.SETS]
        assert all(set(s) == set(sets[0]) for s in sets)
        for key in sets[0]:
            assert all(s[key].shape == sets[0][key].shape and s[key].dtype == sets[0][key].dtype for s in sets), key
        differ = [any(not np.array_equal(a[key], b[key], equal_nan=a[key].dtype.kind == "f") for key in a)
                  for a, b in ((sets[0], sets[1]), (sets[1], sets[2]), (sets[0], sets[2]))]
        assert all(differ), (name, shape, differ)
        assert row.inputs(shape, 0) is sets[0] and row.reference(shape, 0) is row.reference(shape, 0)      # computed once, shared
        assert not any(a.flags.writeable for a in sets[0].values())


@pytest.mark.parametrize("name", [n for n in ROWS if n.startswith("ortho")])
def test_ortho_sets_drop_some_none_some(name):
    row = cc.ROWS[name]
    for shape in row.shapes.values():
        d = [row.reference(shape, k)["dropped"] for k in cc.SETS]
        assert d[0] > 0 and d[1] == 0 and d[2] > 0 and d[0] != d[2], d
        outs = [row.reference(shape, k)["out"] for k in cc.SETS]
        assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])
    s, b = row.shapes["small"], row.shapes["big"]
    assert -(-s.gw // 64) * s.gh != -(-b.gw // 64) * b.gh                    # a workgroup owns 64 pixels of an output row
    assert s.gw % 64 and b.gw % 64
    assert {(r.shapes["small"].layout, r.shapes["small"].q, r.shapes["small"].bm) for r in cc.ROWS.values() if r.name.startswith("ortho")} \
        == {(0, True, False), (1, False, True)}                               # both layouts, both masks


def test_scan_sets_border_clean_all_black():
    row = cc.ROWS["scene-black-counts"]
    for shape in row.shapes.values():
        c = [row.reference(shape, k)["counts"] for k in cc.SETS]
        full = shape.th * shape.tw
        assert c[0].size == (shape.H // shape.th) * (shape.W // shape.tw)
        grid = c[0].reshape(shape.H // shape.th, shape.W // shape.tw)
        edge = np.concatenate([grid[0], grid[-1], grid[:, 0]])           # the strip right of the last window belongs to none
        assert (edge > 0).all() and (c[0] < full).all() and (c[1] == 0).all() and (c[2] == full).all(), c
    assert row.reference(row.shapes["small"], 0)["counts"].size != row.reference(row.shapes["big"], 0)["counts"].size


@pytest.mark.parametrize("name", ["chol", "chol-batched"])
def test_chol_flags_set_1_only_in_a_later_block(name):
    row = cc.ROWS[name]
    for shape in row.shapes.values():
        infos = [[r["info"] for r in row.reference(shape, k)] for k in cc.SETS]
        kp = cc.chol_bad_pivot(shape)
        assert infos[0] == [0] * shape.P and infos[2] == [0] * shape.P
        assert infos[1] == [0] * (shape.P - 1) + [kp + 1] and 64 <= kp < shape.n            # from the third 32-block on
        for k in cc.SETS:
            for (a, _, info), r in zip(row.systems(shape, k), row.reference(shape, k)):
                lead = [np.linalg.slogdet(a[:j, :j])[0] > 0 for j in (kp, kp + 1)]
                assert lead == [True, info == 0], (k, lead)                                   # the FIRST non-positive pivot is kp
                if info == 0:
                    assert np.linalg.cond(a) < 100                                           # the class the numpy bars are for
        assert shape.n % 32 == 0 and shape.n <= 288                                          # chol_factor_res_kernel: nothing above the diagonal is written
    assert nat.load().hsr_chol_work_bytes(row.shapes["small"].n) < nat.load().hsr_chol_work_bytes(row.shapes["big"].n)


@pytest.mark.parametrize("name", [n for n in ROWS if n.startswith("percentile")])
def test_percentile_sets_nan_empty_ties(name):
    row = cc.ROWS[name]
    for shape in row.shapes.values():
        i, ref = [row.inputs(shape, k) for k in cc.SETS], [row.reference(shape, k)["lohi"] for k in cc.SETS]
        assert np.isnan(i[0]["x"][0]).any() and not np.isnan(i[0]["x"][0][i[0]["mask"] != 0]).any()          # band 0: NaN, all masked out
        assert np.isfinite(ref[0][0]).all() and np.isnan(ref[0][1]).all() and np.isfinite(ref[0][2:]).all()  # band 1: a NaN sample counts
        assert not i[1]["mask"].any() and np.isnan(ref[1]).all()
        assert np.isfinite(ref[2]).all()
        vals = np.sort(i[2]["x"][0][i[2]["mask"] != 0])
        lo, hi = vals[(len(vals) - 1) // 2], vals[(len(vals) - 1) // 2 + 1]
        assert len(vals) % 2 == 0 and (lo, hi) == (0.25, 0.75) and ref[2][0][0] == 0.5                         # between the two ranks
        assert lo.view(np.uint32) >> 21 != hi.view(np.uint32) >> 21                                          # in different pass-1 bins
        assert len(np.unique(i[2]["x"][1])) < 40                                                             # ties
    s, b = row.shapes["small"], row.shapes["big"]
    assert (s.npix <= cc.TINY_MAX) == (name != "percentile-passes") and b.npix > cc.TINY_MAX and s.nb < b.nb
    lib = nat.load()
    assert lib.hsr_percentile_work_bytes(s.nb) < lib.hsr_percentile_work_bytes(b.nb)


@pytest.mark.parametrize("name", ["k2-fit-apply", "k2-f64-fit"])
def test_fit_sets_fall_back_in_set_1_only(name):
    row = cc.ROWS[name]
    ident = np.zeros(row.shapes["small"].deg + 1)
    ident[-2] = 1.0
    for shape in row.shapes.values():
        refs = [row.reference(shape, k) for k in cc.SETS]
        assert [list(r["fitted"]) for r in refs] == [[True] * 3, [True, False, True], [True] * 3]
        assert refs[1]["moments"][1][0] == cc.FIT_MIN_COUNT - 1 and np.array_equal(refs[1]["coeffs"][1], ident)
        for k in cc.SETS:
            assert all(not np.array_equal(refs[k]["coeffs"][b], ident) for b in range(3) if refs[k]["fitted"][b])
            assert (refs[k]["moments"][refs[k]["fitted"], 0] >= 200).all()                  # the sample sizes np.polyfit's bar is pinned at
        if not row.f64:
            m = [row.inputs(shape, k)["mask"] for k in cc.SETS]
            assert 0 < m[0].sum() < m[0].size and 0 < m[1].sum() < m[1].size and m[2].all()
    s, b = row.shapes["small"], row.shapes["big"]
    assert cc.fit_slots(s.npix) == 8 and cc.fit_slots(b.npix) == 40 and s.npix % 64
    assert nat.load().hsr_partials_bytes(b.nb, b.deg) >= cc.fit_slots(b.npix) * b.nb * (3 * b.deg + 2) * 8


@pytest.mark.parametrize("name", ["ot-staged", "ot-one-call"])
def test_ot_sets_run_out_break_down_and_converge(name):
    row = cc.ROWS[name]
    for shape in row.shapes.values():
        refs = [row.reference(shape, k) for k in cc.SETS]
        brk = otc.ROWS[cc.OT_BREAK[shape]]
        assert (brk["n"], brk["m"], brk["reg"], brk["itmax"], brk["thr"]) == (shape.n, shape.m, cc.OT_REG, cc.OT_ITMAX, cc.OT_THR)
        assert (refs[0]["break_iter"], refs[0]["conv_iter"], refs[0]["checks"]) == (None, None, 4)           # checks at 0, 10, 20, 30
        assert (refs[1]["break_iter"], refs[1]["conv_iter"]) == (brk["expect"]["break_iter"], None) and refs[1]["break_iter"] >= 1
        assert (refs[2]["break_iter"], refs[2]["conv_iter"], refs[2]["checks"]) == (None, 0, 1)
        # decided far from the threshold and from DBL_MAX: a last-bit difference of the device cannot move a stop
        assert all(err > 1e3 * cc.OT_THR for _, err, _ in refs[0]["errs"]), refs[0]["errs"]
        assert refs[2]["errs"][0][1] < 1e-3 * cc.OT_THR, refs[2]["errs"]
        assert max(refs[0]["q"]) < -1 and max(refs[2]["q"]) < -1
        assert all(abs(q) > otc.MARGIN for q in refs[1]["q"])
    s, b = row.shapes["small"], row.shapes["big"]
    assert otc.paths(*s)["nchunks"] != otc.paths(*b)["nchunks"] and otc.paths(*s)["col_double2"] != otc.paths(*b)["col_double2"]
    lib = nat.load()
    assert 0 < lib.hsr_ot_work_bytes(*s) < lib.hsr_ot_work_bytes(*b)
    assert cc.ot_regions(*s) != cc.ot_regions(*b)                             # the big call's scratch lies elsewhere in the workspace


@pytest.mark.parametrize("name", [n for n in ROWS if isinstance(cc.ROWS[n], cc.K1Row)])
def test_k1_sets_fall_back_in_set_1_only(name):
    row, nb = cc.ROWS[name], cc.k1_table()[3].nb
    assert nb == 12 and cc.k1_table()[3].B == 285
    lib = nat.load()
    for shape in row.shapes.values():
        npix = shape.H * shape.W
        refs, ins = [row.reference(shape, k) for k in cc.SETS], [row.inputs(shape, k) for k in cc.SETS]
        nanpix = [np.isnan(r["planes"]).all(axis=0) for r in refs]
        assert [int(n.sum()) for n in nanpix] == [0, 1, 0]                               # the non-finite / nodata sample of set 1
        assert ins[0]["cube"].dtype == (np.uint16 if row.u16 else np.float32)
        if row.mode == "k1":
            continue
        assert [list(r["fitted"]) for r in refs] == [[True] * nb, [True] + [False] + [True] * (nb - 2), [True] * nb]
        assert refs[1]["counts"][1] == cc.K1_MIN_COUNT - 1
        assert ins[0]["mask"].all() and ins[2]["mask"].all() and 0 < ins[1]["mask"].sum() < npix
    s, b = (row.shapes[k].H * row.shapes[k].W for k in ("small", "big"))
    assert lib.hsr_partial_slots(s, None) != lib.hsr_partial_slots(b, None)
    if row.mode == "fit":                                                                # does the fit ride where 16 workgroups >= 12 bands
        assert (lib.hsr_partial_slots(s, None) >= nb) == (name.startswith("fused-fit-16x64"))


def test_ridge_set_1_has_a_zero_pivot():
    row, d, lib = cc.ROWS["k4-fit"], cc.ridge_dims(), nat.load()
    assert (d.nf, d.na, d.ldq, d.npad, d.kpad) == (34, 48, 64, 64, 34)
    for shape in row.shapes.values():
        assert [row.reference(shape, k)["info"] for k in cc.SETS] == [0, 1, 0]
        X = [row.inputs(shape, k)["X"] for k in cc.SETS]
        assert (X[1] == X[1][0]).all() and all((x.std(axis=0) > 100).all() for x in (X[0], X[2]))
        assert (row.reference(shape, 1)["scale"] == 1).all()                             # zero variance -> 1
    s, b = row.shapes["small"].n, row.shapes["big"].n
    assert -(-s // 1024) == 1 and -(-b // 1024) == 3
    assert lib.hsr_gram_work_bytes(d.na, d.ldq, s) < lib.hsr_gram_work_bytes(d.na, d.ldq, b)


def test_score_sets_empty_a_group_in_sets_1_and_2():
    import pair_cases as pc
    row, lib = cc.ROWS["pairs-holdout-score"], nat.load()
    for shape in row.shapes.values():
        n = [[r["n"] for r in row.reference(shape, k)["score"]] for k in cc.SETS]        # [set][pair] -> (2, T): training, hold-out
        assert all((n[0][p].max(axis=1) > 0).all() for p in range(cc.SCORE_P))
        assert not n[1][1][0].any() and n[1][1][1].any() and n[1][0].max(axis=1).all()   # set 1: pair 1 has no training pixel
        assert not n[2][0][1].any() and n[2][0][0].any() and n[2][1].max(axis=1).all()   # set 2: pair 0 has no hold-out pixel
        assert np.isnan(row.reference(shape, 1)["score"][1]["rmse"][0]).all()
        groups = [row.reference(shape, k)["group"] for k in cc.SETS]
        assert all(set(np.unique(g)) <= {0, 1, 2} for g in groups) and not np.array_equal(groups[0], groups[2])
    s, b = row.shapes["small"], row.shapes["big"]
    assert pc.score_chunks(s.npix) == 2 and pc.score_chunks(b.npix) == 6
    assert lib.hsr_pair_score_work_bytes(s.npix, s.T) == pc.score_chunks(s.npix) * (s.T * 8 + 4) * 8 < lib.hsr_pair_score_work_bytes(b.npix, b.T)


def test_aux_sets_carry_the_non_finite_samples_where_the_row_says():
    row = cc.ROWS["aux-upsample-hist"]
    for shape in row.shapes.values():
        m = [row.reference(shape, k)["mask"] for k in cc.SETS]
        assert 0 < m[0].sum() < m[0].size and not m[1].any() and m[2].all()              # some pixels valid, none, all
        lohi = [row.reference(shape, k)["lohi"] for k in cc.SETS]
        assert np.isfinite(lohi[0]).all() and np.isnan(lohi[1]).all() and np.isfinite(lohi[2]).all()
        assert shape.nb <= 4
    row = cc.ROWS["aux-valid-mask"]
    for shape in row.shapes.values():
        m = [row.reference(shape, k)["mask"] for k in cc.SETS]
        assert all(0 < x.sum() < x.size for x in m) and row.inputs(shape, 2)["mask_in"].all() and not row.inputs(shape, 0)["mask_in"].all()
    row = cc.ROWS["aux-codec"]
    for shape in row.shapes.values():
        u = [row.reference(shape, k)["u16"] for k in cc.SETS]
        assert not (u[0] == 65535).any() and (u[1] == 65535).sum() >= 4 and not (u[2] == 65535).any()
        assert np.isnan(row.reference(shape, 1)["dec"]).sum() == (u[1] == 65535).sum()


@pytest.mark.parametrize("name", [n for n in ROWS if n.startswith("scene-gather")])
def test_tile_sets_drop_a_window_in_set_1_only(name):
    row = cc.ROWS[name]
    for shape in row.shapes.values():
        inside = [row.reference(shape, k)["inside"] for k in cc.SETS]
        assert inside[0].all() and (~inside[1]).sum() == 1 and inside[2].all()
        org = [row.inputs(shape, k)["origins"] for k in cc.SETS]
        assert not np.array_equal(org[0], org[2])                                       # the order of the stack changes with the set
        if row.mode != "encode":
            t = [row.inputs(shape, k)["table"] for k in cc.SETS]
            P = t[0].size
            assert sorted(t[2].reshape(-1)) == list(range(P)) and (t[1] == -1).any() and (t[1] >= P).any() and (t[0] == -1).sum() == 1
        if row.mode == "blend":
            cover = [row.reference(shape, k)["blend"]["cover"] for k in cc.SETS]
            assert cover[2].max() == (shape.th // shape.sy) * (shape.tw // shape.sx) == 4 and cover[1].min() == 0


def test_batch_rotates_the_fallback_tile():
    row, lib = cc.ROWS["batch"], nat.load()
    for shape in row.shapes.values():
        assert len(set(shape.npix)) == 3                                                # ragged
        for k in cc.SETS:
            fitted = [r["fitted"][1] for r in row.reference(shape, k)]
            assert fitted.count(False) == 1 and fitted.index(False) == (1 - k) % 3      # the tile that holds set 1
    slots = [[lib.hsr_partial_slots(n, None) for n in row.shapes[key].npix] for key in ("small", "big")]
    assert slots == [[8, 5, 16], [40, 8, 18]]


def test_report_pool_predict_and_pair_fit_sets_flip_what_they_name():
    import pair_cases as pc
    lib = nat.load()
    row = cc.ROWS["pairs-report"]
    for shape in row.shapes.values():
        nan = [[bool(np.isnan(r2).all()) for r2, _ in row.reference(shape, k)] for k in cc.SETS]
        assert nan == [[False] * 3, [False, True, True], [False] * 3]                   # statuses 0 0 0 / 0 2 1 / 0 0 0
        assert (np.abs(row.inputs(shape, 2)["b64"]) == 80).any() and not (np.abs(row.inputs(shape, 0)["b64"]) == 80).any()
    s, b = row.shapes["small"], row.shapes["big"]
    assert pc.report_chunks(s.npix) == 1 < pc.report_chunks(b.npix)
    assert lib.hsr_pair_report_work_bytes(s.npix, s.T) == pc.report_chunks(s.npix) * s.T * 4 * 8 < lib.hsr_pair_report_work_bytes(b.npix, b.T)
    row = cc.ROWS["pairs-pool"]
    for shape in row.shapes.values():
        refs = [row.reference(shape, k) for k in cc.SETS]
        assert refs[0]["untouched"] == [] and len(refs[1]["untouched"]) == 4 and refs[2]["untouched"] == []
        assert refs[0]["members"][:-1] == refs[2]["members"][1:] and refs[0]["members"] != refs[1]["members"]   # every group under the next id
        assert not np.array_equal(refs[0]["gram"], refs[1]["gram"]) and np.array_equal(refs[0]["gram"][:-1], refs[2]["gram"][1:])
    assert pc.pool_gram_blocks(row.shapes["small"].n_elems) < pc.pool_gram_blocks(row.shapes["big"].n_elems)
    for name in ("k4-predict-generic", "k4-predict-orbit"):
        row = cc.ROWS[name]
        s = row.shapes["small"]
        assert (lib.hsr_polyfeat_predict_kernel(s.n_in, s.degree, s.T, 1) >= 4) == (name == "k4-predict-generic")
        for shape in row.shapes.values():
            nan = [int(np.isnan(row.reference(shape, k)["refl"]).all(axis=0).sum()) for k in cc.SETS]
            assert nan[0] == 0 and nan[1] >= 5 and nan[2] == 0, nan
    row = cc.ROWS["pairs-fit-predict"]
    for shape in row.shapes.values():
        n = [[st[0] for st in row.reference(shape, k)["stats"]] for k in cc.SETS]
        npix = shape.H * shape.W
        assert 34 < n[0][0] < npix and n[1][1] == 0 and n[1][0] > 34 and n[2] == [npix, npix], n
    s, b = (row.shapes[k].H * row.shapes[k].W for k in ("small", "big"))
    d = cc.ridge_dims()
    assert lib.hsr_gram_work_bytes(d.na, d.ldq, s) < lib.hsr_gram_work_bytes(d.na, d.ldq, b)
