"""What the tables of tests/pair_cases.py claim, checked without a GPU: every edge value the rows are there for is present, the
mirrors of the two `vec` predicates name both instances of both templated kernels and flip on every term alone, the chunk plans
make the trips the rows are named for, and the references agree with each other on the dyadic data."""
import numpy as np

import pair_cases as pc


# ---- the mirrors -----------------------------------------------------------------------------------------------------------------
def test_tables_name_all_twelve_instances_and_both_arms_of_both_templates():
    assert len(pc.NAMES) == pc.INSTANCE_COUNT == len(set(pc.NAMES))
    names = pc.all_expected_names()
    assert names == set(pc.NAMES)
    for arm in ("<false>", "<true>"):
        assert "pair_score_partial_kernel" + arm in names and "pool_gram_kernel" + arm in names
    for seq in pc.DRIVER_RECORDS.values():
        assert set(seq) <= set(pc.NAMES)
    assert not any(n.startswith("pool_") for k, s in pc.DRIVER_RECORDS.items() if k != "pool" for n in s)
    assert [k for k, s in pc.DRIVER_RECORDS.items() if "pair_holdout_kernel" in s] == ["train_mask+validate"]


def test_score_predicate_rows_flip_one_term_each():
    base = pc.SCORE_BASE.layout()
    assert pc.SCORE_BASE.vec and pc.SCORE_BASE.npix % 4 == 0 and pc.score_chunks(pc.SCORE_BASE.npix) == 2
    flipped = set()
    for row in pc.SCORE_FLIP_ROWS:
        lay = row.layout()
        diff = [k for k in lay if lay[k] != base[k]]
        assert len(diff) == 1 and not row.vec and row.expect[0] == "pair_score_partial_kernel<false>", row.name
        assert (row.T, row.npix, row.groups) == (pc.SCORE_BASE.T, pc.SCORE_BASE.npix, pc.SCORE_BASE.groups)
        flipped.add(diff[0])
        ok = dict(lay)
        ok[diff[0]] = base[diff[0]]
        assert pc.score_vec(row.npix, **ok)
    assert flipped == set(base) and len(flipped) == 8
    odd = [r for r in pc.SCORE_ROWS if r.flip == "npix"]
    assert len(odd) == 1 and odd[0].npix % 4 != 0 and not odd[0].vec and pc.score_vec(odd[0].npix - 1, **odd[0].layout())
    assert all(r.layout()["pair_pred"] >= r.T * r.npix and r.layout()["pair_y"] >= r.T * r.npix and      # every stride covers its pair
               r.layout()["pair_group"] >= r.npix and r.layout()["pair_map"] >= r.npix for r in pc.SCORE_ROWS + pc.SCORE_FLIP_ROWS)


def test_gram_predicate_rows_flip_one_term_each():
    base = pc.GRAM_BASE.layout()
    assert pc.GRAM_BASE.expect == ["pool_gram_kernel<true>"] and pc.pool_gram_blocks(pc.GRAM_BASE.n_elems) == 2
    seen = set()
    for row in pc.GRAM_FLIP_ROWS:
        lay = row.layout()
        assert row.expect == ["pool_gram_kernel<false>"]
        terms = [row.n_elems % 2 != 0, lay["pair_g"] % 2 != 0, lay["group_out"] % 2 != 0, lay["off_g"] % 16 != 0, lay["off_out"] % 16 != 0]
        assert sum(terms) == 1, row.name
        seen.add(terms.index(True))
        assert lay["pair_g"] >= row.n_elems and lay["group_out"] >= row.n_elems
    assert seen == {0, 1, 2, 3, 4}
    assert {r.expect[0] for r in pc.GRAM_ROWS} == {"pool_gram_kernel<false>", "pool_gram_kernel<true>"}
    assert {pc.pool_gram_blocks(r.n_elems) for r in pc.GRAM_ROWS} >= {1, 2, 3}
    assert {r.n_elems for r in pc.GRAM_ROWS} >= {1, 511, 512, 513}


# ---- prep ------------------------------------------------------------------------------------------------------------------------
def test_prep_rows_hold_every_listed_edge():
    rows = pc.PREP_ROWS
    assert {(r.H, r.W) for r in rows} >= {(1, 1), (15, 17), (16, 16), (257, 1), (7, 37), (2, 3)}
    assert 15 * 17 == 255 and {r.f for r in rows} == {0, 1, 2, 6, 7, 64} and {r.nb for r in rows} >= {1, 10, 16}
    assert any(r.f == 64 and (r.H, r.W) == (2, 3) for r in rows)
    assert any(r.T == 1 for r in rows) and any(r.T == r.B and r.bands == tuple(range(r.B)) for r in rows)
    mixed = [r for r in rows if r.bands == pc.MIXED]
    assert mixed and all(0 in r.bands and r.B - 1 in r.bands and len(set(r.bands)) < len(r.bands) and
                         list(r.bands) != sorted(r.bands) for r in mixed)
    assert {(r.edt, r.sdt) for r in rows if r.f > 0} == {(a, b) for a in ("uint16", "float32") for b in ("uint16", "float32")}
    assert all(r.sdt == "float32" for r in rows if r.f == 0)
    assert any(r.end is None and r.snd is None for r in rows)
    assert any(r.snd == 0.0 and r.sdt == "uint16" for r in rows) and any(r.end == -9999.0 and r.edt == "float32" for r in rows)
    assert any(r.snd == 1000.0 for r in rows) and any(r.end == 1000.0 for r in rows)
    assert any(r.pad % 2 == 1 and r.pad > 0 and r.edt == "uint16" for r in rows) and any(r.pad % 2 == 1 and r.edt == "float32" for r in rows)
    assert all(max(r.bands) < r.B and r.T <= r.B and r.nb <= pc.PAIR_MAX_IN for r in rows)
    assert len({r.name for r in rows}) == len(rows)
    assert [c[0] for c in pc.PREP_REFUSED] == ["T > emit_bands", "nb = 17", "factor = 65", "uint16 coarse image",
                                               "overlapping emit stride", "overlapping s2 stride", "P = 0"]
    b = pc.PREP_REFUSED_BASE
    over = dict(pc.PREP_REFUSED)
    assert over["T > emit_bands"]["T"] == b.B + 1 and over["overlapping emit stride"]["pair_emit"] == b.B * b.npix - 1
    assert over["overlapping s2 stride"]["pair_s2"] == b.nb * b.npix * b.f ** 2 - 1


def test_closeness_rule_and_its_edges():
    up_in, up_out, lo_in, lo_out = pc.closeness_edge(1000.0)
    assert up_in > 1000 > lo_in and up_out == np.nextafter(up_in, np.float32(np.inf)) and lo_out == np.nextafter(lo_in, np.float32(-np.inf))
    assert pc.close32([up_in, lo_in, 1000.0], 1000.0).all() and not pc.close32([up_out, lo_out, np.nan, np.inf, -np.inf], 1000.0).any()
    tol = np.float32(1e-8) + np.float32(1e-5) * np.float32(1000.0)
    assert np.float32(up_in - np.float32(1000)) <= tol < np.float32(up_out - np.float32(1000))
    assert pc.close32(np.float32(-9999.0), -9999.0) and pc.close32(np.float32(0), 0.0) and not pc.close32(np.float32(1e-7), 0.0)
    assert not pc.close32(np.array([1, 65535], np.uint16).astype(np.float32), 0.0).any()


def test_prep_reference_on_the_planted_samples():
    seen = dict(nan_x=0, inf_coarse=0, nan_y=0, edge_in=0, edge_out=0, mean=0, u16_emit=0, u16_s2=0)
    for row in pc.PREP_ROWS:
        emit, s2 = pc.prep_inputs(row)
        assert emit.shape == (pc.P, row.B, row.H, row.W) and s2.shape == (pc.P,) + row.s2_shape
        assert emit.dtype == pc.NP_DT[row.edt] and s2.dtype == pc.NP_DT[row.sdt]
        x0, y0, m0 = pc.prep_reference(row, emit[0], s2[0])
        assert m0.all() and np.isfinite(x0).all() and np.isfinite(y0).all(), row.name      # pair 0 is clean
        for p in (1, 2):
            x, y, mask = pc.prep_reference(row, emit[p], s2[p])
            assert x.dtype == np.float32 and y.dtype == np.float32 and mask.dtype == np.uint8 and not mask.all(), row.name
            assert mask.any() or row.npix == 1
            seen["nan_x"] += int(np.isnan(x).sum())
            seen["nan_y"] += int(np.isnan(y).sum())
            if row.f == 0:
                seen["inf_coarse"] += int(np.isinf(x).sum())
                assert np.array_equal(x.view(np.uint32), s2[p].reshape(row.nb, -1).view(np.uint32))
            else:
                assert not np.isinf(x).any()
            if row.edt == "uint16":
                sel = emit[p][list(row.bands)].reshape(row.T, -1)
                assert np.array_equal(np.isnan(y), sel == 65535)
                seen["u16_emit"] += int((sel == 65535).sum())
                assert np.array_equal(y[sel != 65535], sel[sel != 65535].astype(np.float32) * np.float32(1e-4))
            if row.sdt == "uint16":                          # 65535 is an ordinary S2 value
                blocks = (s2[p].reshape(row.nb, row.H, row.f, row.W, row.f) == 65535).any(axis=(2, 4)).reshape(row.nb, -1)
                if row.snd is not None:                      # unless the block also holds a nodata sample (the 1 x 1 tile)
                    blocks &= ~pc.close32(s2[p].astype(np.float32), row.snd).reshape(row.nb, row.H, row.f, row.W, row.f).any(
                        axis=(2, 4)).reshape(row.nb, -1)
                seen["u16_s2"] += int(blocks.sum())
                assert (blocks.any() or row.npix == 1) and np.isfinite(x[blocks]).all() and (x[blocks] >= 65535.0 / row.f ** 2).all()
            if "edge" in row.plant:                          # looked up in the inputs: an inside value makes x NaN for f > 0
                up_in, up_out, lo_in, lo_out = pc.closeness_edge(1000.0)
                for arr in (s2[p].reshape(row.nb, -1), emit[p][list(row.bands)].reshape(row.T, -1)):
                    for v, inside in ((up_in, True), (up_out, False), (lo_in, True), (lo_out, False)):
                        at = np.argwhere(arr == v)
                        assert len(at), (row.name, v)
                        seen["edge_in" if inside else "edge_out"] += len(at)
                        if inside:
                            assert not mask[at[:, 1]].any()
            if "mean" in row.plant:
                at = np.argwhere(x == np.float32(row.snd))
                assert len(at) == 1 and mask[at[0, 1]] == 0
                c, q = at[0]
                blk = s2[p][c].reshape(row.H, 2, row.W, 2)[q // row.W, :, q % row.W, :]
                assert sorted(blk.reshape(-1).tolist()) == [999.0, 999.0, 1001.0, 1001.0] and not pc.close32(blk, row.snd).any()
                seen["mean"] += 1
    assert all(v > 0 for v in seen.values()), seen


def test_prep_outside_edge_value_alone_keeps_its_pixel():
    """On the f = 1 edge row the first value outside the band leaves its pixel valid (no other plant shares it)."""
    row = next(r for r in pc.PREP_ROWS if "edge" in r.plant and r.f == 1)
    emit, s2 = pc.prep_inputs(row)
    up_in, up_out, lo_in, lo_out = pc.closeness_edge(1000.0)
    for p in (1, 2):
        x, y, mask = pc.prep_reference(row, emit[p], s2[p])
        for arr in (x, y):
            for v in (up_out, lo_out):
                at = np.argwhere(arr == v)
                assert len(at) and mask[at[:, 1]].all()


# ---- stats -----------------------------------------------------------------------------------------------------------------------
def test_stats_rows_and_the_bar_that_separates_one_pass_from_two():
    assert {r.npix for r in pc.STATS_ROWS if r.kind == "dyadic"} == set(pc.STATS_NPIX) == {1, 63, 64, 1023, 1024, 1025, 4097}
    assert {r.nb for r in pc.STATS_ROWS} == {1, 16} and {r.kind for r in pc.STATS_ROWS} == {"dyadic", "random"}
    worst_two, best_one = 0.0, np.inf
    for row in pc.STATS_ROWS:
        x, mask = pc.stats_inputs(row)
        assert not mask[0].any() and (mask[1] != 0).sum() == 1 and mask[2, -1] != 0
        if row.npix >= 63:
            assert {1, 2, 255} <= set(mask[2].tolist()) and 0.55 < (mask[2] != 0).mean() < 0.85
        for p in range(pc.P):
            assert np.isnan(x[p][:, mask[p] == 0]).any() or (mask[p] != 0).all()
            assert np.isfinite(x[p][:, mask[p] != 0]).all()
            n, mean, m2, scale = pc.stats_reference(x[p], mask[p])
            assert n == (mask[p] != 0).sum()
            if n == 0:
                assert (mean == 0).all() and (scale == 1).all()
                continue
            if n == 1:
                assert (m2 == 0).all() and (scale == 1).all()
            if row.kind == "dyadic":
                sel = x[p][:, mask[p] != 0]
                assert (sel >= 4096).all() and (sel * 64 == np.rint(sel * 64)).all()
                exact = pc.dyadic_mean(x[p], mask[p])
                np.testing.assert_allclose(exact, mean, rtol=2e-16)
                if row.nb > 1:
                    assert m2[pc.STATS_CONST_BAND] == 0 and scale[pc.STATS_CONST_BAND] == 1
                if n >= 1000:
                    live = m2 != 0
                    s64 = sel.astype(np.float64)
                    two = ((s64 - exact[:, None]) ** 2).sum(axis=1)
                    worst_two = max(worst_two, float(np.abs(two[live] / m2[live] - 1).max()))
                    best_one = min(best_one, float(np.abs(pc.one_pass_m2(x[p], mask[p])[live] / m2[live] - 1).max()))
    # a float64 two-pass M2 (here with NumPy's plain running sum over a strided axis: the worst order) and a one-pass one: the
    # bar of the GPU test, rtol 1e-12, lies an order of magnitude and more from either
    assert worst_two <= 1e-13 and best_one >= 1e-8, (worst_two, best_one)


# ---- report ----------------------------------------------------------------------------------------------------------------------
def test_report_rows_hold_every_listed_value_and_the_references_agree():
    rows = pc.REPORT_ROWS
    assert {r.na for r in rows} == set(pc.REPORT_NA) and {r.T for r in rows} == set(pc.REPORT_T)
    assert {r.npix for r in rows} == set(pc.REPORT_NPIX)
    assert {r.na - r.nf for r in rows} == {1, 13} and all(r.na % 16 == 0 for r in rows)
    assert {pc.report_panels(r.na) for r in rows} == {1, 2, 3} and any(r.na == pc.REP_KC for r in rows)
    assert {pc.report_chunks(r.npix) for r in rows} >= {1, 2, 5}
    assert any(r.padded for r in rows) and any(not r.padded for r in rows)
    for f in ("clip", "status", "empty"):
        assert any(f in r.flags for r in rows)
    for r in rows:
        s, d = r.strides(), pc.report_inputs(r)
        assert s["ldq"] % 2 == 0 and s["pair_q"] % 2 == 0 and s["ldq"] > r.na and s["pair_q"] >= r.npix * s["ldq"]
        assert s["pair_bp"] >= r.rows_bp * s["ldbp"] and s["ldbp"] >= r.T and s["pair_work"] >= r.work
        if r.padded:
            assert s["pair_q"] > r.npix * s["ldq"] and s["ldbp"] > r.T and s["pair_y"] > r.T * r.npix and s["pair_m"] > r.npix
        assert np.isnan(d["Q"][:, :, r.na:]).all() and np.isnan(d["Bp"][:, r.nf:]).all() and np.isfinite(d["Q"][:, :, :r.na]).all()
        assert (d["Q"][:, :, r.nf + 1:r.na] == 0).all()
        off = d["mask"] == 0
        assert np.isnan(d["y"][np.broadcast_to(off[:, None], d["y"].shape)]).all() and (d["Q"][off][:, :r.na] == 0).all()
        assert off[:2].any() or r.npix == 1
        for p in range(pc.P):
            r2, rmse = pc.report_expected(r, d, p)
            if d["status"][p] != 0:
                assert np.isnan(r2).all() and np.isnan(rmse).all()
                continue
            r2d, rmsed, z = pc.report_direct(r, d, p)
            assert (z * 32 == np.rint(z * 32)).all()                       # exact logits: multiples of 1 / 32
            np.testing.assert_array_equal(r2, r2d)
            np.testing.assert_array_equal(rmse, rmsed)
            if "clip" in r.flags:
                assert (z > 50).any() and (z < -50).any()
            if r.npix == 1:
                assert set(np.unique(z).tolist()) <= {0.0, 64.0} and len(np.unique(z)) == 2
        if "empty" in r.flags:
            assert not d["mask"][2].any() and d["status"][2] == 1
        if "status" in r.flags:
            assert d["status"][1] == 2 and d["mask"][1].any()


# ---- holdout / score -------------------------------------------------------------------------------------------------------------
def test_holdout_rows():
    assert {n for n, _ in pc.HOLDOUT_ROWS} == {1, 255, 256, 257} and any(pad % 2 == 1 for _, pad in pc.HOLDOUT_ROWS)
    valid, train = pc.holdout_inputs(257)
    mask, group = pc.holdout_reference(valid, train)
    assert set(np.unique(group)) == {0, 1, 2} and ((group == 1) == (mask == 1)).all() and (valid > 1).any() and (train > 1).any()


def test_score_rows_hold_every_listed_value():
    rows = pc.SCORE_ROWS
    assert {r.T for r in rows} >= set(pc.SCORE_T) and {r.npix for r in rows} >= set(pc.SCORE_NPIX)
    assert {pc.score_chunks(r.npix) for r in rows} >= {1, 2, 6, 8}
    assert pc.score_finish_trips(2564) == 2 and pc.score_chunks(2564) % pc.SCORE_AHEAD == 2 and pc.score_finish_trips(4096) == 2
    assert any(r.T > pc.SCORE_FINISH_THREADS for r in rows) and any(r.T < 4 for r in rows)
    kinds = {k for r in rows for k in r.groups}
    assert kinds == {"mix", "ones", "twos", "zeros", "lastlane"}
    assert {r.expect[0] for r in rows} == {"pair_score_partial_kernel<false>", "pair_score_partial_kernel<true>"}
    assert pc.LASTLANE_PIXEL == 256 * 1 + 4 * 63 + 3
    for r in rows:
        pred, y, group = pc.score_inputs(r.T, r.npix, r.groups)
        assert (y * 64 == np.rint(y * 64)).all() and (y > 0).all()
        fin = np.isfinite(pred)
        assert (pred[fin] * 64 == np.rint(pred[fin] * 64)).all()
        for p, kind in enumerate(r.groups):
            ref = pc.score_reference(pred[p], y[p], group[p])
            if kind == "mix" and r.npix >= 511:
                assert {0, 1, 2, 3, 255} <= set(group[p].tolist())
                assert ref["n"].min() > 0 and (ref["m2"][:, min(3, r.T - 1)] == 0).all()
                assert ref["n"].sum(axis=0).max() <= np.isin(group[p], (1, 2)).sum()      # 3 and 255 are in no group
            if kind == "zeros":
                assert not ref["n"].any() and not ref["n_sam"].any() and np.isnan(ref["angle"]).all() and np.isnan(ref["rmse"]).all()
            if kind == "ones":
                assert not ref["n"][1].any() and ref["n"][0].all()
            if kind == "twos":
                assert not ref["n"][0].any() and ref["n"][1].all()
            if kind == "lastlane":
                held = np.flatnonzero(group[p] == 2)
                assert len(held) == r.npix // pc.SCORE_PIX > 0 and (held % pc.SCORE_PIX == pc.SCORE_PIX - 1).all()
                assert (group[p] != 0).all() and ref["n"][1].max() == len(held)


# ---- pooling ---------------------------------------------------------------------------------------------------------------------
def test_pool_membership_and_skip_layouts():
    from s2_emit.pairs import pool_layout
    ids = np.array(pc.pool_ids())
    assert len(ids) == pc.POOL_P and pc.POOL_M <= pc.POOL_P
    members = pc.pool_members()
    assert [len(m) for m in members] == list(pc.POOL_SIZES) and {1, 3, 4, 5, 8, 9} <= set(pc.POOL_SIZES)
    order, start = pc.pool_layout(ids)
    o2, s2 = pool_layout(ids)
    assert np.array_equal(order, o2) and np.array_equal(start, s2) and not np.array_equal(order, np.arange(pc.POOL_P))
    empty = set(pc.pool_empty_pairs())
    first = [g for g, m in enumerate(members) if m[0] in empty and not set(m) <= empty]
    last = [g for g, m in enumerate(members) if m[-1] in empty and not set(m) <= empty]
    middle = [g for g, m in enumerate(members) if set(m[1:-1]) & empty and not set(m) <= empty]
    allempty = [g for g, m in enumerate(members) if set(m) <= empty]
    assert first and last and middle and allempty == [pc.POOL_M - 1]
    assert all(len(members[g]) > pc.POOL_AHEAD for g in first + last + middle)
    for nb in (1, 16):
        samples, stats = pc.pool_stats_inputs(nb)
        assert [p for p in range(pc.POOL_P) if stats[p, 0] == 0] == sorted(empty)
        n, mean, m2, scale = pc.pool_stats_reference(samples, members[1], nb)
        assert n == sum(samples[p].shape[1] for p in members[1]) and mean.shape == (nb,)
        # Chan's merge of the members' statistics in float64 lands within the bar of the concatenation's
        tot, mu, mm = 0.0, np.zeros(nb), np.zeros(nb)
        for p in members[1]:
            nb_, mb, m2b = stats[p, 0], stats[p, 1:1 + nb], stats[p, 1 + nb:]
            if tot == 0:
                tot, mu, mm = nb_, mb.copy(), m2b.copy()
                continue
            t, delta = tot + nb_, mb - mu
            mu, mm, tot = mu + delta * (nb_ / t), mm + m2b + delta * delta * (tot * nb_ / t), t
        np.testing.assert_allclose(mu, mean, rtol=1e-13)
        np.testing.assert_allclose(mm, m2, rtol=1e-13)
    (_, e_order), (_, e_start) = pc.POOL_SKIPS
    order, start, mem, untouched = pc.pool_skip_layout(e_order)
    bad = [int(v) for v in order if not 0 <= v < pc.POOL_P]
    assert sorted(bad) == sorted([-1, pc.POOL_P, 2 ** 31 - 1, -(2 ** 31)]) and len(untouched) == 4
    assert all(p not in m for p in untouched for m in mem) and sum(map(len, mem)) == pc.POOL_P - 4
    assert all(len(mem[g]) > 0 for g in range(pc.POOL_M)) and np.array_equal(start, pc.pool_layout(ids)[1])
    order, start, mem, untouched = pc.pool_skip_layout(e_start)
    assert start[0] < 0 and start[pc.POOL_M] > pc.POOL_P and start[pc.POOL_M - 1] > start[pc.POOL_M] and not untouched

    def clamp(g):                                            # pool_slice of the kernels
        k0 = min(max(int(start[g]), 0), pc.POOL_P)
        k1 = int(start[g + 1])
        k1 = k0 if k1 < k0 else min(k1, pc.POOL_P)
        return [int(order[k]) for k in range(k0, k1)]
    assert [clamp(g) for g in range(pc.POOL_M)] == mem
    assert np.array_equal(order, pc.pool_layout(ids)[0])


def test_gram_reference_is_exact_and_copies_the_first_member():
    src, cnt = pc.gram_inputs(600)
    members = pc.pool_members()
    ref = pc.gram_reference(src, cnt, members)
    for g, mem in enumerate(members):
        live = [p for p in mem if cnt[p] != 0]
        np.testing.assert_array_equal(ref[g], src[live].sum(axis=0) if live else 0.0)
    one = members[0][0]
    assert np.signbit(src[one, 0]) and np.signbit(ref[0, 0]) and (ref[pc.POOL_M - 1] == 0).all()
    assert np.abs(ref).max() < 2 ** 53 and (src == np.rint(src)).all()


def test_models_rows():
    rows = pc.MODELS_ROWS
    blocks = [pc.pool_models_blocks(r.npad, r.kpad, r.T, r.nb) for r in rows]
    assert min(blocks) == 1 and max(blocks) == pc.POOL_MODEL_BLOCKS and pc.pool_models_total(16, 8, 3, 2) < 1024
    big = [r for r in rows if r.npad == 288 and r.T == 285]
    assert big and all(pc.pool_models_total(r.npad, r.kpad, r.T, r.nb) > pc.POOL_MODEL_BLOCKS * pc.POOL_MODEL_ELEMS for r in big)
    assert all(r.nf < r.npad and r.kpad >= r.nf for r in rows) and any(r.kpad > r.nf for r in rows) and any(r.padded for r in rows)
    assert all(r.group_bp >= r.nf * r.T and r.group_w32 >= r.kpad * r.T for r in rows)
    assert pc.MODELS_P == 5 and pc.MODELS_M == 2 and -1 in pc.MODELS_GROUP_OF and pc.MODELS_M in pc.MODELS_GROUP_OF
    assert len(pc.MODELS_GROUP_OF) == len(pc.MODELS_N_TRAIN) == pc.MODELS_P
    words = {pc.models_status(g, n) for g, n in zip(pc.MODELS_GROUP_OF, pc.MODELS_N_TRAIN) if 0 <= g < pc.MODELS_M}
    assert words == {(0, 1), (0, 0), (3, 3)}
    r = rows[0]
    g = pc.models_inputs(r)
    assert np.isnan(g["bp"][:, r.nf:]).all()
    want = pc.models_expected(r, g, 1)
    assert want["bp"].shape == (r.npad, r.T) and (want["bp"][r.nf:] == 0).all() and np.isfinite(want["bp"]).all()


def test_pack_and_unpack_keep_the_gaps():
    parts = [np.arange(5, dtype=np.float32) + 10 * i for i in range(3)]
    flat = pc.pack(parts, 8)
    assert flat.size == pc.span(3, 8, 5) and (flat[5:8].view(np.uint8) == pc.FILL).all()
    np.testing.assert_array_equal(pc.unpack(flat, 3, 8, 5), np.stack(parts))
    flat[6] = 0.0
    try:
        pc.unpack(flat, 3, 8, 5)
    except AssertionError:
        return
    raise AssertionError("a write into a gap went unnoticed")
