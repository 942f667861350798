"""tests/ot_cases.py holds what it says (CPU): the shapes reach the loops they are named for, every row stops where the table says
under the long-double reference, the breakdown rows keep their break iteration under a +-4 ulp change of K and their margin to
DBL_MAX, and the convergence rows are decided far from their threshold."""
import numpy as np
import pytest

import ot_cases as oc


def test_shapes_reach_the_paths_they_name():
    p = {s: oc.paths(*s) for s in oc.SHAPES}
    for n in (1, 63, 64, 65):
        assert p[(n, 2)]["col_double2"] and p[(n, 2)]["row_rem"] == 1 and p[(n, 2)]["row_rem_partial_wave"]
    assert p[(1, 2)]["nchunks"] == 1 and p[(1, 2)]["col_unrolled"] == [0] and p[(1, 2)]["col_tail"] == [1]
    assert p[(63, 2)]["col_unrolled"] == [7] and p[(63, 2)]["col_tail"] == [7]                  # fewer than 8 rows in the tail
    assert p[(64, 2)]["col_unrolled"] == [8] and p[(64, 2)]["col_tail"] == [0]                  # exactly 8 k rows
    assert p[(65, 2)]["nchunks"] == 2 and p[(65, 2)]["last_rows"] == 1 and p[(65, 2)]["col_unrolled"] == [0, 8]
    assert p[(61, 66)]["col_double2"] and p[(61, 66)]["col_unrolled"] == [7] and p[(61, 66)]["col_tail"] == [5]
    q = p[(257, 129)]
    assert q["nchunks"] == 5 and q["quarters"] == [2, 2, 1, 0] and q["quarter_past_end"]
    assert not q["col_double2"] and q["lone_last_column"] and q["row_unrolled"] == 0
    q = p[(520, 130)]
    assert q["nchunks"] == 9 and q["quarters"] == [3, 3, 3, 0] and q["last_rows"] == 8
    assert q["row_unrolled"] == 0 and q["row_rem"] == 2 and q["row_rem_partial_wave"]
    q = p[(66, 512)]
    assert q["row_unrolled"] == 1 and q["row_rem"] == 0 and q["col_blocks"] == 1
    q = p[(70, 646)]
    assert q["row_unrolled"] == 1 and q["row_rem"] == 2 and q["row_rem_partial_wave"] and q["col_blocks"] == 2 and q["init_blocks"] == 3
    assert p[(3, 4162)]["err_parts"] == 66 and p[(3, 4162)]["err_trips"] == 2 and p[(3, 4162)]["col_double2"]
    assert p[(3, 4161)]["err_parts"] == 66 and p[(3, 4161)]["err_trips"] == 2 and p[(3, 4161)]["lone_last_column"]
    assert max(v["err_trips"] for s, v in p.items() if s[1] <= 4096) == 1                      # only m > 4096 takes the second trip
    assert all(("shape-%dx%d" % s) in oc.ROWS for s in oc.SHAPES)
    # the clamp of d at 0: one row in which float64 gives d < 0 where the points nearly coincide, large enough to show in K
    d = oc.device_sqdist(*oc.inputs("clamp-61x66"))
    assert (d < 0).sum() >= 3 and (np.exp(d[d < 0] / -0.05) > 1.0).any()
    assert not any((oc.device_sqdist(*oc.inputs(n)) < 0).any() for n in oc.ROWS if n.startswith("shape-"))


def test_stop_rules_named_by_the_issue_have_a_row():
    rows = oc.ROWS.values()
    assert {0, 1, 2, 11} <= {r["itmax"] for r in rows if r["thr"] == 0.0}
    assert any(r["thr"] == 1e30 and r["expect"]["conv_iter"] == 0 for r in rows)
    assert any((r["expect"]["conv_iter"] or 0) >= 10 for r in rows)
    assert any(r["thr"] == 0.0 and r["itmax"] > 20 for r in rows)
    brk = [r["expect"] for r in rows if r["expect"]["break_iter"] is not None]
    assert any(e["break_iter"] % 2 == 1 and e["through"] == "v" for e in brk)
    assert any(e["break_iter"] % 2 == 0 and e["break_iter"] > 0 for e in brk)
    assert any(e["through"] == "u" for e in brk)
    assert any(e["break_iter"] == 0 and e["through"] == "zero" for e in brk)
    K = oc.reference("break0-v")["K"]
    assert (K[:, 0] > 0).all() and K[:, 0].max() < 1e-310                 # no 0 x inf in the row pass: u stays finite there
    # both values of every buffer choice of the projection
    bufs = {(k, oc.final_buffer(e["break_iter"], e["conv_iter"], r["itmax"]))
            for r in rows for e in [r["expect"]] for k in ["break" if e["break_iter"] is not None else "conv" if e["conv_iter"] is not None else "count"]}
    assert {("break", 0), ("break", 1), ("count", 0), ("count", 1), ("conv", 1)} <= bufs          # conv_iter is a multiple of 10: buffer 1 only


@pytest.mark.parametrize("name", list(oc.ROWS))
def test_row_ends_where_the_table_says(name):
    r, ref = oc.ROWS[name], oc.reference(name)
    e = r["expect"]
    assert (ref["break_iter"], ref["conv_iter"], ref["checks"]) == (e["break_iter"], e["conv_iter"], e["checks"])
    assert ref["through"] == e.get("through")
    X, Y = oc.inputs(name)
    assert X.shape == (r["n"], 3) and Y.shape == (r["m"], 3)
    if r["thr"] not in (0.0, 1e30):                                       # a decision that the device's rounding cannot move
        for ii, err, bound in ref["errs"]:
            assert abs(err - r["thr"]) > 100 * bound, (ii, err, bound)
        assert all(np.isfinite(b) and b < 1e-12 for _, _, b in ref["errs"])


@pytest.mark.parametrize("name", [n for n, r in oc.ROWS.items() if r["expect"]["break_iter"] is not None])
def test_breakdown_rows_are_robust(name):
    r, ref = oc.ROWS[name], oc.reference(name)
    X, Y = oc.inputs(name)
    bi = ref["break_iter"]
    assert len(ref["q"]) == bi + 1 and ref["q"][bi] > oc.MARGIN and all(q < -oc.MARGIN for q in ref["q"][:bi]), ref["q"]
    for how in (1, -1, 0):
        got = oc.solve(X, Y, r["reg"], r["itmax"], r["thr"], K=oc.perturbed(ref["K"], how), upto=bi + 2)
        assert got["break_iter"] == bi, (how, got["break_iter"])
        assert got["q"][bi] > oc.MARGIN and all(q < -oc.MARGIN for q in got["q"][:bi])


def test_perturbed_moves_every_element_by_four_spacings():
    K = np.array([[0.0, 5e-324, 1e-310, 1.0, 0.75]])
    up, down = oc.perturbed(K, 1), oc.perturbed(K, -1)
    assert np.array_equal(up.view(np.int64) - K.view(np.int64), np.full(K.shape, 4))
    assert np.array_equal(down.view(np.int64)[:, 2:] - K.view(np.int64)[:, 2:], np.full((1, 3), -4)) and (down[:, :2] == 0).all()
    assert set(np.unique(np.abs(oc.perturbed(np.ones((8, 8)), 0).view(np.int64) - np.ones((8, 8)).view(np.int64)))) == {4}


def test_references_against_the_oracle_restatement():
    """The long-double pieces chained by solve() are the schedule of oracle_np.sinkhorn_knopp: the same stop, the same targets."""
    from oracle import oracle_np as onp
    for name in ("conv10-61x66", "count2-257x129", "break0-zero"):
        r, ref = oc.ROWS[name], oc.reference(name)
        X, Y = oc.inputs(name)
        with np.errstate(all="ignore"):
            want = onp.ot_barycentric_targets(X, Y, r["reg"], r["itmax"], r["thr"])
        got, bound = oc.projection(ref["K"], ref["u"], ref["v"], Y)
        np.testing.assert_allclose(oc.f64(got), want, rtol=1e-9, atol=1e-12)
        assert float(bound.max()) < 1e-12
    K = oc.kernel_matrix(*oc.inputs("shape-61x66"), 0.05)
    np.testing.assert_allclose(oc.f64(K), np.exp(onp.sqeuclidean_cost(*oc.inputs("shape-61x66")) / -0.05), rtol=1e-12)
