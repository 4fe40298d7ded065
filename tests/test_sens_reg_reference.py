"""The rows of sens_reg_cases.py on the CPU: the conditions that make a row a test of the regularised and zero-pivot branches, and the
spread of the numpy evaluations the device is later held to.

Per row, at the oracle's solve with stationarityTolerance 1e-12 (status 0), with the row's options:
- the blocks sens_ref.dual_form and adj_ref.dual_form shift are exactly the row's, n_reg is the row's, guard >= 1.01 (no first-pass pivot
  within 1 % of regTol), in_range of the matrix actually solved < 1e-10;
- pinned rows: strict complementarity (|mu| > 1e-6) on every bound but the pinned states' own, the pinned entries' first-pass pivots
  == 0.0, and with regType 0 exactly those entries are zero columns;
- the spreads max |(b) - (c)| of K, dx, du, dlam and of gq, gr, gb, gx0 between dual_form and dense_shifted (one dense solve of the
  shifted system; no elimination shared) are printed with -s, kept in sens_reg_cases.SPREAD and asserted at 2 x recorded + 1e-16;
- regType 0 pinned rows: K, dx, du of dual_form against sens_ref.dense_kkt, the lstsq route (SPREAD_KKT): the zero-column convention
  gives the exact derivative of the singular system;
- gx0 of the adjoint against dZ' w of the sensitivities at the same options.
The shifted rows are NOT the exact derivative: the last test measures how far the default on-the-fly shift moves dZ (O(regValue))."""
import functools

import numpy as np
import pytest

import adj_ref as AR
import sens_cases as SN
import sens_ref as SR
import sens_reg_cases as RC


@functools.lru_cache(maxsize=None)
def _solved(name, mult=0):
    import oracle_py as orc
    c = RC.tree(name)
    x0 = c["x0"] + c["dx"] * 2.0 ** 10 * mult
    d = c["d"] if mult == 0 else SN.problem_at(c, x0)
    return d, SN.oracle_solve(orc, c, d)


@functools.lru_cache(maxsize=None)
def _evaluated(rid):
    """(row, the problem, the oracle's point, sens (b), sens (c), adjoint (b), adjoint (c))"""
    r = RC.row(rid)
    c = r["case"]
    d, s = _solved(c["id"])
    sb = SR.dual_form(d, s["x"], s["u"], c["param"], c["kinds"], **r["opts"])
    sc = SR.dense_shifted(d, s["x"], s["u"], c["param"], sb["shift"], sb["zero"], c["kinds"])
    ab = AR.dual_form(d, s["x"], s["u"], c["param"], c["w"], c["kinds"], **r["opts"])
    ac = AR.dense_shifted(d, s["x"], s["u"], c["param"], c["w"], ab["shift"], ab["zero"], c["kinds"])
    return r, d, s, sb, sc, ab, ac


def _diff(a, b):
    return float(np.max(np.abs(a - b), initial=0.0))


def _strict_complementarity(c, d, s):
    on = SR.pinned(d, s["x"], s["u"], c["kinds"])
    mu = np.concatenate([s["mu_x"], s["mu_u"]])
    skip = np.zeros(len(on), dtype=bool)
    skip[:c["nx0"] if c["form"] == "states" else 0] = True
    for row in RC.pinned_entries(c)[0] if "pins" in c else ():
        skip[row + int(d["nx"][0])] = True
    assert np.all(on[skip])
    act = on & ~skip
    assert act.any() and not (on | skip).all()
    assert np.all(np.abs(mu[act]) > 1e-6)


def test_ids_and_trees():
    import adj_cases as AC
    assert len(set(RC.ROW_IDS)) == len(RC.ROW_IDS)
    assert all(t in AC.CASE_IDS for t in RC.THRESHOLD) and all(t in AC.CASE_IDS for t, _ in RC.PINNED.values())
    blocks = {RC.THRESHOLD[t][1] for t in RC.THRESHOLD}
    assert 0 in blocks and len(blocks) > 1, "`one` must flag the root block on one tree and a non-root block on another"
    forms = {RC.tree("pin-" + p)["form"] for p in RC.PINNED}
    assert forms == {"states", "eliminated"}
    assert all(rid in RC.ROW_IDS for rid in RC.ZEROCOL_IDS + [RC.NW3_ID] + list(RC.PREDICT_IDS))
    assert all(rid == "regular" or rid in RC.ROW_IDS for b in RC.BATCHES.values() for rid, _ in b)
    assert set(RC.SPREAD) == set(RC.ROW_IDS) and set(RC.SPREAD_KKT) == set(RC.ZEROCOL_IDS)


@pytest.mark.parametrize("rid", RC.ROW_IDS)
def test_row_conditions(orc, rid):
    r, d, s, sb, sc, ab, ac = _evaluated(rid)
    c = r["case"]
    assert s["status"] == 0
    for what, b in (("sensitivity", sb), ("adjoint", ab)):
        assert b["flagged"] == r["flagged"], (what, b["flagged"])
        assert b["n_reg"] == r["n_reg"], what
        assert b["guard"] >= 1.01, (what, b["guard"])
        assert b["in_range"] < 1e-10, (what, b["in_range"])
        assert list(np.flatnonzero(b["zero"])) == (r["zero"] if r["opts"]["regType"] == 0 else []), what
    for key in ("shift", "zero"):
        assert np.array_equal(sb[key], ab[key])
    print(f"{rid}: flagged {sb['flagged']} of {len(sb['pivots'])} blocks, guard {sb['guard']:.4g}, in_range {sb['in_range']:.1e} / {ab['in_range']:.1e}")
    if r["group"] == "threshold":
        want = np.zeros(len(sb["shift"]))
        for p in r["flagged"]:
            want[RC.block_rows(d, p)] = r["opts"]["regValue"]
        assert np.array_equal(sb["shift"], want)
        return
    _strict_complementarity(c, d, s)
    for row in r["zero"]:
        p, j = RC.block_of(d, row)
        assert sb["pivots"][p][j] == 0.0, "the triggering pivot is not an exact zero"
    assert sum(int(np.count_nonzero(v == 0.0)) for v in sb["pivots"].values()) == len(r["zero"])


@pytest.mark.parametrize("rid", RC.ROW_IDS)
def test_the_two_evaluations_agree(orc, rid):
    r, d, s, sb, sc, ab, ac = _evaluated(rid)
    got = [_diff(sb[k], sc[k]) for k in ("K", "dx", "du", "dlam")] + [_diff(ab[k], ac[k]) for k in ("gq", "gr", "gb", "gx0")]
    print(f'    "{rid}":' + " " * max(1, 46 - len(rid)) + "(" + ", ".join(f"{v:.1e}" for v in got) + "),")
    for what, v, rec in zip(RC.WHAT, got, RC.SPREAD[rid]):
        assert v <= 2.0 * rec + 1e-16, (what, v, rec)          # (2 x: another BLAS may sum in another order)
    c = r["case"]
    if c["form"] == "states":
        assert np.array_equal(sb["dx"][:c["nx0"]], np.eye(c["nx0"]))
    want = np.vstack([sb["dx"], sb["du"]]).T @ np.vstack(c["w"])
    err = _diff(ab["gx0"], want)
    print(f"{rid}: |gx0 - dZ' w| = {err:.3e}, bound {RC.tol(rid, 'gx0'):.1e}")
    assert err <= RC.tol(rid, "gx0")


@pytest.mark.parametrize("rid", RC.ZEROCOL_IDS)
def test_the_zero_column_is_the_exact_derivative(orc, rid):
    r, d, s, sb, sc, ab, ac = _evaluated(rid)
    c = r["case"]
    a = SR.dense_kkt(d, s["x"], s["u"], c["param"], c["kinds"])
    assert a["residual"] < 1e-9 * a["scale"], a["residual"]
    got = [_diff(sb[k], a[k]) for k in ("K", "dx", "du")]
    print(f'    "{rid}":' + " " * max(1, 46 - len(rid)) + "(" + ", ".join(f"{v:.1e}" for v in got) + f"),   # lstsq residual {a['residual']:.1e}")
    for what, v, rec in zip(RC.WHAT, got, RC.SPREAD_KKT[rid]):
        assert v <= 2.0 * rec + 1e-16, (what, v, rec)
    assert np.all(sb["dlam"][r["zero"]] == 0.0)


@pytest.mark.parametrize("pid", list(RC.PINNED))
def test_the_default_shift_moves_dz_by_its_size(orc, pid):
    """what DESIGN.md and the header say of the on-the-fly shift: dZ is the exact derivative under regType 0, and O(regValue) away from it
    under the default regType 2 / 1e-6 / 1e-6 (measured: at most 2.2e-6 in dx, 7.5e-8 in K)"""
    exact = _evaluated(f"pin-{pid}-zerocol")[3]
    shifted = _evaluated(f"pin-{pid}-default")[3]
    moved = {k: _diff(exact[k], shifted[k]) for k in ("K", "dx", "du")}
    print(f"{pid}: default shift against the zero column: " + ", ".join(f"{k} {v:.1e}" for k, v in moved.items()))
    assert 0.0 < max(moved.values()) <= 10.0 * RC.DEFAULT["regValue"]


@pytest.mark.parametrize("bid", RC.BATCH_IDS)
def test_batch_members(orc, bid):
    mem = RC.members(bid)
    assert len({(c["id"], x0.tobytes()) for c, x0, _ in mem}) == len(mem), "two members are the same tree at the same x0"
    for (c, x0, n_reg), (rid, mult) in zip(mem, RC.BATCHES[bid]):
        d, s = _solved(c["id"], mult)
        assert s["status"] == 0 and np.array_equal(x0, c["x0"] + c["dx"] * 2.0 ** 10 * mult)
        _strict_complementarity(c, d, s)
        b = SR.dual_form(d, s["x"], s["u"], c["param"], c["kinds"], **RC.DEFAULT)
        assert b["n_reg"] == n_reg and b["flagged"] == (RC.pinned_entries(c)[1] if "pins" in c else [])
        a = AR.dual_form(d, s["x"], s["u"], c["param"], c["w"], c["kinds"], **RC.DEFAULT)
        assert a["n_reg"] == n_reg
        if rid != "regular":          # the device test judges the member by the row's recorded spread: it must hold at the member's x0 too
            sc = SR.dense_shifted(d, s["x"], s["u"], c["param"], b["shift"], b["zero"], c["kinds"])
            ac = AR.dense_shifted(d, s["x"], s["u"], c["param"], c["w"], a["shift"], a["zero"], c["kinds"])
            got = [_diff(b[k], sc[k]) for k in ("K", "dx", "du", "dlam")] + [_diff(a[k], ac[k]) for k in ("gq", "gr", "gb", "gx0")]
            print(f"{bid} {rid} x0 + {mult} steps: " + ", ".join(f"{v:.1e}" for v in got))
            for what, v, rec in zip(RC.WHAT, got, RC.SPREAD[rid]):
                assert v <= 2.0 * rec + 1e-16, (what, v, rec)
    if bid == "mixed_reg":
        assert [n for _, _, n in mem] == [0, 1, 2, 1]
