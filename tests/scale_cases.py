"""Power-of-two rescaling of a tree QP and of everything a solve, an MPC step and their derivatives return (pure numpy: no device
code and no oracle is imported).  test_scale_reference.py holds the transform to the longdouble references and the oracle to exact
equivariance under it; test_gpu_scale.py holds every device route to the same.

New units: x' = Dx x, u' = Du u with Dx = 2^sx, Du = 2^su PER ENTRY (sx: sum_nx integers, su: sum_nu integers, in the flat layout
of the solution), objective' = alpha objective with alpha = 2^a, row r of [C | D] times 2^sc[r].  Then

    A_k' = Dx_k A_k Dx_p^-1     B_k' = Dx_k B_k Du_p^-1     b_k' = Dx_k b_k          H' = alpha D^-1 H D^-1     (q, r)' = alpha D^-1 (q, r)
    bounds' = D bounds          [C | D]' = 2^sc [C | D] D^-1                         (dmin, dmax)' = 2^sc (dmin, dmax)
    (x, u)' = D (x, u)          lam' = alpha Dx^-1 lam      (mu_x, mu_u)' = alpha D^-1 (mu_x, mu_u)      mu_d' = alpha 2^-sc mu_d
    dual value' = alpha dual value

Every factor is a power of two, applied with ldexp: exact unless a result leaves the range of normal doubles.  A dual Newton iteration
on the primed problem from lam0' is then, operation by operation (add, multiply, fma, divide, square root), the image of the iteration
on the original: only the termination norms sum entries of different units, and a comparison against an absolute constant (the
reference's dotp > 1e-10) may fall the other way.  `a` is even everywhere, so that with Dx^2 every pivot's exponent moves by an even
amount and the mantissa that reaches a reciprocal square root is the same.

A scaling is the dict `sc = scaling(d, ...)`: sx, su, a, sc (rows), x0 (the exponents of the parameter x0 of an MPC step: the root's
own sx where it keeps its states, given for an eliminated root)."""
from __future__ import annotations

import numpy as np

DEFAULT_OPTS = dict(termCondition=2, stationarityTolerance=1e-8, regTol=1e-6, regValue=1e-6)      # the solver's defaults (tqgpu_opts, oracle_opts_set_default)


def parents(nk):
    """dad[k] of a tree given by its children counts in breadth-first order"""
    nk = np.asarray(nk, int)
    dad, c = np.full(len(nk), -1), 1
    for k in range(len(nk)):
        dad[c:c + nk[k]] = k
        c += nk[k]
    return dad


def _offsets(d):
    nx, nu = np.asarray(d["nx"], int), np.asarray(d["nu"], int)
    nc = np.asarray(d.get("nc", np.zeros(len(nx), int)), int)
    return nx, nu, nc, np.concatenate([[0], np.cumsum(nx)]), np.concatenate([[0], np.cumsum(nu)]), np.concatenate([[0], np.cumsum(nc)])


def _i(e):
    return np.asarray(e, dtype=np.int64)


def shift(v, e):
    """v 2^e entry by entry, exactly (ldexp)"""
    v = np.asarray(v, dtype=np.float64)
    return np.ldexp(v, np.broadcast_to(_i(e), v.shape).astype(np.int32))


def shift_mat(M, rows, cols, a=0):
    """M[i, j, ...] 2^(a + rows[i] + cols[j]) (M with two or three axes: a trailing axis of columns of w is left alone)"""
    M = np.asarray(M, dtype=np.float64)
    e = a + _i(rows)[:, None] + _i(cols)[None, :]
    return shift(M, e if M.ndim == 2 else e[:, :, None])


def _blocks(flat, rows, cols, erow, ecol, a=0):
    """the column-major blocks (rows[i] x cols[i]) of `flat`, block i times 2^(a + erow[i][r] + ecol[i][c])"""
    out, o = [], 0
    for m, n, er, ec in zip(rows, cols, erow, ecol):
        M = np.reshape(np.asarray(flat[o:o + m * n], dtype=np.float64), (m, n), order="F")
        out.append(shift_mat(M, er, ec, a).ravel(order="F"))
        o += m * n
    assert o == len(flat), (o, len(flat))
    return np.concatenate(out) if out else np.zeros(0)


def scaling(d, sx=0, su=0, a=0, sc=0, x0=None):
    """a scaling of problem d: sx, su, sc scalars (uniform) or arrays per entry / row; x0: the exponents of the parameter of an MPC step on
    an eliminated root (nx0 integers; None: the root's own sx)"""
    nx, nu, nc, xo, uo, ro = _offsets(d)
    assert a % 2 == 0, "alpha = 2^a with a even"
    out = dict(sx=np.broadcast_to(_i(sx), (xo[-1],)).copy(), su=np.broadcast_to(_i(su), (uo[-1],)).copy(), a=int(a),
               sc=np.broadcast_to(_i(sc), (ro[-1],)).copy())
    out["nlam"] = int(nx[1:].sum())          # lam has no entries for the root's states
    out["x0"] = out["sx"][:nx[0]].copy() if x0 is None else _i(x0).copy()
    return out


def random_scaling(d, seed, a=30, lo=-20, hi=20, rows=True, nx0=None):
    """per-entry exponents in [lo, hi], drawn from `seed`"""
    nx, nu, nc, xo, uo, ro = _offsets(d)
    rng = np.random.Generator(np.random.PCG64(seed))
    sx, su, sc = (rng.integers(lo, hi + 1, n) for n in (xo[-1], uo[-1], ro[-1]))
    x0 = rng.integers(lo, hi + 1, nx0) if nx0 is not None else None
    return scaling(d, sx, su, a, sc if rows else 0, x0)


def is_uniform(sc):
    return all(len(np.unique(sc[k])) <= 1 for k in ("sx", "su")) and (len(sc["x0"]) == 0 or len(sc["sx"]) == 0 or np.all(sc["x0"] == sc["sx"][0]))


def scaled(d, sx, su=None, a=None, sc=None):
    """The flat problem d (nk, nx, nu, A, B, b, Qd / Rd or Q, R, S column major, q, r, bounds, optionally nc, C, D, dmin, dmax) in the
    new units.  scaled(d, scaling_dict) or scaled(d, sx, su, a, sc)."""
    s = sx if isinstance(sx, dict) else scaling(d, sx, su, a, 0 if sc is None else sc)
    nx, nu, nc, xo, uo, ro = _offsets(d)
    Nn, dad = len(nx), parents(d["nk"])
    ex = [s["sx"][xo[k]:xo[k + 1]] for k in range(Nn)]
    eu = [s["su"][uo[k]:uo[k + 1]] for k in range(Nn)]
    er = [s["sc"][ro[k]:ro[k + 1]] for k in range(Nn)]
    a = s["a"]
    out = {k: np.array(v, copy=True) for k, v in d.items()}
    kid = range(1, Nn)
    out["A"] = _blocks(d["A"], [nx[k] for k in kid], [nx[dad[k]] for k in kid], [ex[k] for k in kid], [-ex[dad[k]] for k in kid])
    out["B"] = _blocks(d["B"], [nx[k] for k in kid], [nu[dad[k]] for k in kid], [ex[k] for k in kid], [-eu[dad[k]] for k in kid])
    out["b"] = shift(d["b"], s["sx"][nx[0]:])
    if "Qd" in d:
        out["Qd"], out["Rd"] = shift(d["Qd"], a - 2 * s["sx"]), shift(d["Rd"], a - 2 * s["su"])
    if "Q" in d:
        nex, neu = [-e for e in ex], [-e for e in eu]
        out["Q"] = _blocks(d["Q"], nx, nx, nex, nex, a)
        out["R"] = _blocks(d["R"], nu, nu, neu, neu, a)
        out["S"] = _blocks(d["S"], nu, nx, neu, nex, a)
    out["q"], out["r"] = shift(d["q"], a - s["sx"]), shift(d["r"], a - s["su"])
    for k in ("xmin", "xmax"):
        if k in d:
            out[k] = shift(d[k], s["sx"])
    for k in ("umin", "umax"):
        if k in d:
            out[k] = shift(d[k], s["su"])
    if "nc" in d:
        out["C"] = _blocks(d["C"], nc, nx, er, [-e for e in ex])
        out["D"] = _blocks(d["D"], nc, nu, er, [-e for e in eu])
        out["dmin"], out["dmax"] = shift(d["dmin"], s["sc"]), shift(d["dmax"], s["sc"])
    return out


# ---- what comes back: `to` = +1 maps a quantity of the original problem into the new units, -1 back ----

def _lam_exp(s):
    return s["a"] - s["sx"][len(s["sx"]) - s["nlam"]:]


def map_lam(lam, s, to=1):
    return shift(lam, to * _lam_exp(s))


def map_solution(sol, s, to=1):
    """x, u, lam, dlam, mu_x, mu_u, mu_d of a solution dict (other keys are passed on)"""
    e = dict(x=s["sx"], u=s["su"], lam=_lam_exp(s), dlam=_lam_exp(s), mu_x=s["a"] - s["sx"], mu_u=s["a"] - s["su"], mu_d=s["a"] - s["sc"])
    return {k: (shift(v, to * e[k]) if k in e and v is not None else v) for k, v in sol.items()}


def map_fval(v, s, to=1):
    return shift(v, to * s["a"])


def map_x0(x0, s, to=1):
    return shift(x0, to * s["x0"])


def _root(d):
    """(nx of the root's children concatenated as index ranges into sx, nu[0] range, rows of the root)"""
    nx, nu, nc, xo, uo, ro = _offsets(d)
    nk0 = int(np.asarray(d["nk"], int)[0])
    return slice(xo[1], xo[1 + nk0]), slice(0, uo[1]), slice(0, ro[1])


def map_root_terms(root, d, s, to=1):
    """The originals of an eliminated root (mpc_cases.root_terms: A0 a list of (nx[kid], nx0) matrices, b0, S0 (nu[0], nx0), r0, and
    C0 (nc[0], nx0), dmin0, dmax0 where the root has rows) and the folded terms tqgpu_get_root_terms returns (b, r, dmin, dmax)."""
    nx, nu, nc, xo, uo, ro = _offsets(d)
    kx, ku, kr = _root(d)
    ekid, eu0, er0, e0, a = s["sx"][kx], s["su"][ku], s["sc"][kr], s["x0"], s["a"]
    out = dict(root)
    if root.get("A0") is not None:
        A0, o = [], 0
        for M in root["A0"]:
            m = np.asarray(M).shape[0]
            A0.append(shift_mat(M, to * ekid[o:o + m], -to * e0)); o += m
        out["A0"] = A0
    for k in ("b0", "b"):
        if root.get(k) is not None:
            out[k] = shift(root[k], to * ekid)
    if root.get("S0") is not None:
        out["S0"] = shift_mat(root["S0"], -to * eu0, -to * e0, to * a)
    for k in ("r0", "r"):
        if root.get(k) is not None:
            out[k] = shift(root[k], to * (a - eu0))
    if root.get("C0") is not None:
        out["C0"] = shift_mat(root["C0"], to * er0, -to * e0)
    for k in ("dmin0", "dmax0", "dmin", "dmax"):
        if root.get(k) is not None:
            out[k] = shift(root[k], to * er0)
    return out


def map_reference(xtraj, utraj, s, to=1):
    """xref, uref of a tracking window, one row per stage: every node of a stage reads the same row, so the scaling must be uniform"""
    assert is_uniform(s)
    es = int(s["sx"][0]) if len(s["sx"]) else 0
    et = int(s["su"][0]) if len(s["su"]) else 0
    return shift(xtraj, to * es), shift(utraj, to * et)


def map_linear_terms(q, r, s, to=1):
    return shift(q, to * (s["a"] - s["sx"])), shift(r, to * (s["a"] - s["su"]))


def map_gain(K, s, d, to=1):
    """K = du0/dx0 (nu[0], nx0)"""
    return shift_mat(K, to * s["su"][_root(d)[1]], -to * s["x0"])


def map_sensitivities(sens, s, to=1):
    """dx (sum_nx, nx0), du (sum_nu, nx0), dlam (sum_lam, nx0)"""
    e = dict(dx=s["sx"], du=s["su"], dlam=_lam_exp(s))
    return {k: shift_mat(v, to * e[k], -to * s["x0"]) for k, v in sens.items()}


def map_w(wx, wu, s, to=1):
    """w = dL/dz of a loss L that does not change with the units: (sum_nx, nw) and (sum_nu, nw), or 1-D"""
    f = lambda w, e: None if w is None else shift(w, -to * (e if np.ndim(w) == 1 else e[:, None]))
    return f(wx, s["sx"]), f(wu, s["su"])


def map_adjoint(g, s, to=1):
    """gq (sum_nx, nw), gr (sum_nu, nw), gb (sum_lam, nw), gx0 (nx0, nw): dL/dp' = dL/dp / (dp'/dp)"""
    e = dict(gq=s["sx"] - s["a"], gr=s["su"] - s["a"], gb=-s["sx"][len(s["sx"]) - s["nlam"]:], gx0=-s["x0"])
    return {k: (shift(v, to * e[k][:, None]) if k in e else v) for k, v in g.items()}


def map_adjoint_matrices(g, s, d, groups, to=1):
    """gH, gh, gA, gB, gb, gA0, gS0 of tqgpu_mpc_adjoint_matrices under a UNIFORM scaling (a group sums nodes, whose entries must share
    their units): lists of arrays with the column of w last.  groups: group_dims(d, hgroup, pad)."""
    assert is_uniform(s)
    es = int(s["sx"][0]) if len(s["sx"]) else int(s["x0"][0])
    et, a = int(s["su"][0]) if len(s["su"]) else 0, s["a"]
    out = {}
    for key, arrs in g.items():
        new = []
        for i, M in enumerate(arrs):
            M = np.asarray(M, dtype=np.float64)
            if key == "gb":
                new.append(shift(M, -to * es))
            elif key in ("gA", "gA0"):
                new.append(M.copy())                                   # Dx_p / Dx_k = 1
            elif key == "gB":
                new.append(shift(M, to * (et - es)))
            elif key == "gS0":
                new.append(shift(M, to * (et + es - a)))
            else:                                                      # gH, gh: the first nxg entries are states, the others inputs
                nxg = groups[i]["nx"]
                ez = np.concatenate([np.full(nxg, es), np.full(M.shape[0] - nxg, et)])
                if key == "gh" or M.ndim == 2:                          # (a kind-0 group holds the diagonal of H alone)
                    new.append(shift(M, to * ((2 if key == "gH" else 1) * ez - a)[:, None]))
                else:
                    new.append(shift_mat(M, to * ez, to * ez, -to * a))
        out[key] = new
    return out


def scaled_opts(opts, s):
    """The options under which a solve of the scaled problem is the image of a solve of the original under `opts`; uniform scalings
    only.  The termination norms are norms of the dynamics' residual (units of x): 2^s for the 2-norm and the maximum norm
    (termCondition 1, 2), 2^(2s) for the sum of squares (0); the dual Hessian A H^-1 A' has units Dx^2 / alpha, so regValue scales
    by 2^(2s - a) and regTol, which is compared as pivot <= regTol^2, by 2^(s - a/2)."""
    assert is_uniform(s) and s["a"] % 2 == 0
    es = int(s["sx"][0]) if len(s["sx"]) else int(s["x0"][0])
    o = dict(DEFAULT_OPTS)
    o.update(opts)
    o["stationarityTolerance"] = float(shift(o["stationarityTolerance"], (2 if o["termCondition"] == 0 else 1) * es))
    o["regValue"] = float(shift(o["regValue"], 2 * es - s["a"]))
    o["regTol"] = float(shift(o["regTol"], es - s["a"] // 2))
    return o


def map_error_norm(v, s, term, to=1):
    assert is_uniform(s)
    es = int(s["sx"][0]) if len(s["sx"]) else int(s["x0"][0])
    return shift(v, to * (2 if term == 0 else 1) * es)


def map_kkt(res, s, to=1):
    """the six class maxima of tqgpu_kkt_residual under a uniform scaling with su = sx (classes whose entries mix x and u rows share
    one unit only then) and rows scaled by sc = sx: stat alpha / D, dyn D, bfeas D, bcompl alpha, gfeas 2^sc, gcompl alpha"""
    assert is_uniform(s)
    es, a = int(s["sx"][0]), s["a"]
    assert np.all(s["su"] == es) and np.all(s["sc"] == s["sc"][:1])
    er = int(s["sc"][0]) if len(s["sc"]) else 0
    return shift(res, to * np.array([a - es, es, es, a, er, a]))


# ---- the cases of test_gpu_scale.py (and of the oracle's equivariance check in test_scale_reference.py) ----
# One row of trace_cases.py per route and node kind: the smallest problem the suite has for each.
ROUTE_ROWS = (
    "single_wg-clip-small8", "single_wg-clip",                      # single workgroup (g_persist), both node-size classes
    "persist-chain7", "persist-x0_eliminated",                      # persistent: uniform, multistage (root eliminated)
    "tiered", "tiered-near_start",                                  # (the far start backtracks: equivariance only, see NO_ORACLE)
    "fused_tails-backtracking",                                     # wide blocks on the launch-per-phase kernels with fused tails
    "three_launch-merged", "three_launch-backtracking",             # three-launch MFMA family
    "per_phase-backtracking",                                       # launch per phase
    "batch-single_wg-clip", "batch-persist",                        # batched launches: two members, two scalings
    "single_wg-dense", "batch-single_wg-dense",                     # dense single-launch and dense batch-launch opt-ins (kind 2)
    "fused_tails-dense", "per_phase-box", "per_phase-gen",          # node kinds 1, 2, 3 (kind 0: every row above the dense ones)
)
FIXED_ITERS = (1, 2, 3)
UNIFORM = dict(sx=12, su=-9, a=20)
FAR = (dict(sx=0, su=0, a=400), dict(sx=0, su=0, a=-400))


def entry_scaling(d, i, nx0=None):
    """the per-entry scaling number i of a problem: exponents in [-20, 20], a = 30 for even i and -30 for odd i"""
    return random_scaling(d, 7000 + i, a=30 if i % 2 == 0 else -30, nx0=nx0)


def uniform_scalings(d):
    """(name, scaling): the uniform set and the two far sets"""
    return [("uniform", scaling(d, **UNIFORM))] + [(f"far{'+' if f['a'] > 0 else '-'}", scaling(d, **f)) for f in FAR]


# rows of reg_cases.py for the whole solves under uniform scalings: an exact zero pivot (flag_*), a first-pass pivot at regTol / 2
# (threshold_below), ALWAYS; every route of reg_cases.ROUTES
REG_ROWS = ("generic-flag_mid_level", "generic-threshold_below", "generic-always", "gpersist-flag_mid_level", "gpersist-threshold_below",
            "dense_single-flag_mid_level", "persist_one-flag_mid_level-u6", "persist_two-flag_mid_level-u6", "persist_one-always-u6",
            "tiered-flag_mid_level-u6", "tiered-always-u6", "wide-flag_root", "wide-threshold_below", "wide3-flag_root", "wide3-threshold_below",
            "wide3-always")

# cases of mpc_cases.py (eliminated root): steps, and for the clipping ones sensitivities and adjoints
MPC_IDS = ("single_wg", "persist_c1", "three_launch", "generic", "dense_kind2_root", "dense_kind3_root")
SENS_IDS = ("single_wg", "persist_c1", "three_launch", "generic")


def mpc_scalings(c):
    """(name, scaling) for a case of mpc_cases.py: the parameter x0 has the units of the states"""
    d, nx0 = c["d"], c["nx0"]
    return [("uniform", scaling(d, 12, -9, 20, 5, x0=np.full(nx0, 12))), ("far+", scaling(d, 0, 0, 400, x0=np.zeros(nx0))),
            ("far-", scaling(d, 0, 0, -400, x0=np.zeros(nx0)))]


# The far start of trace_cases' "tiered" row clips most inputs; without regularisation (regType 0, as the fixed-iteration test asks) the
# oracle's own solution then moves by 3.6e-7 when the data move by one unit in the last place (helpers.ulp_solution_spread): no
# implementation can be held to 1e-10 of another there.  The same route on the same tree from the problem's own start instead.
def _tiered_near_start():
    import trace_cases as TC
    from treeqp_amd import problems as P
    return TC._lti(lambda: P.linear_chain(2, 4, 4, ubound=0.1))


_OWN = {"tiered-near_start": ("tiered", _tiered_near_start)}
_PROBLEMS = {}
NO_ORACLE = ("tiered",)          # rows whose unscaled run is not compared with the oracle at fixed iteration counts


def row(rid):
    """the row of trace_cases.py, or one of this module's own"""
    import trace_cases as TC
    if rid in _OWN:
        return dict(TC.row(_OWN[rid][0]), id=rid, backtracks=False)
    return TC.row(rid)


def problem(rid, capi):
    import trace_cases as TC
    if rid not in _OWN:
        return TC.problem(rid, capi)
    if rid not in _PROBLEMS:
        _PROBLEMS[rid] = _OWN[rid][1]()(capi)
    return _PROBLEMS[rid]


# ---- whole cases of the MPC, sensitivity and adjoint tests in the new units ----

def case_scalings(c):
    """(name, scaling) for a case with the keys d, nx0 (mpc_cases, mpc_root_cases, tracking_cases, sens_cases): uniform, far+, far-"""
    return mpc_scalings(c)


def scaled_base(base, s):
    """a case of mpc_cases (eliminated root: `root` holds its originals) or mpc_root_cases (x0 in the root's bounds) in the new units"""
    out = dict(base, d=scaled(base["d"], s))
    if base.get("root") is not None:
        out["root"] = map_root_terms(base["root"], base["d"], s)
    if "x0" in base:
        out["x0"] = map_x0(base["x0"], s)
    return out


def scaled_tracking_case(c, s):
    """a case of tracking_cases.py: problem, root, reference trajectory, base linear terms and the x0 of the steps"""
    out = scaled_base(c, s)
    out["xtraj"], out["utraj"] = map_reference(c["xtraj"], c["utraj"], s)
    out["q0"], out["r0"] = map_linear_terms(c["q0"], c["r0"], s)
    out["x0s"] = [map_x0(x, s) for x in c["x0s"]]
    return out


def scaled_sens_case(c, s):
    """a case of sens_cases.py / adj_cases.py / adjmat_cases.tree: base, the problem at x0, the parameter form, x0 and w"""
    out = dict(c, base=scaled_base(c["base"], s), d=scaled(c["d"], s), x0=map_x0(c["x0"], s))
    if c["form"] == "eliminated":
        out["param"] = dict(form="eliminated", A0=out["base"]["root"]["A0"], S0=out["base"]["root"]["S0"])
    for k in ("w", "w3"):
        if k in c:
            out[k] = map_w(c[k][0], c[k][1], s)
    return out


def reg_of(opts, s=None):
    """the regularisation rule of an option set as the references take it (scaled along with s)"""
    o = dict(DEFAULT_OPTS, regType=2)
    o.update(opts)
    if s is not None:
        o = scaled_opts(o, s)
    return dict(regType=o["regType"], regTol=o["regTol"], regValue=o["regValue"])


def group_dims(d, hgroup, pad=0):
    """per group of gH / gh: dict(nx = the states at the head of its entries (the root's phantom states `pad` included), diag = the
    group's nodes clip), from the first node of the group; hgroup: the filled-in map, one entry per node"""
    nx = np.asarray(d["nx"], int)
    hg = np.asarray(hgroup, int)
    out = []
    for g in range(int(hg.max(initial=-1)) + 1):
        k = int(np.flatnonzero(hg == g)[0])
        out.append(dict(nx=int(nx[k]) + (pad if k == 0 else 0)))
    return out
