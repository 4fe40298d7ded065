"""The adjoint of a tree QP's solution in its bounds and in the tracking reference, at a point (x, u) with the active set frozen there, two
ways in numpy.  For w = dL/dz:
(a) dense: the transposed KKT system of the whole tree with the active entries as equality rows (adj_ref.dense_kkt's system), by lstsq;
    dL/dl = a_mu, the multiplier of an active entry's row; gxref, guref by the chain rule from its a_z, summed per row by numpy;
(b) dual: adj_ref.dual_form extended with v = w - [Y; 0] + sum_c C_c' Y_c = w + E' Y, which is the bound gradient where an entry sits on a
    bound, and with the sums of include/treeqp_amd.h in the contract's order: members ascending in chunks of 64, one chain per chunk, the
    partials added ascending (bounds: over the groups' chunks; reference: over a row's (stage, chunk)).
Both return the bound gradients as dict(lo, hi), each (SX + SU, nw) in the layout [x | u] of tqgpu_get_solution: the side is the lower one
where the entry equals its lower bound bit for bit (so a pinned entry, min == max, carries the derivative for both bounds moved together
there), the upper one otherwise.  Importing this module does not load the native library."""
from __future__ import annotations

import numpy as np

import adj_ref as AR
import sens_ref as SR

CHUNK = 64


def sides(d, x, u, kinds=None):
    """(on the lower bound, on the upper bound and not on the lower), over [x | u]; kind-1 nodes have neither"""
    on = SR.pinned(d, x, u, kinds)
    z = np.concatenate([x, u])
    lo = on & (z == np.concatenate([d["xmin"], d["umin"]]))
    return lo, on & ~lo


def solve_active_set(d, kinds=None):
    """the solution of a tree QP whose kind-0 nodes carry bounds and whose kind-1 nodes ignore theirs (a mixed tree, which the oracle's two
    solvers do not take), by a primal active-set iteration over helpers.global_kkt: the most violated kind-0 entry is fixed at its bound,
    a fixed entry whose multiplier has the wrong sign is released; the fixed entries come back equal to their bounds bit for bit.
    -> dict(x, u, status, fixed)"""
    import helpers as H
    t = SR._assemble(d, kinds)
    lo, hi = np.concatenate([d["xmin"], d["umin"]]), np.concatenate([d["xmax"], d["umax"]])
    boxed = np.zeros(t["n"], dtype=bool)
    for k in range(t["Nn"]):
        boxed[t["idx"][k]] = t["kinds"][k] == 0
    fixed = {}
    for _ in range(4 * t["n"] + 4):
        z, mu = H.global_kkt(d, fixed)
        out = np.where(boxed, np.maximum(lo - z, z - hi), -1.0)
        i = int(np.argmax(out))
        if out[i] > 1e-12:
            fixed[i] = float(lo[i] if z[i] < lo[i] else hi[i])
            continue
        wrong = [j for j, m in mu.items() if lo[j] != hi[j] and (m < 0.0 if fixed[j] == lo[j] else m > 0.0)]
        if not wrong:
            for j, v in fixed.items():
                z[j] = v
            return dict(x=z[:t["SX"]], u=z[t["SX"]:], status=0, fixed=fixed)
        del fixed[wrong[0]]
    return dict(x=z[:t["SX"]], u=z[t["SX"]:], status=1, fixed=fixed)


def _split(v, lo, hi):
    return dict(lo=np.where(lo[:, None], v, 0.0), hi=np.where(hi[:, None], v, 0.0))


def dense(d, x, u, param, w, kinds=None):
    """(a) -> dict(lo, hi, gq, gr, gx0, residual, scale)"""
    t = SR._assemble(d, kinds)
    W = AR.stack(t, w)
    on = SR.pinned(d, x, u, kinds)
    fi = np.flatnonzero(on)
    F = np.zeros((len(fi), t["n"]))
    F[np.arange(len(fi)), fi] = 1.0
    m = t["SL"] + len(fi)
    Cm = np.vstack([t["E"], F])
    Kmat = np.block([[t["H"], Cm.T], [Cm, np.zeros((m, m))]])
    rhs = np.vstack([W, np.zeros((m, W.shape[1]))])
    a = np.linalg.lstsq(Kmat.T, rhs, rcond=None)[0]
    n, SL, SX = t["n"], t["SL"], t["SX"]
    v = np.zeros((n, W.shape[1]))
    v[fi] = a[n + SL:]
    lo, hi = sides(d, x, u, kinds)
    out = _split(v, lo, hi)
    gz = -a[:n]
    out.update(gq=gz[:SX], gr=gz[SX:], residual=float(np.max(np.abs(Kmat.T @ a - rhs))) if rhs.size else 0.0,
               scale=max(1.0, float(np.max(np.abs(a))) if a.size else 1.0))
    return out


def dual(d, x, u, param, w, kinds=None):
    """(b) -> dict(lo, hi, gq, gr, gx0, n_reg)"""
    t = SR._assemble(d, kinds)
    W = AR.stack(t, w)
    b = AR.dual_form(d, x, u, param, w, kinds)
    v = W + t["E"].T @ b["gb"]
    lo, hi = sides(d, x, u, kinds)
    out = _split(v, lo, hi)
    out.update(gq=b["gq"], gr=b["gr"], gx0=b["gx0"], n_reg=b["n_reg"], v=v)
    return out


def node_blocks(d, g, kinds=None):
    """per node [x | u] rows of a (SX + SU, nw) array"""
    t = SR._assemble(d, kinds)
    return [g[t["idx"][k]] for k in range(t["Nn"])]


def group_sums(d, g, hgroup, kinds=None, chunked=True):
    """one (nx + nu, nw) array per h-group: the members' blocks of g added up; chunked: in the contract's order, else by numpy"""
    blocks = node_blocks(d, g, kinds)
    hgroup = np.arange(len(blocks)) if hgroup is None else np.asarray(hgroup, dtype=int)
    out = []
    for grp in range(int(np.max(hgroup, initial=-1)) + 1):
        mem = [blocks[k] for k in np.flatnonzero(hgroup == grp)]
        if not chunked:
            out.append(np.sum(np.stack(mem), axis=0))
            continue
        total = None
        for at in range(0, len(mem), CHUNK):
            acc = np.zeros_like(mem[0])
            for blk in mem[at:at + CHUNK]:
                acc = acc + blk
            total = acc if total is None else total + acc
        out.append(total)
    return out


def stages(nk):
    nk = np.asarray(nk, dtype=int)
    st, nxt = np.zeros(len(nk), dtype=int), 1
    for k, n in enumerate(nk):
        st[nxt:nxt + n] = st[k] + 1
        nxt += n
    return st


def rows_of(nk, t0, T):
    """(row0, rows) of tqgpu_mpc_adjoint_reference"""
    row0 = min(t0, T - 1)
    return row0, min(t0 + int(stages(nk).max()), T - 1) - row0 + 1


def reference(d, gq, gr, t0, T, NXT, NUT, kinds=None, S0=None, chunked=True):
    """[gxref; guref]_rho = - sum over {k : rho_k = rho} of H_k' [gq_k; gr_k] (and - S0' gr_0 on the root's row) -> (row0, rows,
    gxref (rows, NXT, nw), guref (rows, NUT, nw)).  chunked: per stage in chunks of 64 members, one chain per chunk over its members (per
    member the rows of H_k ascending, then the S0 term), a row's partials added in ascending (stage, chunk) order; else one numpy product
    per node, added per row in node order"""
    t = SR._assemble(d, kinds)
    nw = gq.shape[1]
    st = stages(d["nk"])
    row0, rows = rows_of(d["nk"], t0, T)
    G = np.zeros((rows, NXT + NUT, nw))
    gz = np.vstack([gq, gr])

    def member(k, acc):
        ii = t["idx"][k]
        Hk, g = t["H"][np.ix_(ii, ii)], gz[ii]
        nx, nu = int(t["nx"][k]), int(t["nu"][k])
        cols = np.concatenate([np.arange(nx), NXT + np.arange(nu)]).astype(int)          # where the node's x and u entries lie in [xref | uref]
        if chunked:
            for i in range(nx + nu):
                acc[cols] = acc[cols] - Hk[i][:, None] * g[i][None, :]
            if k == 0 and S0 is not None:
                for m in range(nu):
                    acc[:NXT] = acc[:NXT] - np.asarray(S0)[m][:, None] * g[nx + m][None, :]
        else:
            acc[cols] = acc[cols] - Hk.T @ g
            if k == 0 and S0 is not None:
                acc[:NXT] = acc[:NXT] - np.asarray(S0).T @ g[nx:]
        return acc

    first = np.zeros(rows, dtype=bool)
    for s in range(int(st.max()) + 1):
        rho = min(t0 + s, T - 1) - row0
        mem = np.flatnonzero(st == s)
        for at in range(0, len(mem), CHUNK if chunked else len(mem)):
            acc = np.zeros((NXT + NUT, nw))
            for k in mem[at:at + (CHUNK if chunked else len(mem))]:
                acc = member(int(k), acc)
            G[rho] = acc if not first[rho] else G[rho] + acc
            first[rho] = True
    return row0, rows, G[:, :NXT], G[:, NXT:]
