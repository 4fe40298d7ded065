"""What one step of an MPC loop costs, on the GPU box: the device loop (tqgpu_mpc_step, warm start mode 1: x0 fold, warm start and
u[0] on the device) against the host loop, the only way before these calls existed (numpy fold of x0 into b, tqgpu_set_problem with
the last duals, tqgpu_solve, tqgpu_get_solution).

    python tools/mpc_loop.py [--steps 200] [--skip 10] [--batch 64] [--root-states [--certify]] [c1] [c2] [batch]
    python tools/mpc_loop.py --tracking [--steps 200] [--skip 10] [--batch 64] [c1] [c2] [kind3] [batch]
    python tools/mpc_loop.py --shift --tracking --root-states [--steps 200] [--skip 10] [c1] [c2] [kind3]

Workloads, all x0-eliminated (nx[0] == 0): c1 = problems.spring_mass(), 85 nodes; c2 = problems.linear_chain(2, 9, 9), 1 023 nodes;
batch = 64 mirrors of c1 from different x0 (tqgpu_mpc_step_batch against fold + tqgpu_set_problem per member, tqgpu_solve_batch,
tqgpu_get_solution per member).  x0 moves on a prescribed path around the problem's own x0, entry i at step k
x0_i (1 + 0.05 sin(0.3 k + i + member)): the plant driven through one realisation leaves the feasible set of these benchmark
problems within a few steps, where no solver converges, so x0 is prescribed instead.  The host loop runs first; the device loop
runs the same sequence in the same process, on a mirror of the same problem, so that
step k of both loops is the same QP from the same duals: iterations and trials per step are compared and the steps that differ are
counted.  Per loop: wall time per step (host perf_counter around the step's calls; median, min, p90 over the steps after --skip),
the solve's device time (tqgpu_result.device_time), kernel launches and copies per step (device loop: tqgpu_mpc_stats; host loop:
the solve's launches plus the packing kernel of tqgpu_get_solution, and its three copies: b up, the duals up, the solution down).

--root-states: the same workloads as they are, not eliminated: the root keeps its states and x0 enters as xmin[0] = xmax[0] = x0
(tqgpu_mpc_set_root_states).  The host loop is then tqgpu_set_warm_start(1) once and per step tqgpu_set_problem with the root's
bounds replaced, tqgpu_solve, tqgpu_get_solution (three copies: the two bound arrays up -- the mirror of tqgpu_set_problem finds
them by comparing every array --, the solution down; launches: the warm-start copy, the solve's own with the re-pack of the
persistent route, the packing kernel of the solution).  Both loops run on the same x0 sequence, a prescribed path again, here
x0_i (0.95 + 0.05 sin(0.3 k + i + member)), which stays within the problem's own x0.  --certify adds a third loop and a fourth: the
certified step (tqgpu_mpc_set_certify) against the plain step followed by tqgpu_kkt_residual, the two ways to know the KKT classes
of the point whose u[0] is applied.  The certified loop's launches, copies and waits are counted (tqgpu_mpc_stats); those of the
"step + kkt" loop are the step's counted ones plus what tqgpu_kkt_residual adds by its code, which nothing counts: three launches
(the packing kernel, k_kkt, k_kkt_max), one copy, one stream synchronisation.  The printed line says so.

--tracking: the root-states workloads with a reference trajectory that shifts one stage per step (tqgpu_mpc_set_tracking, and the window
inside tqgpu_mpc_step_at / tqgpu_mpc_step_batch_at; member i of the batch is i stages ahead) against the host loop of the parent
commit's API: numpy fold of the window into q, r, tqgpu_set_problem with the root's bounds replaced, tqgpu_solve, tqgpu_get_solution
(five copies: q, r and the two bound arrays up, the solution down).  kind3 is an 85-node dense tree with 21 kind-3 nodes (kind3_tree:
the shape of tests/gen_cases.scaled_one_row with data that converge): there the host loop has to go through tqgpu_set_objective_mixed,
which empties the stored working sets; the device loop is tqgpu_mpc_step_at, tqgpu_get_solution; active-set steps per kind-3 node and
stage sweep are printed for both.

--shift (on top of --tracking and --root-states): the same closed-loop sequences three ways, warm start mode 2 (tqgpu_mpc_set_shift: the
duals, and on kind3 also the working sets, move a stage on the device), mode 1, and the host loop that the API without the shift allows
(tqgpu_get_solution, numpy gather, tqgpu_set_lambda, tqgpu_mpc_step_at); see shift_compare.

    python tools/mpc_loop.py --gain [--steps 200] [--skip 10] [c1] [c2]
    python tools/mpc_loop.py --predict [--steps 200] [--skip 10] [c1] [c2]

--gain: the time of tqgpu_mpc_sensitivity next to the step, against nx0 finite-difference steps through tqgpu_mpc_step, on c1 and c2
with root states and on c1 x0-eliminated, with the launches, copies and waits of both (gain_compare).  --predict: iterations per step of
the dual predictor (tqgpu_mpc_sensitivity + tqgpu_mpc_predict with duals) against warm start mode 1 over the sequences of --root-states
and --tracking (predict_compare).

    python tools/mpc_loop.py --predict-at [--steps 200] [--skip 10] [c1] [c2] [kind3]
    python tools/mpc_loop.py --tangent [--steps 200] [--skip 10] [c1] [c2] [kind3]

--predict-at: the tracking loop with tqgpu_mpc_predict_at(x0 and window of the next step, duals = 1) ahead of every tqgpu_mpc_step_at, against
the plain loop and the x0-only predictor (predict_at_compare).  --tangent: tqgpu_mpc_tangent (nd = 1) alone behind every step, against
tqgpu_mpc_adjoint + tqgpu_mpc_get_adjoint + numpy, the only route to a directional derivative without it (tangent_compare).  kind3: both
calls refuse trees with nodes of kind 2 or 3; the refusal is printed (refused_kind3).

    python tools/mpc_loop.py --gain-batch N[,N2,..] [--steps 200] [--skip 10] [c1] [c2]

--gain-batch: behind every tqgpu_mpc_step_batch of N trees, the gains and the dual predictor two ways, on c1 x0-eliminated and on c2 with
root states: (a) tqgpu_mpc_sensitivity_batch and tqgpu_mpc_predict_batch, (b) N calls each of tqgpu_mpc_sensitivity and tqgpu_mpc_predict on
mirrors of their own; wall time, launches, copies and waits of each, the largest difference of K and of u0_pred between them, which must be
0, and the iterations per step with the dual predictor against warm start mode 1 alone (gain_batch_compare).

    python tools/mpc_loop.py --adjoint [--steps 200] [--skip 10] [c1] [c2]

--adjoint: behind every step, three ways to the gradient of a scalar loss with one random w = dL/dz, on c1 and c2 with root states and on
c1 x0-eliminated: tqgpu_mpc_adjoint, tqgpu_mpc_sensitivity + tqgpu_mpc_get_sensitivities + the host product dZ' w, and tqgpu_mpc_adjoint
behind tqgpu_mpc_sensitivity (the factor stored), with the launches, copies and waits of each (adjoint_compare).

    python tools/mpc_loop.py --adjoint-batch N[,N2,..] [--steps 200] [--skip 10] [c1] [c2]

--adjoint-batch: behind every tqgpu_mpc_step_batch of N trees, one random w per member and two ways to the members' gradients, on c1 with
both root forms and on c2 with root states: (a) one tqgpu_mpc_adjoint_batch, (b) N calls of tqgpu_mpc_adjoint on mirrors of their own; wall
time, launches, copies and waits of each, and the largest difference of gx0 between them, which must be 0 (adjoint_batch_compare).

    python tools/mpc_loop.py --adjoint-matrices [--adjoint-batch N[,N2,..]] [--steps 200] [--skip 10] [c1] [c2]

--adjoint-matrices: behind every step and adjoint, the gradients of the matrices with one group for all dynamics and one for all stage
Hessians of equal sizes, two ways: tqgpu_mpc_adjoint_matrices (with --adjoint-batch N: tqgpu_mpc_adjoint_matrices_batch, reduce = 1, behind
the batch step and the batch adjoint), and the host route, tqgpu_get_solution + tqgpu_mpc_get_adjoint + numpy outer products and sums
(adjoint_matrices_compare)."""
import ctypes as C
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import numpy as np  # noqa: E402


def stats(ts):
    a = 1e6 * np.asarray(ts)
    return float(np.median(a)), float(a.min()), float(np.percentile(a, 90))


def eliminated(capi, p):
    """(x0-eliminated flat problem, A0 per root child, b0, B of the first edge, x0 of the problem)"""
    import mpc_cases as M
    nk = p.nk()
    flat = capi.TreeQp(np.full(p.Nn, p.nx), np.where(nk > 0, p.nu, 0), nk).fill_lti(p).flat()
    nk0, nx = int(nk[0]), p.nx
    A0 = [flat["A"][k * nx * nx:(k + 1) * nx * nx].reshape((nx, nx), order="F").copy() for k in range(nk0)]
    b0 = flat["b"][:nk0 * nx].copy()
    B0 = flat["B"][:nx * p.nu].reshape((nx, p.nu), order="F").copy()
    d, _ = M.eliminate(flat)
    return d, A0, b0, B0, np.asarray(p.x0, dtype=np.float64).copy()


def moved(x0, k, member):
    return x0 * (1.0 + 0.05 * np.sin(0.3 * k + np.arange(len(x0)) + member))


def moved_inward(x0, k, member):
    """the path of the root-states mode: as `moved`, but never beyond the problem's own x0 (entry i between 0.9 and 1.0 of it): C2's own
    x0 lies at the edge of what its input bounds can hold, and 5 % beyond it no solve converges"""
    return x0 * (0.95 + 0.05 * np.sin(0.3 * k + np.arange(len(x0)) + member))


def fold_b(A0, b0, x0):
    return np.concatenate([b0[i * len(x0):(i + 1) * len(x0)] + A @ x0 for i, A in enumerate(A0)])


def report(name, wall, dev, launches, copies, skip):
    med, lo, p90 = stats(wall[skip:])
    print(f"    {name:12s} wall median {med:8.1f} us  min {lo:8.1f}  p90 {p90:8.1f} | device {1e6 * np.median(dev[skip:]):7.1f} us | "
          f"launches {np.median(launches[skip:]):.0f}  copies {np.median(copies[skip:]):.0f}", flush=True)
    return med


def single(capi, name, p, steps, skip):
    L = capi.lib()
    d, A0, b0, B0, x0 = eliminated(capi, p)
    dp = lambda a: a.ctypes.data_as(capi.c_dbl_p)
    o, r = capi._gpu_opts(), capi.GpuResult()
    nu0, nb = int(d["nu"][0]), len(b0)
    # host loop
    g = capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)
    keep = {k: np.ascontiguousarray(d[k], dtype=np.float64) for k in ("A", "B", "b", "Qd", "Rd", "q", "r", "xmin", "xmax", "umin", "umax")}
    lam = np.zeros(g.sum_lam)
    sol = [np.zeros(n) for n in (g.sum_nx, g.sum_nu, g.sum_lam, g.sum_nx, g.sum_nu, g.sum_lam)]
    sp = [dp(b) for b in sol]
    order = ("A", "B", "b", "Qd", "Rd", "q", "r", "xmin", "xmax", "umin", "umax")
    xs, hw, hd, hl, hc, hcnt, hu = [], [], [], [], [], [], []
    x = moved(x0, 0, 0)
    for _ in range(steps):
        xs.append(x.copy())
        t0 = time.perf_counter()
        keep["b"][:nb] = fold_b(A0, b0, x)
        assert L.tqgpu_set_problem(g.h, *[dp(keep[k]) for k in order], dp(lam)) == 0
        assert L.tqgpu_solve(g.h, C.byref(o), C.byref(r)) == 0
        assert L.tqgpu_get_solution(g.h, *sp) == 0
        hw.append(time.perf_counter() - t0)
        lam[:] = sol[2]
        hu.append(sol[1][:nu0].copy())
        hd.append(r.device_time); hl.append(r.n_launches + 1); hc.append(3); hcnt.append((r.status, r.iter, r.ls_total))
        x = moved(x0, len(xs), 0)
    g.close()
    # device loop, the same x0 sequence
    g = capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)
    g.mpc_set_root(A0, b0)
    g.set_warm_start(1)
    u0 = np.zeros(max(nu0, 1))
    la, co, wa = C.c_int(), C.c_int(), C.c_int()
    dw, dd, dl, dc, dcnt, du = [], [], [], [], [], 0.0
    for k in range(steps):
        xk = xs[k]
        t0 = time.perf_counter()
        assert L.tqgpu_mpc_step(g.h, dp(xk), C.byref(o), C.byref(r), dp(u0)) == 0
        dw.append(time.perf_counter() - t0)
        L.tqgpu_mpc_stats(C.byref(la), C.byref(co), C.byref(wa))
        dd.append(r.device_time); dl.append(la.value); dc.append(co.value); dcnt.append((r.status, r.iter, r.ls_total))
        du = max(du, float(np.max(np.abs(u0[:nu0] - hu[k]))))
    kkt = g.kkt_residual()["max"]
    g.close()
    differ = sum(a != b for a, b in zip(hcnt, dcnt))
    print(f"{name}: {len(d['nk'])} nodes, {steps} steps, iterations per step median {np.median([c[1] for c in hcnt]):.0f} "
          f"(first step {hcnt[0][1]}), all status 0: {all(c[0] == 0 for c in hcnt + dcnt)}")
    h = report("host loop", hw, hd, hl, hc, skip)
    v = report("device loop", dw, dd, dl, dc, skip)
    print(f"    steps with other iterations or trials than the host loop: {differ} of {steps}; largest |u0 (device) - u0 (host)| {du:.2e}; "
          f"KKT of the last device step {kkt:.2e}; host / device wall {h / v:.2f}", flush=True)


def batch(capi, p, n, steps, skip):
    L = capi.lib()
    d, A0, b0, B0, x0 = eliminated(capi, p)
    dp = lambda a: a.ctypes.data_as(capi.c_dbl_p)
    o = capi._gpu_opts()
    nu0, nb, nx = int(d["nu"][0]), len(b0), len(x0)
    order = ("A", "B", "b", "Qd", "Rd", "q", "r", "xmin", "xmax", "umin", "umax")
    mk = lambda: [capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d) for _ in range(n)]
    # host loop
    ms = mk()
    arr = (C.c_void_p * n)(*[m.h for m in ms])
    res = (capi.GpuResult * n)()
    keeps = [{k: np.ascontiguousarray(d[k], dtype=np.float64).copy() for k in order} for _ in range(n)]
    lams = [np.zeros(ms[0].sum_lam) for _ in range(n)]
    sols = [[np.zeros(s) for s in (ms[0].sum_nx, ms[0].sum_nu, ms[0].sum_lam, ms[0].sum_nx, ms[0].sum_nu, ms[0].sum_lam)] for _ in range(n)]
    X = [moved(x0, 0, i) for i in range(n)]
    xs, hw, hcnt = [], [], []
    for _ in range(steps):
        xs.append([x.copy() for x in X])
        t0 = time.perf_counter()
        for i in range(n):
            keeps[i]["b"][:nb] = fold_b(A0, b0, X[i])
            assert L.tqgpu_set_problem(ms[i].h, *[dp(keeps[i][k]) for k in order], dp(lams[i])) == 0
        assert L.tqgpu_solve_batch(arr, n, C.byref(o), res) == 0
        for i in range(n):
            assert L.tqgpu_get_solution(ms[i].h, *[dp(b) for b in sols[i]]) == 0
        hw.append(time.perf_counter() - t0)
        hcnt.append([(res[i].status, res[i].iter, res[i].ls_total) for i in range(n)])
        for i in range(n):
            lams[i][:] = sols[i][2]
            X[i] = moved(x0, len(xs), i)
    for m in ms:
        m.close()
    # device loop
    ms = mk()
    arr = (C.c_void_p * n)(*[m.h for m in ms])
    for m in ms:
        m.mpc_set_root(A0, b0)
        m.set_warm_start(1)
    u0s = np.zeros(n * max(nu0, 1))
    la, co, wa = C.c_int(), C.c_int(), C.c_int()
    dw, dl, dc, dwt, dcnt = [], [], [], [], []
    for k in range(steps):
        xk = np.ascontiguousarray(np.concatenate(xs[k]))
        t0 = time.perf_counter()
        assert L.tqgpu_mpc_step_batch(arr, n, dp(xk), C.byref(o), res, dp(u0s)) == 0
        dw.append(time.perf_counter() - t0)
        L.tqgpu_mpc_stats(C.byref(la), C.byref(co), C.byref(wa))
        dl.append(la.value); dc.append(co.value); dwt.append(wa.value)
        dcnt.append([(res[i].status, res[i].iter, res[i].ls_total) for i in range(n)])
    for m in ms:
        m.close()
    differ = sum(a != b for ha, da in zip(hcnt, dcnt) for a, b in zip(ha, da))
    h, hlo, hp = stats(hw[skip:])
    v, vlo, vp = stats(dw[skip:])
    print(f"batch: {n} mirrors of c1, {steps} steps, all status 0: {all(c[0] == 0 for row in hcnt + dcnt for c in row)}")
    print(f"    host loop    wall median {h:8.1f} us  min {hlo:8.1f}  p90 {hp:8.1f} | copies {3 * n} (three per member)")
    print(f"    device loop  wall median {v:8.1f} us  min {vlo:8.1f}  p90 {vp:8.1f} | launches {np.median(dl[skip:]):.0f}  copies {np.median(dc[skip:]):.0f}  waits {np.median(dwt[skip:]):.0f}")
    print(f"    member steps with other iterations or trials than the host loop: {differ} of {n * steps}; host / device wall {h / v:.2f}", flush=True)


ORDER = ("A", "B", "b", "Qd", "Rd", "q", "r", "xmin", "xmax", "umin", "umax")


def full_root(capi, p):
    """(flat problem with the root's states, x0 of the problem)"""
    nk = p.nk()
    flat = capi.TreeQp(np.full(p.Nn, p.nx), np.where(nk > 0, p.nu, 0), nk).fill_lti(p).flat()
    return flat, np.asarray(p.x0, dtype=np.float64).copy()


def single_root(capi, name, p, steps, skip, certify):
    L = capi.lib()
    d, x0 = full_root(capi, p)
    dp = lambda a: a.ctypes.data_as(capi.c_dbl_p)
    o, r = capi._gpu_opts(), capi.GpuResult()
    nu0, nx0 = int(d["nu"][0]), len(x0)
    xs = [moved_inward(x0, k, 0) for k in range(steps)]
    # host loop
    g = capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)
    g.set_warm_start(1)
    keep = {k: np.ascontiguousarray(d[k], dtype=np.float64).copy() for k in ORDER}
    sol = [np.zeros(n) for n in (g.sum_nx, g.sum_nu, g.sum_lam, g.sum_nx, g.sum_nu, g.sum_lam)]
    sp = [dp(b) for b in sol]
    hw, hd, hl, hc, hcnt, hu = [], [], [], [], [], []
    for x in xs:
        t0 = time.perf_counter()
        keep["xmin"][:nx0] = x
        keep["xmax"][:nx0] = x
        assert L.tqgpu_set_problem(g.h, *[dp(keep[k]) for k in ORDER], None) == 0
        assert L.tqgpu_solve(g.h, C.byref(o), C.byref(r)) == 0
        assert L.tqgpu_get_solution(g.h, *sp) == 0
        hw.append(time.perf_counter() - t0)
        hu.append(sol[1][:nu0].copy())
        hd.append(r.device_time); hl.append(r.n_launches + 2); hc.append(3); hcnt.append((r.status, r.iter, r.ls_total))      # (+ the warm-start copy, the packing kernel of the export)
    g.close()
    u0 = np.zeros(max(nu0, 1))
    la, co, wa = C.c_int(), C.c_int(), C.c_int()
    res6, node6 = np.zeros(6), np.zeros(6, dtype=np.int32)

    def device_loop(mode):
        """mode: 'step', 'certified' (tqgpu_mpc_set_certify), 'step+kkt' (the step, then tqgpu_kkt_residual)"""
        g = capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)
        g.mpc_set_root_states()
        g.set_warm_start(1)
        g.mpc_set_certify(mode == "certified")
        w, dv, ln, cp, wt, cnt, du, same = [], [], [], [], [], [], 0.0, True
        for k in range(steps):
            t0 = time.perf_counter()
            assert L.tqgpu_mpc_step(g.h, dp(xs[k]), C.byref(o), C.byref(r), dp(u0)) == 0
            if mode == "step+kkt":
                assert L.tqgpu_kkt_residual(g.h, dp(res6), node6.ctypes.data_as(capi.c_int_p), None) == 0
            w.append(time.perf_counter() - t0)
            L.tqgpu_mpc_stats(C.byref(la), C.byref(co), C.byref(wa))
            extra = (3, 1, 1) if mode == "step+kkt" else (0, 0, 0)          # (tqgpu_kkt_residual: the packing kernel and the two KKT kernels; the head down; the stream)
            dv.append(r.device_time); ln.append(la.value + extra[0]); cp.append(co.value + extra[1]); wt.append(wa.value + extra[2])
            cnt.append((r.status, r.iter, r.ls_total))
            du = max(du, float(np.max(np.abs(u0[:nu0] - hu[k]))))
            if mode == "certified":
                assert L.tqgpu_mpc_get_certificate(g.h, dp(res6), node6.ctypes.data_as(capi.c_int_p)) == 0
        kkt = float(res6.max()) if mode != "step" else g.kkt_residual()["max"]
        g.close()
        return w, dv, ln, cp, wt, cnt, du, kkt

    dw, dd, dl, dc, dwt, dcnt, du, kkt = device_loop("step")
    differ = sum(a != b for a, b in zip(hcnt, dcnt))
    print(f"{name}, root with states: {len(d['nk'])} nodes, {steps} steps, iterations per step median {np.median([c[1] for c in hcnt]):.0f} "
          f"(first step {hcnt[0][1]}), all status 0: {all(c[0] == 0 for c in hcnt + dcnt)}")
    h = report("host loop", hw, hd, hl, hc, skip)
    v = report("device loop", dw, dd, dl, dc, skip)
    print(f"    device loop waits per step {np.median(dwt[skip:]):.0f}; steps with other iterations or trials than the host loop: {differ} of {steps}; "
          f"largest |u0 (device) - u0 (host)| {du:.2e}; KKT of the last device step {kkt:.2e}; host / device wall {h / v:.2f}", flush=True)
    if certify:
        cw, cd, cl, cc, cwt, ccnt, cu, ck = device_loop("certified")
        kw, kd, kl, kc, kwt, kcnt, ku, kk = device_loop("step+kkt")
        a = report("certified", cw, cd, cl, cc, skip)
        b = report("step + kkt", kw, kd, kl, kc, skip)
        print("    (step + kkt: launches, copies and waits are the step's counted ones + 3, 1, 1 for tqgpu_kkt_residual, derived from its code, not counted)")
        print(f"    waits per step: certified {np.median(cwt[skip:]):.0f} (counted), step + tqgpu_kkt_residual {np.median(kwt[skip:]):.0f} (derived); iterations and trials equal to the plain loop's: "
              f"{ccnt == dcnt and kcnt == dcnt}; last certificate {ck:.2e} / {kk:.2e}; (step + kkt) / certified wall {b / a:.2f}", flush=True)


def batch_root(capi, p, n, steps, skip):
    L = capi.lib()
    d, x0 = full_root(capi, p)
    dp = lambda a: a.ctypes.data_as(capi.c_dbl_p)
    o = capi._gpu_opts()
    nu0, nx0 = int(d["nu"][0]), len(x0)
    mk = lambda: [capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d) for _ in range(n)]
    xs = [[moved_inward(x0, k, i) for i in range(n)] for k in range(steps)]
    # host loop
    ms = mk()
    arr = (C.c_void_p * n)(*[m.h for m in ms])
    res = (capi.GpuResult * n)()
    keeps = [{k: np.ascontiguousarray(d[k], dtype=np.float64).copy() for k in ORDER} for _ in range(n)]
    sols = [[np.zeros(s) for s in (ms[0].sum_nx, ms[0].sum_nu, ms[0].sum_lam, ms[0].sum_nx, ms[0].sum_nu, ms[0].sum_lam)] for _ in range(n)]
    for m in ms:
        m.set_warm_start(1)
    hw, hcnt = [], []
    for k in range(steps):
        t0 = time.perf_counter()
        for i in range(n):
            keeps[i]["xmin"][:nx0] = xs[k][i]
            keeps[i]["xmax"][:nx0] = xs[k][i]
            assert L.tqgpu_set_problem(ms[i].h, *[dp(keeps[i][q]) for q in ORDER], None) == 0
        assert L.tqgpu_solve_batch(arr, n, C.byref(o), res) == 0
        for i in range(n):
            assert L.tqgpu_get_solution(ms[i].h, *[dp(b) for b in sols[i]]) == 0
        hw.append(time.perf_counter() - t0)
        hcnt.append([(res[i].status, res[i].iter, res[i].ls_total) for i in range(n)])
    for m in ms:
        m.close()
    # device loop
    ms = mk()
    arr = (C.c_void_p * n)(*[m.h for m in ms])
    for m in ms:
        m.mpc_set_root_states()
        m.set_warm_start(1)
    u0s = np.zeros(n * max(nu0, 1))
    la, co, wa = C.c_int(), C.c_int(), C.c_int()
    dw, dl, dc, dwt, dcnt = [], [], [], [], []
    for k in range(steps):
        xk = np.ascontiguousarray(np.concatenate(xs[k]))
        t0 = time.perf_counter()
        assert L.tqgpu_mpc_step_batch(arr, n, dp(xk), C.byref(o), res, dp(u0s)) == 0
        dw.append(time.perf_counter() - t0)
        L.tqgpu_mpc_stats(C.byref(la), C.byref(co), C.byref(wa))
        dl.append(la.value); dc.append(co.value); dwt.append(wa.value)
        dcnt.append([(res[i].status, res[i].iter, res[i].ls_total) for i in range(n)])
    for m in ms:
        m.close()
    differ = sum(a != b for ha, da in zip(hcnt, dcnt) for a, b in zip(ha, da))
    h, hlo, hp = stats(hw[skip:])
    v, vlo, vp = stats(dw[skip:])
    print(f"batch, roots with states: {n} mirrors of c1, {steps} steps, all status 0: {all(c[0] == 0 for row in hcnt + dcnt for c in row)}")
    print(f"    host loop    wall median {h:8.1f} us  min {hlo:8.1f}  p90 {hp:8.1f} | copies {3 * n} (three per member)")
    print(f"    device loop  wall median {v:8.1f} us  min {vlo:8.1f}  p90 {vp:8.1f} | launches {np.median(dl[skip:]):.0f}  copies {np.median(dc[skip:]):.0f}  waits {np.median(dwt[skip:]):.0f}")
    print(f"    member steps with other iterations or trials than the host loop: {differ} of {n * steps}; host / device wall {h / v:.2f}", flush=True)


def node_stages(nk):
    st, nxt = np.zeros(len(nk), dtype=int), 1
    for k, n in enumerate(np.asarray(nk, dtype=int)):
        st[nxt:nxt + n] = st[k] + 1
        nxt += n
    return st


def reference(x0, nu, rows):
    """a reference that shifts one stage per step: row t is 2 % of x0, entry i swinging with sin(0.2 t + i); inputs track zero"""
    t = np.arange(rows)[:, None]
    return 0.02 * x0[None, :] * np.sin(0.2 * t + np.arange(len(x0))[None, :]), np.zeros((rows, nu))


def tracking_single(capi, name, p, steps, skip):
    """root with states, clipping: the host loop folds the window in numpy (q = q0 - Qd xref, r = r0 - Rd uref, rows by stage) and
    hands everything to tqgpu_set_problem; the device loop is tqgpu_mpc_step_at"""
    L = capi.lib()
    d, x0 = full_root(capi, p)
    dp = lambda a: a.ctypes.data_as(capi.c_dbl_p)
    o, r = capi._gpu_opts(), capi.GpuResult()
    nu0, nx0, nx, nu = int(d["nu"][0]), len(x0), int(d["nx"][0]), int(d["nu"][0])
    st = node_stages(d["nk"])
    X, U = reference(x0, nu, steps + int(st.max()) + 1)
    stx, stu = np.repeat(st, d["nx"]), np.repeat(st, d["nu"])
    ix, iu = np.tile(np.arange(nx), len(st)), np.tile(np.arange(nu), int((np.asarray(d["nu"]) > 0).sum()))
    xs = [moved_inward(x0, k, 0) for k in range(steps)]
    g = capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)
    g.set_warm_start(1)
    keep = {k: np.ascontiguousarray(d[k], dtype=np.float64).copy() for k in ORDER}
    q0, r0 = keep["q"].copy(), keep["r"].copy()
    sol = [np.zeros(n) for n in (g.sum_nx, g.sum_nu, g.sum_lam, g.sum_nx, g.sum_nu, g.sum_lam)]
    sp = [dp(b) for b in sol]
    hw, hd, hl, hc, hcnt, hu = [], [], [], [], [], []
    for k, x in enumerate(xs):
        t0 = time.perf_counter()
        keep["xmin"][:nx0] = x
        keep["xmax"][:nx0] = x
        keep["q"][:] = q0 - keep["Qd"] * X[k + stx, ix]
        keep["r"][:] = r0 - keep["Rd"] * U[k + stu, iu]
        assert L.tqgpu_set_problem(g.h, *[dp(keep[n]) for n in ORDER], None) == 0
        assert L.tqgpu_solve(g.h, C.byref(o), C.byref(r)) == 0
        assert L.tqgpu_get_solution(g.h, *sp) == 0
        hw.append(time.perf_counter() - t0)
        hu.append(sol[1][:nu0].copy())
        hd.append(r.device_time); hl.append(r.n_launches + 2); hc.append(5); hcnt.append((r.status, r.iter, r.ls_total))      # (copies: q, r, the two bound arrays up, the solution down)
    g.close()
    g = capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)
    g.mpc_set_root_states()
    g.set_warm_start(1)
    g.mpc_set_tracking(X, U, q0, r0)
    u0 = np.zeros(max(nu0, 1))
    la, co, wa = C.c_int(), C.c_int(), C.c_int()
    dw, dd, dl, dc, dwt, dcnt, du = [], [], [], [], [], [], 0.0
    for k in range(steps):
        t0 = time.perf_counter()
        assert L.tqgpu_mpc_step_at(g.h, dp(xs[k]), k, C.byref(o), C.byref(r), dp(u0)) == 0
        dw.append(time.perf_counter() - t0)
        L.tqgpu_mpc_stats(C.byref(la), C.byref(co), C.byref(wa))
        dd.append(r.device_time); dl.append(la.value); dc.append(co.value); dwt.append(wa.value); dcnt.append((r.status, r.iter, r.ls_total))
        du = max(du, float(np.max(np.abs(u0[:nu0] - hu[k]))))
    kkt = g.kkt_residual()["max"]
    g.close()
    differ = sum(a != b for a, b in zip(hcnt, dcnt))
    print(f"{name}, tracking, root with states: {len(d['nk'])} nodes, {steps} steps, iterations per step mean {np.mean([c[1] for c in hcnt]):.2f} / {np.mean([c[1] for c in dcnt]):.2f}, "
          f"trials per step mean {np.mean([c[2] for c in hcnt]):.2f} / {np.mean([c[2] for c in dcnt]):.2f} (host / device), all status 0: {all(c[0] == 0 for c in hcnt + dcnt)}")
    h = report("host loop", hw, hd, hl, hc, skip)
    v = report("device loop", dw, dd, dl, dc, skip)
    print(f"    device loop waits per step {np.median(dwt[skip:]):.0f}; steps with other iterations or trials than the host loop: {differ} of {steps}; "
          f"largest |u0 (device) - u0 (host)| {du:.2e}; KKT of the last device step {kkt:.2e}; host / device wall {h / v:.2f}", flush=True)


def tracking_batch(capi, p, n, steps, skip):
    L = capi.lib()
    d, x0 = full_root(capi, p)
    dp = lambda a: a.ctypes.data_as(capi.c_dbl_p)
    o = capi._gpu_opts()
    nu0, nx0, nx, nu = int(d["nu"][0]), len(x0), int(d["nx"][0]), int(d["nu"][0])
    st = node_stages(d["nk"])
    X, U = reference(x0, nu, steps + n + int(st.max()) + 1)
    stx, stu = np.repeat(st, d["nx"]), np.repeat(st, d["nu"])
    ix, iu = np.tile(np.arange(nx), len(st)), np.tile(np.arange(nu), int((np.asarray(d["nu"]) > 0).sum()))
    mk = lambda: [capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d) for _ in range(n)]
    xs = [[moved_inward(x0, k, i) for i in range(n)] for k in range(steps)]
    ms = mk()
    arr = (C.c_void_p * n)(*[m.h for m in ms])
    res = (capi.GpuResult * n)()
    keeps = [{k: np.ascontiguousarray(d[k], dtype=np.float64).copy() for k in ORDER} for _ in range(n)]
    q0, r0 = keeps[0]["q"].copy(), keeps[0]["r"].copy()
    sols = [[np.zeros(s) for s in (ms[0].sum_nx, ms[0].sum_nu, ms[0].sum_lam, ms[0].sum_nx, ms[0].sum_nu, ms[0].sum_lam)] for _ in range(n)]
    for m in ms:
        m.set_warm_start(1)
    hw, hcnt = [], []
    for k in range(steps):
        t0 = time.perf_counter()
        for i in range(n):          # member i is i stages ahead along the same reference
            keeps[i]["xmin"][:nx0] = xs[k][i]
            keeps[i]["xmax"][:nx0] = xs[k][i]
            keeps[i]["q"][:] = q0 - keeps[i]["Qd"] * X[k + i + stx, ix]
            keeps[i]["r"][:] = r0 - keeps[i]["Rd"] * U[k + i + stu, iu]
            assert L.tqgpu_set_problem(ms[i].h, *[dp(keeps[i][q]) for q in ORDER], None) == 0
        assert L.tqgpu_solve_batch(arr, n, C.byref(o), res) == 0
        for i in range(n):
            assert L.tqgpu_get_solution(ms[i].h, *[dp(b) for b in sols[i]]) == 0
        hw.append(time.perf_counter() - t0)
        hcnt.append([(res[i].status, res[i].iter, res[i].ls_total) for i in range(n)])
    for m in ms:
        m.close()
    ms = mk()
    arr = (C.c_void_p * n)(*[m.h for m in ms])
    for m in ms:
        m.mpc_set_root_states()
        m.set_warm_start(1)
        m.mpc_set_tracking(X, U, q0, r0)
    u0s = np.zeros(n * max(nu0, 1))
    la, co, wa = C.c_int(), C.c_int(), C.c_int()
    dw, dl, dc, dwt, dcnt = [], [], [], [], []
    for k in range(steps):
        xk = np.ascontiguousarray(np.concatenate(xs[k]))
        t0s = np.arange(k, k + n, dtype=np.int32)
        t0 = time.perf_counter()
        assert L.tqgpu_mpc_step_batch_at(arr, n, dp(xk), t0s.ctypes.data_as(capi.c_int_p), C.byref(o), res, dp(u0s)) == 0
        dw.append(time.perf_counter() - t0)
        L.tqgpu_mpc_stats(C.byref(la), C.byref(co), C.byref(wa))
        dl.append(la.value); dc.append(co.value); dwt.append(wa.value)
        dcnt.append([(res[i].status, res[i].iter, res[i].ls_total) for i in range(n)])
    for m in ms:
        m.close()
    differ = sum(a != b for ha, da in zip(hcnt, dcnt) for a, b in zip(ha, da))
    h, hlo, hp = stats(hw[skip:])
    v, vlo, vp = stats(dw[skip:])
    mean = lambda cnt, j: np.mean([c[j] for row in cnt for c in row])
    print(f"batch, tracking, roots with states: {n} mirrors of c1, {steps} steps, iterations per member step mean {mean(hcnt, 1):.2f} / {mean(dcnt, 1):.2f}, trials {mean(hcnt, 2):.2f} / {mean(dcnt, 2):.2f} "
          f"(host / device), all status 0: {all(c[0] == 0 for row in hcnt + dcnt for c in row)}")
    print(f"    host loop    wall median {h:8.1f} us  min {hlo:8.1f}  p90 {hp:8.1f} | copies {5 * n} (five per member)")
    print(f"    device loop  wall median {v:8.1f} us  min {vlo:8.1f}  p90 {vp:8.1f} | launches {np.median(dl[skip:]):.0f}  copies {np.median(dc[skip:]):.0f}  waits {np.median(dwt[skip:]):.0f}")
    print(f"    member steps with other iterations or trials than the host loop: {differ} of {n * steps}; host / device wall {h / v:.2f}", flush=True)


def kind3_tree(seed=7, span=0.0625):
    """85 nodes (1 + 4 + 16 + 64, nx = 2, nu = 1: the shape of tests/gen_cases.scaled_one_row) with dense data that converge
    (helpers.dense_shaped_qp): the 21 parents are kind-3 nodes with one row each, C x + D u within +- span (C = 0 on the root, whose
    states are fixed), the leaves kind 2"""
    import helpers as H
    import limit_shapes as S
    shape = (2, 1, [(2, 1, [(2, 1, [S.leaf(2)] * 4)] * 4)] * 4)
    nk, nx, nu = S.flatten(shape)
    d = H.dense_shaped_qp(nk, nx, nu, seed)
    kinds = np.where(nk > 0, 3, 2).astype(np.int32)
    rng = np.random.Generator(np.random.PCG64(seed + 5))
    n3 = int((nk > 0).sum())
    d["nc"] = (nk > 0).astype(np.int32)
    d["C"] = 0.25 * rng.standard_normal(2 * n3)
    d["C"][:2] = 0.0
    d["D"] = 0.5 + np.abs(rng.standard_normal(n3))
    d["dmin"], d["dmax"] = -span * np.ones(n3), span * np.ones(n3)
    return d, kinds


def tracking_kind3(capi, steps, skip):
    """the 85-node tree of kind3_tree (21 kind-3 nodes): the reference moves one stage per step, x0 stays.  Host loop: vectorised numpy
    fold over the dense blocks, upload_mixed with the last duals (the only way to move r on a dense tree before
    tqgpu_set_linear_terms; tqgpu_set_objective_mixed empties the stored working sets), solve, download.  Device loop:
    tqgpu_mpc_step_at with warm start 1, download."""
    import solve_sequence_cases as SC
    import tracking_cases as K
    d, kinds = kind3_tree()
    nk = np.asarray(d["nk"])
    n3, Np = int((kinds == 3).sum()), int((nk > 0).sum())
    assert np.all(nk[:Np] > 0) and np.all(nk[Np:] == 0)          # breadth first: the parents come first
    st = node_stages(nk)
    t = np.arange(steps + int(st.max()) + 1)[:, None]
    X = 0.05 * np.sin(0.2 * t + np.arange(2)[None, :])
    U = 0.05 * np.sin(0.2 * t + 1.0 + np.arange(1)[None, :])
    Hp = np.stack([np.block([[Q, S_.T], [S_, R_]]) for Q, R_, S_ in (K.blocks(d, k) for k in range(Np))])
    Hl = np.stack([K.blocks(d, k)[0] for k in range(Np, len(nk))])
    q0, r0 = np.array(d["q"], copy=True), np.array(d["r"], copy=True)
    opts = dict(SC.FULL)

    def host_fold(k):
        vp = np.einsum("nij,nj->ni", Hp, np.concatenate([X[k + st[:Np]], U[k + st[:Np]]], axis=1))
        vl = np.einsum("nij,nj->ni", Hl, X[k + st[Np:]])
        return q0 - np.concatenate([vp[:, :2].ravel(), vl.ravel()]), r0 - vp[:, 2:].ravel()

    def mirror():
        g = capi.TqGpu(d["nk"], d["nx"], d["nu"])
        g.set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"])
        g.upload_mixed(d, kinds, None)
        g.set_warm_start(1)
        return g

    qk, rk = host_fold(3)
    qn, rn = K.fold(dict(d=d, form="states", T=len(X), q0=q0, r0=r0, xtraj=X, utraj=U), 3)
    assert np.allclose(qk, qn, rtol=0, atol=1e-14) and np.allclose(rk, rn, rtol=0, atol=1e-14)
    out = {}
    for how in ("host loop", "device loop"):
        g = mirror()
        if how == "device loop":
            g.mpc_set_root_states()
            g.mpc_set_tracking(X, U, q0, r0)
        w, cnt, act, st_, lam, usum = [], [], [], [], None, []
        for k in range(steps):
            t0 = time.perf_counter()
            if how == "host loop":
                q, r = host_fold(k)
                g.upload_mixed(dict(d, q=q, r=r), kinds, lam)
                res = g.solve(**opts)
            else:
                res, _ = g.mpc_step(None, t0=k, **opts)
                st_.append(capi.mpc_stats())
            sol = g.solution()
            w.append(time.perf_counter() - t0)
            lam = sol["lam"]
            usum.append(sol["u"].copy())
            cnt.append((res["status"], res["iter"], res["ls_total"], res["n_launches"]))
            act.append(float(g.stage_steps()["total"].sum()) / (n3 * (res["ls_total"] + 1)))
        rows = int(np.count_nonzero(sol["mu_d"]))
        g.close()
        out[how] = (w, cnt, act, usum, rows, st_)
    hc, dc = out["host loop"][1], out["device loop"][1]
    differ = sum(a[:3] != b[:3] for a, b in zip(hc, dc))
    du = max(float(np.max(np.abs(a - b))) for a, b in zip(out["host loop"][3], out["device loop"][3]))
    print(f"kind3, tracking: 85 nodes, {n3} of kind 3 with one row each, {steps} steps; steps with other iterations or trials than the host loop: {differ} of {steps}; "
          f"largest |u (device) - u (host)| {du:.2e}; rows active at the last solution {out['host loop'][4]} / {out['device loop'][4]}")
    for how, (w, cnt, act, _, _, st_) in out.items():
        med, lo, p90 = stats(w[skip:])
        extra = f" | step launches {np.median([s['launches'] for s in st_[skip:]]):.0f} copies {np.median([s['copies'] for s in st_[skip:]]):.0f} waits {np.median([s['waits'] for s in st_[skip:]]):.0f}" if st_ else ""
        print(f"    {how:12s} wall median {med:9.1f} us  min {lo:9.1f}  p90 {p90:9.1f} | iterations mean {np.mean([c[1] for c in cnt[skip:]]):.2f}  trials mean {np.mean([c[2] for c in cnt[skip:]]):.2f}  "
              f"solve launches median {np.median([c[3] for c in cnt[skip:]]):.0f} | status 0 in {sum(c[0] == 0 for c in cnt)} of {steps} | "
              f"active-set steps per kind-3 node and sweep (ls_total + 1 sweeps) {np.mean(act[skip:]):.2f}{extra}", flush=True)


def shift_compare(capi, name, d, x0, steps, skip, kinds=None, opts=None, X=None, U=None, move_x0=True):
    """--shift: the same closed-loop sequences (root with states, tracking) three ways: warm start mode 2 (the shift on the device), mode 1
    (the unshifted copy), and the host loop that the API without the shift allows: tqgpu_get_solution, numpy gather, tqgpu_set_lambda,
    tqgpu_mpc_step_at.  The realised child cycles through the root's children.  Two sequences: `moving` (the reference shifts one stage
    per step, x0 on its prescribed path) and `standing` (a setpoint and a fixed x0: the same QP at every step, where the unshifted duals
    are the solution already and a shift can only displace them)."""
    L = capi.lib()
    import shift_cases as SH
    dp = lambda a: a.ctypes.data_as(capi.c_dbl_p)
    opts = opts or {}
    o, r = capi._gpu_opts(**opts), capi.GpuResult()
    nk, nx = np.asarray(d["nk"]), np.asarray(d["nx"])
    nk0, nu0 = int(nk[0]), int(d["nu"][0])
    n3 = 0 if kinds is None else int((kinds == 3).sum())
    st = node_stages(nk)
    if X is None:
        X, U = reference(x0, int(d["nu"][0]), steps + int(st.max()) + 1)
    # the host gather as one fancy index: entry i of the start duals (nodes 1 ..) from entry src[j][i] of the last, or 0.0
    off = np.concatenate([[0], np.cumsum(nx[1:])])
    src = []
    for j in range(nk0):
        img = SH.ref_map(nk, nx, j, SH.REPEAT)[0]
        s = np.full(int(nx[1:].sum()), -1, dtype=np.int64)
        for k in range(1, len(nk)):
            if img[k] >= 1:
                s[off[k - 1]:off[k - 1] + nx[k]] = off[img[k] - 1] + np.arange(nx[k])
        src.append(s)

    def mirror():
        g = capi.TqGpu(d["nk"], d["nx"], d["nu"])
        if kinds is None:
            g.upload(d)
        else:
            g.set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"])
            g.upload_mixed(d, kinds, None)
        g.mpc_set_root_states()
        return g

    ways = [("mode 2", 2, capi.SHIFT_DUALS)] + ([("mode 2 + sets", 2, capi.SHIFT_DUALS | capi.SHIFT_WORKING_SETS)] if n3 else []) + [("mode 1", 1, 0), ("host shift", 0, 0)]
    for seq in ("moving", "standing"):
        xs = [moved_inward(x0, k, 0) if seq == "moving" and move_x0 else x0 for k in range(steps)]
        print(f"{name}, --shift, sequence `{seq}`: {len(nk)} nodes, {steps} steps, realised child k mod {nk0}", flush=True)
        base = None
        for how, mode, what in ways:
            g = mirror()
            g.mpc_set_tracking(X if seq == "moving" else X[:1], U if seq == "moving" else U[:1], d["q"], d["r"])
            if what:
                g.mpc_set_shift(SH.REPEAT, what)
            g.set_warm_start(mode)
            sol = [np.zeros(n) for n in (g.sum_nx, g.sum_nu, g.sum_lam, g.sum_nx, g.sum_nu, g.sum_lam)]
            sp = [dp(b) for b in sol]
            start = np.zeros(g.sum_lam)
            u0 = np.zeros(max(nu0, 1))
            w, cnt, act = [], [], []
            for k in range(steps):
                j = k % nk0
                t0 = time.perf_counter()
                if k > 0 and how == "host shift":
                    assert L.tqgpu_get_solution(g.h, *sp) == 0
                    np.take(sol[2], src[j], out=start, mode="clip")
                    start[src[j] < 0] = 0.0
                    assert L.tqgpu_set_lambda(g.h, dp(start)) == 0
                elif mode == 2:
                    assert L.tqgpu_mpc_set_realised(g.h, j) == 0
                assert L.tqgpu_mpc_step_at(g.h, dp(np.ascontiguousarray(xs[k])), k, C.byref(o), C.byref(r), dp(u0)) == 0, L.tqgpu_last_error()
                w.append(time.perf_counter() - t0)
                cnt.append((r.status, r.iter, r.ls_total))
                if n3:
                    act.append(float(g.stage_steps()["total"].sum()) / (n3 * (r.ls_total + 1)))
            g.close()
            med, lo, p90 = stats(w[skip:])
            if how == "host shift":
                same = sum(a == b for a, b in zip(cnt, base))
                tail = f" | steps with the counts of mode 2: {same} of {steps}; mode 2 / host shift wall {base_med / med:.2f}"
            else:
                tail = ""
            if how == "mode 2":
                base, base_med = cnt, med
            extra = f" | active-set steps per kind-3 node and sweep {np.mean(act[skip:]):.2f}" if n3 else ""
            print(f"    {how:14s} wall median {med:8.1f} us  min {lo:8.1f}  p90 {p90:8.1f} | iterations per step mean {np.mean([c[1] for c in cnt[skip:]]):.2f}  "
                  f"trials per step mean {np.mean([c[2] for c in cnt[skip:]]):.2f} | status 0 in {sum(c[0] == 0 for c in cnt)} of {steps}{extra}{tail}", flush=True)


def gain_compare(capi, name, p, root_states, steps, skip, h=2.0 ** -20):
    """--gain: per step of the device loop (warm start mode 1, the x0 path of the plain modes) the time of tqgpu_mpc_sensitivity behind
    the step, against the only way the API without it has to the gain: nx0 more steps at x0 + h e_j through tqgpu_mpc_step (each a fold
    and a solve from the last duals), K[:, j] = (u0_j - u0) / h.  Both are timed around their calls with the host clock, interleaved
    step by step on one mirror each; launches, copies and waits are those tqgpu_mpc_stats counts (summed over the nx0 steps)."""
    L = capi.lib()
    dp = lambda a: a.ctypes.data_as(capi.c_dbl_p)
    o, r = capi._gpu_opts(), capi.GpuResult()
    if root_states:
        d, x0 = full_root(capi, p)
        xs = [moved_inward(x0, k, 0) for k in range(steps)]
    else:
        d, A0, b0, _, x0 = eliminated(capi, p)
        xs = [moved(x0, k, 0) for k in range(steps)]

    def mirror():
        g = capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)
        if root_states:
            g.mpc_set_root_states()
        else:
            g.mpc_set_root(A0, b0)
        g.set_warm_start(1)
        return g

    nu0, nx0 = int(d["nu"][0]), len(x0)
    u0, uj, K = np.zeros(max(nu0, 1)), np.zeros(max(nu0, 1)), np.zeros(nu0 * nx0)
    la, co, wa, nreg = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    gs, gf = mirror(), mirror()
    tw, ts, tf, cs, cf, dk, regs = [], [], [], [], [], 0.0, 0
    for k in range(steps):
        t0 = time.perf_counter()
        assert L.tqgpu_mpc_step(gs.h, dp(xs[k]), C.byref(o), C.byref(r), dp(u0)) == 0
        t1 = time.perf_counter()
        assert L.tqgpu_mpc_sensitivity(gs.h, C.byref(o), C.byref(nreg)) == 0, L.tqgpu_last_error()
        t2 = time.perf_counter()
        L.tqgpu_mpc_stats(C.byref(la), C.byref(co), C.byref(wa))
        assert L.tqgpu_mpc_get_gain(gs.h, dp(K), None, None) == 0
        tw.append(t1 - t0); ts.append(t2 - t1); cs.append((la.value, co.value, wa.value)); regs += nreg.value
        # finite differences on the twin: its own step first (not timed: both ways pay it), then nx0 steps, each from the duals of the one before
        assert L.tqgpu_mpc_step(gf.h, dp(xs[k]), C.byref(o), C.byref(r), dp(u0)) == 0
        Kfd, cnt = np.zeros((nu0, nx0)), np.zeros(3, dtype=int)
        t0 = time.perf_counter()
        for j in range(nx0):
            xj = xs[k].copy()
            xj[j] += h
            assert L.tqgpu_mpc_step(gf.h, dp(xj), C.byref(o), C.byref(r), dp(uj)) == 0
            L.tqgpu_mpc_stats(C.byref(la), C.byref(co), C.byref(wa))
            cnt += (la.value, co.value, wa.value)
            Kfd[:, j] = (uj[:nu0] - u0[:nu0]) / h
        tf.append(time.perf_counter() - t0); cf.append(tuple(cnt))
        dk = max(dk, float(np.max(np.abs(K.reshape((nu0, nx0), order="F") - Kfd))))
    gs.close(); gf.close()
    med = lambda v: tuple(int(np.median([c[i] for c in v[skip:]])) for i in range(3))
    form = "root with states" if root_states else "x0 eliminated"
    print(f"{name}, --gain, {form}: {len(d['nk'])} nodes, nx0 {nx0}, nu[0] {nu0}, {steps} steps; blocks regularised over the run {regs}")
    for what, t, c in (("step", tw, None), ("sensitivity", ts, cs), (f"{nx0} FD steps", tf, cf)):
        m, lo, p90 = stats(t[skip:])
        tail = "" if c is None else "  | launches %d  copies %d  waits %d" % med(c)
        print(f"    {what:14s} wall median {m:8.1f} us  min {lo:8.1f}  p90 {p90:8.1f}{tail}", flush=True)
    print(f"    FD / sensitivity wall {np.median(tf[skip:]) / np.median(ts[skip:]):.2f}; largest |K - K_fd| over the run {dk:.2e} (h = 2^-20; the two differ "
          f"where a step at x0 + h e_j changes the active set or stops at the tolerance)", flush=True)


def adjoint_compare(capi, name, p, root_states, steps, skip):
    """--adjoint: per step of the device loop (warm start mode 1, the x0 path of the plain modes), three ways to a gradient of a scalar
    loss with dL/dz = w, one random w per step, each on a mirror of its own and timed around its calls with the host clock:
    (a) tqgpu_mpc_adjoint + tqgpu_mpc_get_adjoint_x0: dL/dx0, with dL/dq, dL/dr, dL/db left on the device;
    (b) tqgpu_mpc_sensitivity + tqgpu_mpc_get_sensitivities + the host product dZ' w: the only way to dL/dx0 without the adjoint;
    (c) tqgpu_mpc_adjoint after tqgpu_mpc_sensitivity (not timed), which finds the factor stored.
    Launches, copies and waits of (a) and (c) are those tqgpu_mpc_stats counts; (b): the sensitivity's counted ones plus what
    tqgpu_mpc_get_sensitivities adds by its code, which nothing counts: two copies (dx, du) and one stream synchronisation."""
    L = capi.lib()
    dp = lambda a: a.ctypes.data_as(capi.c_dbl_p)
    o, r = capi._gpu_opts(), capi.GpuResult()
    if root_states:
        d, x0 = full_root(capi, p)
        xs = [moved_inward(x0, k, 0) for k in range(steps)]
    else:
        d, A0, b0, _, x0 = eliminated(capi, p)
        xs = [moved(x0, k, 0) for k in range(steps)]

    def mirror():
        g = capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)
        if root_states:
            g.mpc_set_root_states()
        else:
            g.mpc_set_root(A0, b0)
        g.set_warm_start(1)
        return g

    nu0, nx0 = int(d["nu"][0]), len(x0)
    ga, gb_, gc = mirror(), mirror(), mirror()
    snx, snu = int(ga.sum_nx), int(ga.sum_nu)
    u0 = np.zeros(max(nu0, 1))
    gx = [np.zeros(nx0) for _ in range(3)]
    dx, du = np.zeros(snx * nx0), np.zeros(snu * nx0)
    la, co, wa, nreg = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rng = np.random.Generator(np.random.PCG64(2020))
    t = {k: [] for k in "abc"}
    c = {k: [] for k in "abc"}
    dab, dac, regs = 0.0, 0.0, 0

    def counted(extra=(0, 0, 0)):
        L.tqgpu_mpc_stats(C.byref(la), C.byref(co), C.byref(wa))
        return la.value + extra[0], co.value + extra[1], wa.value + extra[2]

    for k in range(steps):
        wx, wu = rng.standard_normal(snx), rng.standard_normal(snu)
        for g in (ga, gb_, gc):
            assert L.tqgpu_mpc_step(g.h, dp(xs[k]), C.byref(o), C.byref(r), dp(u0)) == 0
        t0 = time.perf_counter()
        assert L.tqgpu_mpc_adjoint(ga.h, C.byref(o), dp(wx), dp(wu), 1, C.byref(nreg)) == 0, L.tqgpu_last_error()
        assert L.tqgpu_mpc_get_adjoint_x0(ga.h, dp(gx[0])) == 0
        t["a"].append(time.perf_counter() - t0); c["a"].append(counted()); regs += nreg.value
        t0 = time.perf_counter()
        assert L.tqgpu_mpc_sensitivity(gb_.h, C.byref(o), C.byref(nreg)) == 0, L.tqgpu_last_error()
        cb = counted((0, 2, 1))
        assert L.tqgpu_mpc_get_sensitivities(gb_.h, dp(dx), dp(du), None) == 0
        gx[1][:] = dx.reshape((snx, nx0), order="F").T @ wx + du.reshape((snu, nx0), order="F").T @ wu
        t["b"].append(time.perf_counter() - t0); c["b"].append(cb)
        assert L.tqgpu_mpc_sensitivity(gc.h, C.byref(o), C.byref(nreg)) == 0, L.tqgpu_last_error()
        t0 = time.perf_counter()
        assert L.tqgpu_mpc_adjoint(gc.h, C.byref(o), dp(wx), dp(wu), 1, C.byref(nreg)) == 0, L.tqgpu_last_error()
        assert L.tqgpu_mpc_get_adjoint_x0(gc.h, dp(gx[2])) == 0
        t["c"].append(time.perf_counter() - t0); c["c"].append(counted())
        scale = max(1.0, float(np.max(np.abs(gx[1]))))
        dab, dac = max(dab, float(np.max(np.abs(gx[0] - gx[1]))) / scale), max(dac, float(np.max(np.abs(gx[0] - gx[2]))))
    for g in (ga, gb_, gc):
        g.close()
    med = lambda v: tuple(int(np.median([e[i] for e in v[skip:]])) for i in range(3))
    form = "root with states" if root_states else "x0 eliminated"
    print(f"{name}, --adjoint, {form}: {len(d['nk'])} nodes, nx0 {nx0}, nu[0] {nu0}, {steps} steps; blocks regularised over the run of (a) {regs}")
    for key, what in (("a", "(a) adjoint"), ("b", "(b) sensitivity + dZ' w"), ("c", "(c) adjoint, factor stored")):
        m, lo, p90 = stats(t[key][skip:])
        print(f"    {what:28s} wall median {m:8.1f} us  min {lo:8.1f}  p90 {p90:8.1f}  | launches %d  copies %d  waits %d" % med(c[key]), flush=True)
    print(f"    ((b): the sensitivity's counted launches, copies, waits + 0, 2, 1 for tqgpu_mpc_get_sensitivities, derived from its code, not counted)")
    print(f"    (b) / (a) wall {np.median(t['b'][skip:]) / np.median(t['a'][skip:]):.2f}; (b) / (c) wall {np.median(t['b'][skip:]) / np.median(t['c'][skip:]):.2f}; "
          f"largest |gx0 (a) - gx0 (b)| / max(1, |gx0|) over the run {dab:.2e}; largest |gx0 (a) - gx0 (c)| {dac:.2e}", flush=True)


def adjoint_batch_compare(capi, name, p, root_states, n, steps, skip):
    """--adjoint-batch N: behind every tqgpu_mpc_step_batch of N trees (warm start mode 1), one random w per member and two ways to the
    members' gradients, each on N mirrors of its own, stepped alike, and timed around its calls with the host clock:
    (a) one tqgpu_mpc_adjoint_batch;
    (b) N calls of tqgpu_mpc_adjoint + tqgpu_mpc_get_adjoint_x0, member after member.
    Launches, copies and waits are those tqgpu_mpc_stats counts ((b): summed over the N calls).  The largest difference of gx0 between
    the two must be 0: a member's arithmetic is the same."""
    L = capi.lib()
    dp = lambda a: a.ctypes.data_as(capi.c_dbl_p)
    o = capi._gpu_opts()
    if root_states:
        d, x0 = full_root(capi, p)
        xs = [np.concatenate([moved_inward(x0, k, i) for i in range(n)]) for k in range(steps)]
    else:
        d, A0, b0, _, x0 = eliminated(capi, p)
        xs = [np.concatenate([moved(x0, k, i) for i in range(n)]) for k in range(steps)]

    def mirror():
        g = capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)
        if root_states:
            g.mpc_set_root_states()
        else:
            g.mpc_set_root(A0, b0)
        g.set_warm_start(1)
        return g

    nu0, nx0 = int(d["nu"][0]), len(x0)
    ga, gb_ = [mirror() for _ in range(n)], [mirror() for _ in range(n)]
    arr = {k: (C.c_void_p * n)(*[m.h for m in v]) for k, v in (("a", ga), ("b", gb_))}
    res = (capi.GpuResult * n)()
    snx, snu = int(ga[0].sum_nx), int(ga[0].sum_nu)
    u0 = np.zeros(max(nu0 * n, 1))
    gxa, gxb = np.zeros(nx0 * n), np.zeros(nx0 * n)
    nregs = np.zeros(n, dtype=np.int32)
    la, co, wa, nreg = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rng = np.random.Generator(np.random.PCG64(2121))
    t = {k: [] for k in "ab"}
    c = {k: [] for k in "ab"}
    dab, regs, bad = 0.0, 0, 0

    def counted():
        L.tqgpu_mpc_stats(C.byref(la), C.byref(co), C.byref(wa))
        return la.value, co.value, wa.value

    for k in range(steps):
        wx, wu = rng.standard_normal(snx * n), rng.standard_normal(snu * n)
        for key in "ab":
            assert L.tqgpu_mpc_step_batch(arr[key], n, dp(xs[k]), C.byref(o), res, dp(u0)) == 0, L.tqgpu_last_error()
            bad += sum(res[i].status != 0 for i in range(n))
        t0 = time.perf_counter()
        assert L.tqgpu_mpc_adjoint_batch(arr["a"], n, C.byref(o), dp(wx), dp(wu), 1, dp(gxa), capi._ip(nregs)) == 0, L.tqgpu_last_error()
        t["a"].append(time.perf_counter() - t0); c["a"].append(counted()); regs += int(nregs.sum())
        t0 = time.perf_counter()
        tot = np.zeros(3, dtype=int)
        for i, g in enumerate(gb_):
            assert L.tqgpu_mpc_adjoint(g.h, C.byref(o), dp(wx[i * snx:]), dp(wu[i * snu:]), 1, C.byref(nreg)) == 0, L.tqgpu_last_error()
            assert L.tqgpu_mpc_get_adjoint_x0(g.h, dp(gxb[i * nx0:])) == 0
            tot += counted()
        t["b"].append(time.perf_counter() - t0); c["b"].append(tuple(tot))
        dab = max(dab, float(np.max(np.abs(gxa - gxb))))
    for g in ga + gb_:
        g.close()
    med = lambda v: tuple(int(np.median([e[i] for e in v[skip:]])) for i in range(3))
    form = "roots with states" if root_states else "x0 eliminated"
    print(f"{name}, --adjoint-batch {n}, {form}: {n} mirrors of {len(d['nk'])} nodes, nx0 {nx0}, {steps} steps; member steps with another status than 0: {bad}; "
          f"blocks regularised over the run of (a) {regs}")
    for key, what in (("a", "(a) adjoint_batch"), ("b", f"(b) {n} x adjoint")):
        m, lo, p90 = stats(t[key][skip:])
        print(f"    {what:28s} wall median {m:8.1f} us  min {lo:8.1f}  p90 {p90:8.1f}  | launches %d  copies %d  waits %d" % med(c[key]), flush=True)
    print(f"    (b) / (a) wall {np.median(t['b'][skip:]) / np.median(t['a'][skip:]):.2f}; largest |gx0 (a) - gx0 (b)| over the run {dab:.2e}", flush=True)


def gain_batch_compare(capi, name, p, root_states, n, steps, skip):
    """--gain-batch N: behind every tqgpu_mpc_step_batch of N trees (warm start mode 1), the gains and the dual predictor two ways, each on
    N mirrors of its own, stepped alike, and timed around its calls with the host clock:
    (a) one tqgpu_mpc_sensitivity_batch and one tqgpu_mpc_predict_batch (x0 of the next step, duals = 1);
    (b) N calls of tqgpu_mpc_sensitivity and N of tqgpu_mpc_predict (duals = 1), member after member.
    Launches, copies and waits are those tqgpu_mpc_stats counts ((b): summed over the N calls).  The largest difference of K and of u0_pred
    between the two must be 0: a member's arithmetic is the same.  A third set of mirrors steps in mode 1 without the predictor: iterations
    per step of both.  With a library that lacks the batched calls (TREEQP_AMD_LIB naming an earlier build) only (b) and the third set run."""
    L = capi.lib()
    dp = lambda a: a.ctypes.data_as(capi.c_dbl_p)
    o = capi._gpu_opts()
    batched = hasattr(L, "tqgpu_mpc_sensitivity_batch")
    path = moved_inward if root_states else moved
    if root_states:
        d, x0 = full_root(capi, p)
    else:
        d, A0, b0, _, x0 = eliminated(capi, p)
    xs = [np.concatenate([path(x0, k, i) for i in range(n)]) for k in range(steps + 1)]

    def mirror():
        g = capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)
        if root_states:
            g.mpc_set_root_states()
        else:
            g.mpc_set_root(A0, b0)
        g.set_warm_start(1)
        return g

    nu0, nx0 = int(d["nu"][0]), len(x0)
    legs = ("a", "b", "c") if batched else ("b", "c")
    gs = {key: [mirror() for _ in range(n)] for key in legs}
    arr = {key: (C.c_void_p * n)(*[m.h for m in v]) for key, v in gs.items()}
    res = (capi.GpuResult * n)()
    u0 = np.zeros(max(nu0 * n, 1))
    K = {key: np.zeros(max(nu0 * nx0 * n, 1)) for key in "ab"}
    up = {key: np.zeros(max(nu0 * n, 1)) for key in "ab"}
    nregs, ncl = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    la, co, wa, nreg, nc1 = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
    t = {key: [] for key in ("step", "a_sens", "a_pred", "b_sens", "b_pred")}
    c = {key: [] for key in ("a_sens", "a_pred", "b_sens", "b_pred")}
    iters = {key: [] for key in legs}
    dK, dU, regs, bad = 0.0, 0.0, 0, 0

    def counted():
        L.tqgpu_mpc_stats(C.byref(la), C.byref(co), C.byref(wa))
        return la.value, co.value, wa.value

    for k in range(steps):
        for key in legs:
            t0 = time.perf_counter()
            assert L.tqgpu_mpc_step_batch(arr[key], n, dp(xs[k]), C.byref(o), res, dp(u0)) == 0, L.tqgpu_last_error()
            if key == legs[0]:
                t["step"].append(time.perf_counter() - t0)
            bad += sum(res[i].status != 0 for i in range(n))
            iters[key].append(np.mean([res[i].iter for i in range(n)]))
        if batched:
            t0 = time.perf_counter()
            assert L.tqgpu_mpc_sensitivity_batch(arr["a"], n, C.byref(o), capi._ip(nregs)) == 0, L.tqgpu_last_error()
            t["a_sens"].append(time.perf_counter() - t0); c["a_sens"].append(counted()); regs += int(nregs.sum())
            t0 = time.perf_counter()
            assert L.tqgpu_mpc_predict_batch(arr["a"], n, dp(xs[k + 1]), dp(up["a"]), 1, capi._ip(ncl)) == 0, L.tqgpu_last_error()
            t["a_pred"].append(time.perf_counter() - t0); c["a_pred"].append(counted())
            for i, g in enumerate(gs["a"]):
                assert L.tqgpu_mpc_get_gain(g.h, dp(K["a"][i * nu0 * nx0:]), None, None) == 0
        t0 = time.perf_counter()
        tot = np.zeros(3, dtype=int)
        for g in gs["b"]:
            assert L.tqgpu_mpc_sensitivity(g.h, C.byref(o), C.byref(nreg)) == 0, L.tqgpu_last_error()
            tot += counted()
        t["b_sens"].append(time.perf_counter() - t0); c["b_sens"].append(tuple(tot))
        t0 = time.perf_counter()
        tot = np.zeros(3, dtype=int)
        for i, g in enumerate(gs["b"]):
            assert L.tqgpu_mpc_predict(g.h, dp(xs[k + 1][i * nx0:]), dp(up["b"][i * nu0:]), 1, C.byref(nc1)) == 0, L.tqgpu_last_error()
            tot += counted()
        t["b_pred"].append(time.perf_counter() - t0); c["b_pred"].append(tuple(tot))
        for i, g in enumerate(gs["b"]):
            assert L.tqgpu_mpc_get_gain(g.h, dp(K["b"][i * nu0 * nx0:]), None, None) == 0
        if batched:
            dK = max(dK, float(np.max(np.abs(K["a"] - K["b"])))); dU = max(dU, float(np.max(np.abs(up["a"] - up["b"]))))
    for v in gs.values():
        for g in v:
            g.close()
    med = lambda v: tuple(int(np.median([e[i] for e in v[skip:]])) for i in range(3))
    form = "roots with states" if root_states else "x0 eliminated"
    print(f"{name}, --gain-batch {n}, {form}: {n} mirrors of {len(d['nk'])} nodes, nx0 {nx0}, {steps} steps, library {os.environ.get('TREEQP_AMD_LIB', 'of this tree')}; "
          f"member steps with another status than 0: {bad}; blocks regularised over the run of (a) {regs}")
    m, lo, p90 = stats(t["step"][skip:])
    print(f"    {'batch step':36s} wall median {m:8.1f} us  min {lo:8.1f}  p90 {p90:8.1f}", flush=True)
    rows = [("a_sens", "(a) sensitivity_batch"), ("a_pred", "(a) predict_batch, duals")] if batched else []
    for key, what in rows + [("b_sens", f"(b) {n} x sensitivity"), ("b_pred", f"(b) {n} x predict, duals")]:
        m, lo, p90 = stats(t[key][skip:])
        print(f"    {what:36s} wall median {m:8.1f} us  min {lo:8.1f}  p90 {p90:8.1f}  | launches %d  copies %d  waits %d" % med(c[key]), flush=True)
    if batched:
        print(f"    (b) / (a) wall: sensitivity {np.median(t['b_sens'][skip:]) / np.median(t['a_sens'][skip:]):.2f}, predictor "
              f"{np.median(t['b_pred'][skip:]) / np.median(t['a_pred'][skip:]):.2f}; largest |K (a) - K (b)| over the run {dK:.2e}, largest |u0_pred (a) - u0_pred (b)| {dU:.2e}", flush=True)
    print("    iterations per step, mean over members and steps: " + ", ".join(
        f"{what} {np.mean(iters[key][skip:]):.2f}" for key, what in (("a", "(a) batched dual predictor"), ("b", "(b) single dual predictors"), ("c", "mode 1 alone")) if key in legs), flush=True)


def adjoint_matrices_compare(capi, name, p, root_states, n, steps, skip):
    """--adjoint-matrices [--adjoint-batch N]: behind every step and adjoint of n trees (n == 0: one tree through the single calls), two
    ways to the gradients of the matrices with one group for all dynamics and one for all stage Hessians of equal sizes (the leaves, and
    the root of an x0-eliminated tree, are groups of their own), summed over the members, on the same mirrors (the second leg only reads):
    (a) tqgpu_mpc_adjoint_matrices (n >= 1: tqgpu_mpc_adjoint_matrices_batch with reduce = 1);
    (b) the host route: per member tqgpu_get_solution + tqgpu_mpc_get_adjoint, then numpy outer products summed over nodes and members.
    Wall time is the host clock around each leg.  Launches, copies and waits of (a) are those tqgpu_mpc_stats counts; the calls of (b) are
    not counted there, their numbers are what the two calls do per member: 1 packing launch, 1 + 3 copies, 1 + 1 waits."""
    L = capi.lib()
    dp = lambda a: a.ctypes.data_as(capi.c_dbl_p)
    o = capi._gpu_opts()
    m = max(n, 1)
    if root_states:
        d, x0 = full_root(capi, p)
        xs = [np.concatenate([moved_inward(x0, k, i) for i in range(m)]) for k in range(steps)]
    else:
        d, A0, b0, _, x0 = eliminated(capi, p)
        xs = [np.concatenate([moved(x0, k, i) for i in range(m)]) for k in range(steps)]
    nk, nx, nu = [np.asarray(d[k], dtype=int) for k in ("nk", "nx", "nu")]
    Nn, nxx, nuu = len(nk), int(nx[1]), int(nu[1])
    dad = P_parents(nk)
    inner, leaves = np.flatnonzero((nk > 0) & (np.arange(Nn) > 0)), np.flatnonzero(nk == 0)
    assert np.all(nx[1:] == nxx) and np.all(nu[inner] == nuu) and int(nu[0]) == nuu, "a uniform tree is expected"
    hgroup = np.where(nk > 0, 0, 1).astype(np.int32)
    if not root_states:
        hgroup[0] = 2          # the root of an x0-eliminated tree has other sizes
    cgroup = np.zeros(Nn, dtype=np.int32)
    cgroup[0] = -1

    def mirror():
        g = capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)
        if root_states:
            g.mpc_set_root_states()
        else:
            g.mpc_set_root(A0, b0)
        g.set_warm_start(1)
        g.mpc_set_param_groups(hgroup, cgroup)
        return g

    gs = [mirror() for _ in range(m)]
    arr = (C.c_void_p * m)(*[g.h for g in gs])
    res = (capi.GpuResult * m)()
    snx, snu, snl = int(gs[0].sum_nx), int(gs[0].sum_nu), int(gs[0].sum_lam)
    nx0, nu0 = len(x0), int(nu[0])
    dims = np.zeros(4, dtype=np.int32)
    cd = np.zeros(4, dtype=np.int32)
    assert L.tqgpu_mpc_get_param_groups(gs[0].h, None, None, None, capi._ip(cd), capi._ip(dims)) == 0
    nxp = int(cd[1])          # the device's count: the phantom root states of an embedded tree are columns of gA
    gA, gB, gb = np.zeros(nxx * nxp), np.zeros(nxx * nuu), np.zeros(nxx)
    nzi = nxx + nuu
    gH, gh = np.zeros(4 * (nzi + nxx + nxp + nuu)), np.zeros(4 * (nzi + nxx + nxp + nuu))
    gA0, gS0 = np.zeros(max(int(dims[0]) * nx0, 1)), np.zeros(max(nu0 * nx0, 1))
    u0 = np.zeros(max(nu0 * m, 1))
    gx, nregs, nreg = np.zeros(nx0 * m), np.zeros(m, dtype=np.int32), C.c_int()
    la, co, wa = C.c_int(), C.c_int(), C.c_int()
    x, u, lam = np.zeros(snx), np.zeros(snu), np.zeros(snl)
    gq, gr, gbn = np.zeros(snx), np.zeros(snu), np.zeros(snl)
    xoff = np.concatenate([[0], np.cumsum(nx)])
    rows_x = xoff[1] + np.arange((Nn - 1) * nxx).reshape((Nn - 1, nxx))          # nodes 1 .. Nn - 1 in the flat x
    par = dad[1:]
    rng = np.random.Generator(np.random.PCG64(2222))
    t = {k: [] for k in "ab"}
    cnt, dA, dB, dH, bad = [], 0.0, 0.0, 0.0, 0
    for k in range(steps):
        wx, wu = rng.standard_normal(snx * m), rng.standard_normal(snu * m)
        if n == 0:
            assert L.tqgpu_mpc_step(gs[0].h, dp(xs[k]), C.byref(o), res, dp(u0)) == 0, L.tqgpu_last_error()
            assert L.tqgpu_mpc_adjoint(gs[0].h, C.byref(o), dp(wx), dp(wu), 1, C.byref(nreg)) == 0, L.tqgpu_last_error()
        else:
            assert L.tqgpu_mpc_step_batch(arr, m, dp(xs[k]), C.byref(o), res, dp(u0)) == 0, L.tqgpu_last_error()
            assert L.tqgpu_mpc_adjoint_batch(arr, m, C.byref(o), dp(wx), dp(wu), 1, dp(gx), capi._ip(nregs)) == 0, L.tqgpu_last_error()
        bad += sum(res[i].status != 0 for i in range(m))
        t0 = time.perf_counter()
        if n == 0:
            rc = L.tqgpu_mpc_adjoint_matrices(gs[0].h, dp(gH), dp(gh), dp(gA), dp(gB), dp(gb), dp(gA0), dp(gS0))
        else:
            rc = L.tqgpu_mpc_adjoint_matrices_batch(arr, m, 1, dp(gH), dp(gh), dp(gA), dp(gB), dp(gb), dp(gA0), dp(gS0))
        t["a"].append(time.perf_counter() - t0)
        assert rc == 0, L.tqgpu_last_error()
        L.tqgpu_mpc_stats(C.byref(la), C.byref(co), C.byref(wa))
        cnt.append((la.value, co.value, wa.value))
        t0 = time.perf_counter()
        hA, hB, hHd = np.zeros((nxx, nxx)), np.zeros((nxx, nuu)), np.zeros(nzi)
        for g in gs:
            assert L.tqgpu_get_solution(g.h, dp(x), dp(u), dp(lam), None, None, None) == 0
            assert L.tqgpu_mpc_get_adjoint(g.h, dp(gq), dp(gr), dp(gbn)) == 0
            lamc, gbc = lam.reshape((Nn - 1, nxx)), gbn.reshape((Nn - 1, nxx))
            # the parents' x, gq (a root without states: zeros) and u, gr
            X, GQ = np.zeros((Nn, nxx)), np.zeros((Nn, nxx))
            X[1:], GQ[1:] = x[rows_x], gq[rows_x]
            if root_states:
                X[0], GQ[0] = x[:nxx], gq[:nxx]
            U, GR = u.reshape((-1, nuu)), gr.reshape((-1, nuu))          # the nodes with inputs are the first ones, level by level
            hA += lamc.T @ GQ[par] + gbc.T @ X[par]
            hB += lamc.T @ GR[par] + gbc.T @ U[par]
            hHd += np.concatenate([np.sum(GQ[inner] * X[inner], axis=0), np.sum(GR[inner] * U[inner], axis=0)])
            if root_states:
                hHd += np.concatenate([GQ[0] * X[0], GR[0] * U[0]])
        t["b"].append(time.perf_counter() - t0)
        dA = max(dA, float(np.max(np.abs(gA.reshape((nxx, nxp), order="F")[:, nxp - nxx:] - hA))))
        dB = max(dB, float(np.max(np.abs(gB.reshape((nxx, nuu), order="F") - hB))))
        dH = max(dH, float(np.max(np.abs(gH[:nzi] - hHd))))
    for g in gs:
        g.close()
    med = tuple(int(np.median([e[i] for e in cnt[skip:]])) for i in range(3))
    form = "roots with states" if root_states else "x0 eliminated"
    how = "tqgpu_mpc_adjoint_matrices" if n == 0 else f"tqgpu_mpc_adjoint_matrices_batch, reduce = 1, N = {n}"
    print(f"{name}, --adjoint-matrices, {form}: {m} mirror(s) of {Nn} nodes, {steps} steps, {how}; one c-group of {Nn - 1} nodes, h-groups of {len(inner) + (1 if root_states else 0)} "
          f"and {len(leaves)} nodes{'' if root_states else ' and the root'}; member steps with another status than 0: {bad}")
    ma, lo, p90 = stats(t["a"][skip:])
    print(f"    {'(a) device':34s} wall median {ma:8.1f} us  min {lo:8.1f}  p90 {p90:8.1f}  | launches %d  copies %d  waits %d" % med, flush=True)
    mb, lo, p90 = stats(t["b"][skip:])
    print(f"    {'(b) downloads + numpy, ' + str(m) + ' member(s)':34s} wall median {mb:8.1f} us  min {lo:8.1f}  p90 {p90:8.1f}  | launches %d  copies %d  waits %d (not counted by tqgpu_mpc_stats: per member 1, 1 + 3, 1 + 1)" % (m, 4 * m, 2 * m), flush=True)
    print(f"    (b) / (a) wall {np.median(t['b'][skip:]) / np.median(t['a'][skip:]):.2f}; largest |(a) - (b)| over the run: gA {dA:.2e}, gB {dB:.2e}, gHd of the inner nodes {dH:.2e}", flush=True)


def adjoint_bounds_compare(capi, name, p, root_states, steps, skip):
    """--adjoint-bounds: behind every step and adjoint of one tree, two ways to the gradients of the bounds summed over the h-groups of
    --adjoint-matrices (the inner nodes, the leaves, the root of an x0-eliminated tree), on the same mirror (the second leg only reads):
    (a) tqgpu_mpc_adjoint_bounds;
    (b) the host route: tqgpu_mpc_get_adjoint (gb = Y) + tqgpu_get_solution, then v = w - [Y; 0] + sum_c C_c' Y_c rebuilt with numpy from Y, A, B, w,
        kept where the solution equals a bound, summed per group.
    Wall time is the host clock around each leg.  Launches, copies and waits of (a) are those tqgpu_mpc_stats counts; the calls of (b) are
    not counted there, their numbers are what the two calls do: 1 packing launch, 1 + 3 copies, 1 + 1 waits."""
    L = capi.lib()
    dp = lambda a: a.ctypes.data_as(capi.c_dbl_p)
    o, res = capi._gpu_opts(), capi.GpuResult()
    if root_states:
        d, x0 = full_root(capi, p)
        xs = [moved_inward(x0, k, 0) for k in range(steps)]
    else:
        d, A0, b0, _, x0 = eliminated(capi, p)
        xs = [moved(x0, k, 0) for k in range(steps)]
    nk, nx, nu = [np.asarray(d[k], dtype=int) for k in ("nk", "nx", "nu")]
    Nn, nxx, nuu, nk0 = len(nk), int(nx[1]), int(nu[0]), int(nk[0])
    dad = P_parents(nk)
    inner = np.flatnonzero((nk > 0) & (np.arange(Nn) > 0))
    assert np.all(nx[1:] == nxx) and np.all(nu[inner] == nuu), "a uniform tree is expected"
    hgroup = np.where(nk > 0, 0, 1).astype(np.int32)
    if not root_states:
        hgroup[0] = 2
    g = capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)
    if root_states:
        g.mpc_set_root_states()
    else:
        g.mpc_set_root(A0, b0)
    g.set_warm_start(1)
    cg = np.full(Nn, -1, dtype=np.int32)
    g.mpc_set_param_groups(hgroup, cg)
    snx, snu, snl = int(g.sum_nx), int(g.sum_nu), int(g.sum_lam)
    nzi = nxx + nuu
    glb, gub = np.zeros(4 * (2 * nzi + nxx)), np.zeros(4 * (2 * nzi + nxx))
    # the children's [A B], child after child: the children of an eliminated root have no A
    first = 1 if root_states else 1 + nk0
    A3 = np.asarray(d["A"], dtype=np.float64).reshape((Nn - first, nxx, nxx)).transpose((0, 2, 1))
    B3 = np.asarray(d["B"], dtype=np.float64).reshape((Nn - 1, nuu, nxx)).transpose((0, 2, 1))
    par = dad[1:]
    xoff = int(nx[0])
    lo_b, hi_b = np.concatenate([d["xmin"], d["umin"]]), np.concatenate([d["xmax"], d["umax"]])
    x, u = np.zeros(snx), np.zeros(snu)
    gq, gr, Y = np.zeros(snx), np.zeros(snu), np.zeros(snl)
    u0, nreg = np.zeros(max(nuu, 1)), C.c_int()
    la, co, wa = C.c_int(), C.c_int(), C.c_int()
    rng = np.random.Generator(np.random.PCG64(2323))
    t = {k: [] for k in "ab"}
    cnt, dlo, dhi, bad, hits = [], 0.0, 0.0, 0, 0
    for k in range(steps):
        wx, wu = rng.standard_normal(snx), rng.standard_normal(snu)
        assert L.tqgpu_mpc_step(g.h, dp(xs[k]), C.byref(o), C.byref(res), dp(u0)) == 0, L.tqgpu_last_error()
        assert L.tqgpu_mpc_adjoint(g.h, C.byref(o), dp(wx), dp(wu), 1, C.byref(nreg)) == 0, L.tqgpu_last_error()
        bad += res.status != 0
        t0 = time.perf_counter()
        rc = L.tqgpu_mpc_adjoint_bounds(g.h, dp(glb), dp(gub))
        t["a"].append(time.perf_counter() - t0)
        assert rc == 0, L.tqgpu_last_error()
        L.tqgpu_mpc_stats(C.byref(la), C.byref(co), C.byref(wa))
        cnt.append((la.value, co.value, wa.value))
        t0 = time.perf_counter()
        assert L.tqgpu_get_solution(g.h, dp(x), dp(u), None, None, None, None) == 0
        assert L.tqgpu_mpc_get_adjoint(g.h, dp(gq), dp(gr), dp(Y)) == 0
        Yc = Y.reshape((Nn - 1, nxx))
        vx, vu = wx.copy(), wu.copy()
        vx[xoff:] -= Y
        VX, VU = np.zeros((Nn, nxx)), vu.reshape((-1, nuu))
        np.add.at(VX, par[first - 1:], np.einsum("eij,ei->ej", A3, Yc[first - 1:]))
        np.add.at(VU, par, np.einsum("eij,ei->ej", B3, Yc))
        vx[xoff:] += VX[1:].ravel()
        if root_states:
            vx[:xoff] += VX[0]
        v, z = np.concatenate([vx, vu]), np.concatenate([x, u])
        if root_states:          # the fold has put x0 into both bounds of the root's states
            lo_b[:nxx] = hi_b[:nxx] = xs[k]
        on_lo = z == lo_b
        hlo, hhi = np.where(on_lo, v, 0.0), np.where((z == hi_b) & ~on_lo, v, 0.0)
        sums = []
        for h in (hlo, hhi):
            HX, HU = h[xoff:snx].reshape((Nn - 1, nxx)), h[snx:].reshape((-1, nuu))
            # the nodes with inputs are the first ones, level by level; a root with states belongs to the group of the inner nodes
            sx, su = HX[inner - 1].sum(axis=0), HU[inner].sum(axis=0)
            sums.append(np.concatenate([sx + h[:nxx], su + HU[0]]) if root_states else np.concatenate([sx, su]))
        t["b"].append(time.perf_counter() - t0)
        hits += int(np.count_nonzero(hlo) + np.count_nonzero(hhi))
        dlo, dhi = max(dlo, float(np.max(np.abs(glb[:nzi] - sums[0])))), max(dhi, float(np.max(np.abs(gub[:nzi] - sums[1]))))
    g.close()
    med = tuple(int(np.median([e[i] for e in cnt[skip:]])) for i in range(3))
    form = "root with states" if root_states else "x0 eliminated"
    print(f"{name}, --adjoint-bounds, {form}: {Nn} nodes, {steps} steps; h-groups of the inner nodes, the leaves{'' if root_states else ' and the root'}; "
          f"entries on a bound per step {hits / steps:.1f}; steps with another status than 0: {bad}")
    ma, lo, p90 = stats(t["a"][skip:])
    print(f"    {'(a) tqgpu_mpc_adjoint_bounds':34s} wall median {ma:8.1f} us  min {lo:8.1f}  p90 {p90:8.1f}  | launches %d  copies %d  waits %d" % med, flush=True)
    mb, lo, p90 = stats(t["b"][skip:])
    print(f"    {'(b) downloads + numpy':34s} wall median {mb:8.1f} us  min {lo:8.1f}  p90 {p90:8.1f}  | launches 1  copies 4  waits 2 (not counted by tqgpu_mpc_stats: 1, 1 + 3, 1 + 1)", flush=True)
    print(f"    (b) / (a) wall {np.median(t['b'][skip:]) / np.median(t['a'][skip:]):.2f}; largest |(a) - (b)| over the run, the group of the inner nodes: glb {dlo:.2e}, gub {dhi:.2e}", flush=True)


def adjoint_reference_compare(capi, name, p, steps, skip):
    """--adjoint-reference --tracking: the closed loop of --tracking on a root with states (tqgpu_mpc_step_at moves the window a row per step), behind
    every step an adjoint, then two ways to dL/dxref, dL/duref of the rows the window reads, on the same mirror:
    (a) tqgpu_mpc_adjoint_reference;
    (b) the host route: tqgpu_mpc_get_adjoint, then numpy -H' gz (H diagonal: -Qd gq, -Rd gr) summed per row.
    Counts of (b) are what its one call does: 3 copies, 1 wait, not counted by tqgpu_mpc_stats."""
    L = capi.lib()
    dp = lambda a: a.ctypes.data_as(capi.c_dbl_p)
    o, res = capi._gpu_opts(), capi.GpuResult()
    d, x0 = full_root(capi, p)
    nk, nx, nu = [np.asarray(d[k], dtype=int) for k in ("nk", "nx", "nu")]
    Nn, nxx, nuu = len(nk), int(nx[0]), int(nu[0])
    st = node_stages(nk)
    deep = int(st.max())
    X, U = reference(x0, nuu, steps + deep + 1)
    xs = [moved_inward(x0, k, 0) for k in range(steps)]
    g = capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)
    g.mpc_set_root_states()
    g.set_warm_start(1)
    g.mpc_set_tracking(X, U, d["q"], d["r"])
    snx, snu, snl = int(g.sum_nx), int(g.sum_nu), int(g.sum_lam)
    Qd, Rd = np.asarray(d["Qd"], dtype=np.float64), np.asarray(d["Rd"], dtype=np.float64)
    stu = st[nu > 0]
    gxr, gur = np.zeros((deep + 1) * nxx), np.zeros((deep + 1) * nuu)
    gq, gr, gb = np.zeros(snx), np.zeros(snu), np.zeros(snl)
    u0, nreg, row0, rows = np.zeros(max(nuu, 1)), C.c_int(), C.c_int(), C.c_int()
    la, co, wa = C.c_int(), C.c_int(), C.c_int()
    rng = np.random.Generator(np.random.PCG64(2424))
    t = {k: [] for k in "ab"}
    cnt, dx, du, bad = [], 0.0, 0.0, 0
    for k in range(steps):
        wx, wu = rng.standard_normal(snx), rng.standard_normal(snu)
        assert L.tqgpu_mpc_step_at(g.h, dp(xs[k]), k, C.byref(o), C.byref(res), dp(u0)) == 0, L.tqgpu_last_error()
        assert L.tqgpu_mpc_adjoint(g.h, C.byref(o), dp(wx), dp(wu), 1, C.byref(nreg)) == 0, L.tqgpu_last_error()
        bad += res.status != 0
        t0 = time.perf_counter()
        rc = L.tqgpu_mpc_adjoint_reference(g.h, dp(gxr), dp(gur), C.byref(row0), C.byref(rows))
        t["a"].append(time.perf_counter() - t0)
        assert rc == 0 and (row0.value, rows.value) == (k, deep + 1), L.tqgpu_last_error()
        L.tqgpu_mpc_stats(C.byref(la), C.byref(co), C.byref(wa))
        cnt.append((la.value, co.value, wa.value))
        t0 = time.perf_counter()
        assert L.tqgpu_mpc_get_adjoint(g.h, dp(gq), dp(gr), dp(gb)) == 0
        HX, HU = np.zeros((deep + 1, nxx)), np.zeros((deep + 1, nuu))
        np.add.at(HX, st, (-Qd * gq).reshape((Nn, nxx)))
        np.add.at(HU, stu, (-Rd * gr).reshape((-1, nuu)))
        t["b"].append(time.perf_counter() - t0)
        dx, du = max(dx, float(np.max(np.abs(gxr.reshape((deep + 1, nxx)) - HX)))), max(du, float(np.max(np.abs(gur.reshape((deep + 1, nuu)) - HU))))
    g.close()
    med = tuple(int(np.median([e[i] for e in cnt[skip:]])) for i in range(3))
    print(f"{name}, --adjoint-reference --tracking, root with states: {Nn} nodes, {deep + 1} rows per step, {steps} steps; steps with another status than 0: {bad}")
    ma, lo, p90 = stats(t["a"][skip:])
    print(f"    {'(a) tqgpu_mpc_adjoint_reference':34s} wall median {ma:8.1f} us  min {lo:8.1f}  p90 {p90:8.1f}  | launches %d  copies %d  waits %d" % med, flush=True)
    mb, lo, p90 = stats(t["b"][skip:])
    print(f"    {'(b) tqgpu_mpc_get_adjoint + numpy':34s} wall median {mb:8.1f} us  min {lo:8.1f}  p90 {p90:8.1f}  | launches 0  copies 3  waits 1 (not counted by tqgpu_mpc_stats)", flush=True)
    print(f"    (b) / (a) wall {np.median(t['b'][skip:]) / np.median(t['a'][skip:]):.2f}; largest |(a) - (b)| over the run: gxref {dx:.2e}, guref {du:.2e}", flush=True)


def P_parents(nk):
    from treeqp_amd import problems as P
    return np.asarray(P.parents_of(nk), dtype=int)


def predict_compare(capi, name, p, tracking, steps, skip):
    """--predict: iterations and trials per step over the closed-loop sequence of --root-states (tracking: of --tracking), two ways on a
    root with states: warm start mode 1, and mode 1 with the dual predictor: behind every step tqgpu_mpc_sensitivity, then
    tqgpu_mpc_predict(x0 of the next step, duals = 1), so that the next solve starts from lam* + dlam/dx0 (x0_next - x0).  With tracking
    the window also moves between the steps, which the tangent in x0 does not see.  Wall time per step includes the two extra calls."""
    L = capi.lib()
    dp = lambda a: a.ctypes.data_as(capi.c_dbl_p)
    o, r = capi._gpu_opts(), capi.GpuResult()
    d, x0 = full_root(capi, p)
    nu0 = int(d["nu"][0])
    xs = [moved_inward(x0, k, 0) for k in range(steps + 1)]
    if tracking:
        X, U = reference(x0, nu0, steps + int(node_stages(d["nk"]).max()) + 2)
    u0, up = np.zeros(max(nu0, 1)), np.zeros(max(nu0, 1))
    nreg, ncl = C.c_int(), C.c_int()
    print(f"{name}, --predict, root with states{', tracking' if tracking else ''}: {len(d['nk'])} nodes, {steps} steps", flush=True)
    for how in ("mode 1", "mode 1 + predictor"):
        g = capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)
        g.mpc_set_root_states()
        g.set_warm_start(1)
        if tracking:
            g.mpc_set_tracking(X, U, d["q"], d["r"])
        w, cnt, perr, clipped = [], [], [], 0
        for k in range(steps):
            t0 = time.perf_counter()
            assert L.tqgpu_mpc_step_at(g.h, dp(xs[k]), k if tracking else -1, C.byref(o), C.byref(r), dp(u0)) == 0, L.tqgpu_last_error()
            cnt.append((r.status, r.iter, r.ls_total))
            if k > 0 and how != "mode 1":
                perr.append(float(np.max(np.abs(up[:nu0] - u0[:nu0]))))
            if how != "mode 1":
                assert L.tqgpu_mpc_sensitivity(g.h, C.byref(o), C.byref(nreg)) == 0, L.tqgpu_last_error()
                assert L.tqgpu_mpc_predict(g.h, dp(xs[k + 1]), dp(up), 1, C.byref(ncl)) == 0, L.tqgpu_last_error()
                clipped += ncl.value
            w.append(time.perf_counter() - t0)
        g.close()
        m, lo, p90 = stats(w[skip:])
        tail = f" | largest |u0_pred - u0 of the next solve| {max(perr):.2e}, median {np.median(perr):.2e}; entries clipped {clipped}" if perr else ""
        print(f"    {how:20s} wall median {m:8.1f} us  min {lo:8.1f}  p90 {p90:8.1f} | iterations per step mean {np.mean([c[1] for c in cnt[skip:]]):.2f}  "
              f"trials per step mean {np.mean([c[2] for c in cnt[skip:]]):.2f} | status 0 in {sum(c[0] == 0 for c in cnt)} of {steps}{tail}", flush=True)


def predict_at_compare(capi, name, p, steps, skip):
    """--predict-at: the tracking loop of --predict on a root with states, three ways: warm start mode 1; mode 1 with the x0 predictor
    (tqgpu_mpc_sensitivity + tqgpu_mpc_predict, which does not see the window move); mode 1 with tqgpu_mpc_predict_at(x0 and window of the next
    step, duals = 1), whose direction follows the reference.  Wall time per step includes the extra calls."""
    L = capi.lib()
    dp = lambda a: a.ctypes.data_as(capi.c_dbl_p)
    o, r = capi._gpu_opts(), capi.GpuResult()
    d, x0 = full_root(capi, p)
    nu0 = int(d["nu"][0])
    xs = [moved_inward(x0, k, 0) for k in range(steps + 1)]
    X, U = reference(x0, nu0, steps + int(node_stages(d["nk"]).max()) + 2)
    u0, up = np.zeros(max(nu0, 1)), np.zeros(max(nu0, 1))
    nreg, ncl = C.c_int(), C.c_int()
    print(f"{name}, --predict-at, root with states, tracking: {len(d['nk'])} nodes, {steps} steps", flush=True)
    for how in ("mode 1", "mode 1 + x0 predictor", "mode 1 + predict_at"):
        g = capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)
        g.mpc_set_root_states()
        g.set_warm_start(1)
        g.mpc_set_tracking(X, U, d["q"], d["r"])
        w, cnt, perr, clipped, st = [], [], [], 0, None
        for k in range(steps):
            t0 = time.perf_counter()
            assert L.tqgpu_mpc_step_at(g.h, dp(xs[k]), k, C.byref(o), C.byref(r), dp(u0)) == 0, L.tqgpu_last_error()
            cnt.append((r.status, r.iter, r.ls_total))
            if k > 0 and how != "mode 1":
                perr.append(float(np.max(np.abs(up[:nu0] - u0[:nu0]))))
            if how == "mode 1 + x0 predictor":
                assert L.tqgpu_mpc_sensitivity(g.h, C.byref(o), C.byref(nreg)) == 0, L.tqgpu_last_error()
                assert L.tqgpu_mpc_predict(g.h, dp(xs[k + 1]), dp(up), 1, C.byref(ncl)) == 0, L.tqgpu_last_error()
                clipped += ncl.value
            if how == "mode 1 + predict_at":
                assert L.tqgpu_mpc_predict_at(g.h, C.byref(o), dp(xs[k + 1]), k + 1, dp(up), 1, C.byref(ncl), C.byref(nreg)) == 0, L.tqgpu_last_error()
                clipped += ncl.value
                st = capi.mpc_stats()
            w.append(time.perf_counter() - t0)
        g.close()
        m, lo, p90 = stats(w[skip:])
        tail = f" | largest |u0_pred - u0 of the next solve| {max(perr):.2e}, median {np.median(perr):.2e}; entries clipped {clipped}" if perr else ""
        tail += f" | the call: {st['launches']} launches, {st['copies']} copies, {st['waits']} waits" if st else ""
        print(f"    {how:24s} wall median {m:8.1f} us  min {lo:8.1f}  p90 {p90:8.1f} | iterations per step mean {np.mean([c[1] for c in cnt[skip:]]):.2f}  "
              f"trials per step mean {np.mean([c[2] for c in cnt[skip:]]):.2f} | status 0 in {sum(c[0] == 0 for c in cnt)} of {steps}{tail}", flush=True)


def tangent_compare(capi, name, p, steps, skip):
    """--tangent: behind every step of the tracking loop (root with states) one directional derivative of the step along (dq, dr), two ways:
    tqgpu_mpc_tangent (nd = 1), and the only route there was without it, tqgpu_mpc_adjoint(w = (dq, dr)) + tqgpu_mpc_get_adjoint + numpy, which by
    the symmetry of the KKT system gives the same (dx, du) but cannot carry db or dx0.  Time per call, launches, copies, waits of tqgpu_mpc_stats
    (the downloads of tqgpu_mpc_get_adjoint are not counted there), and the largest difference of the two results."""
    L = capi.lib()
    dp = lambda a: a.ctypes.data_as(capi.c_dbl_p)
    o, r = capi._gpu_opts(), capi.GpuResult()
    d, x0 = full_root(capi, p)
    nu0 = int(d["nu"][0])
    xs = [moved_inward(x0, k, 0) for k in range(steps + 1)]
    X, U = reference(x0, nu0, steps + int(node_stages(d["nk"]).max()) + 2)
    u0 = np.zeros(max(nu0, 1))
    rng = np.random.default_rng(5)
    dq, dr = 2.0 ** -10 * rng.standard_normal(len(d["q"])), 2.0 ** -10 * rng.standard_normal(len(d["r"]))
    nreg = C.c_int()
    print(f"{name}, --tangent, root with states, tracking: {len(d['nk'])} nodes, {steps} steps", flush=True)
    g = capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)
    g.mpc_set_root_states()
    g.set_warm_start(1)
    g.mpc_set_tracking(X, U, d["q"], d["r"])
    gq, gr, gb = np.zeros(max(int(g.sum_nx), 1)), np.zeros(max(int(g.sum_nu), 1)), np.zeros(max(int(g.sum_lam), 1))
    du0 = np.zeros(max(nu0, 1))
    wt, wa, diff, st_t, st_a = [], [], [], None, None
    for k in range(steps):
        assert L.tqgpu_mpc_step_at(g.h, dp(xs[k]), k, C.byref(o), C.byref(r), dp(u0)) == 0, L.tqgpu_last_error()
        assert L.tqgpu_mpc_sensitivity(g.h, C.byref(o), C.byref(nreg)) == 0, L.tqgpu_last_error()          # both legs find the factor stored
        order = ("tangent", "adjoint") if k % 2 == 0 else ("adjoint", "tangent")
        for leg in order:
            t0 = time.perf_counter()
            if leg == "tangent":
                assert L.tqgpu_mpc_tangent(g.h, C.byref(o), dp(dq), dp(dr), None, None, 1, C.byref(nreg)) == 0, L.tqgpu_last_error()
                assert L.tqgpu_mpc_get_tangent_u0(g.h, dp(du0)) == 0
                wt.append(time.perf_counter() - t0)
                st_t = capi.mpc_stats()
            else:
                assert L.tqgpu_mpc_adjoint(g.h, C.byref(o), dp(dq), dp(dr), 1, C.byref(nreg)) == 0, L.tqgpu_last_error()
                st_a = capi.mpc_stats()
                assert L.tqgpu_mpc_get_adjoint(g.h, dp(gq), dp(gr), dp(gb)) == 0
                via = gr[:nu0].copy()          # du0 = the u rows of the root of gr
                wa.append(time.perf_counter() - t0)
        diff.append(float(np.max(np.abs(via - du0[:nu0]))))
    g.close()
    for how, w, st, note in (("tqgpu_mpc_tangent", wt, st_t, ""), ("adjoint + download", wa, st_a, " + 3 uncounted blocking downloads and a stream wait; no db, no dx0")):
        m, lo, p90 = stats(w[skip:])
        print(f"    {how:24s} per call median {m:8.1f} us  min {lo:8.1f}  p90 {p90:8.1f} | {st['launches']} launches, {st['copies']} copies, {st['waits']} waits{note}", flush=True)
    print(f"    largest |du0 (tangent) - du0 (adjoint route)| over the loop: {max(diff):.2e}", flush=True)


def refused_kind3(capi, what):
    """kind3 under --predict-at / --tangent: the calls refuse trees with nodes of kind 2 or 3; the record says so"""
    import solve_sequence_cases as SC
    L = capi.lib()
    d, kinds = kind3_tree()
    g = capi.TqGpu(d["nk"], d["nx"], d["nu"])
    try:
        g.set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"])
        g.upload_mixed(d, kinds, None)
        g.mpc_set_root_states()
        o, r = capi._gpu_opts(**dict(SC.FULL)), capi.GpuResult()
        x0 = np.array(d["xmin"][:2], copy=True)
        u0 = np.zeros(2)
        dp = lambda a: a.ctypes.data_as(capi.c_dbl_p)
        rc_step = L.tqgpu_mpc_step(g.h, dp(x0), C.byref(o), C.byref(r), dp(u0))
        rc = L.tqgpu_mpc_predict_at(g.h, C.byref(o), dp(x0), -1, dp(u0), 1, None, None) if what == "predict-at" else L.tqgpu_mpc_tangent(g.h, C.byref(o), None, None, None, dp(x0), 1, None)
        print(f"kind3, --{what}: step rc {rc_step}; the call returns {rc}: {L.tqgpu_last_error().decode()}", flush=True)
    finally:
        g.close()


def main():
    from treeqp_amd import capi, problems as P
    args = sys.argv[1:]
    take = lambda flag, default: int(args[args.index(flag) + 1]) if flag in args else default
    steps, skip, n = take("--steps", 200), take("--skip", 10), take("--batch", 64)
    names = [a for a in args if a in ("c1", "c2", "batch", "kind3")] or ["c1", "c2", "batch"]
    if capi.device_count() < 1:
        raise SystemExit("no HIP device")
    if "--gain-batch" in args:
        sizes = [int(v) for v in args[args.index("--gain-batch") + 1].split(",")]          # N, or N1,N2,.. in one process
        for nb in sizes:
            if "c1" in names:
                gain_batch_compare(capi, "c1", P.spring_mass(), False, nb, steps, skip)
            if "c2" in names:
                gain_batch_compare(capi, "c2", P.linear_chain(2, 9, 9), True, nb, steps, skip)
        return
    if "--gain" in args:
        if "c1" in names:
            gain_compare(capi, "c1", P.spring_mass(), True, steps, skip)
            gain_compare(capi, "c1", P.spring_mass(), False, steps, skip)
        if "c2" in names:
            gain_compare(capi, "c2", P.linear_chain(2, 9, 9), True, steps, skip)
        return
    if "--adjoint-bounds" in args:
        if "c1" in names:
            adjoint_bounds_compare(capi, "c1", P.spring_mass(), True, steps, skip)
            adjoint_bounds_compare(capi, "c1", P.spring_mass(), False, steps, skip)
        if "c2" in names:
            adjoint_bounds_compare(capi, "c2", P.linear_chain(2, 9, 9), True, steps, skip)
        return
    if "--adjoint-reference" in args:
        if "--tracking" not in args:
            raise SystemExit("--adjoint-reference goes with --tracking")
        if "c1" in names:
            adjoint_reference_compare(capi, "c1", P.spring_mass(), steps, skip)
        if "c2" in names:
            adjoint_reference_compare(capi, "c2", P.linear_chain(2, 9, 9), steps, skip)
        return
    if "--adjoint-matrices" in args:
        sizes = [int(v) for v in args[args.index("--adjoint-batch") + 1].split(",")] if "--adjoint-batch" in args else [0]
        for nb in sizes:
            if "c1" in names:
                adjoint_matrices_compare(capi, "c1", P.spring_mass(), True, nb, steps, skip)
                adjoint_matrices_compare(capi, "c1", P.spring_mass(), False, nb, steps, skip)
            if "c2" in names:
                adjoint_matrices_compare(capi, "c2", P.linear_chain(2, 9, 9), True, nb, steps, skip)
        return
    if "--adjoint-batch" in args:
        sizes = [int(v) for v in args[args.index("--adjoint-batch") + 1].split(",")]          # N, or N1,N2,.. in one process
        for nb in sizes:
            if "c1" in names:
                adjoint_batch_compare(capi, "c1", P.spring_mass(), True, nb, steps, skip)
                adjoint_batch_compare(capi, "c1", P.spring_mass(), False, nb, steps, skip)
            if "c2" in names:
                adjoint_batch_compare(capi, "c2", P.linear_chain(2, 9, 9), True, nb, steps, skip)
        return
    if "--adjoint" in args:
        if "c1" in names:
            adjoint_compare(capi, "c1", P.spring_mass(), True, steps, skip)
            adjoint_compare(capi, "c1", P.spring_mass(), False, steps, skip)
        if "c2" in names:
            adjoint_compare(capi, "c2", P.linear_chain(2, 9, 9), True, steps, skip)
        return
    if "--predict-at" in args or "--tangent" in args:
        fn, what = (predict_at_compare, "predict-at") if "--predict-at" in args else (tangent_compare, "tangent")
        for nm, p in (("c1", P.spring_mass()), ("c2", P.linear_chain(2, 9, 9))):
            if nm in names:
                fn(capi, nm, p, steps, skip)
        if "kind3" in names:
            refused_kind3(capi, what)
        return
    if "--predict" in args:
        for nm, p in (("c1", P.spring_mass()), ("c2", P.linear_chain(2, 9, 9))):
            if nm in names:
                predict_compare(capi, nm, p, False, steps, skip)
                predict_compare(capi, nm, p, True, steps, skip)
        return
    if "--shift" in args:
        import solve_sequence_cases as SC
        for nm, p in (("c1", P.spring_mass()), ("c2", P.linear_chain(2, 9, 9))):
            if nm in names:
                d, x0 = full_root(capi, p)
                shift_compare(capi, nm, d, x0, steps, skip)
        if "kind3" in names:
            d, kinds = kind3_tree()
            st = node_stages(d["nk"])
            t = np.arange(steps + int(st.max()) + 1)[:, None]
            X = 0.05 * np.sin(0.2 * t + np.arange(2)[None, :])
            U = 0.05 * np.sin(0.2 * t + 1.0 + np.arange(1)[None, :])
            x0 = np.array(d["xmin"][:2], copy=True)
            shift_compare(capi, "kind3", d, x0, steps, skip, kinds=kinds, opts=dict(SC.FULL), X=X, U=U, move_x0=False)          # (x0 stays, as in --tracking kind3)
        return
    if "--tracking" in args:
        if "c1" in names:
            tracking_single(capi, "c1", P.spring_mass(), steps, skip)
        if "c2" in names:
            tracking_single(capi, "c2", P.linear_chain(2, 9, 9), steps, skip)
        if "kind3" in names:
            tracking_kind3(capi, steps, skip)
        if "batch" in names:
            tracking_batch(capi, P.spring_mass(), n, steps, skip)
        return
    if "--root-states" in args:
        if "c1" in names:
            single_root(capi, "c1", P.spring_mass(), steps, skip, "--certify" in args)
        if "c2" in names:
            single_root(capi, "c2", P.linear_chain(2, 9, 9), steps, skip, "--certify" in args)
        if "batch" in names:
            batch_root(capi, P.spring_mass(), n, steps, skip)
        return
    if "c1" in names:
        single(capi, "c1", P.spring_mass(), steps, skip)
    if "c2" in names:
        single(capi, "c2", P.linear_chain(2, 9, 9), steps, skip)
    if "batch" in names:
        batch(capi, P.spring_mass(), n, steps, skip)


if __name__ == "__main__":
    main()
