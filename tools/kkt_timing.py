"""What certifying a solve costs, on the GPU box: the KKT residuals evaluated on the device (tqgpu_kkt_residual: two small kernels
behind the packing kernel, 12 values back) against the host path of the reference's drivers (tqgpu_get_solution, then
tree_qp_out_max_KKT_res over the container, as solve_qp_json.c does it).

    python tools/kkt_timing.py [--rounds 300] [--warmup 30] [--batch 2,16,64,256] [c2] [c3] [batch]

Workloads: c2 = problems.linear_chain(2, 9, 9), 1 023 nodes; c3 = linear_chain(2, 11, 11), 4 095 nodes (both one persistent
launch per solve); batch = 2, 16, 64 and 256 mirrors of C1, problems.spring_mass(), through tqgpu_solve_batch.

Per workload, in one process and alternating round by round so that all share the machine's state:

    solve                    tqgpu_solve alone
    solve+kkt                tqgpu_solve, then tqgpu_kkt_residual
    solve+get                tqgpu_solve, then tqgpu_get_solution into caller arrays
    host_kkt                 tree_qp_out_max_KKT_res alone, on a container that holds the solution (no device call)

Every timed call ends in a device synchronisation or is host code; the clock is the host's perf_counter around the calls, made
straight through ctypes with prepared arguments.  Reported: median, min and p90 in microseconds, and the two costs of a check:
device = (solve+kkt) - solve; host = (solve+get) - solve + host_kkt.  The host figure leaves out the caller's copy of the arrays
into tree_qp_out, which the drivers also pay.  For the batch: tqgpu_solve_batch alone, with tqgpu_kkt_residual_batch on both
of its routes (solve+kkt: the members in one set of launches; solve+kkt/m: member by member, TREEQP_AMD_KKT_BATCH=members), with one
tqgpu_get_solution per member, and tree_qp_out_max_KKT_res over every member's container; per route the device cost of every round
(that round minus the median solve) as median, min and p90, and what tqgpu_kkt_batch_stats counted.  A library without that symbol
(TREEQP_AMD_LIB pointing at an earlier build, for the comparison with a parent commit) runs its one route under both names.  The
device figure and the host figure of the last round are printed side by side as a check that both certify the same point."""
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


def line(name, ts):
    med, lo, p90 = stats(ts)
    print(f"    {name:12s} median {med:9.1f} us   min {lo:9.1f}   p90 {p90:9.1f}", flush=True)
    return med


def mirror_of(capi, p):
    from helpers import product_qp_from_lti
    qp = product_qp_from_lti(capi, p)
    flat = qp.flat()
    return qp, capi.TqGpu(flat["nk"], flat["nx"], flat["nu"]).upload(flat, p.lambda0)


def single(capi, name, p, rounds, warmup):
    L = capi.lib()
    qp, g = mirror_of(capi, p)
    o, r = capi._default_opts(), capi.GpuResult()
    res, node = (C.c_double * 6)(), (C.c_int * 6)()
    bufs = [np.zeros(n) for n in (g.sum_nx, g.sum_nu, g.sum_lam, g.sum_nx, g.sum_nu, g.sum_lam)]
    ptrs = [b.ctypes.data_as(capi.c_dbl_p) for b in bufs]
    qi, qo = C.byref(qp.qp_in), C.byref(qp.qp_out)

    def solve():
        assert L.tqgpu_solve(g.h, C.byref(o), C.byref(r)) == 0

    def solve_kkt():
        solve()
        assert L.tqgpu_kkt_residual(g.h, res, node, None) == 0

    def solve_get():
        solve()
        assert L.tqgpu_get_solution(g.h, *ptrs) == 0

    solve()
    qp.set_solution(g.solution())
    host = [0.0]

    def host_kkt():
        host[0] = L.tree_qp_out_max_KKT_res(qi, qo)

    modes = dict(solve=solve, **{"solve+kkt": solve_kkt, "solve+get": solve_get, "host_kkt": host_kkt})
    ts = {k: [] for k in modes}
    for i in range(warmup + rounds):
        for k, f in modes.items():
            t0 = time.perf_counter()
            f()
            if i >= warmup:
                ts[k].append(time.perf_counter() - t0)
    print(f"{name}: {p.Nn} nodes, path {g.path}, status {r.status}, {r.iter} iterations; {rounds} rounds after {warmup}", flush=True)
    med = {k: line(k, v) for k, v in ts.items()}
    dev, hst = med["solve+kkt"] - med["solve"], med["solve+get"] - med["solve"] + med["host_kkt"]
    print(f"    a check costs: device {dev:8.1f} us, host {hst:8.1f} us (download {med['solve+get'] - med['solve']:.1f} + loop {med['host_kkt']:.1f}); "
          f"device / host = {dev / hst:.2f}; the solve alone {med['solve']:.1f} us", flush=True)
    print(f"    max KKT residual: device {max(res):.3e}, host {host[0]:.3e}", flush=True)
    g.close()


def batch(capi, n, rounds, warmup):
    from treeqp_amd import problems as P
    L = capi.lib()
    p = P.spring_mass()
    pairs = [mirror_of(capi, p) for _ in range(n)]
    ms = [g for _, g in pairs]
    arr = (C.c_void_p * n)(*[g.h for g in ms])
    o, rs = capi._default_opts(), (capi.GpuResult * n)()
    res, node = np.zeros((n, 6)), np.zeros((n, 6), dtype=np.int32)
    rp, npn = res.ctypes.data_as(capi.c_dbl_p), node.ctypes.data_as(capi.c_int_p)
    g0 = ms[0]
    bufs = [np.zeros(k) for k in (g0.sum_nx, g0.sum_nu, g0.sum_lam, g0.sum_nx, g0.sum_nu, g0.sum_lam)]
    ptrs = [b.ctypes.data_as(capi.c_dbl_p) for b in bufs]

    def solve():
        assert L.tqgpu_solve_batch(arr, n, C.byref(o), rs) == 0

    def solve_kkt():
        solve()
        assert L.tqgpu_kkt_residual_batch(arr, n, rp, npn) == 0

    cost = {}

    def solve_kkt_members():
        os.environ["TREEQP_AMD_KKT_BATCH"] = "members"          # read by the library at each call
        try:
            solve_kkt()
        finally:
            del os.environ["TREEQP_AMD_KKT_BATCH"]
        cost["members"] = batch_stats()

    def batch_stats():
        return capi.kkt_batch_stats() if hasattr(L, "tqgpu_kkt_batch_stats") else None

    def solve_get():
        solve()
        for g in ms:
            assert L.tqgpu_get_solution(g.h, *ptrs) == 0

    solve()
    for qp, g in pairs:
        qp.set_solution(g.solution())
    refs = [(C.byref(qp.qp_in), C.byref(qp.qp_out)) for qp, _ in pairs]
    host = [0.0]

    def host_kkt():
        host[0] = max(L.tree_qp_out_max_KKT_res(a, b) for a, b in refs)

    modes = dict(solve=solve, **{"solve+kkt": solve_kkt, "solve+kkt/m": solve_kkt_members, "solve+get": solve_get, "host_kkt": host_kkt})
    ts = {k: [] for k in modes}
    for i in range(warmup + rounds):
        for k, f in modes.items():
            t0 = time.perf_counter()
            f()
            if i >= warmup:
                ts[k].append(time.perf_counter() - t0)
            if k == "solve+kkt":
                cost["batched"] = batch_stats()
    print(f"batch of {n} x C1 ({p.Nn} nodes each, path {g0.path}), status {sorted({rs[i].status for i in range(n)})}; {rounds} rounds after {warmup}", flush=True)
    med = {k: line(k, v) for k, v in ts.items()}
    hst = med["solve+get"] - med["solve"] + med["host_kkt"]
    # the device cost round by round (the check's round minus the median solve), so that a route's median can be held against the
    # other's minimum
    for k, what in (("solve+kkt", "one set of launches"), ("solve+kkt/m", "member by member (TREEQP_AMD_KKT_BATCH=members)")):
        d = np.asarray(ts[k]) - 1e-6 * med["solve"]
        dm, dlo, dp90 = stats(d)
        c = cost.get("batched" if k == "solve+kkt" else "members")
        print(f"    a check of the batch costs, {what}: device {dm:8.1f} us median, {dlo:8.1f} min, {dp90:8.1f} p90"
              + (f"; {c['launches']} launches, {c['copies']} copies, {c['waits']} waits, {c['batched_members']} members batched" if c else ""), flush=True)
    print(f"    host {hst:8.1f} us (downloads {med['solve+get'] - med['solve']:.1f} + loops {med['host_kkt']:.1f}); "
          f"the batch solve alone {med['solve']:.1f} us", flush=True)
    print(f"    max KKT residual over the batch: device {res.max():.3e}, host {host[0]:.3e}", flush=True)
    for g in ms:
        g.close()


def main():
    args = sys.argv[1:]
    rounds, warmup, nb = 300, 30, "2,16,64,256"
    while args and args[0].startswith("--"):
        if args[0] == "--rounds": rounds = int(args[1])
        if args[0] == "--warmup": warmup = int(args[1])
        if args[0] == "--batch": nb = args[1]
        args = args[2:]
    from treeqp_amd import capi, problems as P
    if capi.device_count() < 1:
        raise SystemExit("kkt_timing: no HIP device visible (times are taken on the GPU box only)")
    todo = args or ["c2", "c3", "batch"]
    if "c2" in todo:
        single(capi, "C2", P.linear_chain(2, 9, 9), rounds, warmup)
    if "c3" in todo:
        single(capi, "C3", P.linear_chain(2, 11, 11), rounds, warmup)
    if "batch" in todo:
        for n in (int(v) for v in nb.split(",")):
            batch(capi, n, max(rounds // 3, 20), max(warmup // 3, 5))
    return 0


if __name__ == "__main__":
    sys.exit(main())
