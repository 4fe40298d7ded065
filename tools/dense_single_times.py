"""The two routes of a dense tree side by side, same build, on the GPU box: one launch per phase (the default) against the opt-in
single launch of one workgroup (tqgpu_set_dense_single_launch, g_persist_dense).

    python tools/dense_single_times.py [--solves 40] [--rounds 2] [c1_box] [gen85]

Workloads: c1_box -- spring-mass C1 (85 nodes, x0 eliminated, xmax1 = 0.2) with every node on the box-constrained dense stage solver
(kind 2; tools/box_dense_times.py); gen85 -- tests/gen_cases.scaled_one_row (85 nodes, 21 kind-3 nodes with one row, hot start on;
tools/gen_hot_ab.py: a timing tree, its solve runs into maxIter).  One child process per workload, route and round, one after the
other (the protocol of tools/gen_hot_ab.py): 5 warm-up solves, then --solves timed ones; median, min and p90 of the device time per
solve, the counts of the solve, stage_waves of the plan.

    python tools/dense_single_times.py --child WORKLOAD ROUTE      (what a child runs; ROUTE is default or single)"""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
WORKLOADS = ("c1_box", "gen85")


def child(workload, route, solves):
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import numpy as np
    from treeqp_amd import capi
    if workload == "c1_box":
        from helpers import product_qp_from_lti
        from treeqp_amd import problems as P
        p = P.spring_mass(xmax1=0.2)
        d = dict(product_qp_from_lti(capi, p, eliminate_x0=True).flat())
        xo, uo = np.concatenate([[0], np.cumsum(d["nx"])]), np.concatenate([[0], np.cumsum(d["nu"])])
        d["Q"] = np.concatenate([np.diag(d["Qd"][xo[k]:xo[k + 1]]).ravel(order="F") for k in range(len(d["nx"]))])
        d["R"] = np.concatenate([np.diag(d["Rd"][uo[k]:uo[k + 1]]).ravel(order="F") for k in range(len(d["nx"]))])
        d["S"] = np.zeros(int(np.sum(np.asarray(d["nx"]) * np.asarray(d["nu"]))))
        g = capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload_mixed(d, np.full(len(d["nk"]), 2), p.lambda0)
        opts = {}
    else:
        import gen_cases as GC
        d, kinds = GC.scaled_one_row(85)
        g = capi.TqGpu(d["nk"], d["nx"], d["nu"])
        g.set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"])
        g.upload_mixed(d, kinds, None)
        opts = dict(stationarityTolerance=1e-8, regType=1, regValue=1e-8)
    g.set_dense_single_launch(route == "single")
    on, eligible, waves = g.dense_single_launch
    for _ in range(5):
        r = g.solve(**opts)
    ts = np.array([g.solve(**opts)["device_time"] for _ in range(solves)]) * 1e6
    r = g.solve(**opts)
    print(json.dumps(dict(workload=workload, route=route, path=g.path, eligible=eligible, stage_waves=waves, status=r["status"], iter=r["iter"],
                          trials=r["ls_total"], launches=r["n_launches"], single_wg=bool(g.plan["last_single_wg"]),
                          us_median=float(np.median(ts)), us_min=float(ts.min()), us_p90=float(np.percentile(ts, 90)))), flush=True)
    g.close()


def main():
    args = sys.argv[1:]
    solves, rounds = 40, 2
    while args and args[0].startswith("--"):
        if args[0] == "--child":
            return child(args[1], args[2], int(os.environ.get("DENSE_SINGLE_SOLVES", "40")))
        if args[0] == "--solves": solves = int(args[1])
        if args[0] == "--rounds": rounds = int(args[1])
        args = args[2:]
    med = {}
    for rnd in range(rounds):
        for w in (args or WORKLOADS):
            for route in ("default", "single"):
                env = dict(os.environ, DENSE_SINGLE_SOLVES=str(solves))
                env.pop("TREEQP_AMD_DENSE_SINGLE_LAUNCH", None)
                r = subprocess.run([sys.executable, __file__, "--child", w, route], env=env, capture_output=True, text=True, timeout=300)
                line = [l for l in r.stdout.splitlines() if l.startswith("{")]
                if not line:
                    print(f"{w:8s} {route:8s} FAILED rc={r.returncode} {r.stderr[-400:]}", flush=True)
                    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
                        return 1          # a crashed child: nothing more is started on the device
                    continue
                d = json.loads(line[-1])
                med.setdefault((w, route), []).append(d["us_median"])
                print(f"round {rnd} {w:8s} {route:8s} path {d['path']} single_wg {int(d['single_wg'])} stage_waves {d['stage_waves']:2d} status {d['status']} iter {d['iter']} "
                      f"trials {d['trials']:5d} launches {d['launches']:5d} solve median {d['us_median']:9.0f} us min {d['us_min']:9.0f} p90 {d['us_p90']:9.0f}", flush=True)
    for w in (args or WORKLOADS):
        if (w, "default") in med and (w, "single") in med:
            a, b = min(med[(w, "default")]), min(med[(w, "single")])
            print(f"{w}: single launch / default route = {b / a:.3f} (best round medians {b:.0f} us / {a:.0f} us)", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
