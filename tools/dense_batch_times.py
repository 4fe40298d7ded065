"""Batches of small dense trees through tqgpu_solve_batch, on the GPU box: the members one after the other on the launch-per-phase
route (the default) against the opt-in single launch with one workgroup per tree (tqgpu_set_dense_batch_launch,
g_persist_dense_batch), same build, side by side.

    python tools/dense_batch_times.py [--sizes 2,16,64,256] [--calls 10] [--warmup 2] [--root DIR] [c1_box] [gen85]

Workloads (the two trees of tools/dense_single_times.py): c1_box -- spring-mass C1 (85 nodes, x0 eliminated, xmax1 = 0.2) with every
node on the box-constrained dense stage solver (kind 2); gen85 -- tests/gen_cases.scaled_one_row (85 nodes, 21 kind-3 nodes with one
row, hot start on; a timing tree, its solve runs into maxIter).  A batch is n mirrors of one tree; member k starts from the tree's
starting duals plus newton_ref.seeded_duals(seed k, scale 0.05), so no two members solve the same problem.

One child process per workload, size and mode, one after the other, off and on alternating: --warmup batch calls, then --calls timed
ones; the time of a call is the host clock around tqgpu_solve_batch (it returns when every member's verdict is in).  Per line: median,
min and p90 of the call, the launches of a call (sum over the members), iterations and trials summed over the members and their range,
members whose last solve ran the single-workgroup kernel.  Iterations and trials per member must be the same off and on: checked.

--root DIR: import treeqp_amd (and its built library) and tests/ from another checkout, for the baseline of an earlier commit from this
same script; a checkout without the option runs the off mode only, printed as `base`.

    python tools/dense_batch_times.py --child WORKLOAD N MODE      (what a child runs; MODE is off or on)"""
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(os.environ.get("DENSE_BATCH_ROOT") or Path(__file__).resolve().parent.parent)
WORKLOADS = ("c1_box", "gen85")


def child(workload, n, mode, calls, warmup):
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import numpy as np
    import newton_ref as N
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
        kinds, lam0, opts = np.full(len(d["nk"]), 2), np.asarray(p.lambda0, float), {}
    else:
        import gen_cases as GC
        d, kinds = GC.scaled_one_row(85)
        lam0, opts = np.zeros(int(np.asarray(d["nx"])[1:].sum())), dict(stationarityTolerance=1e-8, regType=1, regValue=1e-8)
    has_option = hasattr(capi.TqGpu, "set_dense_batch_launch")
    if mode == "on" and not has_option:
        raise SystemExit("this checkout has no tqgpu_set_dense_batch_launch")
    mirrors = []
    for k in range(n):
        g = capi.TqGpu(d["nk"], d["nx"], d["nu"])
        if "nc" in d:
            g.set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"])
        g.upload_mixed(d, kinds, lam0 + N.seeded_duals(len(lam0), k, 0.05))
        if has_option:
            g.set_dense_batch_launch(mode == "on")
        mirrors.append(g)
    eligible = mirrors[0].dense_batch_launch()[1] if has_option else -1
    for _ in range(warmup):
        capi.solve_batch(mirrors, **opts)
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        res = capi.solve_batch(mirrors, **opts)
        ts.append(1e3 * (time.perf_counter() - t0))
    ts = np.array(ts)
    it, ls = [r["iter"] for r in res], [r["ls_total"] for r in res]
    status = sorted({r["status"] for r in res})
    print(json.dumps(dict(workload=workload, n=n, mode=mode if has_option else "base", eligible=eligible, status=status, iters=it, trials=ls,
                          launches=int(sum(r["n_launches"] for r in res)), single_wg=int(sum(bool(g.plan["last_single_wg"]) for g in mirrors)),
                          ms_median=float(np.median(ts)), ms_min=float(ts.min()), ms_p90=float(np.percentile(ts, 90)))), flush=True)
    for g in mirrors:
        g.close()


def main():
    args = sys.argv[1:]
    sizes, calls, warmup, root = [2, 16, 64, 256], 10, 2, None
    while args and args[0].startswith("--"):
        if args[0] == "--child":
            return child(args[1], int(args[2]), args[3], int(os.environ.get("DENSE_BATCH_CALLS", "10")), int(os.environ.get("DENSE_BATCH_WARMUP", "2")))
        if args[0] == "--sizes": sizes = [int(x) for x in args[1].split(",")]
        if args[0] == "--calls": calls = int(args[1])
        if args[0] == "--warmup": warmup = int(args[1])
        if args[0] == "--root": root = str(Path(args[1]).resolve())
        args = args[2:]
    env = dict(os.environ, DENSE_BATCH_CALLS=str(calls), DENSE_BATCH_WARMUP=str(warmup))
    env.pop("TREEQP_AMD_DENSE_BATCH_LAUNCH", None)
    env.pop("TREEQP_AMD_DENSE_SINGLE_LAUNCH", None)
    modes = ("off", "on")
    if root:
        env["DENSE_BATCH_ROOT"] = root
        if "tqgpu_set_dense_batch_launch" not in (Path(root) / "include" / "treeqp_amd.h").read_text():
            modes = ("off",)
    seen, differ = {}, False
    for w in (args or WORKLOADS):
        for n in sizes:
            for mode in modes:
                r = subprocess.run([sys.executable, __file__, "--child", w, str(n), mode], env=env, capture_output=True, text=True, timeout=900)
                line = [l for l in r.stdout.splitlines() if l.startswith("{")]
                if not line:
                    print(f"{w:7s} n {n:3d} {mode:4s} FAILED rc={r.returncode} {r.stderr[-400:]}", flush=True)
                    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
                        return 1          # a crashed child: nothing more is started on the device
                    continue
                d = json.loads(line[-1])
                seen[(w, n, d["mode"])] = d
                it, ls = d["iters"], d["trials"]
                print(f"{w:7s} n {n:3d} {d['mode']:4s} single_wg {d['single_wg']:3d} status {d['status']} launches {d['launches']:8d} iter sum {sum(it):6d} ({min(it)}..{max(it)}) "
                      f"trials sum {sum(ls):7d} ({min(ls)}..{max(ls)}) batch median {d['ms_median']:10.2f} ms min {d['ms_min']:10.2f} p90 {d['ms_p90']:10.2f}", flush=True)
            a, b = seen.get((w, n, "off")), seen.get((w, n, "on"))
            if a and b:
                same = a["iters"] == b["iters"] and a["trials"] == b["trials"]
                print(f"{w:7s} n {n:3d} on / off = {b['ms_median'] / a['ms_median']:.3f}; iterations and trials per member {'equal' if same else 'DIFFER'}", flush=True)
                differ |= not same
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
