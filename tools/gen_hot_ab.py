"""A/B of the kind-3 stage solver (stage_gen) on the 85-node tree of tests/gen_cases.scaled_one_row, on the GPU box:

    python tools/gen_hot_ab.py [--solves 40] [--rounds 2] base@hot=1 base@hot=0 parent box

Each name is `build[@hot=0|1]`: `base` is the product library, any other build a directory under treeqp_amd/lib_var/ (as
tools/ab.py; a build without tqgpu_set_gen_hot_start, such as the parent commit's, runs as it is and reports no steps); `box` is
the product library on the same tree with the rows removed (kind 2, k_stage_box).  One child process per name and round, one after
the other.  Per child: whole solves through the C-ABI from lambda = 0 with the options of the gen tests, 5 warm-up solves, then
--solves timed ones: median, min and p90 of the device time per solve (HIP events), iterations, trials, stage sweeps (1 + trials)
and the step totals of tqgpu_get_stage_steps.  The tree is a timing tree: its solve runs into maxIter.

    python tools/gen_hot_ab.py --child NAME     (what a child runs; under rocprofv3 --kernel-trace --stats it gives the time per
                                                 k_stage_gen / k_stage_box launch)"""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
OPTS = dict(stationarityTolerance=1e-8, regType=1, regValue=1e-8)


def child(name, solves):
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import numpy as np
    import gen_cases as GC
    import gen_ref as G
    from treeqp_amd import capi
    d, kinds = GC.scaled_one_row(85)
    build, _, extra = name.partition("@")
    g = capi.TqGpu(d["nk"], d["nx"], d["nu"])
    if build == "box":
        g.upload_mixed(d, G._kinds2(kinds), None)
    else:
        g.set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"])
        g.upload_mixed(d, kinds, None)
    has_hot = hasattr(capi.lib(), "tqgpu_set_gen_hot_start")
    if extra.startswith("hot=") and build != "box":
        g.set_gen_hot_start(extra == "hot=1")
    for _ in range(5):
        r = g.solve(**OPTS)
    ts = np.array([g.solve(**OPTS)["device_time"] for _ in range(solves)]) * 1e6
    r = g.solve(**OPTS)
    st = g.stage_steps() if has_hot else None
    print(json.dumps(dict(name=name, status=r["status"], iter=r["iter"], trials=r["ls_total"], sweeps=1 + r["ls_total"], launches=r["n_launches"],
                          solve_us_median=float(np.median(ts)), solve_us_min=float(ts.min()), solve_us_p90=float(np.percentile(ts, 90)),
                          steps_total=None if st is None else int(st["total"].sum()), steps_last=None if st is None else int(st["last"].sum()),
                          kind3_nodes=int((kinds == 3).sum()))), flush=True)
    g.close()


def main():
    args = sys.argv[1:]
    solves, rounds = 40, 2
    while args and args[0].startswith("--"):
        if args[0] == "--child":
            return child(args[1], int(os.environ.get("GEN_HOT_AB_SOLVES", "40")))
        if args[0] == "--solves": solves = int(args[1])
        if args[0] == "--rounds": rounds = int(args[1])
        args = args[2:]
    for rnd in range(rounds):
        for name in args:
            env = dict(os.environ, GEN_HOT_AB_SOLVES=str(solves))
            build = name.partition("@")[0]
            if build in ("base", "box"):
                env.pop("TREEQP_AMD_LIB", None)
            else:
                env["TREEQP_AMD_LIB"] = str(ROOT / "treeqp_amd" / "lib_var" / build / "libtreeqp_amd.so")
            r = subprocess.run([sys.executable, __file__, "--child", name], env=env, capture_output=True, text=True, timeout=300)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if not line:
                print(f"{name:16s} FAILED rc={r.returncode} {r.stderr[-400:]}", flush=True)
                continue
            d = json.loads(line[-1])
            print(f"round {rnd} {name:12s} status {d['status']} iter {d['iter']} sweeps {d['sweeps']:5d} solve median {d['solve_us_median']:8.0f} us min {d['solve_us_min']:8.0f} "
                  f"p90 {d['solve_us_p90']:8.0f} per sweep {d['solve_us_median'] / d['sweeps']:6.1f} us steps total {d['steps_total']} last {d['steps_last']}", flush=True)


if __name__ == "__main__":
    main()
