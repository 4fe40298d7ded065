"""Per-solve device time of spring-mass C1 (x0 eliminated, xmax1 = 0.2: 58 Newton iterations) through the C-ABI: every node on the
clipping stage solver against every node on the box-constrained dense stage solver (tqgpu_set_objective_mixed kind 2, the diagonal
weights as dense blocks).  python tools/box_dense_times.py [clip|box|both] [solves]"""
import sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import numpy as np
from treeqp_amd import capi, problems as P
from helpers import product_qp_from_lti


def with_dense_blocks(d):
    xo, uo = np.concatenate([[0], np.cumsum(d["nx"])]), np.concatenate([[0], np.cumsum(d["nu"])])
    out = dict(d)
    out["Q"] = np.concatenate([np.diag(d["Qd"][xo[k]:xo[k + 1]]).ravel(order="F") for k in range(len(d["nx"]))])
    out["R"] = np.concatenate([np.diag(d["Rd"][uo[k]:uo[k + 1]]).ravel(order="F") for k in range(len(d["nx"]))])
    out["S"] = np.zeros(int(np.sum(np.asarray(d["nx"]) * np.asarray(d["nu"]))))
    return out


p = P.spring_mass(xmax1=0.2)
d = product_qp_from_lti(capi, p, eliminate_x0=True).flat()
which = sys.argv[1] if len(sys.argv) > 1 else "both"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 50
for name in (("clip", "box") if which == "both" else (which,)):
    g = capi.TqGpu(d["nk"], d["nx"], d["nu"])
    if name == "clip":
        g.upload(d, p.lambda0)
    else:
        g.upload_mixed(with_dense_blocks(d), np.full(len(d["nk"]), 2), p.lambda0)
    r = g.solve()
    t0 = time.perf_counter()
    for _ in range(N):
        r = g.solve()
    wall = (time.perf_counter() - t0) / N
    dt = g.device_times(N)
    print(f"{name}: path {g.path} status {r['status']} iter {r['iter']} ls_total {r['ls_total']} launches {r['n_launches']} "
          f"device {1e3 * float(np.median(dt)):.3f} ms/solve (median of {N}), wall {1e3 * wall:.3f} ms/solve", flush=True)
    g.close()
