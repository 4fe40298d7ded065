"""Batches of the batched-adjoint tests (test_mpc_adjoint_batch_abi.py on the CPU, test_gpu_mpc_adjoint_batch.py on the device): every batch is
a tuple of case ids of adj_cases.py, all of them trees that run in seconds.

  mixed   eight trees: both root forms, a kind-1 root with S0, Nh from 1 upward, a block of 65 rows (a second stride of the wave), and
          different nx0, Np and Nn, so that every early exit of the batch kernels has members on both sides of it
  same4   four copies of one tree from different x0: the batch whose launch, copy and wait counts must not depend on n
  pair    the shallowest and the deepest tree of the set: the smallest batch in which the alignment of the level sweeps can go wrong

Like adj_cases.py this module must not load the native library on import: the case modules are imported where a member is built."""
from __future__ import annotations

import numpy as np

BATCHES = {
    "mixed": ("Nh1-one_leaf", "smallest-nx0_1_nu0_1", "elim-one_child", "states-three_children", "elim-dense_kind1_root", "node_d-d65",
              "states-generic", "elim-three_children"),
    "same4": ("elim-persist_c1",) * 4,
    "pair": ("Nh1-three_leaves", "states-tiered_ub"),
}
BATCH_IDS = tuple(BATCHES)
NWS = (1, 3)


def members(bid):
    """the adj_cases cases of a batch, one per member"""
    import adj_cases as AC
    return [AC.case(cid) for cid in BATCHES[bid]]


def x0s(bid):
    """the x0 every member is stepped from: the case's own; the copies of same4 start from different exact points around it"""
    out = []
    for m, c in enumerate(members(bid)):
        x0 = np.array(c["x0"], dtype=np.float64, copy=True)
        if bid == "same4" and m > 0:
            x0 = x0 + c["dx"] * 2.0 ** 10 * m          # multiples of 2^-12: exactly representable
        out.append(x0)
    return out


def ws(bid, nw):
    """(wxs, wus): one loss gradient of nw columns per member, multiples of 2^-6 from a generator seeded by batch, member and nw"""
    import mpc_cases as MC
    wxs, wus = [], []
    for m, c in enumerate(members(bid)):
        rng = np.random.Generator(np.random.PCG64(1000 * (1 + BATCH_IDS.index(bid)) + 10 * m + nw))
        sx, su = int(np.sum(c["d"]["nx"])), int(np.sum(c["d"]["nu"]))
        wxs.append(MC.quantised(rng, (sx, nw), 1.0))
        wus.append(MC.quantised(rng, (su, nw), 1.0))
    return wxs, wus
