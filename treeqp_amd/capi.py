"""Python mirror of the treeQP C API served by libtreeqp_amd.so (ctypes, no torch types).

Two levels, both calling straight into the C-ABI:

* ``TreeQp`` / ``TdunesSolver`` -- mirror the reference's own object wrapper
  (interfaces/treeqp_cpp/treeqp_cpp_interface.hpp:36-175: TreeQp, TdunesSolver with string-keyed
  SetOption) on top of the reference-compatible C functions (tree_qp_in_*, treeqp_tdunes_*).
* ``TqGpu`` -- the thin device C-ABI of include/treeqp_amd.h (tqgpu_*), flat arrays in/out.

There is no CPU solve path behind either: constructing a solver without a usable HIP device
raises ``RuntimeError`` (the C function would print the HIP error and ``exit(1)``).
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

_ROOT = Path(__file__).resolve().parent
_LIB = None

c_int_p = C.POINTER(C.c_int)
c_dbl_p = C.POINTER(C.c_double)

RETURN_T = {0: "TREEQP_OPTIMAL_SOLUTION_FOUND", 1: "TREEQP_MAXIMUM_ITERATIONS_REACHED",
            2: "TREEQP_DN_NOT_DESCENT_DIRECTION", 7: "TREEQP_OK", 9: "TREEQP_INVALID_OPTION"}
TERMINATION = {"TREEQP_SUMSQUAREDERRORS": 0, "TREEQP_TWONORM": 1, "TREEQP_INFNORM": 2}
REGTYPE = {"TREEQP_NO_REGULARIZATION": 0, "TREEQP_ALWAYS_LEVENBERG_MARQUARDT": 1,
           "TREEQP_ON_THE_FLY_LEVENBERG_MARQUARDT": 2}


class Dmat(C.Structure):
    _fields_ = [("pA", c_dbl_p), ("m", C.c_int), ("n", C.c_int), ("memsize", C.c_int)]


class Dvec(C.Structure):
    _fields_ = [("pa", c_dbl_p), ("m", C.c_int), ("memsize", C.c_int)]


class Node(C.Structure):
    _fields_ = [("kids", c_int_p), ("idx", C.c_int), ("dad", C.c_int), ("nkids", C.c_int),
                ("stage", C.c_int), ("real", C.c_int), ("idxkid", C.c_int)]


class Info(C.Structure):
    _fields_ = [("Nn", C.c_int), ("iter", C.c_int), ("total_time", C.c_double),
                ("solver_time", C.c_double), ("interface_time", C.c_double)]


class QpInternal(C.Structure):
    _fields_ = [("is_A_initialized", c_int_p), ("is_b_initialized", c_int_p), ("is_C_initialized", C.c_int),
                ("is_dmin_initialized", C.c_int), ("is_dmax_initialized", C.c_int), ("is_S_initialized", C.c_int),
                ("is_r_initialized", C.c_int), ("x0", Dvec), ("A0", C.POINTER(Dmat)), ("b0", C.POINTER(Dvec)),
                ("C0", Dmat), ("dmax0", Dvec), ("dmin0", Dvec), ("S0", Dmat), ("r0", Dvec)]


class QpIn(C.Structure):
    _fields_ = [("N", C.c_int), ("nx", c_int_p), ("nu", c_int_p), ("nc", c_int_p),
                ("A", C.POINTER(Dmat)), ("B", C.POINTER(Dmat)), ("b", C.POINTER(Dvec)),
                ("Q", C.POINTER(Dmat)), ("R", C.POINTER(Dmat)), ("S", C.POINTER(Dmat)),
                ("q", C.POINTER(Dvec)), ("r", C.POINTER(Dvec)),
                ("xmin", C.POINTER(Dvec)), ("xmax", C.POINTER(Dvec)), ("umin", C.POINTER(Dvec)), ("umax", C.POINTER(Dvec)),
                ("C", C.POINTER(Dmat)), ("D", C.POINTER(Dmat)), ("dmin", C.POINTER(Dvec)), ("dmax", C.POINTER(Dvec)),
                ("tree", C.POINTER(Node)), ("internal_memory", QpInternal)]


class QpOut(C.Structure):
    _fields_ = [("info", Info), ("x", C.POINTER(Dvec)), ("u", C.POINTER(Dvec)), ("lam", C.POINTER(Dvec)),
                ("mu_x", C.POINTER(Dvec)), ("mu_u", C.POINTER(Dvec)), ("mu_d", C.POINTER(Dvec))]


class TdunesOpts(C.Structure):
    _fields_ = [("maxIter", C.c_int), ("qp_solver", c_int_p), ("checkLastActiveSet", C.c_int),
                ("stationarityTolerance", C.c_double), ("termCondition", C.c_int), ("regType", C.c_int),
                ("regTol", C.c_double), ("regValue", C.c_double), ("lineSearchMaxIter", C.c_int),
                ("lineSearchGamma", C.c_double), ("lineSearchBeta", C.c_double), ("lineSearchRestartTrigger", C.c_int)]


class Profiling(C.Structure):
    _fields_ = [("num_iter", C.c_int), ("run_indx", C.c_int), ("total_time", C.c_double), ("min_total_time", C.c_double),
                ("total_ls_iter", C.c_int), ("iter_times", c_dbl_p), ("min_iter_times", c_dbl_p), ("ls_iters", c_int_p),
                ("stage_qps_times", c_dbl_p), ("min_stage_qps_times", c_dbl_p), ("build_dual_times", c_dbl_p),
                ("min_build_dual_times", c_dbl_p), ("newton_direction_times", c_dbl_p),
                ("min_newton_direction_times", c_dbl_p), ("line_search_times", c_dbl_p), ("min_line_search_times", c_dbl_p)]


class TdunesWork(C.Structure):
    _fields_ = [("Nn", C.c_int), ("Np", C.c_int), ("lsIter", C.c_int), ("lineSearchRestartCounter", C.c_int),
                ("npar", c_int_p), ("idxpos", c_int_p), ("sx", C.POINTER(Dvec)), ("su", C.POINTER(Dvec)),
                ("slambda", C.POINTER(Dvec)), ("sDeltalambda", C.POINTER(Dvec)), ("timings", Profiling),
                ("device", C.c_void_p), ("stage", c_dbl_p), ("stage_doubles", C.c_int), ("lsTotal", C.c_int),
                ("maxIterAtCreate", C.c_int), ("denseStageSolver", C.c_int)]


class GpuOpts(C.Structure):
    _fields_ = [("maxIter", C.c_int), ("termCondition", C.c_int), ("stationarityTolerance", C.c_double),
                ("regType", C.c_int), ("regTol", C.c_double), ("regValue", C.c_double),
                ("lineSearchMaxIter", C.c_int), ("lineSearchGamma", C.c_double), ("lineSearchBeta", C.c_double),
                ("lineSearchRestartTrigger", C.c_int), ("profile", C.c_int), ("checkLastActiveSet", C.c_int)]


class GpuResult(C.Structure):
    _fields_ = [("status", C.c_int), ("iter", C.c_int), ("ls_total", C.c_int), ("ls_last", C.c_int),
                ("n_launches", C.c_int), ("device_time", C.c_double), ("last_error_norm", C.c_double),
                ("last_fval", C.c_double)]


_SIZEOF_CHECK = [(0, Dmat), (1, Dvec), (2, Node), (3, QpIn), (4, QpOut), (5, TdunesOpts), (6, TdunesWork),
                 (7, Profiling), (8, QpInternal)]


def library_path() -> Path:
    # TREEQP_AMD_LIB: an experiment build of the same library (treeqp_amd/build.py --variant), for A/B timing runs
    override = os.environ.get("TREEQP_AMD_LIB")
    return Path(override) if override else _ROOT / "lib" / "libtreeqp_amd.so"


def lib():
    """Load libtreeqp_amd.so (built in-tree by treeqp_amd/build.py); fail loudly if it is missing."""
    global _LIB
    if _LIB is None:
        so = library_path()
        if not so.exists():
            raise RuntimeError(f"{so} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(the treeqp_amd hot path has no pure-Python or CPU fallback)")
        L = C.CDLL(str(so))
        L.tqgpu_last_error.restype = C.c_char_p
        L.tqgpu_version.restype = C.c_char_p
        L.tree_qp_out_max_KKT_res.restype = C.c_double
        for which, typ in _SIZEOF_CHECK:
            got = L.treeqp_amd_sizeof(which)
            if got != C.sizeof(typ):
                raise RuntimeError(f"ctypes declaration of {typ.__name__} ({C.sizeof(typ)} B) does not match the library ({got} B)")
        _LIB = L
    return _LIB


def device_count() -> int:
    return int(lib().tqgpu_device_count())


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ip(a):
    return a.ctypes.data_as(c_int_p)


def _dp(a):
    return None if a is None else a.ctypes.data_as(c_dbl_p)


def _aligned_buffer(nbytes: int):
    raw = np.zeros(nbytes + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 64
    return raw, C.c_void_p(raw.ctypes.data + off)


# ------------------------------------------------------------------------------------------------
# TreeQp: tree_qp_in + tree_qp_out (reference: TreeQp in treeqp_cpp_interface.hpp:36-99)
# ------------------------------------------------------------------------------------------------

class TreeQp:
    def __init__(self, nx, nu, nk, nc=None):
        L = lib()
        self.nk = _i32(nk)
        self.nx0 = _i32(nx).copy()      # dimensions at creation (before any x0 elimination)
        self.nu0 = _i32(nu).copy()
        self.N = len(self.nk)
        if not (len(self.nx0) == len(self.nu0) == self.N):
            raise ValueError("nx, nu, nk must have one entry per node")
        if L.number_of_nodes_from_nkids(_ip(self.nk)) != self.N:
            raise ValueError("nk does not describe a tree with len(nk) nodes and uniform leaf depth")
        ncp = None if nc is None else _ip(_i32(nc))
        self.qp_in = QpIn()
        self.qp_out = QpOut()
        size_in = L.tree_qp_in_calculate_size(self.N, _ip(self.nx0), _ip(self.nu0), ncp, _ip(self.nk))
        self._mem_in, p_in = _aligned_buffer(size_in)
        L.tree_qp_in_create(self.N, _ip(self.nx0), _ip(self.nu0), ncp, _ip(self.nk), C.byref(self.qp_in), p_in)
        size_out = L.tree_qp_out_calculate_size(self.N, _ip(self.nx0), _ip(self.nu0), ncp)
        self._mem_out, p_out = _aligned_buffer(size_out)
        L.tree_qp_out_create(self.N, _ip(self.nx0), _ip(self.nu0), ncp, C.byref(self.qp_out), p_out)

    # ---- dimensions as the library currently sees them ----
    @property
    def nx(self):
        return np.ctypeslib.as_array(self.qp_in.nx, shape=(self.N,)).copy()

    @property
    def nu(self):
        return np.ctypeslib.as_array(self.qp_in.nu, shape=(self.N,)).copy()

    def tree(self):
        t = self.qp_in.tree
        out = {k: np.asarray([getattr(t[i], k) for i in range(self.N)], dtype=np.int32)
               for k in ("idx", "dad", "nkids", "stage", "real", "idxkid")}
        out["kids"] = [[t[i].kids[c] for c in range(t[i].nkids)] for i in range(self.N)]
        return out

    # ---- setters (names follow the C API / the C++ wrapper) ----
    def set_edge_dynamics(self, e, A, B, b):
        lib().tree_qp_in_set_edge_dynamics_colmajor(_dp(_f64(np.asarray(A).reshape(-1, order="F") if np.ndim(A) == 2 else A)),
                                                    _dp(_f64(np.asarray(B).reshape(-1, order="F") if np.ndim(B) == 2 else B)),
                                                    _dp(_f64(b)), C.byref(self.qp_in), int(e))

    def set_node_objective_diag(self, k, Qd, Rd, q, r):
        lib().tree_qp_in_set_node_objective_diag(_dp(_f64(Qd)), _dp(_f64(Rd)), _dp(_f64(q)), _dp(_f64(r)), C.byref(self.qp_in), int(k))

    def set_node_objective(self, k, Q, R, S, q, r):
        f = lambda M: _dp(_f64(np.asarray(M).reshape(-1, order="F") if np.ndim(M) == 2 else M))
        lib().tree_qp_in_set_node_objective_colmajor(f(Q), f(R), f(S), _dp(_f64(q)), _dp(_f64(r)), C.byref(self.qp_in), int(k))

    def set_node_bounds(self, k, xmin, xmax, umin, umax):
        lib().tree_qp_in_set_node_bounds(_dp(_f64(xmin)), _dp(_f64(xmax)), _dp(_f64(umin)), _dp(_f64(umax)), C.byref(self.qp_in), int(k))

    def set_node_general_constraints(self, k, C_, D, dmin, dmax):
        f = lambda M: _dp(_f64(np.asarray(M).reshape(-1, order="F") if np.ndim(M) == 2 else M))
        lib().tree_qp_in_set_node_general_constraints(f(C_), f(D), _dp(_f64(dmin)), _dp(_f64(dmax)), C.byref(self.qp_in), int(k))

    def set_ltv_dynamics(self, A, B, b):
        lib().tree_qp_in_set_ltv_dynamics_colmajor(_dp(_f64(A)), _dp(_f64(B)), _dp(_f64(b)), C.byref(self.qp_in))

    def set_ltv_objective_diag(self, Qd, Rd, q, r):
        lib().tree_qp_in_set_ltv_objective_diag(_dp(_f64(Qd)), _dp(_f64(Rd)), _dp(_f64(q)), _dp(_f64(r)), C.byref(self.qp_in))

    def set_ltv_bounds(self, xmin, xmax, umin, umax):
        lib().tree_qp_in_set_ltv_bounds(_dp(_f64(xmin)), _dp(_f64(xmax)), _dp(_f64(umin)), _dp(_f64(umax)), C.byref(self.qp_in))

    def set_inf_bounds(self):
        lib().tree_qp_in_set_inf_bounds(C.byref(self.qp_in))

    def set_flat(self, p):
        """Load a problems.FlatProblem (or mapping with the same keys)."""
        g = (lambda k: getattr(p, k)) if not isinstance(p, dict) else (lambda k: p[k])
        self.set_ltv_dynamics(g("A"), g("B"), g("b"))
        self.set_ltv_objective_diag(g("Qd"), g("Rd"), g("q"), g("r"))
        self.set_ltv_bounds(g("xmin"), g("xmax"), g("umin"), g("umax"))
        return self

    def fill_lti(self, p):
        """tree_qp_in_fill_lti_data_diag_weights with a problems.LtiProblem."""
        a = [_f64(v) for v in (p.A, p.B, p.b, p.Qd, p.q, p.Pd, p.p, p.Rd, p.r, p.xmin, p.xmax, p.umin, p.umax, p.x0)]
        lib().tree_qp_in_fill_lti_data_diag_weights(*[_dp(v) for v in a], None, None, None, None, None, C.byref(self.qp_in))
        return self

    def eliminate_x0(self):
        lib().tree_qp_in_eliminate_x0(C.byref(self.qp_in))
        lib().tree_qp_out_eliminate_x0(C.byref(self.qp_out))

    def set_x0(self, x0):
        lib().tree_qp_in_set_x0_colmaj(C.byref(self.qp_in), _dp(_f64(x0)))

    # ---- getters ----
    def _cat_vec(self, arr, n):
        return np.concatenate([np.ctypeslib.as_array(arr[i].pa, shape=(arr[i].m,)) if arr[i].m > 0 else np.zeros(0) for i in range(n)] or [np.zeros(0)]).copy()

    def _cat_mat(self, arr, n):
        return np.concatenate([np.ctypeslib.as_array(arr[i].pA, shape=(arr[i].m * arr[i].n,)) if arr[i].m * arr[i].n > 0 and arr[i].pA else np.zeros(0) for i in range(n)] or [np.zeros(0)]).copy()

    def flat(self) -> dict:
        """Flat ("ltv" order) copy of the data currently stored in the container."""
        q = self.qp_in
        N = self.N
        Qd = np.concatenate([np.asarray([q.Q[k].pA[j * q.Q[k].m + j] for j in range(q.Q[k].m)], dtype=float) for k in range(N)] or [np.zeros(0)])
        Rd = np.concatenate([np.asarray([q.R[k].pA[j * q.R[k].m + j] for j in range(q.R[k].m)], dtype=float) for k in range(N)] or [np.zeros(0)])
        return dict(nk=self.nk.copy(), nx=self.nx, nu=self.nu, A=self._cat_mat(q.A, N - 1), B=self._cat_mat(q.B, N - 1),
                    b=self._cat_vec(q.b, N - 1), Qd=Qd, Rd=Rd, q=self._cat_vec(q.q, N), r=self._cat_vec(q.r, N),
                    xmin=self._cat_vec(q.xmin, N), xmax=self._cat_vec(q.xmax, N),
                    umin=self._cat_vec(q.umin, N), umax=self._cat_vec(q.umax, N))

    def solution(self) -> dict:
        o = self.qp_out
        N = self.N
        out = dict(x=self._cat_vec(o.x, N), u=self._cat_vec(o.u, N), lam=self._cat_vec(o.lam, N - 1),
                   mu_x=self._cat_vec(o.mu_x, N), mu_u=self._cat_vec(o.mu_u, N))
        if any(o.mu_d[k].m for k in range(N)):
            out["mu_d"] = self._cat_vec(o.mu_d, N)
        return out

    def set_solution(self, sol: dict):
        """Write a flat solution into qp_out (used to exercise the host KKT check without a GPU)."""
        L = lib()
        off = {"x": 0, "u": 0, "lam": 0, "mu_x": 0, "mu_u": 0}
        o = self.qp_out
        for k in range(self.N):
            for name, arr, setter in (("x", o.x, L.tree_qp_out_set_node_x), ("u", o.u, L.tree_qp_out_set_node_u),
                                      ("mu_x", o.mu_x, L.tree_qp_out_set_node_mu_x), ("mu_u", o.mu_u, L.tree_qp_out_set_node_mu_u)):
                m = arr[k].m
                setter(_dp(_f64(sol[name][off[name]:off[name] + m])), C.byref(o), k)
                off[name] += m
            if "mu_d" in sol and o.mu_d[k].m:
                m = o.mu_d[k].m
                at = off.setdefault("mu_d", 0)
                L.tree_qp_out_set_node_mu_d(_dp(_f64(sol["mu_d"][at:at + m])), C.byref(o), k)
                off["mu_d"] = at + m
            if k > 0:
                m = o.lam[k - 1].m
                L.tree_qp_out_set_edge_lam(_dp(_f64(sol["lam"][off["lam"]:off["lam"] + m])), C.byref(o), k - 1)
                off["lam"] += m

    def max_kkt_res(self) -> float:
        return float(lib().tree_qp_out_max_KKT_res(C.byref(self.qp_in), C.byref(self.qp_out)))

    @property
    def info(self):
        i = self.qp_out.info
        return dict(iter=i.iter, total_time=i.total_time, solver_time=i.solver_time, interface_time=i.interface_time)


# ------------------------------------------------------------------------------------------------
# TdunesSolver (reference: TdunesSolver in treeqp_cpp_interface.hpp:127-152, SetOption strings
# of treeqp_cpp_interface.cpp:185-262)
# ------------------------------------------------------------------------------------------------

class TdunesSolver:
    _INT_OPTS = {"maxIter", "checkLastActiveSet", "lineSearchMaxIter", "lineSearchRestartTrigger"}
    _DBL_OPTS = {"stationarityTolerance", "regTol", "regValue", "lineSearchGamma", "lineSearchBeta"}

    def __init__(self, qp: TreeQp, **options):
        L = lib()
        self.qp = qp
        N = qp.N
        self.opts = TdunesOpts()
        self._opts_mem = np.zeros(max(L.treeqp_tdunes_opts_calculate_size(N), 4), dtype=np.uint8)
        L.treeqp_tdunes_opts_create(N, C.byref(self.opts), C.c_void_p(self._opts_mem.ctypes.data))
        L.treeqp_tdunes_opts_set_default(N, C.byref(self.opts))
        for k, v in options.items():
            self.set_option(k, v)
        self.work = TdunesWork()
        self._created = False

    def set_option(self, name, value):
        # validate BEFORE assigning: a rejected value must not stay in the options struct
        if getattr(self, "_created", False) and name == "maxIter" and int(value) > self.work.maxIterAtCreate:
            raise ValueError("maxIter cannot be increased after the solver was created")
        if name in self._INT_OPTS:
            setattr(self.opts, name, int(value))
        elif name in self._DBL_OPTS:
            setattr(self.opts, name, float(value))
        elif name == "termCondition":
            self.opts.termCondition = TERMINATION[value] if isinstance(value, str) else int(value)
        elif name == "regType":
            self.opts.regType = REGTYPE[value] if isinstance(value, str) else int(value)
        elif name == "clipping":
            for k in range(self.qp.N):
                self.opts.qp_solver[k] = 0 if value else 1
        else:
            raise KeyError(f"unknown tdunes option {name!r}")

    def create(self):
        """treeqp_tdunes_calculate_size + caller-owned buffer + treeqp_tdunes_create."""
        if self._created:
            return self
        L = lib()
        if device_count() < 1:
            raise RuntimeError("treeqp_tdunes_create needs a HIP device (MI355X): none is visible and the "
                               "tdunes hot path has no CPU fallback")
        size = L.treeqp_tdunes_calculate_size(C.byref(self.qp.qp_in), C.byref(self.opts))
        self._mem, p = _aligned_buffer(size)
        L.treeqp_tdunes_create(C.byref(self.qp.qp_in), C.byref(self.opts), C.byref(self.work), p)
        self._created = True
        return self

    def set_dual_initialization(self, lam):
        self.create()
        lam = _f64(lam)
        lib().treeqp_tdunes_set_dual_initialization(_dp(lam), C.byref(self.work))

    def solve(self) -> int:
        self.create()
        return int(lib().treeqp_tdunes_solve(C.byref(self.qp.qp_in), C.byref(self.qp.qp_out), C.byref(self.opts), C.byref(self.work)))

    def idxpos(self):
        self.create()
        return np.ctypeslib.as_array(self.work.idxpos, shape=(self.qp.N,)).copy()

    def npar(self):
        self.create()
        Nh = int(self.qp.tree()["stage"][-1])
        return np.ctypeslib.as_array(self.work.npar, shape=(Nh + 1,)).copy()

    @property
    def ls_total(self):
        return int(self.work.lsTotal)

    def ls_iters(self):
        n = self.qp.qp_out.info.iter
        return np.ctypeslib.as_array(self.work.timings.ls_iters, shape=(self.work.timings.num_iter,))[:n].copy()

    def destroy(self):
        if self._created:
            lib().treeqp_tdunes_destroy(C.byref(self.work))
            self._created = False

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------
# TqGpu: the device C-ABI proper (include/treeqp_amd.h)
# ------------------------------------------------------------------------------------------------

def shard_unique_id() -> bytes:
    """128-byte RCCL unique id (call on rank 0, broadcast to the other ranks)."""
    buf = C.create_string_buffer(128)
    rc = lib().tqgpu_shard_unique_id(buf)
    if rc != 0:
        raise RuntimeError(f"tqgpu_shard_unique_id failed ({rc}): {lib().tqgpu_last_error().decode()}")
    return buf.raw


def solve_virtual_ranks(mirrors, **kw) -> dict:
    """Lock-step sharded solve of n mirrors of one problem in this process (diagnostic / tests)."""
    o = GpuOpts(maxIter=100, termCondition=2, stationarityTolerance=1e-8, regType=2, regTol=1e-6, regValue=1e-6,
                lineSearchMaxIter=50, lineSearchGamma=0.1, lineSearchBeta=0.6, lineSearchRestartTrigger=-1, profile=0, checkLastActiveSet=1)
    for k, v in kw.items():
        if not hasattr(o, k):
            raise KeyError(k)
        setattr(o, k, v)
    arr = (C.c_void_p * len(mirrors))(*[m.h for m in mirrors])
    r = GpuResult()
    rc = lib().tqgpu_solve_virtual_ranks(arr, len(mirrors), C.byref(o), C.byref(r))
    if rc != 0:
        raise RuntimeError(f"tqgpu_solve_virtual_ranks failed ({rc}): {lib().tqgpu_last_error().decode()}")
    return {f: getattr(r, f) for f, _ in GpuResult._fields_}


def _default_opts(**kw):
    o = GpuOpts(maxIter=100, termCondition=2, stationarityTolerance=1e-8, regType=2, regTol=1e-6, regValue=1e-6,
                lineSearchMaxIter=50, lineSearchGamma=0.1, lineSearchBeta=0.6, lineSearchRestartTrigger=-1, profile=0, checkLastActiveSet=1)
    for k, v in kw.items():
        if not hasattr(o, k):
            raise KeyError(k)
        setattr(o, k, v)
    return o


def pshard_solve_local(mirrors, **kw) -> list:
    """ONE tree over the n mirrors of this process, inside the persistent launch: n launches that wait for each other (tagged
    words in every mirror's slab).  Every mirror must be pshard_init(r, n); the solution is collected into every mirror."""
    o = _default_opts(**kw)
    n = len(mirrors)
    arr = (C.c_void_p * n)(*[m.h for m in mirrors])
    res = (GpuResult * n)()
    rc = lib().tqgpu_pshard_solve_local(arr, n, C.byref(o), res)
    if rc != 0:
        raise RuntimeError(f"tqgpu_pshard_solve_local failed ({rc}): {lib().tqgpu_last_error().decode()}")
    return [{f: getattr(res[i], f) for f, _ in GpuResult._fields_} for i in range(n)]


def solve_batch(mirrors, profile=0, **kw) -> list:
    """Batched multi-tree solve: independent mirrors, same options; persistent launches run concurrently."""
    o = GpuOpts(maxIter=100, termCondition=2, stationarityTolerance=1e-8, regType=2, regTol=1e-6, regValue=1e-6,
                lineSearchMaxIter=50, lineSearchGamma=0.1, lineSearchBeta=0.6, lineSearchRestartTrigger=-1, profile=profile, checkLastActiveSet=1)
    for k, v in kw.items():
        if not hasattr(o, k):
            raise KeyError(k)
        setattr(o, k, v)
    n = len(mirrors)
    arr = (C.c_void_p * n)(*[m.h for m in mirrors])
    res = (GpuResult * n)()
    rc = lib().tqgpu_solve_batch(arr, n, C.byref(o), res)
    if rc != 0:
        raise RuntimeError(f"tqgpu_solve_batch failed ({rc}): {lib().tqgpu_last_error().decode()}")
    return [{f: getattr(res[i], f) for f, _ in GpuResult._fields_} for i in range(n)]


KKT_CLASSES = ("stat", "dyn", "bfeas", "bcompl", "gfeas", "gcompl")      # TQGPU_KKT_* of include/treeqp_amd.h, in order


def _kkt_dict(res, node, per_node=None) -> dict:
    out = dict(res=res, node=node, max=float("nan") if np.isnan(res).any() else float(res.max()))
    if per_node is not None:
        out["per_node"] = per_node
    return out


def kkt_residual_batch(mirrors) -> list:
    """KKT residuals of the last solve of every mirror, evaluated on the device: the members of one device in one set of launches
    and one wait (tqgpu_kkt_residual_batch; what it cost: kkt_batch_stats) -> one dict of TqGpu.kkt_residual per member."""
    n = len(mirrors)
    arr = (C.c_void_p * n)(*[m.h for m in mirrors])
    res, node = np.zeros((n, 6)), np.zeros((n, 6), dtype=np.int32)
    rc = lib().tqgpu_kkt_residual_batch(arr, n, _dp(res), _ip(node))
    if rc != 0:
        raise RuntimeError(f"tqgpu_kkt_residual_batch failed ({rc}): {lib().tqgpu_last_error().decode()}")
    return [_kkt_dict(res[i].copy(), node[i].copy()) for i in range(n)]


def kkt_batch_stats() -> dict:
    """What this thread's last kkt_residual_batch cost, summed over devices (tqgpu_kkt_batch_stats): kernel launches, copies, stream
    waits, and batched_members, the members that went through the batched kernels (0 with TREEQP_AMD_KKT_BATCH=members)."""
    v = [C.c_int(0) for _ in range(4)]
    rc = lib().tqgpu_kkt_batch_stats(*[C.byref(x) for x in v])
    if rc != 0:
        raise RuntimeError(f"tqgpu_kkt_batch_stats failed ({rc}): {lib().tqgpu_last_error().decode()}")
    return dict(zip(("launches", "copies", "waits", "batched_members"), (x.value for x in v)))


def solve_batch_n(mirrors, steps: int, profile=0, **kw):
    """`steps` batched solves back to back in C (tqgpu_solve_batch_n) -> (results of the last call, sum of iterations, of trials, of launches)."""
    o = GpuOpts(maxIter=100, termCondition=2, stationarityTolerance=1e-8, regType=2, regTol=1e-6, regValue=1e-6,
                lineSearchMaxIter=50, lineSearchGamma=0.1, lineSearchBeta=0.6, lineSearchRestartTrigger=-1, profile=profile, checkLastActiveSet=1)
    for k, v in kw.items():
        if not hasattr(o, k):
            raise KeyError(k)
        setattr(o, k, v)
    n = len(mirrors)
    arr = (C.c_void_p * n)(*[m.h for m in mirrors])
    res = (GpuResult * n)()
    it, ls, la = C.c_long(0), C.c_long(0), C.c_long(0)
    rc = lib().tqgpu_solve_batch_n(arr, n, C.byref(o), int(steps), res, C.byref(it), C.byref(ls), C.byref(la))
    if rc != 0:
        raise RuntimeError(f"tqgpu_solve_batch_n failed ({rc}): {lib().tqgpu_last_error().decode()}")
    return [{f: getattr(res[i], f) for f, _ in GpuResult._fields_} for i in range(n)], it.value, ls.value, la.value


def _gpu_opts(profile=0, **kw) -> GpuOpts:
    o = GpuOpts(maxIter=100, termCondition=2, stationarityTolerance=1e-8, regType=2, regTol=1e-6, regValue=1e-6,
                lineSearchMaxIter=50, lineSearchGamma=0.1, lineSearchBeta=0.6, lineSearchRestartTrigger=-1, profile=profile, checkLastActiveSet=1)
    for k, v in kw.items():
        if not hasattr(o, k):
            raise KeyError(k)
        setattr(o, k, v)
    return o


def mpc_step_batch(mirrors, x0s=None, profile=0, **kw):
    """One MPC step of every mirror (tqgpu_mpc_step_batch): x0s, one vector per member (None: all keep theirs; nx0 entries each, members
    with an eliminated root and members whose root keeps its states may be mixed), is folded in on the
    device, the warm start of each member's mode is taken, the batch is solved and u[0] of every member comes back
    -> (list of result dicts, list of u0 arrays).  t0s (tqgpu_mpc_step_batch_at): one reference window per member, folded into q, r in
    the same launch; an entry < 0 keeps the member's window (members without tracking take -1).  t0s is a keyword like the options."""
    t0s = kw.pop("t0s", None)
    o = _gpu_opts(profile, **kw)
    n = len(mirrors)
    arr = (C.c_void_p * n)(*[m.h for m in mirrors])
    res = (GpuResult * n)()
    if x0s is not None:
        assert len(x0s) == n and all(len(np.ravel(v)) == m.nx0 for v, m in zip(x0s, mirrors)), "x0s: nx0 entries per member"
    x = None if x0s is None else _f64(np.concatenate([np.asarray(v, dtype=np.float64).ravel() for v in x0s]))
    nu0 = [int(m.nu[0]) for m in mirrors]
    u = np.zeros(max(sum(nu0), 1))
    if t0s is None:
        rc = lib().tqgpu_mpc_step_batch(arr, n, _dp(x), C.byref(o), res, _dp(u))
    else:
        t = _i32(t0s)
        assert len(t) == n, "t0s: one window per member"
        rc = lib().tqgpu_mpc_step_batch_at(arr, n, _dp(x), _ip(t), C.byref(o), res, _dp(u))
    if rc != 0:
        raise RuntimeError(f"tqgpu_mpc_step_batch{'' if t0s is None else '_at'} failed ({rc}): {lib().tqgpu_last_error().decode()}")
    at = np.concatenate([[0], np.cumsum(nu0)]).astype(int)
    return ([{f: getattr(res[i], f) for f, _ in GpuResult._fields_} for i in range(n)],
            [u[at[i]:at[i + 1]].copy() for i in range(n)])


def mpc_adjoint_batch(mirrors, wxs=None, wus=None, profile=0, **kw) -> list:
    """Adjoint of the last solve's point of every mirror (tqgpu_mpc_adjoint_batch): the members of one device in one set of launches,
    three copies and one wait.  wxs, wus: one array per member as TqGpu.mpc_adjoint takes them ((sum_nx, nw) and (sum_nu, nw), a 1-D
    array one column), or None for zeros throughout; nw is the same for every member.  Returns one dict(gx0 (nx0, nw), n_reg) per
    member; gq, gr, gb stay on the device in the member's own buffers (TqGpu.mpc_adjoint_grads of the member)."""
    n = len(mirrors)
    nw, parts = None, []
    for given, rows_of in ((wxs, lambda m: int(m.sum_nx)), (wus, lambda m: int(m.sum_nu))):
        if given is None:
            parts.append(None)
            continue
        assert len(given) == n, "one array per member"
        cols = []
        for a, m in zip(given, mirrors):
            a = np.asarray(a, dtype=np.float64)
            a = a.reshape((rows_of(m), -1), order="F") if a.ndim == 1 else a
            assert a.shape[0] == rows_of(m) and (nw is None or a.shape[1] == nw), a.shape
            nw = a.shape[1]
            cols.append(np.asfortranarray(a).ravel(order="F"))
        parts.append(_f64(np.concatenate(cols)) if cols else _f64(np.zeros(1)))
    nw = int(kw.pop("nw", 1)) if nw is None else nw
    o = _gpu_opts(profile, **kw)
    arr = (C.c_void_p * max(n, 1))(*[m.h for m in mirrors])
    nx0 = [int(m.nx0) for m in mirrors]
    g, nr = np.zeros(max(sum(nx0) * max(nw, 0), 1)), np.zeros(max(n, 1), dtype=np.int32)
    rc = lib().tqgpu_mpc_adjoint_batch(arr, n, C.byref(o), _dp(parts[0]), _dp(parts[1]), int(nw), _dp(g), _ip(nr))
    if rc != 0:
        raise RuntimeError(f"tqgpu_mpc_adjoint_batch failed ({rc}): {lib().tqgpu_last_error().decode()}")
    at = np.concatenate([[0], np.cumsum(nx0)]).astype(int) * nw
    for m in mirrors:
        m._adj_nw = int(nw)
    return [dict(gx0=g[at[i]:at[i + 1]].copy().reshape((nx0[i], nw), order="F"), n_reg=int(nr[i])) for i in range(n)]


def mpc_sensitivity_batch(mirrors, profile=0, **kw) -> list:
    """Sensitivities of the last solve's point of every mirror (tqgpu_mpc_sensitivity_batch): the members of one device in one set of
    launches, two copies and one wait.  Returns n_reg per member; the results stay on the device in every member's own buffers
    (TqGpu.mpc_gain, mpc_sensitivities, mpc_predict of the member, or mpc_predict_batch)."""
    n = len(mirrors)
    o = _gpu_opts(profile, **kw)
    arr = (C.c_void_p * max(n, 1))(*[m.h for m in mirrors])
    nr = np.zeros(max(n, 1), dtype=np.int32)
    rc = lib().tqgpu_mpc_sensitivity_batch(arr, n, C.byref(o), _ip(nr))
    if rc != 0:
        raise RuntimeError(f"tqgpu_mpc_sensitivity_batch failed ({rc}): {lib().tqgpu_last_error().decode()}")
    return [int(v) for v in nr[:n]]


def mpc_predict_batch(mirrors, x0s, duals=False) -> tuple:
    """u0* + K (x0_new - x0_ref) of every mirror in one launch per device (tqgpu_mpc_predict_batch): x0s, one vector of nx0 entries per
    member -> (list of u0_pred, list of n_clipped).  duals: the same launch writes every member's predicted duals into its start buffer,
    for one solve, as TqGpu.mpc_predict does."""
    n = len(mirrors)
    assert len(x0s) == n and all(len(np.ravel(v)) == m.nx0 for v, m in zip(x0s, mirrors)), "x0s: nx0 entries per member"
    x = _f64(np.concatenate([np.asarray(v, dtype=np.float64).ravel() for v in x0s])) if n else _f64(np.zeros(1))
    nu0 = [int(m.nu[0]) for m in mirrors]
    u, nc = np.zeros(max(sum(nu0), 1)), np.zeros(max(n, 1), dtype=np.int32)
    arr = (C.c_void_p * max(n, 1))(*[m.h for m in mirrors])
    rc = lib().tqgpu_mpc_predict_batch(arr, n, _dp(x), _dp(u), int(bool(duals)), _ip(nc))
    if rc != 0:
        raise RuntimeError(f"tqgpu_mpc_predict_batch failed ({rc}): {lib().tqgpu_last_error().decode()}")
    at = np.concatenate([[0], np.cumsum(nu0)]).astype(int)
    return [u[at[i]:at[i + 1]].copy() for i in range(n)], [int(v) for v in nc[:n]]


ADJMAT_KEYS = ("gH", "gh", "gA", "gB", "gb", "gA0", "gS0")


def _adjmat_sizes(m):
    """(per output of tqgpu_mpc_adjoint_matrices the list of its blocks' shapes per column of w, the columns of the stored adjoint), both as
    the library reports them; gH: (nz,) for a kind-0 group, (nz, nz) for a kind-1 group.  Without a stored adjoint the columns read 1: the
    buffers are then never written, the call is refused"""
    nh, nc, root = C.c_int(0), C.c_int(0), np.zeros(4, dtype=np.int32)
    m._chk(lib().tqgpu_mpc_get_param_groups(m.h, C.byref(nh), C.byref(nc), None, None, None))
    hd, cd = np.zeros(max(5 * nh.value, 1), dtype=np.int32), np.zeros(max(4 * nc.value, 1), dtype=np.int32)
    m._chk(lib().tqgpu_mpc_get_param_groups(m.h, None, None, _ip(hd), _ip(cd), _ip(root)))
    hd, cd = hd[:5 * nh.value].reshape((-1, 5)), cd[:4 * nc.value].reshape((-1, 4))
    dense = [bool(k) for k in hd[:, 4]]
    hd = hd[:, :4]
    nb, nu0, nx0, nw = [int(v) for v in root]
    root = nb > 0
    return dict(gH=[(int(a + b), int(a + b)) if dn else (int(a + b),) for (a, b, _, _), dn in zip(hd, dense)], gh=[(int(a + b),) for a, b, _, _ in hd],
                gA=[(int(a), int(b)) for a, b, _, _ in cd], gB=[(int(a), int(c)) for a, _, c, _ in cd], gb=[(int(a),) for a, _, _, _ in cd],
                gA0=[(int(m.nx[k]), nx0) for k in range(1, 1 + int(m.nk[0]))] if root else [], gS0=[(nu0, nx0)] if root else []), max(nw, 1)


def _adjmat_split(flat, shapes, nw, by_column=False):
    """one output of nw columns -> a list with one array per group, shape + (nw,); by_column (gA0): the blocks lie column after column,
    within a column one behind the other"""
    out, at = [], 0
    if by_column:
        total = sum(int(np.prod(shp)) for shp in shapes)
        cols = flat[:total * nw].reshape((total, nw), order="F")
        for shp in shapes:
            n = int(np.prod(shp))
            out.append(cols[at:at + n].reshape(shp + (nw,), order="F").copy())
            at += n
        return out
    for shp in shapes:
        n = int(np.prod(shp))
        out.append(flat[at:at + n * nw].reshape(shp + (nw,), order="F").copy())
        at += n * nw
    return out


def mpc_adjoint_matrices_batch(mirrors, reduce: bool = False) -> list | dict:
    """The matrix gradients of every mirror's stored adjoint (tqgpu_mpc_adjoint_matrices_batch, behind mpc_adjoint_batch): per device one copy
    of descriptors, one or two launches, one copy back and one wait.  reduce False: a list with one dict per member as
    TqGpu.mpc_adjoint_matrices returns it; reduce True: one dict, the sum over the members in member order (equal group tables required)."""
    n = len(mirrors)
    both = [_adjmat_sizes(m) for m in mirrors]
    sizes, nws = [b[0] for b in both], [b[1] for b in both]
    if n == 0:          # the library's refusal, not an index error here
        rc = lib().tqgpu_mpc_adjoint_matrices_batch(None, 0, int(bool(reduce)), *([None] * 7))
        raise RuntimeError(f"tqgpu_mpc_adjoint_matrices_batch failed ({rc}): {lib().tqgpu_last_error().decode()}")
    use = range(1) if reduce else range(n)
    total = {key: sum(sum(int(np.prod(shp)) for shp in sizes[i][key]) * nws[i] for i in use) for key in ADJMAT_KEYS}
    bufs = {key: np.zeros(max(total[key], 1)) for key in ADJMAT_KEYS}
    arr = (C.c_void_p * max(n, 1))(*[m.h for m in mirrors])
    rc = lib().tqgpu_mpc_adjoint_matrices_batch(arr, n, int(bool(reduce)), *[_dp(bufs[key]) for key in ADJMAT_KEYS])
    if rc != 0:
        raise RuntimeError(f"tqgpu_mpc_adjoint_matrices_batch failed ({rc}): {lib().tqgpu_last_error().decode()}")
    out, at = [], {key: 0 for key in ADJMAT_KEYS}
    for i in use:
        one = {}
        for key in ADJMAT_KEYS:
            cnt = sum(int(np.prod(shp)) for shp in sizes[i][key]) * nws[i]
            one[key] = _adjmat_split(bufs[key][at[key]:at[key] + cnt], sizes[i][key], nws[i], key == "gA0")
            at[key] += cnt
        out.append(one)
    return out[0] if reduce else out


SHIFT_LEAF_REPEAT, SHIFT_LEAF_ZERO = 0, 1          # TQGPU_SHIFT_LEAF_* of include/treeqp_amd.h
SHIFT_DUALS, SHIFT_WORKING_SETS = 1, 2             # TQGPU_SHIFT_*
c_u64_p = C.POINTER(C.c_uint64)


def shift_map(nk, nx, realised: int, leaf: int = SHIFT_LEAF_REPEAT) -> np.ndarray:
    """img[Nn] of tqgpu_shift_map: the node of the old problem every node of the new one starts from after child `realised` of the root
    became the root (-1: none); host arithmetic only.  A tree of one node gives an empty array."""
    a, b = _i32(nk), _i32(nx)
    assert len(a) == len(b)
    img = np.full(len(a), -1, dtype=np.int32)
    rc = lib().tqgpu_shift_map(len(a), _ip(a), _ip(b), int(realised), int(leaf), _ip(img))
    if rc != 0:
        raise RuntimeError(f"tqgpu_shift_map failed ({rc}): {lib().tqgpu_last_error().decode()}")
    return img if len(a) > 1 else img[:0]


def mpc_stats() -> dict:
    """What this thread's last mpc_step / mpc_step_batch cost (tqgpu_mpc_stats): kernel launches, copies in either direction, waits
    of the host for the device."""
    v = [C.c_int(0) for _ in range(3)]
    rc = lib().tqgpu_mpc_stats(*[C.byref(x) for x in v])
    if rc != 0:
        raise RuntimeError(f"tqgpu_mpc_stats failed ({rc}): {lib().tqgpu_last_error().decode()}")
    return dict(zip(("launches", "copies", "waits"), (x.value for x in v)))


class TqGpu:
    def __init__(self, nk, nx, nu, device: int = -1):
        L = lib()
        self.nk, self.nx, self.nu = _i32(nk), _i32(nx), _i32(nu)
        self.h = C.c_void_p()
        rc = L.tqgpu_create(C.byref(self.h), int(device), len(self.nk), _ip(self.nk), _ip(self.nx), _ip(self.nu))
        if rc != 0:
            raise RuntimeError(f"tqgpu_create failed ({rc}): {L.tqgpu_last_error().decode()}")
        d = [C.c_int() for _ in range(5)]
        L.tqgpu_dims(self.h, *[C.byref(v) for v in d])
        self.sum_nx, self.sum_nu, self.sum_lam, self.sum_A, self.sum_B = [v.value for v in d]

    @property
    def fused(self) -> bool:
        return bool(lib().tqgpu_uses_fused_path(self.h))

    def device_times(self, n: int) -> np.ndarray:
        """HIP-event device times [s] of the last n solves (oldest first); synchronises the stream."""
        out = np.zeros(int(n), dtype=np.float64)
        got = lib().tqgpu_get_device_times(self.h, _dp(out), int(n))
        if got < 0:
            raise RuntimeError("tqgpu_get_device_times failed")
        return out[:got]

    @property
    def path(self) -> int:
        """Route under default options: 0 generic kernels (three launches per iteration, or per phase), 1 tiered fused kernels,
        2 persistent single launch, 3 single-workgroup persistent launch."""
        return int(lib().tqgpu_uses_fused_path(self.h))

    PLAN_FLAGS = ("wide", "wide_small", "w3", "w3_sgp", "w3_merge", "fwd_chain", "fuse", "persist", "persist_one", "gpersist",
                  "gp_state_lds", "gp_const_lds", "gp_tables_lds", "gp_small16", "gp_small8", "dense", "box",
                  "last_single_wg", "gen", "dense_single_wg")

    @property
    def plan(self) -> dict:
        """The kernel variants tqgpu_create and the last tqgpu_set_objective_mixed chose, and whether the last solve ran the
        single-workgroup kernel (tqgpu_debug_plan): name -> bool for each
        of PLAN_FLAGS (bit i of the mask is PLAN_FLAGS[i]), and sgp_accs, the children's entries k_sgp keeps in LDS per parent."""
        f, a = C.c_uint(), C.c_int()
        self._chk(lib().tqgpu_debug_plan(self.h, C.byref(f), C.byref(a)))
        out = {n: bool(f.value >> i & 1) for i, n in enumerate(self.PLAN_FLAGS)}
        out["sgp_accs"] = a.value
        return out

    def _chk(self, rc):
        if rc != 0:
            raise RuntimeError(f"tqgpu call failed ({rc}): {lib().tqgpu_last_error().decode()}")

    def upload(self, p, lambda0=None):
        g = (lambda k: getattr(p, k)) if not isinstance(p, dict) else (lambda k: p[k])
        L = lib()
        keep = {k: _f64(g(k)) for k in ("A", "B", "b", "Qd", "Rd", "q", "r", "xmin", "xmax", "umin", "umax")}
        assert len(keep["A"]) == self.sum_A and len(keep["B"]) == self.sum_B and len(keep["b"]) == self.sum_lam
        assert len(keep["Qd"]) == self.sum_nx and len(keep["Rd"]) == self.sum_nu
        self._chk(L.tqgpu_set_dynamics(self.h, _dp(keep["A"]), _dp(keep["B"]), _dp(keep["b"])))
        self._chk(L.tqgpu_set_objective_diag(self.h, _dp(keep["Qd"]), _dp(keep["Rd"]), _dp(keep["q"]), _dp(keep["r"])))
        self._chk(L.tqgpu_set_bounds(self.h, _dp(keep["xmin"]), _dp(keep["xmax"]), _dp(keep["umin"]), _dp(keep["umax"])))
        self.set_lambda(lambda0)
        return self

    def upload_dense(self, p, lambda0=None):
        """Dense objective (Q, R, S per node, column major) + the dense unconstrained stage solver."""
        g = (lambda k: getattr(p, k)) if not isinstance(p, dict) else (lambda k: p[k])
        L = lib()
        keep = {k: _f64(g(k)) for k in ("A", "B", "b", "Q", "R", "S", "q", "r")}
        assert len(keep["A"]) == self.sum_A and len(keep["B"]) == self.sum_B and len(keep["b"]) == self.sum_lam
        assert len(keep["Q"]) == int((self.nx.astype(np.int64) ** 2).sum()) and len(keep["R"]) == int((self.nu.astype(np.int64) ** 2).sum())
        assert len(keep["S"]) == int((self.nx.astype(np.int64) * self.nu).sum())
        self._chk(L.tqgpu_set_dynamics(self.h, _dp(keep["A"]), _dp(keep["B"]), _dp(keep["b"])))
        self._chk(L.tqgpu_set_objective_dense(self.h, _dp(keep["Q"]), _dp(keep["R"]), _dp(keep["S"]), _dp(keep["q"]), _dp(keep["r"])))
        self.set_lambda(lambda0)
        return self

    def upload_mixed(self, p, kind, lambda0=None):
        """Per-node choice of the stage solver: kind[k] = 0 clipping (diagonal Q_k, R_k, S_k = 0, box bounds), 1 dense unconstrained
        (full Q_k, R_k, S_k, bounds ignored), 2 dense with box bounds (full Q_k, R_k, S_k, nx + nu <= 64, the bounds apply).
        p holds A, B, b, Q, R, S (dense layout, column major), q, r and the bounds."""
        g = (lambda k: getattr(p, k)) if not isinstance(p, dict) else (lambda k: p[k])
        L = lib()
        keep = {k: _f64(g(k)) for k in ("A", "B", "b", "Q", "R", "S", "q", "r", "xmin", "xmax", "umin", "umax")}
        kd = _i32(kind)
        assert len(kd) == len(self.nk)
        self._chk(L.tqgpu_set_dynamics(self.h, _dp(keep["A"]), _dp(keep["B"]), _dp(keep["b"])))
        self._chk(L.tqgpu_set_objective_mixed(self.h, _ip(kd), _dp(keep["Q"]), _dp(keep["R"]), _dp(keep["S"]), _dp(keep["q"]), _dp(keep["r"])))
        self._chk(L.tqgpu_set_bounds(self.h, _dp(keep["xmin"]), _dp(keep["xmax"]), _dp(keep["umin"]), _dp(keep["umax"])))
        self.set_lambda(lambda0)
        return self

    def set_constraints(self, nc=None, C_=None, D=None, dmin=None, dmax=None):
        """General constraints dmin <= C x + D u <= dmax of the kind-3 nodes: nc rows per node, C (nc x nx) and D (nc x nu) column
        major, flat, node after node; None = leave alone (nc given: C, D not given are zero, dmin, dmax unbounded)."""
        keep = [None if a is None else _f64(a) for a in (C_, D, dmin, dmax)]
        n = None if nc is None else _i32(nc)
        self._chk(lib().tqgpu_set_constraints(self.h, None if n is None else _ip(n), *[_dp(a) for a in keep]))
        v = C.c_int()
        self._chk(lib().tqgpu_dims2(self.h, C.byref(v)))
        self.sum_nc = v.value
        if n is not None:
            self._nc = n
        return self

    def set_gen_hot_start(self, on: bool):
        """the kind-3 stage solver starts from the working set of its node's last stage solve (default) or cold; empties the stored sets"""
        self._chk(lib().tqgpu_set_gen_hot_start(self.h, int(bool(on))))
        return self

    def set_dense_single_launch(self, on: bool):
        """opt-in: a dense tree (kinds 1 / 2 / 3) that fits runs its whole solve as one launch of one workgroup"""
        self._chk(lib().tqgpu_set_dense_single_launch(self.h, int(bool(on))))
        return self

    @property
    def dense_single_launch(self) -> tuple:
        """(on, eligible, stage_waves): the setting, whether the current kinds / rows fit, waves of the stage sweep (0: not eligible)"""
        v = [C.c_int() for _ in range(3)]
        self._chk(lib().tqgpu_get_dense_single_launch(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def set_dense_batch_launch(self, on: bool):
        """opt-in: dense trees that fit go out of solve_batch together, as one launch with a workgroup per tree (says nothing about solve())"""
        self._chk(lib().tqgpu_set_dense_batch_launch(self.h, int(bool(on))))
        return self

    def dense_batch_launch(self) -> tuple:
        """(on, eligible): the setting, whether the current kinds / rows fit (the `eligible` of dense_single_launch)"""
        v = [C.c_int() for _ in range(2)]
        self._chk(lib().tqgpu_get_dense_batch_launch(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def stage_steps(self) -> dict:
        """active-set steps of the kind-3 stage solver per node: last (the last stage sweep), total (summed over the last solve)"""
        last, total = np.zeros(len(self.nk), dtype=np.int32), np.zeros(len(self.nk), dtype=np.int64)
        self._chk(lib().tqgpu_get_stage_steps(self.h, _ip(last), total.ctypes.data_as(C.POINTER(C.c_long))))
        return dict(last=last, total=total)

    def set_lambda(self, lam):
        a = None if lam is None else _f64(lam)
        if a is not None:
            assert len(a) == self.sum_lam
        self._chk(lib().tqgpu_set_lambda(self.h, _dp(a)))

    # ---- MPC steps: x0 fold, warm start and u[0] on the device (tqgpu_mpc_*) ----
    def _root_sizes(self):
        """(rows of b0 = the nx of the root's children, nu[0], nc[0])"""
        nk0 = int(self.nk[0])
        nc0 = 0
        if getattr(self, "_nc", None) is not None:
            nc0 = int(self._nc[0])
        return int(self.nx[1:1 + nk0].sum()), int(self.nu[0]), nc0

    def mpc_set_root(self, A0, b0, S0=None, r0=None, C0=None, dmin0=None, dmax0=None):
        """The originals of everything that multiplies x0 on an x0-eliminated tree, kept on the device (tqgpu_mpc_set_root): A0 a list
        of (nx[kid], nx0) matrices, one per child of the root (or their column-major concatenation), b0 the children's b
        concatenated; S0 (nu[0], nx0) with r0; C0 (nc[0], nx0) with dmin0, dmax0.  None for S0 / C0 means zero."""
        if isinstance(A0, (list, tuple)):
            nx0 = int(np.asarray(A0[0]).shape[1])
            a = _f64(np.concatenate([np.asarray(M, dtype=np.float64).ravel(order="F") for M in A0]))
        else:
            a = _f64(A0)
            nx0 = len(a) // max(self._root_sizes()[0], 1)
        mat = lambda M: None if M is None else _f64(np.asarray(M, dtype=np.float64).ravel(order="F"))
        vec = lambda v: None if v is None else _f64(v)
        keep = [a, vec(b0), mat(S0), vec(r0), mat(C0), vec(dmin0), vec(dmax0)]
        self._chk(lib().tqgpu_mpc_set_root(self.h, int(nx0), *[_dp(k) for k in keep]))
        self.nx0 = int(nx0)
        return self

    def mpc_set_root_states(self):
        """The root keeps its nx[0] states and x0 enters as xmin[0] = xmax[0] = x0 (tqgpu_mpc_set_root_states): afterwards mpc_set_x0,
        mpc_step and mpc_step_batch work as on an x0-eliminated tree, with nx0 = nx[0]."""
        self._chk(lib().tqgpu_mpc_set_root_states(self.h))
        self.nx0 = int(self.nx[0])
        return self

    def root_bounds(self) -> tuple:
        """(xmin[0], xmax[0]) as the device holds them now (tqgpu_get_root_bounds); waits for the stream."""
        lo, hi = np.zeros(int(self.nx[0])), np.zeros(int(self.nx[0]))
        self._chk(lib().tqgpu_get_root_bounds(self.h, _dp(lo), _dp(hi)))
        return lo, hi

    def mpc_set_certify(self, on: bool):
        """on: every mpc_step also evaluates the KKT residuals of its point on the device, in the same wait (tqgpu_mpc_set_certify)"""
        self._chk(lib().tqgpu_mpc_set_certify(self.h, int(bool(on))))
        return self

    def mpc_certificate(self) -> dict:
        """The KKT residuals of the last (certified) mpc_step, as kkt_residual() would return them right after it
        (tqgpu_mpc_get_certificate; host state only)."""
        res, node = np.zeros(6), np.zeros(6, dtype=np.int32)
        self._chk(lib().tqgpu_mpc_get_certificate(self.h, _dp(res), _ip(node)))
        return _kkt_dict(res, node)

    def mpc_set_x0(self, x0):
        """Fold x0 into b of the root's children, r[0], dmin[0], dmax[0] on the device, in place, without synchronisation."""
        a = _f64(x0)
        assert len(a) == self.nx0
        self._chk(lib().tqgpu_mpc_set_x0(self.h, _dp(a)))
        return self

    # ---- the shifted warm start: duals and working sets move a stage (tqgpu_mpc_set_shift, tqgpu_mpc_shift) ----
    def mpc_set_shift(self, leaf: int = SHIFT_LEAF_REPEAT, what: int = SHIFT_DUALS):
        """Build the shift maps of all nk[0] realisations on the device (tqgpu_mpc_set_shift): leaf SHIFT_LEAF_REPEAT or SHIFT_LEAF_ZERO,
        what SHIFT_DUALS, optionally | SHIFT_WORKING_SETS; what == 0 forgets them and returns warm start mode 2 to mode 1."""
        self._chk(lib().tqgpu_mpc_set_shift(self.h, int(leaf), C.c_uint(int(what))))
        return self

    def mpc_set_realised(self, child: int):
        """The child of the root that the last step realised (tqgpu_mpc_set_realised; host state only, default 0)."""
        self._chk(lib().tqgpu_mpc_set_realised(self.h, int(child)))
        return self

    @property
    def mpc_shift_state(self) -> dict:
        """leaf policy, what and the realisation in force (tqgpu_mpc_get_shift)"""
        leaf, what, real = C.c_int(), C.c_uint(), C.c_int()
        self._chk(lib().tqgpu_mpc_get_shift(self.h, C.byref(leaf), C.byref(what), C.byref(real)))
        return dict(leaf=leaf.value, what=what.value, realised=real.value)

    def mpc_shift(self):
        """The shift alone (tqgpu_mpc_shift): one kernel, no synchronisation; the next solve starts from the shifted duals, in any mode,
        and the working sets have moved if they were asked for."""
        self._chk(lib().tqgpu_mpc_shift(self.h))
        return self

    def working_sets(self) -> dict:
        """The hot-start halves of the stored working sets (tqgpu_get_working_sets), one uint64 per node each: bounds, rows, bound_sides,
        row_sides; 0 on nodes of kinds 0 and 1.  Waits for the stream."""
        out = {k: np.zeros(len(self.nk), dtype=np.uint64) for k in ("bounds", "rows", "bound_sides", "row_sides")}
        self._chk(lib().tqgpu_get_working_sets(self.h, *[out[k].ctypes.data_as(c_u64_p) for k in ("bounds", "rows", "bound_sides", "row_sides")]))
        return out

    def set_working_sets(self, bounds=None, rows=None, bound_sides=None, row_sides=None):
        """Upload hot-start working sets (tqgpu_set_working_sets; None: left alone); nodes of kinds 0 and 1 ignore theirs."""
        keep = [None if a is None else np.ascontiguousarray(a, dtype=np.uint64) for a in (bounds, rows, bound_sides, row_sides)]
        for a in keep:
            assert a is None or len(a) == len(self.nk)
        self._chk(lib().tqgpu_set_working_sets(self.h, *[None if a is None else a.ctypes.data_as(c_u64_p) for a in keep]))
        return self

    def set_warm_start(self, mode: int):
        """0: every solve starts from the buffer of set_lambda (default); 1: from the duals of the last solve, copied on the device;
        2: from the duals of every node's image under the shift map of the realised child (mpc_set_shift first)"""
        self._chk(lib().tqgpu_set_warm_start(self.h, int(mode)))
        return self

    @property
    def warm_start(self) -> int:
        v = C.c_int()
        self._chk(lib().tqgpu_get_warm_start(self.h, C.byref(v)))
        return v.value

    def root_terms(self, nc0=None) -> dict:
        """What the device holds now (tqgpu_get_root_terms): b of the root's children, r[0], and dmin[0], dmax[0] where the root has
        rows (nc0: their number, by default what set_constraints was given)."""
        nb, nu0, nc = self._root_sizes()
        nc = nc if nc0 is None else int(nc0)
        out = dict(b=np.zeros(nb), r=np.zeros(nu0))
        if nc:
            out["dmin"], out["dmax"] = np.zeros(nc), np.zeros(nc)
        self._chk(lib().tqgpu_get_root_terms(self.h, _dp(out["b"]), _dp(out["r"]), _dp(out.get("dmin")), _dp(out.get("dmax"))))
        return out

    # ---- tracking: the linear terms alone, a reference window folded into q, r on the device ----
    def set_linear_terms(self, q=None, r=None):
        """q, r alone (tqgpu_set_linear_terms; None: left alone): kinds, H, factors and the stored working sets of kinds 2 and 3 stay."""
        a, b = (None if q is None else _f64(q)), (None if r is None else _f64(r))
        assert a is None or len(a) == self.sum_nx
        assert b is None or len(b) == self.sum_nu
        self._chk(lib().tqgpu_set_linear_terms(self.h, _dp(a), _dp(b)))
        return self

    def linear_terms(self) -> tuple:
        """(q, r) as the device holds them now (tqgpu_get_linear_terms); waits for the stream."""
        q, r = np.zeros(self.sum_nx), np.zeros(self.sum_nu)
        self._chk(lib().tqgpu_get_linear_terms(self.h, _dp(q), _dp(r)))
        return q, r

    def mpc_set_tracking(self, xtraj, utraj, q0=None, r0=None):
        """The reference trajectory, xtraj (T, NXT) and utraj (T, NUT), one row per stage, and the base linear terms q0, r0 (flat; None:
        zeros), kept on the device (tqgpu_mpc_set_tracking).  The window is set by mpc_set_window, mpc_step(t0=) or mpc_step_batch(t0s=)."""
        X, U = np.atleast_2d(_f64(xtraj)), np.atleast_2d(_f64(utraj))
        assert X.shape[0] == U.shape[0], "xtraj and utraj: one row per stage each"
        a, b = (None if q0 is None else _f64(q0)), (None if r0 is None else _f64(r0))
        assert a is None or len(a) == self.sum_nx
        assert b is None or len(b) == self.sum_nu
        X, U = np.ascontiguousarray(X), np.ascontiguousarray(U)
        self._chk(lib().tqgpu_mpc_set_tracking(self.h, int(X.shape[1]), int(U.shape[1]), int(X.shape[0]),
                                               _dp(X) if X.size else None, _dp(U) if U.size else None, _dp(a), _dp(b)))
        return self

    def mpc_set_window(self, t0: int):
        """Fold the reference window that starts at row t0 into q, r on the device, in place, without synchronisation (tqgpu_mpc_set_window)."""
        self._chk(lib().tqgpu_mpc_set_window(self.h, int(t0)))
        return self

    @property
    def mpc_window(self) -> int:
        v = C.c_int()
        self._chk(lib().tqgpu_mpc_get_window(self.h, C.byref(v)))
        return v.value

    def mpc_step(self, x0=None, profile=0, **kw):
        """One MPC step (tqgpu_mpc_step): fold x0 (None: keep the current one), warm start of the current mode, solve
        -> (result dict, u[0]).  t0=, a keyword like the options (tqgpu_mpc_step_at): the reference window to fold into q, r in the same
        launch; None or < 0 keeps the window in force."""
        t0 = kw.pop("t0", None)
        key = (profile, tuple(sorted(kw.items())))
        cache = self.__dict__.setdefault("_opts_cache", {})
        o = cache.get(key)
        if o is None:
            o = cache[key] = _gpu_opts(profile, **kw)
        a = None if x0 is None else _f64(x0)
        if a is not None:
            assert len(a) == self.nx0
        r = GpuResult()
        u0 = np.zeros(max(int(self.nu[0]), 1))
        if t0 is None:
            self._chk(lib().tqgpu_mpc_step(self.h, _dp(a), C.byref(o), C.byref(r), _dp(u0)))
        else:
            self._chk(lib().tqgpu_mpc_step_at(self.h, _dp(a), int(t0), C.byref(o), C.byref(r), _dp(u0)))
        return {f: getattr(r, f) for f, _ in GpuResult._fields_}, u0[:int(self.nu[0])]

    # ---- parametric sensitivities of an MPC step: du0/dx0, dz/dx0, dlam/dx0 (tqgpu_mpc_sensitivity, tqgpu_mpc_predict) ----
    def mpc_sensitivity(self, profile=0, **kw) -> int:
        """Sensitivities of the last solve's point with respect to x0, active set frozen (tqgpu_mpc_sensitivity); the options give the
        regularisation rule of the factorisation.  Returns n_reg, the blocks regularised; the results stay on the device
        (mpc_gain, mpc_sensitivities, mpc_predict)."""
        n = C.c_int(0)
        o = _gpu_opts(profile, **kw)
        self._chk(lib().tqgpu_mpc_sensitivity(self.h, C.byref(o), C.byref(n)))
        return n.value

    def mpc_gain(self) -> tuple:
        """(K (nu[0], nx0), u0*, x0_ref) of the last mpc_sensitivity (tqgpu_mpc_get_gain; host state only)."""
        nu0, nx0 = int(self.nu[0]), int(self.nx0)
        K, u0, x0 = np.zeros(max(nu0 * nx0, 1)), np.zeros(max(nu0, 1)), np.zeros(max(nx0, 1))
        self._chk(lib().tqgpu_mpc_get_gain(self.h, _dp(K), _dp(u0), _dp(x0)))
        return K[:nu0 * nx0].reshape((nu0, nx0), order="F"), u0[:nu0], x0[:nx0]

    def mpc_sensitivities(self) -> dict:
        """dx (sum_nx, nx0), du (sum_nu, nx0), dlam (sum_lam, nx0): column j is the flat layout of get_solution for parameter x0[j]
        (tqgpu_mpc_get_sensitivities; downloads and waits)."""
        nx0 = int(self.nx0)
        out = {}
        for key, n in (("dx", self.sum_nx), ("du", self.sum_nu), ("dlam", self.sum_lam)):
            out[key] = np.zeros(max(int(n) * nx0, 1))
        self._chk(lib().tqgpu_mpc_get_sensitivities(self.h, _dp(out["dx"]), _dp(out["du"]), _dp(out["dlam"])))
        return {key: out[key][:int(n) * nx0].reshape((int(n), nx0), order="F") for key, n in (("dx", self.sum_nx), ("du", self.sum_nu), ("dlam", self.sum_lam))}

    def mpc_predict(self, x0_new, duals: bool = False) -> tuple:
        """(u0_pred, n_clipped): u0* + K (x0_new - x0_ref), one fma chain per entry, clipped into the root's bounds on a root of kind 0
        (tqgpu_mpc_predict).  duals: the same launch writes lam* + dlam/dx0 (x0_new - x0_ref) into the start buffer, for one solve."""
        a = _f64(x0_new)
        assert len(a) == self.nx0
        u0, n = np.zeros(max(int(self.nu[0]), 1)), C.c_int(0)
        self._chk(lib().tqgpu_mpc_predict(self.h, _dp(a), _dp(u0), int(bool(duals)), C.byref(n)))
        return u0[:int(self.nu[0])], n.value

    # ---- the adjoint of an MPC step: dL/dq, dL/dr, dL/db, dL/dx0 for w = dL/dz (tqgpu_mpc_adjoint) ----
    def mpc_adjoint(self, wx=None, wu=None, profile=0, **kw) -> dict:
        """Adjoint of the last solve's point, active set frozen (tqgpu_mpc_adjoint): wx (sum_nx, nw) and wu (sum_nu, nw) are the loss
        gradient in the flat layout of get_solution, None meaning zero, a 1-D array one column.  Returns dict(gx0 (nx0, nw), n_reg); gq, gr,
        gb stay on the device (mpc_adjoint_grads).  The options give the regularisation rule where the call has to factorise."""
        nw, arrs = None, []
        for a, rows in ((wx, int(self.sum_nx)), (wu, int(self.sum_nu))):
            if a is None:
                arrs.append(None)
                continue
            a = np.asarray(a, dtype=np.float64)
            a = a.reshape((rows, -1), order="F") if a.ndim == 1 else a
            assert a.shape[0] == rows and (nw is None or a.shape[1] == nw), a.shape
            nw = a.shape[1]
            arrs.append(np.asfortranarray(a))
        nw = 1 if nw is None else nw
        n, nx0 = C.c_int(0), int(self.nx0)
        o = _gpu_opts(profile, **kw)
        ptr = [None if a is None else a.ctypes.data_as(c_dbl_p) for a in arrs]
        self._chk(lib().tqgpu_mpc_adjoint(self.h, C.byref(o), ptr[0], ptr[1], int(nw), C.byref(n)))
        self._adj_nw = int(nw)
        g = np.zeros(max(nx0 * nw, 1))
        self._chk(lib().tqgpu_mpc_get_adjoint_x0(self.h, _dp(g)))
        return dict(gx0=g[:nx0 * nw].reshape((nx0, nw), order="F"), n_reg=n.value)

    def mpc_adjoint_grads(self) -> dict:
        """gq (sum_nx, nw), gr (sum_nu, nw), gb (sum_lam, nw) of the last mpc_adjoint: column j is the flat layout of get_solution
        (tqgpu_mpc_get_adjoint; downloads and waits)."""
        sizes = (("gq", int(self.sum_nx)), ("gr", int(self.sum_nu)), ("gb", int(self.sum_lam)))
        nw = self.__dict__.get("_adj_nw", 1)          # (a stale count meets a refusal: the stored adjoint went with what made it stale)
        out = {key: np.zeros(max(n * nw, 1)) for key, n in sizes}
        self._chk(lib().tqgpu_mpc_get_adjoint(self.h, _dp(out["gq"]), _dp(out["gr"]), _dp(out["gb"])))
        return {key: out[key][:n * nw].reshape((n, nw), order="F") for key, n in sizes}

    # ---- the tangent of an MPC step along directions in q, r, b, x0 (tqgpu_mpc_tangent), and the predictor built on it (tqgpu_mpc_predict_at) ----
    def mpc_tangent(self, dq=None, dr=None, db=None, dx0=None, profile=0, **kw) -> dict:
        """Tangent of the last solve's point, active set frozen (tqgpu_mpc_tangent): dq (sum_nx, nd), dr (sum_nu, nd), db (sum_lam, nd) and dx0
        (nx0, nd) are directions in the flat layouts of q, r, b and x0, None meaning zero, a 1-D array one column.  Returns dict(du0 (nu[0], nd),
        n_reg); dx, du, dlam stay on the device (mpc_tangent_values).  The options give the regularisation rule where the call has to factorise."""
        nd, arrs = None, []
        for a, rows in ((dq, int(self.sum_nx)), (dr, int(self.sum_nu)), (db, int(self.sum_lam)), (dx0, int(self.nx0))):
            if a is None:
                arrs.append(None)
                continue
            a = np.asarray(a, dtype=np.float64)
            a = a.reshape((rows, -1), order="F") if a.ndim == 1 else a
            assert a.shape[0] == rows and (nd is None or a.shape[1] == nd), a.shape
            nd = a.shape[1]
            arrs.append(np.asfortranarray(a))
        nd = 1 if nd is None else nd
        n, nu0 = C.c_int(0), int(self.nu[0])
        o = _gpu_opts(profile, **kw)
        ptr = [None if a is None else a.ctypes.data_as(c_dbl_p) for a in arrs]
        self._chk(lib().tqgpu_mpc_tangent(self.h, C.byref(o), ptr[0], ptr[1], ptr[2], ptr[3], int(nd), C.byref(n)))
        self._tan_nd = int(nd)
        return dict(du0=self.mpc_tangent_u0(), n_reg=n.value)

    def mpc_tangent_u0(self) -> np.ndarray:
        """du0 (nu[0], nd) of the last mpc_tangent or mpc_predict_at (tqgpu_mpc_get_tangent_u0; host state only)."""
        nd, nu0 = self.__dict__.get("_tan_nd", 1), int(self.nu[0])
        g = np.zeros(max(nu0 * nd, 1))
        self._chk(lib().tqgpu_mpc_get_tangent_u0(self.h, _dp(g)))
        return g[:nu0 * nd].reshape((nu0, nd), order="F")

    def mpc_tangent_values(self) -> dict:
        """dx (sum_nx, nd), du (sum_nu, nd), dlam (sum_lam, nd) of the last mpc_tangent or mpc_predict_at: column j is the flat layout of
        get_solution (tqgpu_mpc_get_tangent; downloads and waits)."""
        sizes = (("dx", int(self.sum_nx)), ("du", int(self.sum_nu)), ("dlam", int(self.sum_lam)))
        nd = self.__dict__.get("_tan_nd", 1)          # (a stale count meets a refusal: the stored tangent went with what made it stale)
        out = {key: np.zeros(max(n * nd, 1)) for key, n in sizes}
        self._chk(lib().tqgpu_mpc_get_tangent(self.h, _dp(out["dx"]), _dp(out["du"]), _dp(out["dlam"])))
        return {key: out[key][:n * nd].reshape((n, nd), order="F") for key, n in sizes}

    def mpc_predict_at(self, x0_new=None, t0=-1, duals: bool = False, profile=0, **kw) -> dict:
        """The change the next mpc_step(x0_new, t0=t0) will fold in, as one direction built on the device, and the tangent along it
        (tqgpu_mpc_predict_at): dict(u0 = u0* + du0 clipped into the root's bounds on a root of kind 0, n_clipped, n_reg).  duals: the same
        call writes lam* + dlam into the start buffer, for one solve.  Neither the window nor x0 moves."""
        a = None if x0_new is None else _f64(x0_new)
        assert a is None or len(a) == self.nx0
        u0, nc, nr = np.zeros(max(int(self.nu[0]), 1)), C.c_int(0), C.c_int(0)
        o = _gpu_opts(profile, **kw)
        self._chk(lib().tqgpu_mpc_predict_at(self.h, C.byref(o), _dp(a), int(t0), _dp(u0), int(bool(duals)), C.byref(nc), C.byref(nr)))
        self._tan_nd = 1
        return dict(u0=u0[:int(self.nu[0])], n_clipped=nc.value, n_reg=nr.value)

    # ---- the adjoint in H, A, B: outer products summed over parameter groups (tqgpu_mpc_adjoint_matrices) ----
    def mpc_set_param_groups(self, hgroup=None, cgroup=None):
        """The parameter groups of mpc_adjoint_matrices (tqgpu_mpc_set_param_groups): hgroup[k], cgroup[c] in [-1, groups), -1 meaning in
        no group, None meaning every node its own group; the number of groups is the largest index + 1."""
        Nn = len(self.nk)
        hg = None if hgroup is None else _i32(hgroup)
        cg = None if cgroup is None else _i32(cgroup)
        assert (hg is None or len(hg) == Nn) and (cg is None or len(cg) == Nn), "one entry per node"
        self._chk(lib().tqgpu_mpc_set_param_groups(self.h, None if hg is None else _ip(hg), None if cg is None else _ip(cg),
                                                   0 if hg is None else int(hg.max(initial=-1)) + 1, 0 if cg is None else int(cg.max(initial=-1)) + 1))

    def mpc_adjoint_matrices(self) -> dict:
        """The gradients of the stored adjoint with respect to the matrices the device holds (tqgpu_mpc_adjoint_matrices): a dict of lists,
        one array per group with the column of w as its last axis: gH ((nz, nw) for a kind-0 group, (nz, nz, nw) for a kind-1 group), gh
        (nz, nw), gA (nx_c, nx_p, nw), gB (nx_c, nu_p, nw), gb (nx_c, nw), and for an eliminated root gA0 (one (nx_c, nx0, nw) array per child of
        the root) and gS0 [(nu[0], nx0, nw)]; sizes count the phantom root states of an embedded tree."""
        sizes, nw = _adjmat_sizes(self)
        bufs = {key: np.zeros(max(sum(int(np.prod(shp)) for shp in sizes[key]) * nw, 1)) for key in ADJMAT_KEYS}
        self._chk(lib().tqgpu_mpc_adjoint_matrices(self.h, *[_dp(bufs[key]) for key in ADJMAT_KEYS]))
        return {key: _adjmat_split(bufs[key], sizes[key], nw, key == "gA0") for key in ADJMAT_KEYS}

    # ---- the adjoint in the bounds and in the tracking reference (tqgpu_mpc_get_adjoint_bounds, tqgpu_mpc_adjoint_bounds, tqgpu_mpc_adjoint_reference) ----
    def mpc_get_adjoint_bounds(self) -> dict:
        """gxmin, gxmax (sum_nx, nw), gumin, gumax (sum_nu, nw) of the last mpc_adjoint: v on the side the exported value sits on, 0.0
        elsewhere; column j is the flat layout of get_solution (tqgpu_mpc_get_adjoint_bounds; downloads and waits)."""
        sizes = (("gxmin", int(self.sum_nx)), ("gxmax", int(self.sum_nx)), ("gumin", int(self.sum_nu)), ("gumax", int(self.sum_nu)))
        nw = self.__dict__.get("_adj_nw", 1)
        out = {key: np.zeros(max(n * nw, 1)) for key, n in sizes}
        self._chk(lib().tqgpu_mpc_get_adjoint_bounds(self.h, *[_dp(out[key]) for key, _ in sizes]))
        return {key: out[key][:n * nw].reshape((n, nw), order="F") for key, n in sizes}

    def mpc_adjoint_bounds(self) -> dict:
        """The bound gradients of the stored adjoint summed over the h-groups of mpc_set_param_groups (tqgpu_mpc_adjoint_bounds): glb, gub, lists
        with one (nx + nu, nw) array per group, shaped like gh of mpc_adjoint_matrices."""
        sizes, nw = _adjmat_sizes(self)
        bufs = {key: np.zeros(max(sum(int(np.prod(shp)) for shp in sizes["gh"]) * nw, 1)) for key in ("glb", "gub")}
        self._chk(lib().tqgpu_mpc_adjoint_bounds(self.h, _dp(bufs["glb"]), _dp(bufs["gub"])))
        return {key: _adjmat_split(bufs[key], sizes["gh"], nw) for key in ("glb", "gub")}

    def mpc_adjoint_reference(self) -> dict:
        """The gradient of the stored adjoint in the reference trajectory of mpc_set_tracking (tqgpu_mpc_adjoint_reference): dict(row0, rows, gxref
        (rows, NXT, nw), guref (rows, NUT, nw)) for the rows the window in force reads."""
        row0, rows = C.c_int(0), C.c_int(0)
        self._chk(lib().tqgpu_mpc_adjoint_reference(self.h, None, None, C.byref(row0), C.byref(rows)))
        nxt, nut = int(np.max(self.nx, initial=0)), int(np.max(self.nu, initial=0))          # tracking takes trees of one nx and one nu (0 apart)
        nw = self.__dict__.get("_adj_nw", 1)
        gx, gu = np.zeros(max(rows.value * nxt * nw, 1)), np.zeros(max(rows.value * nut * nw, 1))
        self._chk(lib().tqgpu_mpc_adjoint_reference(self.h, _dp(gx), _dp(gu), None, None))
        return dict(row0=row0.value, rows=rows.value,
                    gxref=np.moveaxis(gx[:rows.value * nxt * nw].reshape((nw, rows.value, nxt)), 0, 2).copy(),
                    guref=np.moveaxis(gu[:rows.value * nut * nw].reshape((nw, rows.value, nut)), 0, 2).copy())

    def export_ahead(self, on: bool) -> None:
        """the solution's packing kernel and download go out behind the solve's launch (callers that fetch the solution after every solve)"""
        self._chk(lib().tqgpu_set_export_ahead(self.h, int(bool(on))))

    def event_timing(self, on: bool) -> None:
        """Per-solve HIP event pairs on / off (off: device_times() gives NaN for single-launch solves)."""
        self._chk(lib().tqgpu_set_event_timing(self.h, int(bool(on))))

    def solve(self, profile=0, **kw) -> dict:
        key = (profile, tuple(sorted(kw.items())))
        cache = self.__dict__.setdefault("_opts_cache", {})
        o = cache.get(key)
        if o is None:                       # the options struct of a (profile, kwargs) combination is built once
            o = GpuOpts(maxIter=100, termCondition=2, stationarityTolerance=1e-8, regType=2, regTol=1e-6, regValue=1e-6,
                        lineSearchMaxIter=50, lineSearchGamma=0.1, lineSearchBeta=0.6, lineSearchRestartTrigger=-1, profile=profile, checkLastActiveSet=1)
            for k, v in kw.items():
                if not hasattr(o, k):
                    raise KeyError(k)
                setattr(o, k, v)
            cache[key] = o
        r = GpuResult()
        self._chk(lib().tqgpu_solve(self.h, C.byref(o), C.byref(r)))
        return {f: getattr(r, f) for f, _ in GpuResult._fields_}

    def solve_n(self, n: int, profile=0, **kw):
        """n solves back to back (the reference drivers' NREP loop, in C) -> (last result, sum of iterations, of trials, of launches)."""
        key = (profile, tuple(sorted(kw.items())))
        cache = self.__dict__.setdefault("_opts_cache", {})
        o = cache.get(key)
        if o is None:
            o = GpuOpts(maxIter=100, termCondition=2, stationarityTolerance=1e-8, regType=2, regTol=1e-6, regValue=1e-6,
                        lineSearchMaxIter=50, lineSearchGamma=0.1, lineSearchBeta=0.6, lineSearchRestartTrigger=-1, profile=profile, checkLastActiveSet=1)
            for k, v in kw.items():
                if not hasattr(o, k):
                    raise KeyError(k)
                setattr(o, k, v)
            cache[key] = o
        r = GpuResult()
        it, ls, la = C.c_long(0), C.c_long(0), C.c_long(0)
        self._chk(lib().tqgpu_solve_n(self.h, C.byref(o), int(n), C.byref(r), C.byref(it), C.byref(ls), C.byref(la)))
        return {f: getattr(r, f) for f, _ in GpuResult._fields_}, it.value, ls.value, la.value

    def solution(self) -> dict:
        out = dict(x=np.zeros(self.sum_nx), u=np.zeros(self.sum_nu), lam=np.zeros(self.sum_lam),
                   mu_x=np.zeros(self.sum_nx), mu_u=np.zeros(self.sum_nu), dlam=np.zeros(self.sum_lam))
        self._chk(lib().tqgpu_get_solution(self.h, _dp(out["x"]), _dp(out["u"]), _dp(out["lam"]), _dp(out["mu_x"]), _dp(out["mu_u"]), _dp(out["dlam"])))
        if getattr(self, "sum_nc", 0):          # general constraints were set: the multipliers of the rows
            out["mu_d"] = np.zeros(self.sum_nc)
            self._chk(lib().tqgpu_get_mu_d(self.h, _dp(out["mu_d"])))
        return out

    def kkt_residual(self, per_node=False) -> dict:
        """KKT residuals of the last solve's point, evaluated on the device (tqgpu_kkt_residual): res[6] the largest absolute entry of
        each class of KKT_CLASSES, node[6] the lowest node that attains it (-1: class without entries), max the largest of res (NaN if
        any is) -- the figure tree_qp_out_max_KKT_res gives; per_node=True adds the (Nn, 6) maxima of every node."""
        res, node = np.zeros(6), np.zeros(6, dtype=np.int32)
        pn = np.zeros((len(self.nk), 6)) if per_node else None
        self._chk(lib().tqgpu_kkt_residual(self.h, _dp(res), _ip(node), _dp(pn)))
        return _kkt_dict(res, node, pn)

    def kkt_residual_at(self, sol: dict, mu_d=None, per_node=False) -> dict:
        """The same for any point: sol as solution() returns it (x, u, lam required; mu_x, mu_u and mu_d -- the argument, else
        sol["mu_d"] -- may be missing or None: zeros).  Needs an uploaded problem, no solve; changes nothing a solve reads."""
        if mu_d is None:
            mu_d = sol.get("mu_d")
        want = dict(x=self.sum_nx, u=self.sum_nu, lam=self.sum_lam, mu_x=self.sum_nx, mu_u=self.sum_nu)
        keep = {}
        for k, n in want.items():
            a = sol.get(k)
            if a is None:
                if k in ("x", "u", "lam"):
                    raise ValueError(f"kkt_residual_at: {k} is required")
                keep[k] = None
                continue
            keep[k] = _f64(a)
            if len(keep[k]) != n:
                raise ValueError(f"kkt_residual_at: {k} has {len(keep[k])} entries, the tree {n}")
        if mu_d is not None:
            mu_d = _f64(mu_d)
            if len(mu_d) != getattr(self, "sum_nc", 0):
                raise ValueError(f"kkt_residual_at: mu_d has {len(mu_d)} entries, the tree {getattr(self, 'sum_nc', 0)} rows")
        res, node = np.zeros(6), np.zeros(6, dtype=np.int32)
        pn = np.zeros((len(self.nk), 6)) if per_node else None
        self._chk(lib().tqgpu_kkt_residual_at(self.h, _dp(keep["x"]), _dp(keep["u"]), _dp(keep["lam"]), _dp(keep["mu_x"]), _dp(keep["mu_u"]),
                                              _dp(mu_d), _dp(res), _ip(node), _dp(pn)))
        return _kkt_dict(res, node, pn)

    def iteration_log(self, cap=4096):
        ls = np.zeros(cap, dtype=np.int32)
        tt = np.full(cap, np.nan)
        self._chk(lib().tqgpu_get_iteration_log(self.h, _ip(ls), _dp(tt), cap))
        return ls, tt

    def geometry(self) -> dict:
        """block levels, tiers and workgroups of the persistent launch, and how many such workgroups the device holds at once"""
        v = [C.c_int() for _ in range(5)]
        self._chk(lib().tqgpu_geometry(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("levels", "tiers", "workgroups", "capacity", "compute_units"), [x.value for x in v]))

    def iteration_cost(self, n_ls=1):
        b, f = C.c_double(), C.c_double()
        self._chk(lib().tqgpu_iteration_cost(self.h, int(n_ls), C.byref(b), C.byref(f)))
        return b.value, f.value

    # ---- one tree sharded over several devices ----
    def shard_init(self, rank: int, nranks: int, unique_id: bytes | None = None):
        """Restrict this mirror to rank `rank` of `nranks`.  unique_id: 128-byte RCCL id from
        ``shard_unique_id()`` of rank 0 (broadcast by the caller); None = virtual rank (no communicator)."""
        buf = None if unique_id is None else C.create_string_buffer(bytes(unique_id), 128)
        self._chk(lib().tqgpu_shard_init(self.h, int(rank), int(nranks), buf))
        return self

    def shard_gather_solution(self):
        self._chk(lib().tqgpu_shard_gather_solution(self.h))

    # ---- one tree sharded over several devices inside the persistent launch ----
    def pshard_init(self, rank: int, nranks: int):
        self._chk(lib().tqgpu_pshard_init(self.h, int(rank), int(nranks)))
        return self

    def pshard_ipc_export(self) -> bytes:
        buf = C.create_string_buffer(64)
        self._chk(lib().tqgpu_pshard_ipc_export(self.h, buf))
        return bytes(buf.raw)

    def pshard_ipc_connect(self, r: int, handle: bytes):
        self._chk(lib().tqgpu_pshard_ipc_connect(self.h, int(r), C.create_string_buffer(bytes(handle), 64)))

    def pshard_begin(self, **kw):
        o = _default_opts(**kw)
        self._chk(lib().tqgpu_pshard_begin(self.h, C.byref(o)))

    def pshard_rewind(self):
        self._chk(lib().tqgpu_pshard_rewind(self.h))

    def pshard_end(self) -> dict:
        r = GpuResult()
        self._chk(lib().tqgpu_pshard_end(self.h, C.byref(r)))
        return {f: getattr(r, f) for f, _ in GpuResult._fields_}

    def pshard_pack(self) -> np.ndarray:
        L = lib()
        L.tqgpu_pshard_pack_size.restype = C.c_long
        n = int(L.tqgpu_pshard_pack_size(self.h))
        out = np.zeros(max(n, 1), dtype=np.float64)
        self._chk(L.tqgpu_pshard_pack(self.h, _dp(out), C.c_long(n)))
        return out

    def pshard_unpack(self, src_rank: int, buf: np.ndarray):
        buf = _f64(buf)
        self._chk(lib().tqgpu_pshard_unpack(self.h, int(src_rank), _dp(buf), C.c_long(len(buf))))

    def close(self):
        if self.h:
            lib().tqgpu_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
