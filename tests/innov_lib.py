"""What the innovation tests share (test_innovation.py, test_gpu_innovation.py): the limits, the oracle reference, the error
measures, the lane-sequential harness (tests/hostsim/innov_hostsim.cpp) and the GPU runner.
TEST INFRASTRUCTURE ONLY.  Importing this module does not touch the GPU."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import direct_lib as DL
import hostsim_lib as HL
import oracle_lib as O
from decentralized_ekf_mhe_amd import cassie_params, go1_params, pogox_params

KEYS = ("innov", "innov_cov", "nis", "nis_leg", "loglik")
INNOV_KERNELS = [f"k_mhe_innov_{L}{t}" for L in (1, 2, 3, 4) for t in ("", "_ep")]
MAX_VGPRS = 72   # the direct kernels' class

# The limits.  The reference frees the newest Meas rows of the oracle's window QP, takes x^- and P^- from the inverse of its KKT matrix
# and forms nu = y - H x^- and S = H P^- H' + Q_m^-1; the core takes the posterior route (mhe_innov_core.h).  Measured, lane-sequential
# build against that reference, worst over every checked tick and instance of CPU_CASES (test_innovation.py prints them):
#     nu         6.6e-12 of sqrt(S*_ii)      (Go1; Cassie 5.3e-12, tripod 4.3e-12, PogoX 3.7e-22)
#     S          4.0e-15 by direct_lib.cov_err (tripod)     limit: the project's covariance yardstick CREL = 1e-7
#     NIS        5.9e-12 relative (Cassie); in the flight phases, where NIS is about 1e-15, 3.0e-27 absolute
#     nis_leg    6.3e-12 relative (tripod); on legs in flight 4.5e-27 absolute
#     loglik     9.9e-11 absolute (Go1; log det S = 386.8 in flight)
# The limits are ten times those: the device build differs from the lane-sequential one only by the register sweep and libm's log.
# The absolute floor of the NIS limits is not measured but reasoned: in flight every Q_m entry is 1e-14 and NIS = 1e-14 |nu|^2, so an
# error dx in x^- moves it by 2 |nu|_1 1e-14 dx; with |nu|_1 <= 12 * 0.5 and dx the project's own yardstick for x (direct_lib.XABS =
# 1e-10) that is 1.2e-23.  Eight orders below the flight phases' NIS itself and twenty-three below a NIS that means anything.
NU_TOL = 6.6e-11                    # |nu - nu*|_i <= NU_TOL sqrt(S*_ii)
NIS_REL, NIS_ABS = 6.3e-11, 1.2e-23  # |nis - nis*| <= NIS_REL nis* + NIS_ABS, whole and per leg
LOGLIK_ABS = 1e-9                   # |loglik - loglik*|


# ------------------------------------------------------------------ the oracle reference
def reference_of_qp(p, qp, k):
    """The innovation statistics of the oracle's window QP `qp` (Est.qp()) at step k >= 1: the newest Meas rows are made free, x^- and
    P^- come from direct_lib.kkt_of_qp of that QP, then nu, S, NIS, the per-leg NIS and log det S by slogdet.  Also the VO equality rows
    of the window"""
    ns, nm, L = p.dim_state, 3 * p.num_legs, p.num_legs
    H, g, A, l, u = qp
    n = H.shape[0]
    xo_T = n - ns - nm                                  # the newest block: x_T (ns) | its Meas slacks (nm)
    sl = np.arange(xo_T + ns, xo_T + ns + nm)
    rows = np.nonzero(np.abs(A[:, sl]).sum(axis=1))[0]
    assert len(rows) == nm
    assert np.array_equal(A[rows][:, sl], -np.eye(nm))  # each with slack coefficient -1, in the slacks' order
    assert np.array_equal(l[rows], u[rows])
    l2, u2 = l.copy(), u.copy()
    l2[rows], u2[rows] = -1e30, 1e30
    x, Ki, xo, nv = DL.kkt_of_qp(p, (H, g, A, l2, u2), k)
    assert xo[-1] == xo_T
    Hm, y, Qm = A[rows][:, xo_T:xo_T + ns], l[rows], H[np.ix_(sl, sl)]
    xm, Pm = x[xo_T:xo_T + ns], Ki[xo_T:xo_T + ns, xo_T:xo_T + ns]
    nu = y - Hm @ xm
    S = Hm @ Pm @ Hm.T + np.linalg.inv(Qm)
    S = 0.5 * (S + S.T)
    nis = float(nu @ np.linalg.solve(S, nu))
    nis_leg = np.array([nu[3 * i:3 * i + 3] @ np.linalg.solve(S[3 * i:3 * i + 3, 3 * i:3 * i + 3], nu[3 * i:3 * i + 3]) for i in range(L)])
    sign, logdet = np.linalg.slogdet(S)
    assert sign > 0
    return dict(innov=nu, innov_cov=S, nis=nis, nis_leg=nis_leg, logdet=float(logdet),
                loglik=-0.5 * (nis + float(logdet) + nm * np.log(2 * np.pi)), vo=nv)


def reference(p, s, b, ticks):
    """{tick: reference_of_qp} of instance b of the streams through the oracle's pipe"""
    pipe = O.Pipe(p)
    out = {}
    for k in range(max(ticks) + 1):
        pipe.feed(s, k, b)
        pipe.step(k)
        if k in ticks:
            out[k] = reference_of_qp(p, pipe.est.qp(), k)
    return out


# ------------------------------------------------------------------ error measures
def errors(got, ref):
    """the five errors of one instance at one tick, got: {key: array of the instance}: nu in units of sqrt(S*_ii), S by cov_err, NIS and
    the per-leg NIS in units of their limit (<= 1 passes), loglik absolute"""
    d = np.sqrt(np.diagonal(ref["innov_cov"]))
    return dict(nu=float((np.abs(got["innov"] - ref["innov"]) / d).max()),
                S=DL.cov_err(got["innov_cov"], ref["innov_cov"]),
                nis=float(abs(got["nis"] - ref["nis"]) / (NIS_REL * ref["nis"] + NIS_ABS)),
                nis_leg=float((np.abs(got["nis_leg"] - ref["nis_leg"]) / (NIS_REL * ref["nis_leg"] + NIS_ABS)).max()),
                loglik=float(abs(got["loglik"] - ref["loglik"])))


def assert_within_limits(e, what):
    assert e["nu"] <= NU_TOL and e["S"] <= DL.CREL and e["nis"] <= 1.0 and e["nis_leg"] <= 1.0 and e["loglik"] <= LOGLIK_ABS, (what, e)


def check_identities(g, L, what):
    """what the five arrays of one instance owe each other: S symmetric to the bit, nis = nu'S^-1 nu and loglik its definition from the
    returned arrays"""
    nu, S = g["innov"], g["innov_cov"]
    nm = 3 * L
    assert np.array_equal(S, S.T), what
    # (S spans 1e14 against 1e-6 inside one matrix on a tick with mixed contact: the check scales it by its diagonal, as the core does)
    d = 1.0 / np.sqrt(np.diagonal(S))
    nis = float((nu * d) @ np.linalg.solve(S * d[:, None] * d[None, :], nu * d))
    assert abs(g["nis"] - nis) <= 1e-9 * nis + NIS_ABS, (what, g["nis"], nis)
    sign, logdet = np.linalg.slogdet(S * d[:, None] * d[None, :])
    logdet = float(logdet) - 2.0 * float(np.log(d).sum())
    assert sign > 0
    want = -0.5 * (g["nis"] + logdet + nm * np.log(2 * np.pi))
    assert abs(g["loglik"] - want) <= 1e-9 * abs(want), (what, g["loglik"], want)
    assert (g["nis_leg"] >= 0).all() and np.isfinite(g["nis_leg"]).all(), what


def contact_kind(s, k, b):
    """'flight' (no leg in contact), 'stance' (all) or 'mixed' at tick k of instance b"""
    c = s["contact"][k, b]
    return "flight" if not c.any() else ("stance" if c.all() else "mixed")


# ------------------------------------------------------------------ the lane-sequential harness
LIB = os.path.join(DL.HOSTSIM, "libinnov_hostsim.so")
_libs = {}


def innov_hostsim():
    """tests/hostsim/innov_hostsim.cpp as libinnov_hostsim.so, rebuilt when a source is newer, and bound"""
    if "lib" not in _libs:
        srcs = [os.path.join(DL.HOSTSIM, f) for f in ("hostsim.cpp", "direct_hostsim.cpp", "innov_hostsim.cpp")] + \
            [os.path.join(DL.CSRC, f) for f in os.listdir(DL.CSRC) if f.endswith(".h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(f) > os.path.getmtime(LIB) for f in srcs):
            subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-DDEKF_HOSTSIM", "-w", "-O2", "-o", LIB,
                                   os.path.join(DL.HOSTSIM, "innov_hostsim.cpp")])
        L = HL._bind(C.CDLL(LIB))
        L.hs_update_direct_innov.argtypes = [C.c_void_p, C.c_int] + [HL._dp] * 6
        L.hs_update_direct_innov.restype = C.c_int
        _libs["lib"] = L
    return _libs["lib"]


class InnovSim(HL.HostSim):
    """hostsim_lib.HostSim on the innovation harness: step(T) runs the assemble step, the plain direct core and the innovation core,
    and keeps Cov(x_T) and the five arrays (NaN before the update)"""

    def __init__(self, params, batch):
        self.p, self.B, self.L = params, batch, innov_hostsim()
        self.h = self.L.hs_create(C.byref(params), batch)
        assert self.h, "hs_create rejected the parameters"
        self.cov, self.out = None, None

    def step(self, T):
        self.L.hs_ekf_step(self.h)
        if T == 0:
            self.L.hs_initialize(self.h)
            return
        B, ns, L = self.B, self.p.dim_state, self.p.num_legs
        nm = 3 * L
        self.cov = np.zeros((B, ns, ns))
        self.out = dict(innov=np.full((B, nm), np.nan), innov_cov=np.full((B, nm, nm), np.nan), nis=np.full(B, np.nan),
                        nis_leg=np.full((B, L), np.nan), loglik=np.full(B, np.nan))
        assert self.L.hs_update_direct_innov(self.h, T, HL._p(self.cov), *(HL._p(self.out[k]) for k in KEYS)) == 0


def run_sim(p, s, B, K, ticks):
    """{tick: the five arrays, status and Cov(x_T)} of a lane-sequential run"""
    sim = InnovSim(p, B)
    out = {}
    for k in range(K):
        sim.feed(s, k)
        sim.step(k)
        if k in ticks:
            out[k] = dict({key: a.copy() for key, a in sim.out.items()}, status=sim.get()["status"], cov=sim.cov.copy())
    return out


def instance(rec, b):
    return {key: rec[key][b] for key in KEYS}


# name: (params, B, ticks run, ticks checked).  Go1, Cassie and the tripod on the ticks of direct_lib.CORE_CASES (fill, full windows,
# the flight phase of instance 0 from tick 22 on, VO equality rows from tick 40 on), PogoX (N = 100) inside its window fill
_CORE_TICKS = list(range(1, 48, 3)) + [41, 44, 47]
CPU_CASES = {
    "go1": (lambda: DL._params(go1_params), 2, 48, _CORE_TICKS),
    "cassie": (lambda: DL._params(cassie_params), 2, 48, _CORE_TICKS),
    "tripod": (lambda: DL.tripod_params(), 2, 48, _CORE_TICKS),
    "pogox": (lambda: DL._params(pogox_params), 1, 13, list(range(1, 13))),
}
# the GPU's: (params, B, ticks run, instances held against the oracle, innovation kernel).  Every tick from 1 on is checked
GPU_CASES = {
    "go1": (lambda: DL._params(go1_params), 6, 48, [0, 1], "k_mhe_innov_4"),
    "cassie": (lambda: DL._params(cassie_params), 2, 48, [0, 1], "k_mhe_innov_2"),
    "tripod": (lambda: DL.tripod_params(), 2, 24, [0, 1], "k_mhe_innov_3"),
    "pogox": (lambda: DL._params(pogox_params), 2, 12, [0, 1], "k_mhe_innov_1"),
}


BIG = 70   # the batch of which the Go1 GPU case is the first six instances (more than one wavefront's worth of workgroups per launch)


@functools.lru_cache(maxsize=None)
def gpu_streams(name):
    """(params, streams) of a GPU case; Go1's are the first six robots of a fleet of BIG (big_streams)"""
    mk, B, K, _, _ = GPU_CASES[name]
    p = mk()
    if name == "go1":
        return p, DL.sub_streams(big_streams()[1], np.arange(B), BIG)
    return p, DL.rough_streams(p, B, K)


@functools.lru_cache(maxsize=None)
def big_streams():
    mk, _, K, _, _ = GPU_CASES["go1"]
    p = mk()
    return p, DL.rough_streams(p, BIG, K)


@functools.lru_cache(maxsize=None)
def case_reference(name, gpu=False):
    """(params, streams, {instance: {tick: reference}}) of a case, once per process"""
    if gpu:
        mk, B, K, sub, _ = GPU_CASES[name]
        ticks = list(range(1, K))
        p, s = gpu_streams(name)
    else:
        mk, B, K, ticks = CPU_CASES[name]
        sub = list(range(B))
        p = mk()
        s = DL.rough_streams(p, B, K)
    return p, s, {b: reference(p, s, b, ticks) for b in sub}


@functools.lru_cache(maxsize=None)
def case_sim(name):
    """the lane-sequential run of a case of CPU_CASES, once per process"""
    mk, B, K, ticks = CPU_CASES[name]
    p, s, _ = case_reference(name)
    return run_sim(p, s, B, K, ticks)


# ------------------------------------------------------------------ the GPU runner
def gpu_record(est, variant=None):
    """what a handle returns after an update besides the five arrays: dekf_get, the iteration counts, Cov(x_T), and the window (and
    cross) arrays of a smoothing (cross) handle"""
    o, info = est.get(), est.solver_info()
    r = dict(x=o["x"], v_b=o["v_b"], status=o["status"], iters=info["iters"], cov=est.mhe_cov())
    if variant in ("smooth", "cross"):
        r["K"], r["xw"], r["cw"] = est.window()
    if variant == "cross":
        _, r["l1"], r["zn"] = est.window_cross()
    return r


@functools.lru_cache(maxsize=None)
def gpu_case_run(name, variant="plain", innovation=True):
    """run_gpu of a GPU case, once per process: (records, kernel names)"""
    mk, B, K, _, _ = GPU_CASES[name]
    p, s = gpu_streams(name)
    return run_gpu(p, s, B, K, variant, innovation)[:2]


def run_gpu(p, s, B, K, variant="plain", innovation=True, est=None, close=True):
    """a list over the ticks 1 .. K - 1 of gpu_record, with the five arrays of an innovation handle"""
    from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host
    if est is None:
        est = BatchedEstimator(p, B, solver="direct", innovation=innovation, **DL.VARIANTS[variant])
    sh = streams_host(s)
    out = []
    for k in range(K):
        est.push_stream_step(sh, k)
        est.step(k)
        if k:
            r = gpu_record(est, variant)
            if innovation:
                r.update(est.innovation())
            out.append(r)
    names = (est.solve_kernel_name(True), est.solve_kernel_name(False))
    if close:
        est.close()
    return out, names, est
