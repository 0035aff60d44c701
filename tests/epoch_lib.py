"""What the instance-reset tests share (test_instance_reset.py, test_gpu_instance_reset.py): the reset schedules, the log of one life, the
lane-sequential harness with epochs (tests/hostsim/epoch_hostsim.cpp) and the GPU runners.  A life is (instance, T0, end): the
instance restarted before tick T0 (dekf_reset_instances) and running until its next restart or the end of the log; it must equal a
fresh simulation of the log sliced from T0, tick T0 + j against the fresh run's tick j.
TEST INFRASTRUCTURE ONLY.  Importing this module does not touch the GPU."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import direct_lib as DL
import hostsim_lib as HL
from decentralized_ekf_mhe_amd import go1_params

LIB = os.path.join(DL.HOSTSIM, "libepoch_hostsim.so")
K_LOG = 100
# {tick: instances restarted before that tick}.  rough_streams: the even instances carry the 30 Hz camera, whose VO rows turn into
# equalities from local tick 40 on.  An odd instance before tick 5, the same one again before tick 12 (inside its own window fill),
# an even one before tick 30, one before tick 45 (a full window that holds VO equality rows)
CPU_RESETS = {"go1": {5: [1], 12: [1], 30: [2], 45: [0]},
              "tripod": {5: [1], 12: [1], 30: [2], 45: [0]},
              "go1_foot": {5: [1], 12: [1], 30: [0], 45: [1]}}   # (B = 2: before tick 45 instance 1 again, from a full window)
# name: (params, B).  Until its first restart every instance is an untouched one
CPU_SHAPES = {"go1": (lambda: DL._params(go1_params), 3),
              "tripod": (lambda: DL.tripod_params(), 3),
              "go1_foot": (lambda: DL._params(go1_params, leg_odom_type=1), 2)}
# the GPU schedules: Go1 at B = 6 takes CPU test 2's resets (instance 3 the odd one, 4 the even one) plus {2, 4} together before tick
# 45; the other shapes one restart in the window fill and one in full windows
GPU_RESETS = {"go1": {5: [3], 12: [3], 30: [4], 45: [2, 4]},
              "tripod": {7: [1], 40: [2]},
              "go1_foot": {7: [1], 40: [2]}}
GPU_SHAPES = {"go1": (lambda: DL._params(go1_params), 6, 100, "k_mhe_solve_direct_4_n20"),
              "tripod": (lambda: DL.tripod_params(), 6, 60, "k_mhe_solve_direct_3"),
              "go1_foot": (lambda: DL._params(go1_params, leg_odom_type=1), 4, 60, "k_mhe_solve_direct_foot_4")}
WINDOW_KEYS = ("xw", "cw", "l1", "zn")
TWIN_SUFFIX = {"plain": "_ep", "smooth": "_smooth_ep", "cross": "_smooth_cross_ep"}
SIBLING_SUFFIX = {"plain": "", "smooth": "_smooth", "cross": "_smooth_cross"}


def lives(resets, K):
    """[(instance, T0, end)] of a schedule over a log of K ticks: every restart opens a life that ends at the instance's next one"""
    out = []
    for T0 in sorted(resets):
        for b in resets[T0]:
            later = [t for t in sorted(resets) if t > T0 and b in resets[t]]
            out.append((b, T0, later[0] if later else K))
    return out


def untouched(resets, B):
    return [b for b in range(B) if all(b not in v for v in resets.values())]


def slice_streams(s, T0):
    """the log from tick T0 on: what a fresh handle is fed from its tick 0"""
    K, B = s["imu_t"].shape
    so = {k: (np.ascontiguousarray(v[T0:]) if isinstance(v, np.ndarray) and v.shape[:2] == (K, B) else v) for k, v in s.items()}
    so["vo_any"] = so["vo_mask"].any(axis=1)
    return so


def local_K(tick, N):
    """window length of an instance at its local tick (0 at local tick 0: the initialise path solves nothing)"""
    return min(tick + 1, N) if tick >= 1 else 0


def window_lengths(key, K):
    """written entries of the window array `key` in a window of K steps"""
    return max(K - 1, 0) if key == "l1" else K


# ------------------------------------------------------------------ the lane-sequential harness with epochs
_libs = {}


def epoch_hostsim():
    """tests/hostsim/epoch_hostsim.cpp as libepoch_hostsim.so, rebuilt when a source is newer, and bound"""
    if "lib" not in _libs:
        srcs = [os.path.join(DL.HOSTSIM, f) for f in ("hostsim.cpp", "direct_hostsim.cpp", "epoch_hostsim.cpp")] + \
            [os.path.join(DL.CSRC, f) for f in os.listdir(DL.CSRC) if f.endswith(".h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in srcs):
            subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-DDEKF_HOSTSIM", "-w", "-O2", "-o", LIB,
                                   os.path.join(DL.HOSTSIM, "epoch_hostsim.cpp")])
        L = HL._bind(C.CDLL(LIB))
        vp, dp, ip = C.c_void_p, HL._dp, HL._ip
        L.hs_epochs_create.restype = vp
        L.hs_epochs_create.argtypes = [C.c_int]
        L.hs_epochs_destroy.argtypes = [vp]
        L.hs_reset_instances.argtypes = [vp, vp, ip, dp]
        L.hs_ekf_step_epoch.argtypes = [vp, vp]
        L.hs_instance_ticks.argtypes = [vp, C.c_int, ip]
        L.hs_epochs_copy.argtypes = [vp, ip, ip]
        L.hs_update_direct_epoch.argtypes = [vp, vp, C.c_int, dp]
        L.hs_update_direct_smooth_epoch.argtypes = [vp, vp, C.c_int, dp, dp, dp]
        L.hs_update_direct_cross_epoch.argtypes = [vp, vp, C.c_int, dp, dp, dp, dp, dp]
        L.hs_fold_epoch.restype = C.c_int
        L.hs_fold_epoch.argtypes = [C.c_int] * 4
        _libs["lib"] = L
    return _libs["lib"]


class EpochSim(HL.HostSim):
    """hostsim_lib.HostSim on the epoch harness: what a direct handle runs once dekf_reset_instances has restarted an instance, from
    tick 0 on (every epoch 0 until reset()).  cov is the handle's Cov(x_T) store (persistent: a restarted instance's block stays NaN
    until its first solve); the window arrays of `win` are those of DirectSim, pre-filled with FILL at every step"""

    def __init__(self, params, batch, variant="plain"):
        assert variant in DL.VARIANTS
        self.p, self.B, self.L, self.variant = params, batch, epoch_hostsim(), variant
        self.h = self.L.hs_create(C.byref(params), batch)
        assert self.h, "hs_create rejected the parameters"
        self.e = self.L.hs_epochs_create(batch)
        ns = params.dim_state
        self.cov = np.full((batch, ns, ns), np.nan)   # (no instance has solved yet)
        self.win = {}

    def __del__(self):
        if getattr(self, "e", None):
            self.L.hs_epochs_destroy(self.e)
            self.e = None
        super().__del__()

    def reset(self, instances):
        mask = np.zeros(self.B, np.int32)
        mask[list(instances)] = 1
        self.L.hs_reset_instances(self.h, self.e, HL._p(mask), HL._p(self.cov))

    def ticks(self, T):
        t = np.zeros(self.B, np.int32)
        self.L.hs_instance_ticks(self.e, T, HL._p(t))
        return t

    def epochs(self):
        """(t0, c0): the handle's step and its EKF tick count at every instance's last restart"""
        t0, c0 = np.zeros(self.B, np.int32), np.zeros(self.B, np.int32)
        self.L.hs_epochs_copy(self.e, HL._p(t0), HL._p(c0))
        return t0, c0

    def ekf_step(self):
        self.L.hs_ekf_step_epoch(self.h, self.e)

    def step(self, T):
        self.ekf_step()
        self.update(T)

    def update(self, T):
        """the MHE timer's event alone (T = 0: every instance takes the initialise path)"""
        ns, N, B = self.p.dim_state, self.p.N, self.B
        if self.variant == "plain":
            self.L.hs_update_direct_epoch(self.h, self.e, T, HL._p(self.cov))
            return
        self.win = dict(xw=np.full((B, N, ns), DL.FILL), cw=np.full((B, N, ns, ns), DL.FILL))
        if self.variant == "smooth":
            self.L.hs_update_direct_smooth_epoch(self.h, self.e, T, HL._p(self.cov), HL._p(self.win["xw"]), HL._p(self.win["cw"]))
        else:
            self.win.update(l1=np.full((B, N - 1, ns, ns), DL.FILL), zn=np.full((B, N, ns, ns), DL.FILL))
            self.L.hs_update_direct_cross_epoch(self.h, self.e, T, HL._p(self.cov), *(HL._p(self.win[k]) for k in WINDOW_KEYS))


def _record(sim, cov):
    M, n = sim.arrival()
    out = dict(sim.get(), ekf_cov=sim.ekf_cov(), cov=cov.copy(), M=M, n=n)
    out.update({key: a.copy() for key, a in sim.win.items()})
    return out


def run_epoch_sim(p, s, B, K, variant, resets):
    """[tick] -> what the epoch harness left at every tick of the log, with the schedule `resets` ({} for none)"""
    sim = EpochSim(p, B, variant)
    out = []
    for k in range(K):
        if k in resets:
            sim.reset(resets[k])
        sim.feed(s, k)
        sim.step(k)
        out.append(dict(_record(sim, sim.cov), ticks=sim.ticks(k)))
    return out


def run_fresh_sim(p, s, B, K, variant):
    """[tick] -> what the harness WITHOUT epochs (direct_lib.DirectSim: hs_initialize, hs_update_direct*) left at every tick"""
    sim = DL.DirectSim(p, B, variant)
    out = []
    for k in range(K):
        sim.feed(s, k)
        sim.step(k)
        out.append(_record(sim, sim.cov if sim.cov is not None else np.full((B, p.dim_state, p.dim_state), np.nan)))
    return out


SIM_KEYS = ("x", "v_b", "quat", "p_vo", "status", "iters", "ekf_cov", "cov", "M", "n")


def assert_life_equal(got, fresh, b, T0, end, N, keys, what):
    """instance b of `got` at ticks T0 .. end - 1 against instance b of `fresh` at ticks 0 .. end - T0 - 1: array_equal on `keys`
    and on the first K_b entries of the window arrays (NaN where both are NaN: a block before its first solve)"""
    for j in range(end - T0):
        g, f = got[T0 + j], fresh[j]
        for key in keys:
            assert np.array_equal(g[key][b], f[key][b], equal_nan=True), (what, b, T0, j, key)
        Kb = local_K(j, N)
        for key in WINDOW_KEYS:
            if key in g and Kb:
                n = window_lengths(key, Kb)
                assert np.array_equal(g[key][b, :n], f[key][b, :n]), (what, b, T0, j, key)


# ------------------------------------------------------------------ the GPU runners
def gpu_record(est):
    """what dekf_get, dekf_get_ekf_cov and dekf_get_solver_info hand out after the last update"""
    o, info = est.get(), est.solver_info()
    return dict(x=o["x"], v_b=o["v_b"], quat=o["quat"], p_vo=o["p_vo"], status=o["status"], ekf_cov=est.ekf_cov(),
                iters=info["iters"], rho_updates=info["rho_updates"], pri_res=info["pri_res"], dua_res=info["dua_res"])


GPU_KEYS = ("x", "v_b", "quat", "p_vo", "status", "ekf_cov", "iters", "rho_updates", "pri_res", "dua_res", "cov")


def run_gpu(p, s, B, K, variant, resets=None, device_mask=False, poke=None, est=None, close=True):
    """([tick] -> every getter the contract of dekf_reset_instances names, kernel names, handle) of a direct handle over the log,
    restarting the instances of `resets` ({tick: instances}) before their ticks.  Tick 0 has no cov / window entries, and a tick at
    which no instance has solved since its restart no window entries.  names: (full-window, window-fill) kernel at the start and after
    every call.  poke(est, k) runs before tick k.  est: a handle to run on (after reset()), else a new one"""
    from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host
    resets = resets or {}
    est = est or BatchedEstimator(p, B, solver="direct", **DL.VARIANTS[variant])
    sh = streams_host(s)
    out = []
    names = [(est.solve_kernel_name(True), est.solve_kernel_name(False))]
    for k in range(K):
        if poke:
            poke(est, k)
        if k in resets:
            mask = np.zeros(B, np.int32)
            mask[list(resets[k])] = 1
            if device_mask:
                import torch
                mask = torch.from_numpy(mask).cuda()
                torch.cuda.synchronize()
            est.reset_instances(mask)
            names.append((est.solve_kernel_name(True), est.solve_kernel_name(False)))
        est.push_stream_step(sh, k)
        est.step(k)
        r = gpu_record(est)
        r["ticks"] = est.instance_ticks()
        if k:
            r["cov"] = est.mhe_cov()
            r["Kmax"] = max(local_K(int(t), p.N) for t in r["ticks"])
            if variant != "plain" and r["Kmax"]:
                r["K"], r["xw"], r["cw"] = est.window()
            if variant == "cross" and r["Kmax"]:
                Kc, r["l1"], r["zn"] = est.window_cross()
                assert Kc == r["K"]
        out.append(r)
    if close:
        est.close()
    return out, names, est


@functools.lru_cache(maxsize=None)
def gpu_streams(name):
    mk, B, K, _ = GPU_SHAPES[name]
    p = mk()
    return p, DL.rough_streams(p, B, K)


@functools.lru_cache(maxsize=None)
def gpu_fresh(name, variant, T0):
    """the reference of every life that starts at T0: a fresh handle on the log sliced from T0, once per process"""
    p, s = gpu_streams(name)
    _, B, K, _ = GPU_SHAPES[name]
    return run_gpu(p, slice_streams(s, T0), B, K - T0, variant)[0]


def assert_gpu_life_equal(got, fresh, b, T0, end, N, what):
    """instance b of `got` at ticks T0 .. end - 1 against instance b of `fresh` at ticks 0 .. end - T0 - 1: array_equal on every getter
    (NaN where both are NaN: the residuals of a direct solve, a covariance block before its first solve), the local tick, and the
    first K_b entries of the window arrays"""
    for j in range(end - T0):
        g, f = got[T0 + j], fresh[j]
        for key in GPU_KEYS:
            if key == "cov" and "cov" not in f:     # the fresh handle's tick 0: dekf_get_mhe_cov refuses; the restarted block is NaN
                assert "cov" not in g or np.isnan(g["cov"][b]).all(), (what, b, T0, j)
                continue
            assert np.array_equal(g[key][b], f[key][b], equal_nan=True), (what, b, T0, j, key)
        assert g["ticks"][b] == j, (what, b, T0, j, g["ticks"])
        Kb = local_K(j, N)
        for key in WINDOW_KEYS:
            if key in f and Kb:
                n = window_lengths(key, Kb)
                assert g["K"] == g["Kmax"] >= Kb and f["K"] == Kb, (what, b, T0, j, g["K"], g["Kmax"])
                assert np.array_equal(g[key][b, :n], f[key][b, :n]), (what, b, T0, j, key)
