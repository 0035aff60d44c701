"""What the instance-parameter tests share (test_instance_params.py, test_gpu_instance_params.py): the parameter sets, the lane-sequential
harness with a parameter table (tests/hostsim/params_hostsim.cpp) and the GPU runners.  Instance b of a handle with a table must equal,
to the bit, instance b of a uniform handle (same batch, same samples) created with the instance's set.
TEST INFRASTRUCTURE ONLY.  Importing this module does not touch the GPU."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import direct_lib as DL
import epoch_lib as EL
import hostsim_lib as HL
from decentralized_ekf_mhe_amd import go1_params
from decentralized_ekf_mhe_amd.params import DekfParams

LIB = os.path.join(DL.HOSTSIM, "libparams_hostsim.so")
# the per-instance fields of dekf_params (include/dekf.h: dekf_set_instance_params)
NOISE_FIELDS = ("p_init_std", "v_init_std", "foot_init_std", "accel_bias_init_std", "p_process_std", "accel_input_std", "gyro_input_std",
                "accel_bias_std", "joint_position_std", "joint_velocity_std", "foot_slide_std", "foot_swing_std", "vo_p_std", "ekf_init_std",
                "ekf_process_std", "ekf_gravity_meas_std", "ekf_vo_meas_std", "ekf_quaternion_init")
# Set 0 is the shape's defaults.  Sets 1 and 2 scale every std by factors within x / / 4, another factor on every component (so a
# component taken from the wrong slot shows), and turn the initial quaternion by a few degrees.  Set 1 changes every noise field, set
# 2 every one again by other factors: a field the table forgets is a mismatch in both.
_AXES = {1: (2.0, 0.5, 1.5, 0.75, 3.0, 0.4, 1.25, 2.5), 2: (0.6, 1.8, 0.3, 2.2, 0.9, 3.5, 0.45, 1.6)}
_FIELD = {1: 1.0, 2: 1.1}
_QUAT = {1: (0.03, -0.02, 0.05), 2: (-0.04, 0.025, -0.03)}   # rotation vectors (rad) of the initial orientation


def _quat(rv):
    a = float(np.linalg.norm(rv))
    return np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * np.asarray(rv) / a])


def param_set(p, k):
    """set k (0, 1, 2) of the shape whose parameters are p"""
    q = p.copy()
    if k == 0:
        return q
    for i, f in enumerate(NOISE_FIELDS[:-1]):
        a = getattr(q, f)
        for j in range(len(a)):
            fac = _AXES[k][(i + j) % 8] * _FIELD[k]
            assert 0.25 <= fac <= 4.0 and fac != 1.0
            a[j] = a[j] * fac
    for j, v in enumerate(_quat(_QUAT[k])):
        q.ekf_quaternion_init[j] = v
    return q


def param_sets(p):
    return [param_set(p, k) for k in range(3)]


def changed_fields(a, b):
    """names of the dekf_params fields in which a and b differ"""
    out = []
    for f, _ in DekfParams._fields_:
        va, vb = getattr(a, f), getattr(b, f)
        if (list(va) != list(vb)) if hasattr(va, "__len__") else (va != vb):
            out.append(f)
    return out


# name: (params, B, set_of).  Go1 with every set, the tripod (generic kernel, 6 joints per leg) and Go1 with foot states (ns = 21)
CPU_SHAPES = {"go1": (lambda: DL._params(go1_params), 3, [2, 0, 1]),
              "tripod": (lambda: DL.tripod_params(), 2, [1, 2]),
              "go1_foot": (lambda: DL._params(go1_params, leg_odom_type=1), 2, [2, 1])}
K_LOG = 60
GPU_SHAPES = {"go1": (lambda: DL._params(go1_params), 6, [0, 1, 2, 2, 0, 1], "k_mhe_solve_direct_4_n20"),
              "tripod": (lambda: DL.tripod_params(), 3, [1, 2, 0], "k_mhe_solve_direct_3"),
              "go1_foot": (lambda: DL._params(go1_params, leg_odom_type=1), 4, [2, 1, 0, 2], "k_mhe_solve_direct_foot_4")}
TWIN_SUFFIX = {"plain": "_pp", "smooth": "_smooth_pp", "cross": "_smooth_cross_pp"}

# ------------------------------------------------------------------ the lane-sequential harness with a table
_libs = {}


def params_hostsim():
    """tests/hostsim/params_hostsim.cpp as libparams_hostsim.so, rebuilt when a source is newer, and bound"""
    if "lib" not in _libs:
        srcs = [os.path.join(DL.HOSTSIM, f) for f in ("hostsim.cpp", "direct_hostsim.cpp", "epoch_hostsim.cpp", "params_hostsim.cpp")] + \
            [os.path.join(DL.CSRC, f) for f in os.listdir(DL.CSRC) if f.endswith(".h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in srcs):
            subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-DDEKF_HOSTSIM", "-w", "-O2", "-o", LIB,
                                   os.path.join(DL.HOSTSIM, "params_hostsim.cpp")])
        L = HL._bind(C.CDLL(LIB))
        vp, dp, ip, pp = C.c_void_p, HL._dp, HL._ip, C.POINTER(DekfParams)
        L.hs_epochs_create.restype = vp
        L.hs_epochs_create.argtypes = [C.c_int]
        L.hs_epochs_destroy.argtypes = [vp]
        L.hs_instance_ticks.argtypes = [vp, C.c_int, ip]
        L.hs_epochs_copy.argtypes = [vp, ip, ip]
        L.hs_tables_create.restype = vp
        L.hs_tables_create.argtypes = [vp]
        L.hs_tables_destroy.argtypes = [vp]
        L.hs_set_instance_params.restype = C.c_int
        L.hs_set_instance_params.argtypes = [vp, vp, pp, vp, C.c_int, ip]
        L.hs_reset_instances_pp.argtypes = [vp, vp, vp, ip, dp]
        L.hs_ekf_step_pp.argtypes = [vp, vp, vp]
        L.hs_update_direct_pp.argtypes = [vp, vp, vp, C.c_int, dp]
        L.hs_update_direct_smooth_pp.argtypes = [vp, vp, vp, C.c_int, dp, dp, dp]
        L.hs_update_direct_cross_pp.argtypes = [vp, vp, vp, C.c_int, dp, dp, dp, dp, dp]
        L.hs_cfg_bytes.restype = C.c_int
        L.hs_cfg_bytes.argtypes = [pp, pp, C.c_int, C.c_int, vp]
        L.hs_ekf_table_len.restype = C.c_int
        _libs["lib"] = L
    return _libs["lib"]


class ParamsSim(HL.HostSim):
    """hostsim_lib.HostSim on the parameter harness: what a direct handle with a table runs from tick 0 on (epoch_lib.EpochSim with
    the table as one more argument)"""

    def __init__(self, params, batch, variant="plain"):
        assert variant in DL.VARIANTS
        self.p, self.B, self.L, self.variant = params, batch, params_hostsim(), variant
        self.h = self.L.hs_create(C.byref(params), batch)
        assert self.h, "hs_create rejected the parameters"
        self.e = self.L.hs_epochs_create(batch)
        self.t = self.L.hs_tables_create(self.h)
        ns = params.dim_state
        self.cov = np.full((batch, ns, ns), np.nan)
        self.win = {}

    def __del__(self):
        if getattr(self, "t", None):
            self.L.hs_tables_destroy(self.t)
            self.t = None
        if getattr(self, "e", None):
            self.L.hs_epochs_destroy(self.e)
            self.e = None
        super().__del__()

    def set_params(self, sets, set_of):
        arr = (DekfParams * len(sets))(*[s.copy() for s in sets])
        so = np.ascontiguousarray(set_of, np.int32)
        return self.L.hs_set_instance_params(self.h, self.t, C.byref(self.p), C.cast(arr, C.c_void_p), len(sets), HL._p(so))

    def reset(self, instances):
        mask = np.zeros(self.B, np.int32)
        mask[list(instances)] = 1
        self.L.hs_reset_instances_pp(self.h, self.e, self.t, HL._p(mask), HL._p(self.cov))

    def ticks(self, T):
        t = np.zeros(self.B, np.int32)
        self.L.hs_instance_ticks(self.e, T, HL._p(t))
        return t

    def epochs(self):
        t0, c0 = np.zeros(self.B, np.int32), np.zeros(self.B, np.int32)
        self.L.hs_epochs_copy(self.e, HL._p(t0), HL._p(c0))
        return t0, c0

    def ekf_step(self):
        self.L.hs_ekf_step_pp(self.h, self.e, self.t)

    def step(self, T):
        self.ekf_step()
        self.update(T)

    def update(self, T):
        ns, N, B = self.p.dim_state, self.p.N, self.B
        if self.variant == "plain":
            self.L.hs_update_direct_pp(self.h, self.e, self.t, T, HL._p(self.cov))
            return
        self.win = dict(xw=np.full((B, N, ns), DL.FILL), cw=np.full((B, N, ns, ns), DL.FILL))
        if self.variant == "smooth":
            self.L.hs_update_direct_smooth_pp(self.h, self.e, self.t, T, HL._p(self.cov), HL._p(self.win["xw"]), HL._p(self.win["cw"]))
        else:
            self.win.update(l1=np.full((B, N - 1, ns, ns), DL.FILL), zn=np.full((B, N, ns, ns), DL.FILL))
            self.L.hs_update_direct_cross_pp(self.h, self.e, self.t, T, HL._p(self.cov), *(HL._p(self.win[k]) for k in EL.WINDOW_KEYS))


def run_params_sim(p, s, B, K, variant, sets, set_of, resets=None, new_sets=None):
    """[tick] -> what the parameter harness left at every tick of the log: the table (sets, set_of) set before tick 0; the instances of
    resets[k] restarted before tick k and then given new_sets[k] ({instance: set index}; none: they keep their set)"""
    sim = ParamsSim(p, B, variant)
    assert sim.set_params(sets, set_of) == 0
    resets, new_sets = resets or {}, new_sets or {}
    out = []
    for k in range(K):
        if k in resets:
            sim.reset(resets[k])
            if k in new_sets:
                so = np.full(B, -1, np.int32)
                for b, i in new_sets[k].items():
                    so[b] = i
                assert sim.set_params(sets, so) == 0
        sim.feed(s, k)
        sim.step(k)
        out.append(dict(EL._record(sim, sim.cov), ticks=sim.ticks(k)))
    return out


@functools.lru_cache(maxsize=None)
def cpu_streams(name):
    mk, B, _ = CPU_SHAPES[name]
    p = mk()
    return p, DL.rough_streams(p, B, K_LOG)


@functools.lru_cache(maxsize=None)
def cpu_uniform(name, variant, k, T0=0):
    """the reference: the harness WITHOUT table or epochs (direct_lib.DirectSim) created with set k of the shape, on the log from T0"""
    p, s = cpu_streams(name)
    B = CPU_SHAPES[name][1]
    return EL.run_fresh_sim(param_set(p, k), EL.slice_streams(s, T0) if T0 else s, B, K_LOG - T0, variant)


# ------------------------------------------------------------------ the GPU runners
GPU_KEYS = EL.GPU_KEYS


def run_gpu(p, s, B, K, variant, sets=None, set_of=None, resets=None, new_sets=None, est=None, close=True):
    """epoch_lib.run_gpu's loop on a handle with the table (sets, set_of) set before tick 0 (sets None: no table): ([tick] -> every
    getter, kernel names at the start and after every restart, handle).  The instances of resets[k] are restarted before tick k and
    then given new_sets[k] ({instance: set index}; none: they keep their set)"""
    from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host
    est = est or BatchedEstimator(p, B, solver="direct", **DL.VARIANTS[variant])
    if sets is not None:
        est.set_instance_params(sets, set_of)
    resets, new_sets = resets or {}, new_sets or {}
    sh = streams_host(s)
    out = []
    names = [(est.solve_kernel_name(True), est.solve_kernel_name(False))]
    for k in range(K):
        if k in resets:
            mask = np.zeros(B, np.int32)
            mask[list(resets[k])] = 1
            est.reset_instances(mask)
            if k in new_sets:
                so = np.full(B, -1, np.int32)
                for b, i in new_sets[k].items():
                    so[b] = i
                est.set_instance_params(sets, so)
            names.append((est.solve_kernel_name(True), est.solve_kernel_name(False)))
        est.push_stream_step(sh, k)
        est.step(k)
        r = EL.gpu_record(est)
        r["ticks"] = est.instance_ticks()
        if k:
            r["cov"] = est.mhe_cov()
            r["Kmax"] = max(EL.local_K(int(t), p.N) for t in r["ticks"])
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
def gpu_streams(name, K=K_LOG):
    mk, B, _, _ = GPU_SHAPES[name]
    p = mk()
    return p, DL.rough_streams(p, B, K)


@functools.lru_cache(maxsize=None)
def gpu_uniform(name, variant, k, T0=0):
    """the reference of every instance on set k: a uniform handle created with that set (same batch, same samples) on the log from
    T0, once per process"""
    p, s = gpu_streams(name)
    B = GPU_SHAPES[name][1]
    return EL.run_gpu(param_set(p, k), EL.slice_streams(s, T0) if T0 else s, B, K_LOG - T0, variant)[0]
