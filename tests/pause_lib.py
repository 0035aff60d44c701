"""What the instance-pause tests share (test_instance_pause.py, test_gpu_instance_pause.py, test_gpu_tworate_pause.py): the schedules, the
cut logs, the lane-sequential harness with pauses (tests/hostsim/pause_hostsim.cpp) and the GPU runners.

A schedule is {tick: dict(reset=[instances], active=[B ints])}: before the pushes of that tick the instances of `reset` are restarted
(dekf_reset_instances) and then the whole mask `active` is stated (dekf_set_active); either key may be missing.  A life of instance b is
the list of ticks at which it ran between two restarts (or the start and the end of the log).  Its reference is a run WITHOUT this
interface on the log cut down to those ticks: tick life[j] of the handle against tick j of the reference, instance b of both.  While
the instance is paused every output keeps the bits of the last tick it ran.
TEST INFRASTRUCTURE ONLY.  Importing this module does not touch the GPU."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import direct_lib as DL
import epoch_lib as EL
import hostsim_lib as HL
import tworate_lib as TL
from decentralized_ekf_mhe_amd import capi

LIB = os.path.join(DL.HOSTSIM, "libpause_hostsim.so")
K_LOG = 100


def _mask(B, paused):
    return [0 if b in paused else 1 for b in range(B)]


def cpu_schedule(B):
    """Instance 1 (the slow camera): paused over ticks 5 .. 8 (inside the window fill), over 14 .. 26 (the handle passes from the fill
    into full windows meanwhile, the instance resumes inside its own fill and goes on into full windows), paused before tick 60 and
    restarted while paused before tick 66, restarted before tick 80 and paused in the same gap (local tick -1) until tick 84.
    Instance 0 (the 30 Hz camera): paused over ticks 50 .. 57, from and into full windows that hold VO equality rows, and before
    tick 90 for good.  Every other instance is never named"""
    return {5: dict(active=_mask(B, {1})), 9: dict(active=_mask(B, ())),
            14: dict(active=_mask(B, {1})), 27: dict(active=_mask(B, ())),
            50: dict(active=_mask(B, {0})), 58: dict(active=_mask(B, ())),
            60: dict(active=_mask(B, {1})), 66: dict(reset=[1]),
            80: dict(reset=[1], active=_mask(B, {1})), 84: dict(active=_mask(B, ())),
            90: dict(active=_mask(B, {0}))}


def gpu_schedule(B, K):
    """cpu_schedule for a log of K ticks (60 ticks: the later events pulled in), with two instances paused at once in between"""
    if K >= 100:
        sch = cpu_schedule(B)
        sch[30] = dict(active=_mask(B, {3, 4}))
        sch[37] = dict(active=_mask(B, {4}))
        sch[41] = dict(active=_mask(B, ()))
        return sch
    return {5: dict(active=_mask(B, {1})), 9: dict(active=_mask(B, ())),
            11: dict(active=_mask(B, {1})), 20: dict(active=_mask(B, ())),
            30: dict(active=_mask(B, {0, 1})), 36: dict(reset=[1]), 38: dict(active=_mask(B, ())),
            44: dict(reset=[1], active=_mask(B, {1})), 47: dict(active=_mask(B, ())),
            52: dict(active=_mask(B, {0}))}


# name: (params, B).  The shapes of epoch_lib
CPU_SHAPES = EL.CPU_SHAPES
GPU_SHAPES = EL.GPU_SHAPES


def walk(schedule, B, K):
    """(lives, frozen): lives = [(b, [ticks of the life])] in the order they begin, the first one of every instance from tick 0;
    frozen = [(b, tick, last tick it ran or None)] for every tick at which b is paused"""
    active, cur = [1] * B, [[] for _ in range(B)]
    lives, frozen = [(b, cur[b]) for b in range(B)], []
    for k in range(K):
        ev = schedule.get(k, {})
        for b in ev.get("reset", ()):
            cur[b] = []
            lives.append((b, cur[b]))
            active[b] = 1
        active = list(ev.get("active", active))
        for b in range(B):
            if active[b]:
                cur[b].append(k)
            else:
                frozen.append((b, k, cur[b][-1] if cur[b] else None))
    return [(b, tuple(t)) for b, t in lives], frozen


def cut_streams(s, ticks):
    """the log cut down to `ticks`: what the reference of a life is fed"""
    K, B = s["imu_t"].shape
    idx = np.asarray(ticks, int)
    so = {k: (np.ascontiguousarray(v[idx]) if isinstance(v, np.ndarray) and v.shape[:2] == (K, B) else v) for k, v in s.items()}
    so["vo_any"] = so["vo_mask"].any(axis=1)
    return so


# ------------------------------------------------------------------ the lane-sequential harness with pauses
_libs = {}


def pause_hostsim():
    """tests/hostsim/pause_hostsim.cpp as libpause_hostsim.so, rebuilt when a source is newer, and bound"""
    if "lib" not in _libs:
        srcs = [os.path.join(DL.HOSTSIM, f) for f in os.listdir(DL.HOSTSIM) if f.endswith(".cpp")] + \
            [os.path.join(DL.CSRC, f) for f in os.listdir(DL.CSRC) if f.endswith(".h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in srcs):
            subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-DDEKF_HOSTSIM", "-w", "-O2", "-o", LIB,
                                   os.path.join(DL.HOSTSIM, "pause_hostsim.cpp")])
        L = HL._bind(C.CDLL(LIB))
        vp, dp, ip = C.c_void_p, HL._dp, HL._ip
        L.hs_epochs_create.restype = vp
        L.hs_epochs_create.argtypes = [C.c_int]
        L.hs_epochs_destroy.argtypes = [vp]
        L.hs_epochs_copy.argtypes = [vp, ip, ip]
        L.hs_pauses_create.restype = vp
        L.hs_pauses_create.argtypes = [C.c_int]
        L.hs_pauses_destroy.argtypes = [vp]
        L.hs_set_active.restype = C.c_int
        L.hs_set_active.argtypes = [vp, vp, vp, ip]
        L.hs_get_active.argtypes = [vp, ip]
        L.hs_reset_instances_pause.argtypes = [vp, vp, vp, ip, dp]
        L.hs_push_vo_pause.argtypes = [vp, vp, ip, dp, dp, dp, dp, dp]
        L.hs_ekf_step_pause.argtypes = [vp, vp]
        L.hs_instance_ticks_pause.argtypes = [vp, vp, C.c_int, ip]
        L.hs_update_direct_pause.argtypes = [vp, vp, C.c_int, dp]
        L.hs_update_direct_smooth_pause.argtypes = [vp, vp, C.c_int, dp, dp, dp]
        L.hs_update_direct_cross_pause.argtypes = [vp, vp, C.c_int, dp, dp, dp, dp, dp]
        L.hs_pause_fold_resume.argtypes = [C.c_int] * 5 + [ip]
        L.hs_epoch_paused_sentinel.restype = C.c_int
        _libs["lib"] = L
    return _libs["lib"]


class PauseSim(HL.HostSim):
    """hostsim_lib.HostSim on the pause harness: what a direct handle runs once dekf_set_active has paused an instance, from tick 0 on
    (every instance active until set_active()).  cov and win as epoch_lib.EpochSim's"""

    def __init__(self, params, batch, variant="plain"):
        assert variant in DL.VARIANTS
        self.p, self.B, self.L, self.variant = params, batch, pause_hostsim(), variant
        self.h = self.L.hs_create(C.byref(params), batch)
        assert self.h, "hs_create rejected the parameters"
        self.e = self.L.hs_epochs_create(batch)
        self.z = self.L.hs_pauses_create(batch)
        ns = params.dim_state
        self.cov = np.full((batch, ns, ns), np.nan)
        self.win = {}

    def __del__(self):
        if getattr(self, "z", None):
            self.L.hs_pauses_destroy(self.z)
            self.z = None
        if getattr(self, "e", None):
            self.L.hs_epochs_destroy(self.e)
            self.e = None
        super().__del__()

    def set_active(self, mask):
        return self.L.hs_set_active(self.h, self.e, self.z, HL._p(np.ascontiguousarray(mask, np.int32)))

    def active(self):
        a = np.zeros(self.B, np.int32)
        self.L.hs_get_active(self.z, HL._p(a))
        return a

    def reset(self, instances):
        mask = np.zeros(self.B, np.int32)
        mask[list(instances)] = 1
        self.L.hs_reset_instances_pause(self.h, self.e, self.z, HL._p(mask), HL._p(self.cov))

    def ticks(self, T):
        t = np.zeros(self.B, np.int32)
        self.L.hs_instance_ticks_pause(self.e, self.z, T, HL._p(t))
        return t

    def epochs(self):
        t0, c0 = np.zeros(self.B, np.int32), np.zeros(self.B, np.int32)
        self.L.hs_epochs_copy(self.e, HL._p(t0), HL._p(c0))
        return t0, c0

    def push_vo(self, mask, t_pre, t_now, dp, t_pose, q):
        self.L.hs_push_vo_pause(self.h, self.e, HL._p(mask), HL._p(t_pre), HL._p(t_now), HL._p(dp), HL._p(t_pose), HL._p(q))

    def feed(self, s, k):
        L = self.L
        L.hs_push_imu(self.h, HL._p(s["imu_t"][k]), HL._p(s["accel"][k]), HL._p(s["gyro"][k]))
        L.hs_push_leg(self.h, HL._p(s["p_foot"][k]), HL._p(s["J"][k]), HL._p(s["qdot"][k]), HL._p(s["contact"][k]))
        if s["vo_mask"][k].any():
            self.push_vo(s["vo_mask"][k], s["vo_t_pre"][k], s["vo_t_now"][k], s["vo_dp"][k], s["vo_t_pose"][k], s["vo_q"][k])

    def ekf_step(self):
        self.L.hs_ekf_step_pause(self.h, self.e)

    def step(self, T):
        self.ekf_step()
        self.update(T)

    def update(self, T):
        ns, N, B = self.p.dim_state, self.p.N, self.B
        if self.variant == "plain":
            self.L.hs_update_direct_pause(self.h, self.e, T, HL._p(self.cov))
            return
        # (the handle's window stores persist: a paused instance's entries are the ones of its last solve)
        if not self.win:
            self.win = dict(xw=np.full((B, N, ns), DL.FILL), cw=np.full((B, N, ns, ns), DL.FILL))
            if self.variant == "cross":
                self.win.update(l1=np.full((B, N - 1, ns, ns), DL.FILL), zn=np.full((B, N, ns, ns), DL.FILL))
        if self.variant == "smooth":
            self.L.hs_update_direct_smooth_pause(self.h, self.e, T, HL._p(self.cov), HL._p(self.win["xw"]), HL._p(self.win["cw"]))
        else:
            self.L.hs_update_direct_cross_pause(self.h, self.e, T, HL._p(self.cov), *(HL._p(self.win[k]) for k in EL.WINDOW_KEYS))


def stray_vo(sim_or_est, s, k, paused):
    """a VO sample (interval and pose) made up for the paused instances alone, pushed behind the log's own of tick k"""
    B = s["imu_t"].shape[1]
    mask = np.zeros(B, np.int32)
    mask[list(paused)] = 1
    t = np.ascontiguousarray(s["imu_t"][k])
    q = np.tile(np.array([0.6, 0.0, 0.8, 0.0]), (B, 1))
    sim_or_est.push_vo(mask, t - 0.03, t - 0.004, np.full((B, 3), 0.25), t - 0.004, q)


def run_pause_sim(p, s, B, K, variant, schedule, stray=False):
    """[tick] -> what the pause harness left at every tick of the log under `schedule`.  stray: a made-up VO sample is pushed for the
    paused instances at every tick"""
    sim = PauseSim(p, B, variant)
    out = []
    for k in range(K):
        ev = schedule.get(k, {})
        if "reset" in ev:
            sim.reset(ev["reset"])
        if "active" in ev:
            sim.set_active(ev["active"])
        sim.feed(s, k)
        paused = np.flatnonzero(sim.active() == 0)
        if stray and len(paused):
            stray_vo(sim, s, k, paused)
        sim.step(k)
        t0, c0 = sim.epochs()
        out.append(dict(EL._record(sim, sim.cov), ticks=sim.ticks(k), active=sim.active(), t0=t0, c0=c0))
    return out


SIM_KEYS = EL.SIM_KEYS + ("pri_res", "dua_res")


def assert_cut_life_equal(got, fresh, b, life, N, keys, what, ticks=True):
    """instance b of `got` at the ticks of `life` against instance b of `fresh` (the run on the cut log) at ticks 0, 1, ...: array_equal
    on `keys`, the local tick, and the first K_b window and cross entries.  The reference holds DEKF_SOLVE_OK at every tick from 1 on"""
    for j, k in enumerate(life):
        g, f = got[k], fresh[j]
        if j:
            assert f["status"][b] == capi.DEKF_SOLVE_OK, (what, b, k, j, "the reference's status", f["status"][b])
        for key in keys:
            if key == "cov" and "cov" not in f:   # a fresh GPU handle's tick 0: no covariance yet; the handle's block is NaN or absent
                assert j == 0 and ("cov" not in g or np.isnan(g["cov"][b]).all()), (what, b, k)
                continue
            assert np.array_equal(g[key][b], f[key][b], equal_nan=True), (what, b, k, j, key)
        if ticks:
            assert g["ticks"][b] == j, (what, b, k, j, g["ticks"])
        Kb = EL.local_K(j, N)
        for key in EL.WINDOW_KEYS:
            if key in f and Kb:
                n = EL.window_lengths(key, Kb)
                assert np.array_equal(g[key][b, :n], f[key][b, :n]), (what, b, k, j, key)


def assert_frozen(got, b, k, last, N, keys, what):
    """instance b at tick k, paused since it ran tick `last`: every output, the local tick and its window entries keep their bits"""
    g, f = got[k], got[last]
    assert g["active"][b] == 0 and g["ticks"][b] == f["ticks"][b], (what, b, k, g["ticks"], f["ticks"])
    for key in keys:
        if key in f and key in g:   # (a GPU record of tick 0 has no covariance)
            assert np.array_equal(g[key][b], f[key][b], equal_nan=True), (what, b, k, last, key)
    Kb = EL.local_K(int(f["ticks"][b]), N)
    for key in EL.WINDOW_KEYS:
        if key in f and Kb:
            n = EL.window_lengths(key, Kb)
            assert np.array_equal(g[key][b, :n], f[key][b, :n]), (what, b, k, last, key)


def check_against_cut_logs(got, fresh_of, schedule, B, K, N, keys, what):
    """every life of `schedule` against fresh_of(ticks of the life), every paused tick against the last tick that ran.  Returns the
    lives"""
    lives, frozen = walk(schedule, B, K)
    for b, life in lives:
        if life:
            assert_cut_life_equal(got, fresh_of(life), b, life, N, keys, what)
    for b, k, last in frozen:
        if last is not None:
            assert_frozen(got, b, k, last, N, keys, what)
        else:   # restarted and paused in one gap: local tick -1, nothing has run
            assert got[k]["ticks"][b] == -1 and got[k]["status"][b] == capi.DEKF_SOLVE_NONE, (what, b, k)
    return lives


@functools.lru_cache(maxsize=None)
def cpu_streams(name):
    mk, B = CPU_SHAPES[name]
    p = mk()
    return p, DL.rough_streams(p, B, K_LOG)


@functools.lru_cache(maxsize=None)
def cpu_fresh(name, variant, life):
    """the reference of a life: the harness WITHOUT epochs or pauses (direct_lib.DirectSim) on the log cut down to its ticks"""
    p, s = cpu_streams(name)
    return EL.run_fresh_sim(p, cut_streams(s, life), CPU_SHAPES[name][1], len(life), variant)


def vo_equality_rows(p, s, b, life, at):
    """VO equality rows in the window of the reference of `life` (the oracle on the cut log) at its tick `at`"""
    (_, _, _, _, nv), = DL.kkt_reference(p, cut_streams(s, life), b, {at}, solve=False, invert=False)
    return nv


# ------------------------------------------------------------------ the two rates: tworate_lib's grid as a list of ms
def drive_ms(dev, s, ms, pokes=None):
    """tworate_lib.drive's events at the grid ms of `ms` (a run without pauses: every ms of the grid; the reference of a paused
    instance: the grid without the ms it was paused at), step T counted by the timer events: [record after every timer event]"""
    pokes = pokes or {}
    out = []
    for i in ms:
        if i in pokes:
            pokes[i](dev)
        if s["vo_mask"][i].any():
            dev.vo(s, i)
        if i % 2 == 0:
            dev.sensors(s, i)
            dev.ekf_step()
        if i % 5 == 0:
            T = len(out)
            dev.timer(T)
            out.append(dev.record(T))
    return out


class PauseDev(TL.SimDev):
    """tworate_lib.SimDev on a PauseSim: the VO latch that knows the pauses, dekf_set_active, the mask in every record"""

    def vo(self, s, i):
        self.sim.push_vo(s["vo_mask"][i], s["vo_t_pre"][i], s["vo_t_now"][i], s["vo_dp"][i], s["vo_t_pose"][i], s["vo_q"][i])

    def set_active(self, mask):
        self.sim.set_active(mask)

    def record(self, T):
        return dict(super().record(T), active=self.sim.active())


def two_rate_pauses(s):
    """[(instance, first paused ms, ms of the resume or None)].  Instance 0 is paused before ms 63, behind the EKF tick of ms 62 in the
    gap between the updates of ms 60 and 65, and resumed before the events of the first ms at which one of its VO poses arrives that
    was stamped during the pause; instance 1 directly behind the update of ms 130, until ms 176; instance 2 before ms 226 for good"""
    g0 = 63
    arrivals = [i for i in range(g0 + 12, s["imu_t"].shape[0])
                if s["vo_mask"][i, 0] and s["imu_t"][g0 + 1, 0] <= s["vo_t_pose"][i, 0] < s["imu_t"][i - 1, 0]]
    assert arrivals, "no VO pose of instance 0 stamped inside a pause from ms 63 on"
    return [(0, g0, arrivals[0]), (1, 131, 176), (2, 226, None)]


def two_rate_run(name, H, B, make_dev, fresh_dev):
    """(parameters, streams, records of the paused run, {instance: (its ms, records of its reference)}, pauses): the grid under
    two_rate_pauses on make_dev(), and per paused instance the grid without its paused ms on fresh_dev()"""
    p, s, n_grid = TL.streams(name, H, B)
    pauses = two_rate_pauses(s)
    state, pokes = [1] * B, {}

    def poke_of(mask):
        return lambda dev: dev.set_active(mask)

    for g, b, v in sorted([(a, b, 0) for b, a, _ in pauses] + [(r, b, 1) for b, _, r in pauses if r is not None]):
        state[b] = v
        pokes[g] = poke_of(list(state))
    got = drive_ms(make_dev(), s, range(n_grid), pokes)
    refs = {}
    for b, a, r in pauses:
        ms = [i for i in range(n_grid) if not a <= i < (n_grid if r is None else r)]
        refs[b] = (ms, drive_ms(fresh_dev(), s, ms))
    return p, s, got, refs, pauses


def check_two_rate(p, got, refs, plain, pauses, B, keys):
    """every paused instance against its reference at the handle's steps at which it ran and against its own last step where it did
    not; every other instance against `plain`, the run of the whole grid without this interface"""
    for b, a, r in pauses:
        ms, fresh = refs[b]
        steps = [i // 5 for i in ms if i % 5 == 0]
        assert_cut_life_equal(got, fresh, b, steps, p.N, keys, ("two rates", b))
        # (EKF ticks may lie between the last update it ran and the pause: the filter's outputs stand as the last of them left them,
        # so they are held against the first paused step, everything else against the last step the instance ran too)
        last, first_paused = None, None
        for T in range(len(got)):
            if T in steps:
                last, first_paused = T, None
                continue
            first_paused = T if first_paused is None else first_paused
            assert_frozen(got, b, T, last, p.N, [k for k in keys if k not in ("quat", "ekf_cov")], ("two rates", b))
            assert_frozen(got, b, T, first_paused, p.N, keys, ("two rates", b))
    assert len(plain) == len(got)
    for b in range(len(pauses), B):
        assert_cut_life_equal(got, plain, b, list(range(len(got))), p.N, keys, ("two rates, untouched", b))


# ------------------------------------------------------------------ the GPU runners
GPU_KEYS = EL.GPU_KEYS


def gpu_record(est, k, variant):
    p = est.params
    r = EL.gpu_record(est)
    r["ticks"], r["active"] = est.instance_ticks(), est.active()
    if k:
        r["cov"] = est.mhe_cov()
        r["Kmax"] = max(EL.local_K(int(t), p.N) for t in r["ticks"])
        if variant != "plain" and r["Kmax"]:
            r["K"], r["xw"], r["cw"] = est.window()
        if variant == "cross" and r["Kmax"]:
            Kc, r["l1"], r["zn"] = est.window_cross()
            assert Kc == r["K"]
    return r


def run_gpu(p, s, B, K, variant, schedule=None, device_mask=False, stray=False, est=None, close=True, sets=None, set_of=None):
    """([tick] -> every getter the contract of dekf_set_active names, kernel names at the start and after every call, handle) of a
    direct handle over the log under `schedule`.  sets, set_of: a parameter table set before tick 0"""
    from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host
    schedule = schedule or {}
    est = est or BatchedEstimator(p, B, solver="direct", **DL.VARIANTS[variant])
    if sets is not None:
        est.set_instance_params(sets, set_of)
    sh = streams_host(s)
    out = []
    names = [(est.solve_kernel_name(True), est.solve_kernel_name(False))]

    def arg(m):
        m = np.ascontiguousarray(m, np.int32)
        if device_mask:
            import torch
            m = torch.from_numpy(m).cuda()
            torch.cuda.synchronize()
        return m

    for k in range(K):
        ev = schedule.get(k, {})
        if "reset" in ev:
            mask = np.zeros(B, np.int32)
            mask[list(ev["reset"])] = 1
            est.reset_instances(arg(mask))
        if "active" in ev:
            est.set_active(arg(ev["active"]))
        if ev:
            names.append((est.solve_kernel_name(True), est.solve_kernel_name(False)))
        est.push_stream_step(sh, k)
        paused = np.flatnonzero(est.active() == 0) if k else []
        if stray and len(paused):
            stray_vo(est, s, k, paused)
        est.step(k)
        out.append(gpu_record(est, k, variant))
    if close:
        est.close()
    return out, names, est


@functools.lru_cache(maxsize=None)
def gpu_fresh(name, variant, life):
    """the reference of a life: a fresh handle that never hears of this interface, on the log cut down to its ticks"""
    p, s = EL.gpu_streams(name)
    B = GPU_SHAPES[name][1]
    return EL.run_gpu(p, cut_streams(s, life), B, len(life), variant)[0]
