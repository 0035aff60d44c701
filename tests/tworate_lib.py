"""What the two-rate tests share (test_gpu_configs.py's multirate cases, test_instance_reset.py, test_instance_params.py,
test_gpu_tworate_reset.py, test_gpu_tworate_params.py): the reference's two timers on one 1 ms event grid, the restart schedule on that
grid, the drivers of the lane-sequential harnesses and of a GPU handle, and the oracle driven by the same events.

The grid (orien_ekf.cpp:43, EstSub.cpp:25, parameters_go1.yaml:33,75).  At grid ms i, in this order: the instances of resets[i] are
restarted; a VO sample that arrives is latched; on every even ms IMU and leg samples are pushed and the EKF ticks once (500 Hz); on
every 5th ms the MHE timer fires (200 Hz): initialise at the run's first timer event, update(T) after it.  So 2 or 3 EKF ticks lie
between two updates, and a restart's two epochs differ: t0[b] counts timer events, c0[b] EKF ticks.

A life is (instance, g0, g_end): the instance restarted before the events of ms g0 and running until its next restart or the end of
the grid.  Its reference is a fresh handle (or simulation) driven by the same loop started at ms g0: the EKF ticks before the life's
first timer event belong to it, and its MHE step j is the handle's step ceil(g0 / 5) + j.
TEST INFRASTRUCTURE ONLY.  Importing this module does not touch the GPU."""
import functools

import numpy as np

import direct_lib as DL
import epoch_lib as EL
import hostsim_lib as HL
import instance_params_lib as PL
import oracle_lib as O
from decentralized_ekf_mhe_amd import go1_params
from decentralized_ekf_mhe_amd.streams import make_streams

N_MHE = 70                     # MHE steps of a run from ms 0: 346 ms, 173 EKF ticks, 69 updates
VO = dict(vo_rate=30.0, vo_latency=0.02)
# {grid ms: instances restarted before that ms's events}.  63: EKF ticks lie between the last update (ms 60) and the restart; 78: a VO
# pose STRADDLES the restart (it arrives at ms 87 with a pose time of 66.7 ms: older than the new life, which must drop it as a fresh
# handle does, while the ring still holds the earlier life's samples of that time: the one event at which a wrong EKF epoch changes
# bits, since ekf_tick takes from its count only how far back it may search); 131: directly behind an update; 132: the same instance
# again inside its own window fill, on an EKF-tick ms; 226: two instances at once, from full windows.  Every instance from 3 on is
# never restarted
RESETS = {63: [1], 78: [0], 131: [2], 132: [1], 226: [0, 2]}
# the parameter tests: set_of at the start, and the set every restarted instance takes at its restart (another one than it had)
SET_OF = [0, 1, 0, 0, 0, 0]
NEW_SETS = {63: {1: 2}, 78: {0: 2}, 131: {2: 1}, 132: {1: 0}, 226: {0: 1, 2: 2}}


def two_rate(p, **kw):
    """p at the reference's rates (EKF 500 Hz, MHE 200 Hz) with the members of kw set"""
    q = p.copy()
    q.ekf_rate, q.rate = 500, 200
    for k, v in kw.items():
        setattr(q, k, v)
    return q


# name: parameters at ekf_history H.  The shapes of epoch_lib.CPU_SHAPES / GPU_SHAPES at the two rates
SHAPES = {"go1": lambda H: two_rate(go1_params(), ekf_history=H),
          "tripod": lambda H: two_rate(DL.tripod_params(), ekf_history=H),
          "go1_foot": lambda H: two_rate(go1_params(), ekf_history=H, leg_odom_type=1)}


def schedule(p, B, n_mhe, seed_first=0, **stream_kw):
    """Sensor events on a 1 ms grid: IMU + joint states every 2 ms (500 Hz, each followed by one EKF timer tick,
    orien_ekf.cpp:43), the MHE timer every 5 ms (EstSub.cpp:25, parameters_go1.yaml:33), VO as it arrives."""
    grid = p.copy()
    grid.rate = 1000
    n_grid = 5 * (n_mhe - 1) + 1
    return make_streams(grid, B, n_grid, first_instance=seed_first, **stream_kw), n_grid


@functools.lru_cache(maxsize=None)
def streams(name, H, B):
    """(parameters, streams on the grid, grid length) of a shape"""
    p = SHAPES[name](H)
    s, n_grid = schedule(p, B, N_MHE, **VO)
    return p, s, n_grid


def first_step(g0):
    """the handle's MHE step at the first timer event of a run (or life) started at ms g0"""
    return -(-g0 // 5)


def ekf_ticks(g0, g_end):
    """EKF ticks (even ms) in [g0, g_end)"""
    return len(range(g0 + g0 % 2, g_end, 2))


def lives(resets, n_grid):
    """[(instance, g0, g_end)] of a schedule (epoch_lib.lives on the grid)"""
    return EL.lives(resets, n_grid)


def straddling_poses(s, b, g0, g_end):
    """VO poses of instance b that arrive inside the life (b, g0, g_end) with a pose time before the life's first IMU sample"""
    first = s["imu_t"][g0 + g0 % 2, b]
    return [i for i in range(g0, g_end) if s["vo_mask"][i, b] and s["vo_t_pose"][i, b] < first]


def steps_of(g0, g_end):
    """how many timer events fall into [g0, g_end)"""
    return len(range(5 * first_step(g0), g_end, 5))


def drive(dev, s, g0, n_grid, resets=None, pokes=None):
    """the event loop from ms g0 on a device adapter (vo, sensors, ekf_step, timer, restart, record): [record after every timer event],
    entry j the run's MHE step j.  pokes[i](dev) runs behind the restarts of ms i, before its events"""
    resets, pokes = resets or {}, pokes or {}
    base = first_step(g0)
    # a restart (or start) must see a sample before its first timer event, as a fresh handle would: else the handle's latches hold the
    # samples of the earlier life where the fresh handle's hold none
    for g in [g0] + sorted(resets):
        assert g + g % 2 <= 5 * first_step(g), g
    out = []
    for i in range(g0, n_grid):
        if i in resets:
            dev.restart(resets[i])
        if i in pokes:
            pokes[i](dev)
        if s["vo_mask"][i].any():
            dev.vo(s, i)
        if i % 2 == 0:
            dev.sensors(s, i)
            dev.ekf_step()
        if i % 5 == 0:
            T = i // 5 - base
            dev.timer(T)
            out.append(dev.record(T))
    return out


# ------------------------------------------------------------------ the lane-sequential harnesses
class SimDev:
    """adapter of a lane-sequential simulation (direct_lib.DirectSim, epoch_lib.EpochSim, instance_params_lib.ParamsSim)"""

    def __init__(self, sim):
        self.sim = sim
        self.nan = np.full((sim.B, sim.p.dim_state, sim.p.dim_state), np.nan)

    def vo(self, s, i):
        self.sim.L.hs_push_vo(self.sim.h, HL._p(s["vo_mask"][i]), HL._p(s["vo_t_pre"][i]), HL._p(s["vo_t_now"][i]), HL._p(s["vo_dp"][i]),
                              HL._p(s["vo_t_pose"][i]), HL._p(s["vo_q"][i]))

    def sensors(self, s, i):
        L, h = self.sim.L, self.sim.h
        L.hs_push_imu(h, HL._p(s["imu_t"][i]), HL._p(s["accel"][i]), HL._p(s["gyro"][i]))
        L.hs_push_leg(h, HL._p(s["p_foot"][i]), HL._p(s["J"][i]), HL._p(s["qdot"][i]), HL._p(s["contact"][i]))

    def ekf_step(self):
        self.sim.ekf_step()

    def timer(self, T):
        self.sim.update(T)

    def restart(self, instances):
        self.sim.reset(instances)

    def record(self, T):
        r = EL._record(self.sim, self.sim.cov if self.sim.cov is not None else self.nan)
        if hasattr(self.sim, "ticks"):
            r["ticks"] = self.sim.ticks(T)
            r["t0"], r["c0"] = self.sim.epochs()
        return r


@functools.lru_cache(maxsize=None)
def cpu_fresh(name, H, B, variant, g0=0, k=0):
    """the reference of every life that starts at ms g0 on set k: the harness WITHOUT epochs or table (direct_lib.DirectSim) created
    with that set and driven from ms g0, once per process"""
    p, s, n_grid = streams(name, H, B)
    return drive(SimDev(DL.DirectSim(PL.param_set(p, k), B, variant)), s, g0, n_grid)


def set_of_at(new, B):
    """set_of of a call that gives the instances of `new` ({instance: set index}) their sets and leaves every other one"""
    so = np.full(B, -1, np.int32)
    for b, k in new.items():
        so[b] = k
    return so


def run_epoch_sim(name, H, B, variant, resets):
    p, s, n_grid = streams(name, H, B)
    return drive(SimDev(EL.EpochSim(p, B, variant)), s, 0, n_grid, resets)


def run_params_sim(name, H, B, variant, set_of, resets, new_sets):
    """the parameter harness with the table (param_sets, set_of) set before ms 0; the restarted instances of ms i take new_sets[i]"""
    p, s, n_grid = streams(name, H, B)
    sets = PL.param_sets(p)
    sim = PL.ParamsSim(p, B, variant)
    assert sim.set_params(sets, set_of) == 0

    def take(i):
        def poke(dev):
            assert dev.sim.set_params(sets, set_of_at(new_sets[i], B)) == 0
        return poke

    return drive(SimDev(sim), s, 0, n_grid, resets, {i: take(i) for i in new_sets})


def assert_life_equal(got, fresh, b, g0, g_end, N, keys, what):
    """epoch_lib.assert_life_equal on the grid: the handle's step ceil(g0 / 5) + j against the fresh run's step j"""
    T0 = first_step(g0)
    EL.assert_life_equal(got, fresh, b, T0, T0 + steps_of(g0, g_end), N, keys, (what, g0))


# ------------------------------------------------------------------ the oracle on the grid
def oracle_replays(p, s, b, g0, g_end):
    """(EKF ticks of the life (b, g0, g_end) at which the oracle's filter replayed history, its deepest replay)"""
    ekf = O.Ekf(p)
    n, deepest = 0, 0
    for i in range(g0, g_end):
        if s["vo_mask"][i, b]:
            ekf.set_vo(s["vo_t_pose"][i, b], s["vo_q"][i, b])
        if i % 2 == 0:
            ekf.set_imu(s["imu_t"][i, b], s["accel"][i, b], s["gyro"][i, b])
            ekf.step()
            n += ekf.last_replay() > 0
            deepest = max(deepest, ekf.last_replay())
    return n, deepest


@functools.lru_cache(maxsize=None)
def oracle_life(name, H, B, b, g0, g_end):
    """The oracle's orientation filter and estimator (O.Ekf, O.Est) driven by the events of the life (b, g0, g_end), as
    test_gpu_configs._multirate_case drives them: [step j] -> (quaternion, x*, Cov*(x_T)); x* the exact optimum of the oracle's window QP
    at that step and Cov* the newest state's block of the inverse of its KKT matrix (direct_lib.kkt_of_qp); None, None at step 0"""
    p, s, _ = streams(name, H, B)
    ns = p.dim_state
    ekf, mhe = O.Ekf(p), O.Est(p)
    out = []
    for i in range(g0, g_end):
        if s["vo_mask"][i, b]:
            ekf.set_vo(s["vo_t_pose"][i, b], s["vo_q"][i, b])
            mhe.set_vo(s["vo_t_pre"][i, b], s["vo_t_now"][i, b], s["vo_dp"][i, b])
        if i % 2 == 0:
            ekf.set_imu(s["imu_t"][i, b], s["accel"][i, b], s["gyro"][i, b])
            mhe.set_imu(s["imu_t"][i, b], s["accel"][i, b], s["gyro"][i, b])
            mhe.set_leg(s["p_foot"][i, b], s["J"][i, b], s["qdot"][i, b], s["contact"][i, b])
            ekf.step()
            mhe.set_quat(ekf.get()[0])
        if i % 5 == 0:
            j = len(out)
            if j == 0:
                mhe.initialize()
                out.append((ekf.get()[0], None, None))
                continue
            mhe.update(j)
            x, Ki, xo, _ = DL.kkt_of_qp(p, mhe.qp(), j)
            o = xo[-1]
            out.append((ekf.get()[0], x[o:o + ns].copy(), Ki[o:o + ns, o:o + ns].copy()))
    return out


# ------------------------------------------------------------------ a GPU handle on the grid
class GpuDev:
    """adapter of a BatchedEstimator (direct); record() reads every getter the contracts of dekf_reset_instances and
    dekf_set_instance_params name, as epoch_lib.run_gpu does"""

    def __init__(self, est, variant, device_mask=False):
        self.est, self.variant, self.device_mask = est, variant, device_mask
        self.names = [(est.solve_kernel_name(True), est.solve_kernel_name(False))]

    def vo(self, s, i):
        self.est.push_vo(s["vo_mask"][i], s["vo_t_pre"][i], s["vo_t_now"][i], s["vo_dp"][i], s["vo_t_pose"][i], s["vo_q"][i])

    def sensors(self, s, i):
        self.est.push_imu(s["imu_t"][i], s["accel"][i], s["gyro"][i])
        self.est.push_leg(s["p_foot"][i], s["J"][i], s["qdot"][i], s["contact"][i])

    def ekf_step(self):
        self.est.ekf_step()

    def timer(self, T):
        if T == 0:
            self.est.initialize()
        else:
            self.est.update(T)

    def restart(self, instances):
        mask = np.zeros(self.est.batch, np.int32)
        mask[list(instances)] = 1
        if self.device_mask:
            import torch
            mask = torch.from_numpy(mask).cuda()
            torch.cuda.synchronize()
        self.est.reset_instances(mask)
        self.names.append((self.est.solve_kernel_name(True), self.est.solve_kernel_name(False)))

    def record(self, T):
        est, p = self.est, self.est.params
        r = EL.gpu_record(est)
        r["ticks"] = est.instance_ticks()
        if T:
            r["cov"] = est.mhe_cov()
            r["Kmax"] = max(EL.local_K(int(t), p.N) for t in r["ticks"])
            if self.variant != "plain" and r["Kmax"]:
                r["K"], r["xw"], r["cw"] = est.window()
            if self.variant == "cross" and r["Kmax"]:
                Kc, r["l1"], r["zn"] = est.window_cross()
                assert Kc == r["K"]
        return r


def run_gpu(name, H, B, variant, g0=0, k=0, resets=None, device_mask=False, set_of=None, new_sets=None, pokes=None):
    """([MHE step] -> every getter, kernel names at the start and after every restart) of a direct handle created with set k of the shape
    and driven from ms g0.  set_of: the table (param_sets, set_of) is set before the first event (None: no table); the restarted
    instances of ms i take new_sets[i] ({instance: set index}); pokes as drive's, with the estimator as dev.est"""
    from decentralized_ekf_mhe_amd.estimator import BatchedEstimator
    p, s, n_grid = streams(name, H, B)
    sets = PL.param_sets(p)
    est = BatchedEstimator(PL.param_set(p, k), B, solver="direct", **DL.VARIANTS[variant])
    if set_of is not None:
        est.set_instance_params(sets, set_of)
    dev = GpuDev(est, variant, device_mask)

    def take(i):
        def poke(dev):
            est.set_instance_params(sets, set_of_at(new_sets[i], B))
            dev.names[-1] = (est.solve_kernel_name(True), est.solve_kernel_name(False))
        return poke

    pokes = dict(pokes or {})
    pokes.update({i: take(i) for i in (new_sets or {})})
    out = drive(dev, s, g0, n_grid, resets, pokes)
    est.close()
    return out, dev.names


@functools.lru_cache(maxsize=None)
def gpu_fresh(name, H, B, variant, g0=0, k=0):
    """the reference of every life that starts at ms g0 on set k: a fresh uniform handle driven from ms g0, once per process"""
    return run_gpu(name, H, B, variant, g0, k)[0]


def assert_gpu_life_equal(got, fresh, b, g0, g_end, N, what):
    """epoch_lib.assert_gpu_life_equal on the grid: every getter, the local step, and the first K_b window and cross entries of the
    handle's step ceil(g0 / 5) + j against the fresh handle's step j"""
    T0 = first_step(g0)
    EL.assert_gpu_life_equal(got, fresh, b, T0, T0 + steps_of(g0, g_end), N, (what, g0))
