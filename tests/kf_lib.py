"""What the Kalman-filter-mode tests share (est_type 1: test_kf_mode.py, test_gpu_kf_mode.py): the four leg
counts with and without foot-position states, one log that wraps the record ring about twenty times and sends instances through a
flight and an all-stance phase, the two references of every tick (the oracle, one O.Pipe per instance, and ref_numpy's textbook filter
fed the oracle's quaternions), the error measures and the lane-sequential and GPU runners.
TEST INFRASTRUCTURE ONLY.  Importing this module does not touch the GPU: torch and the estimator are imported where they are used."""
import functools

import numpy as np

import hostsim_lib as HS
import oracle_lib as O
import ref_numpy as RN
from decentralized_ekf_mhe_amd import cassie_params, go1_params, pogox_params
from decentralized_ekf_mhe_amd.streams import make_streams
from direct_lib import block_err, blocks3, cov_err  # noqa: F401  (cov_err: max |C - C*|_ij / sqrt(C*_ii C*_jj))

N, B, K = 5, 3, 130           # record ring of N + 1 = 6: it wraps about 20 times
RTOL, ATOL = 1e-4, 1e-6       # the project's tolerance per 3-vector block of x (foot-state rule)
SPREAD_CAP_FULL, SPREAD_CAP_BASE = 0.1, 1e-3   # what the two references may differ by with foot states (measured 1.3e-2, 1.3e-5)


def _tripod():
    p = go1_params()
    p.num_legs, p.joints_per_leg = 3, 6
    return p


# name -> maker: 1 leg, 2 legs x 5 joints, 3 legs x 6 joints, 4 legs
SHAPES = {"pogox": pogox_params, "cassie": cassie_params, "tripod": _tripod, "go1": go1_params}
LEGS = {"pogox": 1, "cassie": 2, "tripod": 3, "go1": 4}


def params(shape, foot):
    p = SHAPES[shape]()
    p.ekf_rate = p.rate
    p.est_type, p.N, p.leg_odom_type = 1, N, int(foot)
    assert p.num_legs == LEGS[shape] and p.dim_state == 9 + (3 * p.num_legs if foot else 0)
    return p


def streams(p, batch=B, nsteps=K, first_instance=0):
    """make_streams with instance 0 in flight for 30 ticks, instance 1 with every foot down for 25 and a 3-tick flight of instance 2"""
    s = make_streams(p, batch, nsteps, first_instance=first_instance)
    if nsteps > 25:
        s["contact"][25:55, 0] = 0.0
    if batch > 1 and nsteps > 60:
        s["contact"][60:85, 1] = 1.0
    if batch > 2 and nsteps > 90:
        s["contact"][90:93, 2] = 0.0
    return s


def oracle_run(p, s):
    """every tick of every instance through the oracle: x [K, B, ns], v_b [K, B, 3], quat [K, B, 4], cov [K, B, ns, ns]"""
    Kk, Bb = s["imu_t"].shape
    ns = p.dim_state
    out = dict(x=np.zeros((Kk, Bb, ns)), v_b=np.zeros((Kk, Bb, 3)), quat=np.zeros((Kk, Bb, 4)), cov=np.zeros((Kk, Bb, ns, ns)))
    for b in range(Bb):
        pipe = O.Pipe(p)
        for k in range(Kk):
            pipe.feed(s, k, b)
            pipe.step(k)
            x, vb, _ = pipe.est.get()
            out["x"][k, b], out["v_b"][k, b], out["quat"][k, b], out["cov"][k, b] = x, vb, pipe.quat(), pipe.est.kf_cov()
    return out


def numpy_run(p, s, quats):
    """ref_numpy's filter with the reference's double first step: x [K, B, ns], cov [K, B, ns, ns]"""
    Kk, Bb = s["imu_t"].shape
    ns = p.dim_state
    x, cov = np.zeros((Kk, Bb, ns)), np.zeros((Kk, Bb, ns, ns))
    for b in range(Bb):
        x[:, b], cov[:, b] = RN.kalman_filter(p, s, b, quats[:, b], ref_double_init=True)
    return x, cov


@functools.lru_cache(maxsize=None)
def case(shape, foot):
    """(p, s, oracle dict, numpy dict) of one shape: computed once per process, shared by every test, never written to"""
    p = params(shape, foot)
    s = streams(p)
    orc = oracle_run(p, s)
    xn, cn = numpy_run(p, s, orc["quat"])
    ref = dict(x=xn, cov=cn)
    for d in (orc, ref):
        for a in d.values():
            a.setflags(write=False)
    return p, s, orc, ref


def hostsim_run(p, s):
    """the lane-sequential build of the device cores: x, v_b, quat, cov of every tick"""
    Kk, Bb = s["imu_t"].shape
    hs = HS.HostSim(p, Bb)
    out = dict(x=[], v_b=[], quat=[], cov=[])
    for k in range(Kk):
        hs.feed(s, k)
        hs.step(k)
        o = hs.get()
        out["x"].append(o["x"]); out["v_b"].append(o["v_b"]); out["quat"].append(o["quat"]); out["cov"].append(hs.kf_cov())
    return {k: np.array(v) for k, v in out.items()}


def gpu_run(p, s, est=None):
    """the HIP path through the C ABI: x, v_b, quat, cov of every tick (a handle passed in stays open)"""
    from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host
    Kk, Bb = s["imu_t"].shape
    own = est is None
    if own:
        est = BatchedEstimator(p, Bb)
    sh = streams_host(s)
    out = dict(x=[], v_b=[], quat=[], cov=[])
    for k in range(Kk):
        est.push_stream_step(sh, k)
        est.step(k)
        o = est.get()
        out["x"].append(o["x"]); out["v_b"].append(o["v_b"]); out["quat"].append(o["quat"]); out["cov"].append(est.kf_cov())
    if own:
        est.close()
    return {k: np.array(v) for k, v in out.items()}


# ------------------------------------------------------------------ error measures
def x_err(x, ref):
    """worst |x - ref| / max(1, |ref|), entry by entry"""
    return float((np.abs(x - ref) / np.maximum(1.0, np.abs(ref))).max())


def asymmetry(cov):
    return cov_err(cov, np.swapaxes(cov, -1, -2))


def min_eig_ratio(cov):
    """smallest eigenvalue of the symmetrised covariance over its smallest diagonal entry, worst over ticks and instances"""
    sym = 0.5 * (cov + np.swapaxes(cov, -1, -2))
    ev = np.linalg.eigvalsh(sym)[..., 0]
    return float((ev / np.diagonal(sym, axis1=-2, axis2=-1).min(axis=-1)).min())


def foot_block_err(x, ref):
    """the foot-state rule's measure: worst |x - ref|_inf / (1e-4 |ref|_inf + 1e-6) over the 3-vector blocks of the state"""
    return block_err(x, ref, blocks3(x.shape[-1]), RTOL, ATOL)


def base(cov):
    return cov[..., :9, :9]


def check_nine_states(shape, got, tol_x, tol_vb, tol_cov, who):
    """9 states, every tick (tick 0 included: the reference's InitializeKF + UpdateKF double step, v_b untouched by it): the two
    references agree to rounding — asserted first, so that a failure says so when THEY diverge — and `got` follows the oracle.
    Returns the measured figures"""
    p, s, orc, ref = case(shape, 0)
    m = dict(ref_spread=cov_err(orc["cov"], ref["cov"]), ref_x=x_err(orc["x"], ref["x"]),
             x=x_err(got["x"], orc["x"]), v_b=float(np.abs(got["v_b"] - orc["v_b"]).max()),
             cov=cov_err(got["cov"], orc["cov"]), asym=asymmetry(got["cov"]), eig=min_eig_ratio(got["cov"]),
             quat=float(np.abs(got["quat"] - orc["quat"]).max()))
    print(f"[kf {who}] {shape} L={p.num_legs} ns=9: " + " ".join(f"{k}={v:.2e}" for k, v in m.items()))
    assert m["ref_spread"] <= 1e-13 and m["ref_x"] <= 1e-12, ("the references diverge", m)
    assert not orc["v_b"][0].any() and np.abs(orc["v_b"][1:]).max() > 1e-3   # initialize() leaves v_b alone, update() writes it
    assert not got["v_b"][0].any(), got["v_b"][0]
    assert m["x"] <= tol_x, m
    assert m["v_b"] <= tol_vb, m
    assert m["cov"] <= tol_cov, m
    assert m["asym"] <= tol_cov, m
    assert m["eig"] > 0.0, m
    return m


def check_foot_states(shape, got, who):
    """foot-position states: x by the rule of test_foot_states.py (10 x the tolerance, the first five ticks inside it), the covariance
    within 10 x what the two references differ by on the same ticks — full matrix and base 9 x 9 block —, that spread itself capped.
    The spread is between oracle and numpy, never against `got`.  Returns the measured figures"""
    p, s, orc, ref = case(shape, 1)
    m = dict(spread_full=cov_err(orc["cov"], ref["cov"]), spread_base=cov_err(base(orc["cov"]), base(ref["cov"])),
             ref_x=foot_block_err(ref["x"][1:], orc["x"][1:]),
             x=foot_block_err(got["x"][1:], orc["x"][1:]), x_first=foot_block_err(got["x"][:6], orc["x"][:6]),
             cov_full=cov_err(got["cov"], orc["cov"]), cov_base=cov_err(base(got["cov"]), base(orc["cov"])),
             asym=asymmetry(got["cov"]))
    m["ratio_full"], m["ratio_base"] = m["cov_full"] / m["spread_full"], m["cov_base"] / m["spread_base"]
    print(f"[kf {who}] {shape} L={p.num_legs} ns={p.dim_state}: " + " ".join(f"{k}={v:.2e}" for k, v in m.items()))
    assert 0.0 < m["spread_full"] < SPREAD_CAP_FULL and 0.0 < m["spread_base"] < SPREAD_CAP_BASE, ("the references diverge", m)
    assert m["x"] <= 10.0 and m["x_first"] <= 1.0, m
    assert m["cov_full"] <= 10.0 * m["spread_full"], m
    assert m["cov_base"] <= 10.0 * m["spread_base"], m
    return m
