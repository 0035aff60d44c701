"""What the innovation-gate tests share (test_innovation_gate.py, test_gpu_innovation_gate.py): the cases with their injected foot
slips and gates, the reference (the oracle's pipe replayed with the reference's OWN decisions edited into the contact log), the
lane-sequential harness (tests/hostsim/gate_hostsim.cpp) and the GPU runner.
TEST INFRASTRUCTURE ONLY.  Importing this module does not touch the GPU."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import direct_lib as DL
import hostsim_lib as HL
import innov_lib as IL
import oracle_lib as O

GATE_KERNELS = [f"k_mhe_innov_gate_{L}{t}" for L in (1, 2, 3, 4) for t in ("", "_ep")]
NEVER = 1e300          # a gate that never fires
MARGIN = 1e-6          # no reference nis_leg of any case lies within this relative distance of its gate
# The injected foot slips.  A slip is given in units of the leg's own measurement noise: v = SLIP_SIGMAS[case] * chol(J C_enc_vel J') u
# with u = SLIP_DIR, so that it adds about the same to every leg's NIS whatever its Jacobian (J C_enc_vel J' is the bulk of the
# leg's block of S).  In m/s that is 3 to 8, not the tenths of m/s of a real slip: on these synthetic logs the NOMINAL innovation of a
# stance leg is itself 0.5 to 0.6 m/s at an innovation std of 0.05 to 0.08 m/s (the default stds are tighter than the streams' noise:
# nominal nis_leg up to 615), so a slip whose NIS stands a factor 9 above the nominal maximum, as the high gate needs (a factor 3 to
# either side), has to be some m/s.  Measured with the reference, a slip of (0.55, -0.4, 0.25) m/s: nis_leg 47 .. 309, inside the
# nominal spread; four times that: 1 060 .. 4 290.  The slips are no larger than the high gates need: the absolute limit on loglik
# (innov_lib.LOGLIK_ABS) was measured at nominal NIS values, and loglik's error grows with NIS (it is -NIS / 2 plus terms).
SLIP_DIR = np.array([0.6, -0.64, 0.48])
SLIP_SIGMAS = {"go1": 65.0, "cassie": 85.0, "tripod": 92.0, "pogox": 60.0}


def slip_velocity(p, J, sigmas):
    """the foot velocity of a slip of `sigmas` standard deviations of the leg's encoder-velocity noise J C_enc_vel J' along SLIP_DIR"""
    nj = J.shape[1]
    std = np.array([p.joint_velocity_std[i] for i in range(nj)])
    return sigmas * np.linalg.cholesky((J * std ** 2) @ J.T) @ SLIP_DIR


# The cases.  name: (injected slips [(tick, instance, leg)], high gate, low gate).  The logs are those of innov_lib.CPU_CASES / GPU_CASES
# (instances 0 and 1 of a case are the same robots in both, the GPU's tripod and PogoX logs are shorter: a pair past the end of a log
# is left out there); every injected pair has contact 1 in the log.  PogoX: the two robots of innov_lib's log stay in flight for all
# of its ticks, so the gate's case takes the next two robots of the same fleet (rough_streams' seed_shift 2), of which one touches down
# at tick 6 and the other stands throughout.  What the pairs cover:
#   go1     (7, 1, 2) a window-fill tick with mixed contact | (18, 1, 1) every leg in stance | (21, 0, 2) the first full window |
#           (26, 1, 0) + (26, 1, 3) two legs of one robot at one tick, all of its stance legs | (33, 1, 0) a full window with mixed
#           contact | (44, 1, 0) and (46, 0, 3) windows with VO equality rows (the slow and the fast camera)
#   cassie  (5, 0, 1) fill | (20, 1, 0) + (20, 1, 1) both legs | (27, 1, 0) full, mixed | (46, 0, 0) VO equality rows
#   tripod  (4, 1, 1) fill | (19, 1, 0) + (19, 1, 1) two legs, full (N = 12) | (43, 1, 0) VO equality rows, its only stance leg
#   pogox   (3, 1, 0), (8, 0, 0), (10, 1, 0): its only leg, inside the window fill (N = 100)
# The high gate sits between the nominal maximum and the injected minimum of the reference's nis_leg, a factor 3 or more from each
# (test_innovation_gate.py prints both and asserts it); the low gate sits inside the nominal spread.
CASES = {
    "go1": ([(7, 1, 2), (18, 1, 1), (21, 0, 2), (26, 1, 0), (26, 1, 3), (33, 1, 0), (44, 1, 0), (46, 0, 3)], 950.0, 150.0),
    "cassie": ([(5, 0, 1), (20, 1, 0), (20, 1, 1), (27, 1, 0), (46, 0, 0)], 1800.0, 150.0),
    "tripod": ([(4, 1, 1), (19, 1, 0), (19, 1, 1), (43, 1, 0)], 2100.0, 150.0),
    "pogox": ([(3, 1, 0), (8, 0, 0), (10, 1, 0)], 950.0, 150.0),
}
POGOX_SHIFT = 2


# ------------------------------------------------------------------ logs
def copy_streams(s):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}


def inject_slips(p, s, pairs, sigmas):
    """a copy of the streams with a foot slip at every (tick, instance, leg): the joint velocity of a foot that moves with
    slip_velocity (J^-1 v; the pseudo-inverse for Cassie's 3 x 5 Jacobian) added to qdot.  Pairs outside the log are ignored"""
    so = copy_streams(s)
    K, B = so["contact"].shape[:2]
    for k, b, leg in pairs:
        if k < K and b < B:
            assert so["contact"][k, b, leg] == 1.0, (k, b, leg)
            J = so["J"][k, b, leg]
            so["qdot"][k, b, leg] += np.linalg.pinv(J) @ slip_velocity(p, J, sigmas)
    return so


def edit_contact(s, pairs):
    """a copy of the streams with contact = 0 at every (tick, instance, leg)"""
    so = copy_streams(s)
    for k, b, leg in pairs:
        so["contact"][k, b, leg] = 0.0
    return so


# ------------------------------------------------------------------ the reference
def _replay(p, s, b, upto):
    pipe = O.Pipe(p)
    for k in range(upto + 1):
        pipe.feed(s, k, b)
        pipe.step(k)
    return pipe


def reference(p, s, b, K, gate):
    """{tick: dict} of instance b, ticks 1 .. K - 1, independent of the code under test.  The oracle's pipe cannot be copied, so it is
    replayed: the pipe that reaches tick k has been fed contact = 0 at every (tick, leg) the REFERENCE decided to gate before k (a pipe
    goes on to the next tick as long as nothing new is gated: a replay from tick 0 with the same edits is the same pipe).  At tick k
    innov_lib.reference_of_qp of its QP gives the five arrays of the ungated problem and, from them, the decision nis_leg > gate; where
    legs are gated, a fresh pipe replayed through tick k with the new edits gives the QP whose direct_lib.kkt_of_qp is the gated x_T
    and Cov(x_T), and goes on from there.  Entries: the five arrays (innov_lib.KEYS), gated [L], x [ns], cov [ns, ns], vo"""
    ns, L = p.dim_state, p.num_legs
    edits = []
    se = s
    pipe = O.Pipe(p)
    out = {}
    for k in range(K):
        pipe.feed(se, k, b)
        pipe.step(k)
        if k == 0:
            continue
        qp = pipe.est.qp()
        r = IL.reference_of_qp(p, qp, k)
        gated = (r["nis_leg"] > gate).astype(np.int32)
        if gated.any():
            edits += [(k, b, int(leg)) for leg in np.nonzero(gated)[0]]
            se = edit_contact(s, edits)
            pipe = _replay(p, se, b, k)
            qp = pipe.est.qp()
        x, Ki, xo, nv = DL.kkt_of_qp(p, qp, k)
        o = xo[-1]
        out[k] = dict({key: r[key] for key in IL.KEYS}, gated=gated, x=x[o:o + ns].copy(), cov=Ki[o:o + ns, o:o + ns].copy(), vo=nv)
    return out


def decisions(ref):
    """[(tick, instance, leg)] the reference gated, of {instance: reference()}"""
    return sorted((k, b, int(leg)) for b, rb in ref.items() for k, r in rb.items() for leg in np.nonzero(r["gated"])[0])


def case_streams(name, gpu=False):
    """(params, B, K, instances held against the oracle, the case's log with its slips injected)"""
    if gpu:
        mk, B, K, sub, _ = IL.GPU_CASES[name]
        p, s = IL.gpu_streams(name)
    else:
        mk, B, K, _ = IL.CPU_CASES[name]
        p = mk()
        s = DL.rough_streams(p, B, K)
        sub = list(range(B))
    if name == "pogox":
        B, sub = 2, [0, 1]
        s = DL.rough_streams(p, B, K, seed_shift=POGOX_SHIFT)
    return p, B, K, sub, inject_slips(p, s, CASES[name][0], SLIP_SIGMAS[name])


@functools.lru_cache(maxsize=None)
def case_reference(name, which, gpu=False):
    """(params, streams with the slips, gate, {instance: reference}) of a case at its "high" or "low" gate, once per process"""
    p, B, K, sub, s = case_streams(name, gpu)
    gate = CASES[name][1 if which == "high" else 2]
    return p, s, gate, {b: reference(p, s, b, K, gate) for b in sub}


def check_margin(ref, gate, what):
    """no reference nis_leg within a relative MARGIN of the gate: the decisions do not hang on rounding"""
    for b, rb in ref.items():
        for k, r in rb.items():
            assert (np.abs(r["nis_leg"] - gate) > MARGIN * gate).all(), (what, b, k, r["nis_leg"], gate)


def x_err(x, ref):
    return DL.block_err(x, ref, DL.blocks3(len(ref)), DL.XREL, DL.XABS)


# ------------------------------------------------------------------ the lane-sequential harness
LIB = os.path.join(DL.HOSTSIM, "libgate_hostsim.so")
_libs = {}


def gate_hostsim():
    """tests/hostsim/gate_hostsim.cpp as libgate_hostsim.so, rebuilt when a source is newer, and bound"""
    if "lib" not in _libs:
        srcs = [os.path.join(DL.HOSTSIM, f) for f in ("hostsim.cpp", "direct_hostsim.cpp", "innov_hostsim.cpp", "gate_hostsim.cpp")] + \
            [os.path.join(DL.CSRC, f) for f in os.listdir(DL.CSRC) if f.endswith(".h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(f) > os.path.getmtime(LIB) for f in srcs):
            subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-DDEKF_HOSTSIM", "-w", "-O2", "-o", LIB,
                                   os.path.join(DL.HOSTSIM, "gate_hostsim.cpp")])
        L = HL._bind(C.CDLL(LIB))
        L.hs_update_direct_innov.argtypes = [C.c_void_p, C.c_int] + [HL._dp] * 6
        L.hs_update_direct_innov.restype = C.c_int
        L.hs_update_direct_innov_gate.argtypes = [C.c_void_p, C.c_int, C.c_double] + [HL._dp] * 6 + [HL._ip]
        L.hs_update_direct_innov_gate.restype = C.c_int
        L.hs_get_record_qm.argtypes = [C.c_void_p, C.c_int, HL._dp]
        _libs["lib"] = L
    return _libs["lib"]


class GateSim(HL.HostSim):
    """hostsim_lib.HostSim on the gate harness: step(T) runs the assemble step, the plain direct core, the innovation core and, with
    gate > 0, the gate core; keeps Cov(x_T), the five arrays, gated [B, L] and the Q_m words of the newest record"""

    def __init__(self, params, batch, gate=0.0):
        self.p, self.B, self.L, self.gate = params, batch, gate_hostsim(), gate
        self.h = self.L.hs_create(C.byref(params), batch)
        assert self.h, "hs_create rejected the parameters"

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
        self.gated = np.zeros((B, L), np.int32)
        arrays = [HL._p(self.cov)] + [HL._p(self.out[k]) for k in IL.KEYS]
        if self.gate > 0.0:
            assert self.L.hs_update_direct_innov_gate(self.h, T, self.gate, *arrays, HL._p(self.gated)) == 0
        else:
            assert self.L.hs_update_direct_innov(self.h, T, *arrays) == 0
        self.qm = np.zeros((B, L, 6))
        self.L.hs_get_record_qm(self.h, T, HL._p(self.qm))


def run_sim(p, s, B, K, gate=0.0):
    """a list over the ticks 1 .. K - 1 (entry k - 1: tick k) of what a lane-sequential run left: x, v_b, status, cov, the five
    arrays, gated and the newest record's Q_m words"""
    sim = GateSim(p, B, gate)
    out = []
    for k in range(K):
        sim.feed(s, k)
        sim.step(k)
        if k:
            g = sim.get()
            out.append(dict({key: a.copy() for key, a in sim.out.items()}, x=g["x"], v_b=g["v_b"], status=g["status"], cov=sim.cov.copy(),
                            gated=sim.gated.copy(), qm=sim.qm.copy()))
    return out


@functools.lru_cache(maxsize=None)
def case_sim(name, which):
    """the lane-sequential run of a CPU case at its "high" or "low" gate ("off": the same log without the gate), once per process"""
    p, B, K, _, s = case_streams(name)
    gate = {"high": CASES[name][1], "low": CASES[name][2], "off": 0.0, "never": NEVER}[which]
    return run_sim(p, s, B, K, gate)


OUTPUTS = ("x", "v_b", "status", "cov") + IL.KEYS   # what the bit contracts are about (GPU: and the iteration counts)


def check_against_reference(run, ref, instances, what):
    """every tick of `run` (run_sim or run_gpu) for `instances` against the reference: gated equal; the five arrays within innov_lib's
    limits; x within XREL / XABS and the covariance within CREL.  Returns the worst errors"""
    worst = {}
    for b in instances:
        for k, r in ref[b].items():
            g = run[k - 1]
            assert np.array_equal(g["gated"][b], r["gated"]), (what, b, k, g["gated"][b], r["gated"], g["nis_leg"][b], r["nis_leg"])
            assert g["status"][b] == 1, (what, b, k)
            e = IL.errors(IL.instance(g, b), r)
            e["x"], e["cov"] = x_err(g["x"][b], r["x"]), DL.cov_err(g["cov"][b], r["cov"])
            kind = "gated " if r["gated"].any() else ""
            for key, v in e.items():
                worst[kind + key] = max(v, worst.get(kind + key, 0.0))
            IL.assert_within_limits(e, (what, b, k))
            assert e["x"] <= 1.0 and e["cov"] <= DL.CREL, (what, b, k, e)
    return worst


def edited_copies(s, b, B, dec):
    """(gated ticks of instance b, a log of len(ticks) + 1 copies of robot b): copy i is fed contact = 0 at every pair of `dec` that b
    gated at its i first gated ticks (copy 0: the log as it is)"""
    mine = [d for d in dec if d[1] == b]
    ticks = sorted({d[0] for d in mine})
    so = copy_streams(DL.sub_streams(s, np.full(len(ticks) + 1, b), B))
    for i in range(1, len(ticks) + 1):
        for k, _, leg in mine:
            if k <= ticks[i - 1]:
                so["contact"][k, i, leg] = 0.0
    return ticks, so


def check_bits_on_ungated_ticks(run, off_run, s, dec, B, K, what, keys=OUTPUTS):
    """At every tick at which instance b gates nothing, its outputs equal, to the bit, those of a gate-off innovation run fed the log
    with contact zeroed at every pair b gated before.  off_run: a function (streams, batch) -> the gate-off run of that log; it is
    called once per instance, with edited_copies (a robot's results do not depend on its batch).  Returns how many (instance, tick)
    were compared behind a gated one"""
    behind = 0
    for b in range(B):
        ticks, so = edited_copies(s, b, B, dec)
        off = off_run(so, len(ticks) + 1)
        for i in range(len(ticks) + 1):
            lo = ticks[i - 1] + 1 if i else 1
            hi = ticks[i] if i < len(ticks) else K
            for k in range(lo, hi):
                for key in keys:
                    assert np.array_equal(run[k - 1][key][b], off[k - 1][key][i], equal_nan=True), (what, b, k, key)
                behind += i > 0
    return behind


# ------------------------------------------------------------------ the GPU runner
def run_gpu(p, s, B, K, gate=0.0, est=None, close=True, after=None):
    """a list over the ticks 1 .. K - 1 of innov_lib.gpu_record with the five arrays and, on a gating handle, gated.
    after: called with (tick, estimator) behind every step"""
    from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host
    if est is None:
        est = BatchedEstimator(p, B, solver="direct", innovation=True, innovation_gate=gate)
    sh = streams_host(s)
    out = []
    for k in range(K):
        est.push_stream_step(sh, k)
        est.step(k)
        if k:
            r = IL.gpu_record(est)
            r.update(est.innovation())
            r["gated"] = est.innovation_gate()[1] if gate > 0.0 else np.zeros((B, p.num_legs), np.int32)
            out.append(r)
        if after:
            after(k, est)
    names = (est.solve_kernel_name(True), est.solve_kernel_name(False))
    if close:
        est.close()
    return out, names, est
