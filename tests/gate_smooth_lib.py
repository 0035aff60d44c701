"""What the tests of the window of a gating handle share (dekf_set_gate_smoother; test_gate_smoother.py, test_gpu_gate_smoother.py):
the reference (gate_lib.reference's replay, returning every window block), the lane-sequential harness
(tests/hostsim/gate_smooth_hostsim.cpp) and the runners.  Cases, gates and slips are gate_lib's, unchanged.
TEST INFRASTRUCTURE ONLY.  Importing this module does not touch the GPU."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import direct_lib as DL
import gate_lib as GL
import hostsim_lib as HL
import innov_lib as IL
import oracle_lib as O

KERNELS = [f"k_mhe_innov_gate_{L}_smooth{t}" for L in (1, 2, 3, 4) for t in ("", "_ep")]
WINDOW = ("xw", "cw")   # the window arrays of a record (whole buffers; K says how many entries are written)


# ------------------------------------------------------------------ the reference
def reference(p, s, b, K, gate):
    """gate_lib.reference with the whole window: {tick: dict} of instance b, ticks 1 .. K - 1.  The replay and the decisions are
    gate_lib.reference's; at every tick direct_lib.kkt_of_qp of the replayed pipe's QP (the one with the gated legs' swing blocks where
    legs are gated) gives the state blocks x[xo[j]:...] and the diagonal blocks of Ki, as direct_lib.window_reference does.  Entries:
    gate_lib.reference's, and xw [K, ns], cw [K, ns, ns]"""
    ns = p.dim_state
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
            se = GL.edit_contact(s, edits)
            pipe = GL._replay(p, se, b, k)
            qp = pipe.est.qp()
        x, Ki, xo, nv = DL.kkt_of_qp(p, qp, k)
        xw = np.array([x[o:o + ns] for o in xo])
        cw = np.array([Ki[o:o + ns, o:o + ns] for o in xo])
        out[k] = dict({key: r[key] for key in IL.KEYS}, gated=gated, x=xw[-1].copy(), cov=cw[-1].copy(), vo=nv, xw=xw, cw=cw)
    return out


@functools.lru_cache(maxsize=None)
def case_reference(name, which, gpu=False):
    """(params, streams with the slips, gate, {instance: reference}) of a case of gate_lib.CASES at its "high" or "low" gate, once per
    process"""
    p, B, K, sub, s = GL.case_streams(name, gpu)
    gate = GL.CASES[name][1 if which == "high" else 2]
    return p, s, gate, {b: reference(p, s, b, K, gate) for b in sub}


def check_window_against_reference(run, ref, instances, what):
    """every tick of `run` for `instances`: K equal, the window within direct_lib.window_errors' yardsticks (XREL / XABS per 3-block,
    CREL), entries k >= K at FILL where the run keeps whole buffers.  Returns the worst (x, cov) errors of the gated and ungated ticks"""
    worst = {}
    for b in instances:
        for k, r in ref[b].items():
            g = run[k - 1]
            Kw = len(r["xw"])
            assert g["K"] == Kw, (what, b, k, g["K"], Kw)
            ex, ec, at = DL.window_errors(g["xw"][b][:Kw], g["cw"][b][:Kw], r["xw"], r["cw"], len(r["x"]))
            kind = "gated" if r["gated"].any() else "ungated"
            w = worst.get(kind, (0.0, 0.0))
            worst[kind] = (max(w[0], ex), max(w[1], ec))
            assert ex <= 1.0 and ec <= DL.CREL, (what, b, k, kind, ex, ec, at)
            assert (g["xw"][b][Kw:] == DL.FILL).all() and (g["cw"][b][Kw:] == DL.FILL).all(), (what, b, k)
    return worst


def check_window_bits_at_gated_ticks(run, what):
    """at every (tick, instance) that gated: x_win[K-1] == x_mhe and cov_win[K-1] == the covariance block to the bit, every cov_win[k]
    symmetric to the bit.  Returns how many were seen"""
    seen = 0
    for k, g in enumerate(run):
        Kw = g["K"]
        for b in np.nonzero(g["gated"].any(axis=1))[0]:
            seen += 1
            assert np.array_equal(g["xw"][b][Kw - 1], g["x"][b]), (what, k + 1, b)
            assert np.array_equal(g["cw"][b][Kw - 1], g["cov"][b]), (what, k + 1, b)
            for j in range(Kw):
                assert np.array_equal(g["cw"][b][j], g["cw"][b][j].T), (what, k + 1, b, j)
    return seen


# ------------------------------------------------------------------ the lane-sequential harness
LIB = os.path.join(DL.HOSTSIM, "libgate_smooth_hostsim.so")
_libs = {}


def gate_smooth_hostsim():
    """tests/hostsim/gate_smooth_hostsim.cpp as libgate_smooth_hostsim.so, rebuilt when a source is newer, and bound"""
    if "lib" not in _libs:
        srcs = [os.path.join(DL.HOSTSIM, f) for f in ("hostsim.cpp", "direct_hostsim.cpp", "innov_hostsim.cpp", "gate_hostsim.cpp",
                                                      "gate_smooth_hostsim.cpp")] + \
            [os.path.join(DL.CSRC, f) for f in os.listdir(DL.CSRC) if f.endswith(".h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(f) > os.path.getmtime(LIB) for f in srcs):
            subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-DDEKF_HOSTSIM", "-w", "-O2", "-o", LIB,
                                   os.path.join(DL.HOSTSIM, "gate_smooth_hostsim.cpp")])
        L = HL._bind(C.CDLL(LIB))
        L.hs_update_direct_smooth_innov_gate.argtypes = [C.c_void_p, C.c_int, C.c_double] + [HL._dp] * 8 + [HL._ip]
        L.hs_update_direct_smooth_innov_gate.restype = C.c_int
        L.hs_get_record_qm.argtypes = [C.c_void_p, C.c_int, HL._dp]
        L.hs_gate_window_failed.argtypes = [C.c_void_p, C.c_int, C.c_int, HL._dp, HL._dp]
        _libs["lib"] = L
    return _libs["lib"]


class GateSmoothSim(HL.HostSim):
    """gate_lib.GateSim on the harness of this option: step(T) runs the assemble step, the SMOOTH direct core, the innovation core and,
    with gate > 0, the gate core and the window correction; keeps what GateSim keeps, and K and the window arrays xw, cw ([B][N][...],
    pre-filled with direct_lib.FILL)"""

    def __init__(self, params, batch, gate=0.0):
        self.p, self.B, self.L, self.gate = params, batch, gate_smooth_hostsim(), gate
        self.h = self.L.hs_create(C.byref(params), batch)
        assert self.h, "hs_create rejected the parameters"

    def step(self, T):
        self.L.hs_ekf_step(self.h)
        if T == 0:
            self.L.hs_initialize(self.h)
            return
        B, ns, L, N = self.B, self.p.dim_state, self.p.num_legs, self.p.N
        nm = 3 * L
        self.cov = np.zeros((B, ns, ns))
        self.xw, self.cw = np.full((B, N, ns), DL.FILL), np.full((B, N, ns, ns), DL.FILL)
        self.out = dict(innov=np.full((B, nm), np.nan), innov_cov=np.full((B, nm, nm), np.nan), nis=np.full(B, np.nan),
                        nis_leg=np.full((B, L), np.nan), loglik=np.full(B, np.nan))
        self.gated = np.zeros((B, L), np.int32)
        assert self.L.hs_update_direct_smooth_innov_gate(self.h, T, self.gate, HL._p(self.cov), HL._p(self.xw), HL._p(self.cw),
                                                         *[HL._p(self.out[k]) for k in IL.KEYS], HL._p(self.gated)) == 0
        self.K = min(T + 1, N)
        self.qm = np.zeros((B, L, 6))
        self.L.hs_get_record_qm(self.h, T, HL._p(self.qm))


def run_sim(p, s, B, K, gate=0.0):
    """gate_lib.run_sim on the harness of this option (gate 0: a smoothing innovation handle without the gate): its entries, and K, xw,
    cw (whole buffers: entries k >= K hold direct_lib.FILL)"""
    sim = GateSmoothSim(p, B, gate)
    out = []
    for k in range(K):
        sim.feed(s, k)
        sim.step(k)
        if k:
            g = sim.get()
            out.append(dict({key: a.copy() for key, a in sim.out.items()}, x=g["x"], v_b=g["v_b"], status=g["status"], cov=sim.cov.copy(),
                            gated=sim.gated.copy(), qm=sim.qm.copy(), K=sim.K, xw=sim.xw.copy(), cw=sim.cw.copy()))
    return out


@functools.lru_cache(maxsize=None)
def case_sim(name, which):
    """the lane-sequential run of a CPU case at its "high" or "low" gate, "never", or "off" (the smoothing innovation run without the
    gate), once per process"""
    p, B, K, _, s = GL.case_streams(name)
    gate = {"high": GL.CASES[name][1], "low": GL.CASES[name][2], "off": 0.0, "never": GL.NEVER}[which]
    return run_sim(p, s, B, K, gate)


# ------------------------------------------------------------------ the GPU runner
def make_est(p, B, gate, params=None):
    """a handle with the option (gate > 0) or a smoothing innovation handle without the gate (gate 0)"""
    from decentralized_ekf_mhe_amd.estimator import BatchedEstimator
    if gate > 0.0:
        return BatchedEstimator(p, B, solver="direct", innovation=True, innovation_gate=gate, gate_smoother=True)
    return BatchedEstimator(p, B, solver="direct", smoother=True, innovation=True)


def window_record(est, N):
    """K and the window of the last update in whole buffers [B][N][...], the entries past K at direct_lib.FILL"""
    Kw, xw, cw = est.window()
    B, ns = xw.shape[0], xw.shape[2]
    fx, fc = np.full((B, N, ns), DL.FILL), np.full((B, N, ns, ns), DL.FILL)
    fx[:, :Kw], fc[:, :Kw] = xw, cw
    return dict(K=Kw, xw=fx, cw=fc)


def run_gpu(p, s, B, K, gate=0.0, est=None, close=True, before=None):
    """gate_lib.run_gpu on a handle of make_est, every record with the window (window_record).  before: called with (tick, estimator)
    in front of every step's pushes"""
    from decentralized_ekf_mhe_amd.estimator import streams_host
    if est is None:
        est = make_est(p, B, gate)
    sh = streams_host(s)
    out = []
    for k in range(K):
        if before:
            before(k, est)
        est.push_stream_step(sh, k)
        est.step(k)
        if k:
            r = IL.gpu_record(est)
            r.update(est.innovation())
            r["gated"] = est.innovation_gate()[1] if gate > 0.0 else np.zeros((B, p.num_legs), np.int32)
            r.update(window_record(est, p.N))
            out.append(r)
    names = (est.solve_kernel_name(True), est.solve_kernel_name(False))
    if close:
        est.close()
    return out, names, est
