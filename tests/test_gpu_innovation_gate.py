"""The innovation gate of a direct handle on the GPU (dekf_set_innovation_gate / dekf_get_innovation_gate,
BatchedEstimator(innovation_gate=...) and .innovation_gate()): every tick of the smallest shapes that reach the four kernels against
the reference of gate_lib (the oracle's pipe replayed with the reference's own decisions) at two gates per case; the bit contracts
(a gate that never fires, the batch, the two kinds of pointer, a reset, the ungated ticks against a gate-off handle on the edited
log); restart, pause and parameter table on one handle; the status codes."""
import ctypes as C

import numpy as np
import pytest

import direct_lib as DL
import epoch_lib as EL
import gate_lib as GL
import innov_lib as IL
import pause_lib as PZ
from decentralized_ekf_mhe_amd import capi, go1_params
from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host

pytestmark = pytest.mark.gpu

NAMES = list(GL.CASES)
SOLVE_KERNEL = {"go1": "k_mhe_solve_direct_4_n20", "cassie": "k_mhe_solve_direct_2_n20", "tripod": "k_mhe_solve_direct_3", "pogox": "k_mhe_solve_direct_1"}
OUTPUTS = GL.OUTPUTS + ("iters",)
_runs = {}


def case_run(name, which):
    """(records, kernel names) of a GPU case at its "high" or "low" gate, "never" or "off", once per process"""
    if (name, which) not in _runs:
        p, B, K, sub, s = GL.case_streams(name, gpu=True)
        gate = {"high": GL.CASES[name][1], "low": GL.CASES[name][2], "never": GL.NEVER, "off": 0.0}[which]
        _runs[name, which] = GL.run_gpu(p, s, B, K, gate)[:2]
    return _runs[name, which]


def own_decisions(run):
    """[(tick, instance, leg)] the handle gated"""
    return sorted((k + 1, int(b), int(leg)) for k, r in enumerate(run) for b, leg in zip(*np.nonzero(r["gated"])))


def _equal(a, b, keys, what):
    assert len(a) == len(b), what
    for i, (ra, rb) in enumerate(zip(a, b)):
        for key in keys:
            assert np.array_equal(ra[key], rb[key], equal_nan=True), (what, i + 1, key)


# ------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("which", ["high", "low"])
@pytest.mark.parametrize("name", NAMES)
def test_every_tick_against_the_reference(name, which):
    """Go1 B = 6, 48 ticks, Cassie B = 2, 48 ticks, the tripod B = 2, 24 ticks, PogoX B = 2, 12 ticks: every tick of the oracle
    instances: gated equal to the reference's decisions, the five arrays within innov_lib's limits, x_mhe and Cov(x_T) within the
    direct solve's yardsticks.  The high gate's reference gates exactly the injected slips of the log"""
    p, B, K, sub, _ = GL.case_streams(name, gpu=True)
    _, s, gate, ref = GL.case_reference(name, which, gpu=True)
    GL.check_margin(ref, gate, name)
    if which == "high":
        assert GL.decisions(ref) == sorted(q for q in GL.CASES[name][0] if q[0] < K and q[1] in sub)
    run, names = case_run(name, which)
    assert names == (SOLVE_KERNEL[name],) * 2   # (the solve kernel is the one of a handle without the gate)
    worst = GL.check_against_reference(run, ref, sub, (name, which))
    print(name, which, {key: f"{v:.2e}" for key, v in sorted(worst.items())})
    assert any(key.startswith("gated ") for key in worst)
    for k, r in enumerate(run):   # the corrected covariance is symmetric to the bit
        for b in np.nonzero(r["gated"].any(axis=1))[0]:
            assert np.array_equal(r["cov"][b], r["cov"][b].T), (k + 1, b)


# ------------------------------------------------------------------ the bit contracts
@pytest.mark.parametrize("name", NAMES)
def test_a_gate_that_never_fires_is_the_gate_off(name):
    never, off = case_run(name, "never")[0], case_run(name, "off")[0]
    assert not any(r["gated"].any() for r in never)
    _equal(never, off, OUTPUTS, name)


@pytest.mark.parametrize("name,which", [(n, "low") for n in NAMES] + [("go1", "high")])
def test_ungated_ticks_are_a_gate_off_handle_on_the_edited_log(name, which):
    """at every tick at which an instance gates nothing, dekf_get, Cov(x_T), the solver info and the five arrays are the bits of a
    gate-off innovation handle fed the log with contact = 0 at every (tick, leg) the instance gated before; at a gated tick the five
    arrays are those of the handle that has not seen this tick's edit, and x_mhe, v_b and Cov(x_T) agree with the handle that has"""
    p, B, K, sub, s = GL.case_streams(name, gpu=True)
    run = case_run(name, which)[0]
    dec = own_decisions(run)
    offs = {}

    def off_run(so, n):
        offs[len(offs)] = GL.run_gpu(p, so, n, K)[0]
        return offs[len(offs) - 1]

    behind = GL.check_bits_on_ungated_ticks(run, off_run, s, dec, B, K, (name, which), OUTPUTS)
    assert behind > 0
    for b in range(B):
        ticks, _ = GL.edited_copies(s, b, B, dec)
        for i, k in enumerate(ticks):
            g, o = run[k - 1], offs[b][k - 1]
            for key in IL.KEYS:
                assert np.array_equal(g[key][b], o[key][i]), (name, b, k, key)
            assert GL.x_err(g["x"][b], o["x"][i + 1]) <= 1.0 and DL.cov_err(g["cov"][b], o["cov"][i + 1]) <= DL.CREL, (name, b, k)
            # (v_b = R (v + w x p): a row of a rotation has a 1-norm of at most sqrt(3) < 2)
            assert np.abs(g["v_b"][b] - o["v_b"][i + 1]).max() <= 2.0 * (DL.XREL * np.abs(o["x"][i + 1][3:6]).max() + DL.XABS)


def test_results_do_not_depend_on_the_batch():
    """B = 6 against the first six of B = 70, at the low gate"""
    p, B, K, sub, _ = GL.case_streams("go1", gpu=True)
    pb, sb = IL.big_streams()
    big = GL.run_gpu(pb, GL.inject_slips(pb, sb, GL.CASES["go1"][0], GL.SLIP_SIGMAS["go1"]), IL.BIG, K, GL.CASES["go1"][2])[0]
    small = case_run("go1", "low")[0]
    assert any(r["gated"][B:].any() for r in big)
    for i, (ra, rb) in enumerate(zip(big, small)):
        for key in OUTPUTS + ("gated",):
            assert np.array_equal(ra[key][:B], rb[key]), (i + 1, key)


def test_reset_and_rerun_is_a_fresh_handle_and_pointers():
    """the bound survives dekf_reset, gated is zeroed by it; host and device pointers give the same bits; either pointer may be NULL"""
    import torch
    lib = capi.load()
    p, B, K, sub, s = GL.case_streams("go1", gpu=True)
    gate = GL.CASES["go1"][2]
    seen = []

    def after(k, est):
        if k not in (7, 18, 26):
            return
        bound, host = est.innovation_gate()
        dev = torch.full((B, p.num_legs), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        capi.check(lib.dekf_get_innovation_gate(est.h, None, C.c_void_p(dev.data_ptr()), capi.DEKF_DEVICE))
        est.sync()
        assert bound == gate and np.array_equal(dev.cpu().numpy(), host), k
        only = C.c_double(-1.0)
        capi.check(lib.dekf_get_innovation_gate(est.h, C.byref(only), None, capi.DEKF_HOST))
        capi.check(lib.dekf_get_innovation_gate(est.h, None, None, capi.DEKF_HOST))
        assert only.value == gate
        seen.append(int(host.sum()))

    first, _, est = GL.run_gpu(p, s, B, 30, gate, close=False, after=after)
    assert sum(seen) > 0 and any(r["gated"].any() for r in first)
    est.reset()
    bound, gated = est.innovation_gate()
    assert bound == gate and not gated.any()
    again = GL.run_gpu(p, s, B, 30, gate, est=est)[0]
    fresh = case_run("go1", "low")[0]
    _equal(first, fresh[:29], OUTPUTS + ("gated",), "first run")
    _equal(again, fresh[:29], OUTPUTS + ("gated",), "after the reset")


# ------------------------------------------------------------------ restart, pause and parameter table on one handle
def test_restart_pause_and_parameter_table_on_one_handle():
    """Go1, B = 4, 30 ticks, the low gate, a parameter table.  Instance 3 runs a second set that differs in foot_swing_std alone (0.5
    m/s: a swing gain that shows): its gated records behave as THAT set's swing: the bits of a gate-off handle created with the set,
    fed the edited log, and not those of a handle with the default swing gain.  Instance 1 is restarted before step 12: gated 0 at once,
    then the bits of a fresh gating handle fed the samples from step 12.  Instance 2 is paused for steps 8 to 11: it keeps every bit,
    gated included, then goes on as a handle that never saw those steps.  Instance 0 is untouched."""
    p = DL._params(go1_params)
    B, K, gate = 4, 30, GL.CASES["go1"][2]
    s0 = DL.rough_streams(p, B, K)
    pairs = [q for q in GL.CASES["go1"][0] if q[0] < K]
    pairs += [(k, 3, int(np.nonzero(s0["contact"][k, 3])[0][0])) for k in (9, 16)]
    s = GL.inject_slips(p, s0, pairs, GL.SLIP_SIGMAS["go1"])
    other = p.copy()
    for i in range(3):
        other.foot_swing_std[i] = 0.5
    est = BatchedEstimator(p, B, solver="direct", innovation=True, innovation_gate=gate)
    est.set_instance_params([p, other], [0, 0, 0, 1])
    assert est.solve_kernel_name() == "k_mhe_solve_direct_4_n20_pp"
    sh = streams_host(s)
    got = [None]
    for k in range(K):
        if k == 12:
            before = est.innovation_gate()[1]
            est.reset_instances(np.array([0, 1, 0, 0], np.int32))
            after = est.innovation_gate()[1]
            assert not after[1].any() and np.array_equal(after[[0, 2, 3]], before[[0, 2, 3]])
        if k == 8:
            est.set_active(np.array([1, 1, 0, 1], np.int32))
        if k == 12:
            est.set_active(np.ones(B, np.int32))
        est.push_stream_step(sh, k)
        est.step(k)
        if k:
            got.append(dict(IL.gpu_record(est), **est.innovation(), gated=est.innovation_gate()[1]))
    est.close()
    keys = OUTPUTS + ("gated",)
    whole = GL.run_gpu(p, s, B, K, gate)[0]                            # instance 0: never named
    assert any(r["gated"][0].any() for r in whole)
    for k in range(1, K):
        for key in keys:
            assert np.array_equal(got[k][key][0], whole[k - 1][key][0]), (k, key)
    # instance 1: a fresh gating handle from the restart on (its first solve is step 13)
    assert np.isnan(got[12]["nis_leg"][1]).all() and not got[12]["gated"][1].any()
    fresh = GL.run_gpu(p, EL.slice_streams(s, 12), B, K - 12, gate)[0]
    assert any(r["gated"][1].any() for r in fresh)
    for k in range(13, K):
        for key in keys:
            assert np.array_equal(got[k][key][1], fresh[k - 13][key][1], equal_nan=True), (k, key)
    # instance 2: frozen over steps 8 .. 11, then the log with those steps cut out
    life = tuple(k for k in range(K) if not 8 <= k < 12)
    cut = GL.run_gpu(p, PZ.cut_streams(s, life), B, len(life), gate)[0]
    assert any(r["gated"][2].any() for r in cut)
    for k in range(1, K):
        ref = got[7] if 8 <= k < 12 else cut[life.index(k) - 1]
        for key in keys:
            assert np.array_equal(got[k][key][2], ref[key][2], equal_nan=True), (k, key)
    # instance 3: its ungated ticks are a gate-off handle created with ITS set on the edited log
    run3 = [dict(r) for r in got[1:]]
    dec = own_decisions(run3)
    assert [d for d in dec if d[1] == 3]
    ticks, so = GL.edited_copies(s, 3, B, dec)
    n = len(ticks) + 1
    mine, default = GL.run_gpu(other, so, n, K)[0], GL.run_gpu(p, so, n, K)[0]
    differs = False
    for i in range(n):
        lo, hi = (ticks[i - 1] + 1 if i else 1), (ticks[i] if i < len(ticks) else K)
        for k in range(lo, hi):
            for key in OUTPUTS:
                assert np.array_equal(got[k][key][3], mine[k - 1][key][i], equal_nan=True), (k, key)
            differs = differs or (i > 0 and not np.array_equal(mine[k - 1]["x"][i], default[k - 1]["x"][i]))
    assert differs and ticks[0] + 1 < K   # (the default swing gain gives other bits: the record took the instance's own)


# ------------------------------------------------------------------ the status codes
def test_status_codes():
    lib = capi.load()
    p = DL._params(go1_params)
    B = 3
    sh = streams_host(DL.rough_streams(p, B, 3))
    gated = np.zeros((B, p.num_legs), np.int32)
    bound = C.c_double(-1.0)

    def get(est):
        return lib.dekf_get_innovation_gate(est.h, C.byref(bound), C.c_void_p(gated.ctypes.data), capi.DEKF_HOST)

    # ADMM, KF and foot-state handles cannot be innovation handles: a positive bound is refused, 0 is accepted, gated is refused
    for est in (BatchedEstimator(p, B), BatchedEstimator(DL._params(go1_params, est_type=1), B),
                BatchedEstimator(DL._params(go1_params, leg_odom_type=1), B, solver="direct")):
        assert lib.dekf_set_innovation_gate(est.h, 100.0) == capi.DEKF_ERR_INVALID
        assert lib.dekf_set_innovation_gate(est.h, 0.0) == capi.DEKF_OK
        assert get(est) == capi.DEKF_ERR_INVALID and bound.value == 0.0
        est.close()
    with pytest.raises(capi.DekfError):
        BatchedEstimator(p, B, solver="direct", innovation_gate=100.0)       # a direct handle without the innovation statistics
    with pytest.raises(capi.DekfError):
        BatchedEstimator(p, B, solver="direct", smoother=True, innovation=True, innovation_gate=100.0)   # a smoothing handle
    est = BatchedEstimator(p, B, solver="direct", innovation=True)
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert lib.dekf_set_innovation_gate(est.h, bad) == capi.DEKF_ERR_INVALID
    assert est.solve_kernel_name() == "k_mhe_solve_direct_4_n20"
    assert lib.dekf_set_innovation_gate(est.h, 100.0) == capi.DEKF_OK
    assert est.solve_kernel_name() == "k_mhe_solve_direct_4_n20"              # the solve kernel is the same one
    assert get(est) == capi.DEKF_OK and bound.value == 100.0 and not gated.any()
    assert lib.dekf_set_smoother(est.h, 1) == capi.DEKF_ERR_INVALID           # no smoother on a gating handle
    assert lib.dekf_set_smoother(est.h, 0) == capi.DEKF_OK
    est.push_stream_step(sh, 0)
    est.step(0)
    assert lib.dekf_set_innovation_gate(est.h, 50.0) == capi.DEKF_ERR_ORDER   # not on a running handle
    assert lib.dekf_set_innovation_gate(est.h, 0.0) == capi.DEKF_ERR_ORDER
    est.push_stream_step(sh, 1)
    est.step(1)
    assert get(est) == capi.DEKF_OK and bound.value == 100.0
    est.reset()
    assert get(est) == capi.DEKF_OK and bound.value == 100.0 and not gated.any()   # the setting survives
    assert lib.dekf_set_innovation_gate(est.h, 120.0) == capi.DEKF_OK         # right after dekf_reset
    # dekf_set_innovation(h, 0) switches the gate off; switching the statistics back on does not switch it on again
    capi.check(lib.dekf_set_innovation(est.h, 0))
    assert get(est) == capi.DEKF_ERR_INVALID and bound.value == 0.0
    capi.check(lib.dekf_set_innovation(est.h, 1))
    assert get(est) == capi.DEKF_ERR_INVALID and bound.value == 0.0
    capi.check(lib.dekf_set_smoother(est.h, 1))                               # (the gate is off: the smoother is allowed again)
    assert lib.dekf_set_innovation_gate(est.h, 100.0) == capi.DEKF_ERR_INVALID
    capi.check(lib.dekf_set_smoother(est.h, 0))
    # ... and so does dekf_set_solver(ADMM)
    capi.check(lib.dekf_set_innovation_gate(est.h, 100.0))
    capi.check(lib.dekf_set_solver(est.h, capi.DEKF_SOLVER_ADMM))
    assert get(est) == capi.DEKF_ERR_INVALID and bound.value == 0.0
    capi.check(lib.dekf_set_solver(est.h, capi.DEKF_SOLVER_DIRECT))
    capi.check(lib.dekf_set_innovation(est.h, 1))
    assert get(est) == capi.DEKF_ERR_INVALID and bound.value == 0.0
    for k in range(2):
        est.push_stream_step(sh, k)
        est.step(k)
    assert np.isfinite(est.innovation()["nis"]).all()
    est.close()
