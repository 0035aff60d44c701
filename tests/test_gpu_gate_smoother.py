"""The window of a gating handle on the GPU (dekf_set_gate_smoother, BatchedEstimator(gate_smoother=True)): every tick of the shapes
the gate's GPU tests run, against the reference of gate_smooth_lib at two gates per case; the bit contracts (the gate handle without
the option, a gate that never fires, the ungated ticks against a smoothing innovation handle on the edited log, the batch, the two
kinds of pointer, a reset); restart, pause and parameter table on one handle; the state rules; a snapshot round trip."""
import ctypes as C

import numpy as np
import pytest

import direct_lib as DL
import epoch_lib as EL
import gate_lib as GL
import gate_smooth_lib as GS
import innov_lib as IL
import pause_lib as PZ
import snapshot_lib as SL
from decentralized_ekf_mhe_amd import capi, go1_params
from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host

pytestmark = pytest.mark.gpu

NAMES = list(GL.CASES)
SOLVE_KERNEL = {"go1": "k_mhe_solve_direct_4_n20", "cassie": "k_mhe_solve_direct_2_n20", "tripod": "k_mhe_solve_direct_3", "pogox": "k_mhe_solve_direct_1"}
OUTPUTS = GL.OUTPUTS + ("iters",)
_runs = {}


def case_run(name, which):
    """(records, kernel names) of a GPU case at its "high" or "low" gate or "never" with the option, "off" (a smoothing innovation
    handle without the gate), or "plain high" / "plain low" (the gating handle without the option), once per process"""
    if (name, which) not in _runs:
        p, B, K, sub, s = GL.case_streams(name, gpu=True)
        gates = {"high": GL.CASES[name][1], "low": GL.CASES[name][2], "never": GL.NEVER, "off": 0.0}
        if which.startswith("plain "):
            _runs[name, which] = GL.run_gpu(p, s, B, K, gates[which[6:]])[:2]
        else:
            _runs[name, which] = GS.run_gpu(p, s, B, K, gates[which])[:2]
    return _runs[name, which]


def own_decisions(run):
    """[(tick, instance, leg)] the handle gated"""
    return sorted((k + 1, int(b), int(leg)) for k, r in enumerate(run) for b, leg in zip(*np.nonzero(r["gated"])))


def _equal(a, b, keys, what):
    assert len(a) == len(b), what
    for i, (ra, rb) in enumerate(zip(a, b)):
        for key in keys:
            assert np.array_equal(ra[key], rb[key], equal_nan=True), (what, i + 1, key)


# ------------------------------------------------------------------ accuracy and the bits of a gated tick
@pytest.mark.parametrize("which", ["high", "low"])
@pytest.mark.parametrize("name", NAMES)
def test_every_tick_against_the_reference(name, which):
    """Go1 B = 6, 48 ticks, Cassie B = 2, 48 ticks, the tripod B = 2, 24 ticks, PogoX B = 2, 12 ticks: every tick of the oracle
    instances: the decisions and the newest block as the gate's test holds them, every window block within the direct solve's
    yardsticks.  At gated ticks x_win[K-1] is x_mhe and cov_win[K-1] the covariance block to the bit, every cov_win[k] is symmetric to
    the bit.  Everything but the window is the bits of the gating handle without the option"""
    p, B, K, sub, _ = GL.case_streams(name, gpu=True)
    _, s, gate, ref = GS.case_reference(name, which, gpu=True)
    GL.check_margin(ref, gate, name)
    run, names = case_run(name, which)
    assert names == (SOLVE_KERNEL[name] + "_smooth",) * 2
    GL.check_against_reference(run, ref, sub, (name, which))
    worst = GS.check_window_against_reference(run, ref, sub, (name, which))
    print(name, which, {kind: f"x {v[0]:.2e} of the yardstick, cov {v[1]:.2e}" for kind, v in sorted(worst.items())})
    assert "gated" in worst and "ungated" in worst
    assert GS.check_window_bits_at_gated_ticks(run, (name, which)) == len({d[:2] for d in own_decisions(run)}) > 0
    plain, plain_names = case_run(name, "plain " + which)
    assert plain_names == (SOLVE_KERNEL[name],) * 2
    _equal(run, plain, OUTPUTS + ("gated",), (name, which, "against the handle without the option"))


# ------------------------------------------------------------------ the bit contracts
@pytest.mark.parametrize("name", NAMES)
def test_a_gate_that_never_fires_is_a_smoothing_innovation_handle(name):
    never, off = case_run(name, "never")[0], case_run(name, "off")[0]
    assert not any(r["gated"].any() for r in never)
    _equal(never, off, OUTPUTS + GS.WINDOW, name)
    assert [r["K"] for r in never] == [r["K"] for r in off]


@pytest.mark.parametrize("name,which", [(n, "low") for n in NAMES] + [("go1", "high")])
def test_ungated_ticks_are_a_smoothing_handle_on_the_edited_log(name, which):
    """at every tick at which an instance gates nothing, dekf_get, Cov(x_T), the solver info, the five arrays and the window are the
    bits of a smoothing innovation handle without the gate fed the log with contact = 0 at every (tick, leg) the instance gated before"""
    p, B, K, sub, s = GL.case_streams(name, gpu=True)
    run = case_run(name, which)[0]
    dec = own_decisions(run)
    behind = GL.check_bits_on_ungated_ticks(run, lambda so, n: GS.run_gpu(p, so, n, K)[0], s, dec, B, K, (name, which),
                                            OUTPUTS + GS.WINDOW)
    assert behind > 0


def test_results_do_not_depend_on_the_batch():
    """B = 6 against the first six of B = 70, at the low gate"""
    p, B, K, sub, _ = GL.case_streams("go1", gpu=True)
    pb, sb = IL.big_streams()
    big = GS.run_gpu(pb, GL.inject_slips(pb, sb, GL.CASES["go1"][0], GL.SLIP_SIGMAS["go1"]), IL.BIG, K, GL.CASES["go1"][2])[0]
    small = case_run("go1", "low")[0]
    assert any(r["gated"][B:].any() for r in big)
    for i, (ra, rb) in enumerate(zip(big, small)):
        assert ra["K"] == rb["K"]
        for key in OUTPUTS + ("gated",) + GS.WINDOW:
            assert np.array_equal(ra[key][:B], rb[key]), (i + 1, key)


def test_reset_and_rerun_is_a_fresh_handle_and_pointers():
    """the option survives dekf_reset; host and device pointers of dekf_get_window give the same bits at gated ticks, and the entries
    past K keep what the buffers held"""
    import torch
    lib = capi.load()
    p, B, K, sub, s = GL.case_streams("go1", gpu=True)
    gate, ns, N = GL.CASES["go1"][2], p.dim_state, p.N
    est = GS.make_est(p, B, gate)
    sh = streams_host(s)
    fresh = case_run("go1", "low")[0]
    gated_seen = 0
    for k in range(30):
        est.push_stream_step(sh, k)
        est.step(k)
        if not k or not est.innovation_gate()[1].any():
            continue
        gated_seen += 1
        Kw = min(k + 1, N)
        xh, ch = np.full((B, N, ns), DL.FILL), np.full((B, N, ns, ns), DL.FILL)
        kh = C.c_int(0)
        capi.check(lib.dekf_get_window(est.h, C.byref(kh), xh.ctypes.data, ch.ctypes.data, capi.DEKF_HOST))
        xd = torch.full((B, N, ns), DL.FILL, dtype=torch.float64, device="cuda")
        cd = torch.full((B, N, ns, ns), DL.FILL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        capi.check(lib.dekf_get_window(est.h, None, xd.data_ptr(), cd.data_ptr(), capi.DEKF_DEVICE))
        est.sync()
        assert kh.value == Kw and np.array_equal(xd.cpu().numpy(), xh) and np.array_equal(cd.cpu().numpy(), ch), k
        assert np.array_equal(xh, fresh[k - 1]["xw"]) and np.array_equal(ch, fresh[k - 1]["cw"]), k
    assert gated_seen >= 3
    est.reset()
    assert est.solve_kernel_name() == SOLVE_KERNEL["go1"] + "_smooth" and est.innovation_gate()[0] == gate
    with pytest.raises(capi.DekfError):
        est.window()                                          # (no update since the reset)
    again = GS.run_gpu(p, s, B, 30, gate, est=est)[0]
    _equal(again, fresh[:29], OUTPUTS + ("gated",) + GS.WINDOW, "after the reset")


# ------------------------------------------------------------------ restart, pause and parameter table on one handle
def _assert_instance(got, b, ref, rb, Kb, keys, what):
    for key in keys:
        assert np.array_equal(got[key][b], ref[key][rb], equal_nan=True), (what, key)
    for key in GS.WINDOW:
        assert np.array_equal(got[key][b][:Kb], ref[key][rb][:Kb], equal_nan=True), (what, key)


def test_restart_pause_and_parameter_table_on_one_handle():
    """Go1, B = 4, 30 ticks, the low gate, a parameter table (the _ep twin with pc).  Instance 3 runs a second set with its own
    foot_swing_std: at its ungated ticks it gives the bits, window included, of a smoothing innovation handle created with that set on
    the edited log.  Instance 1 is restarted before step 12 and then gives the bits of a fresh handle with the option.  Instance 2 is
    paused for steps 8 to 11 and keeps every bit, its window included.  Instance 0 is untouched"""
    p = DL._params(go1_params)
    B, K, gate, N = 4, 30, GL.CASES["go1"][2], p.N
    s0 = DL.rough_streams(p, B, K)
    pairs = [q for q in GL.CASES["go1"][0] if q[0] < K]
    pairs += [(k, 3, int(np.nonzero(s0["contact"][k, 3])[0][0])) for k in (9, 16)]
    s = GL.inject_slips(p, s0, pairs, GL.SLIP_SIGMAS["go1"])
    other = p.copy()
    for i in range(3):
        other.foot_swing_std[i] = 0.5
    est = GS.make_est(p, B, gate)
    est.set_instance_params([p, other], [0, 0, 0, 1])
    assert est.solve_kernel_name() == "k_mhe_solve_direct_4_n20_smooth_pp"

    def before(k, e):
        if k == 8:
            e.set_active(np.array([1, 1, 0, 1], np.int32))
        if k == 12:
            e.reset_instances(np.array([0, 1, 0, 0], np.int32))
            e.set_active(np.ones(B, np.int32))

    got = [None] + GS.run_gpu(p, s, B, K, gate, est=est, before=before)[0]
    keys = OUTPUTS + ("gated",)
    whole = GS.run_gpu(p, s, B, K, gate)[0]                            # instance 0: never named
    assert any(r["gated"][0].any() for r in whole)
    for k in range(1, K):
        _assert_instance(got[k], 0, whole[k - 1], 0, min(k + 1, N), keys, (0, k))
    # instance 1: a fresh handle with the option from the restart on (its first solve is step 13)
    fresh = GS.run_gpu(p, EL.slice_streams(s, 12), B, K - 12, gate)[0]
    assert any(r["gated"][1].any() for r in fresh)
    for k in range(13, K):
        _assert_instance(got[k], 1, fresh[k - 13], 1, min(k - 12 + 1, N), keys, (1, k))
    # instance 2: frozen over steps 8 .. 11, then the log with those steps cut out
    life = tuple(k for k in range(K) if not 8 <= k < 12)
    cut = GS.run_gpu(p, PZ.cut_streams(s, life), B, len(life), gate)[0]
    assert any(r["gated"][2].any() for r in cut)
    for k in range(1, K):
        frozen = 8 <= k < 12
        _assert_instance(got[k], 2, got[7] if frozen else cut[life.index(k) - 1], 2, 8 if frozen else min(life.index(k) + 1, N), keys, (2, k))
    # instance 3: its ungated ticks are a smoothing innovation handle created with ITS set on the edited log
    dec = own_decisions(got[1:])
    assert [d for d in dec if d[1] == 3]
    ticks, so = GL.edited_copies(s, 3, B, dec)
    n = len(ticks) + 1
    mine, default = GS.run_gpu(other, so, n, K)[0], GS.run_gpu(p, so, n, K)[0]
    differs = False
    for i in range(n):
        lo, hi = (ticks[i - 1] + 1 if i else 1), (ticks[i] if i < len(ticks) else K)
        for k in range(lo, hi):
            _assert_instance(got[k], 3, mine[k - 1], i, min(k + 1, N), OUTPUTS, (3, k))
            differs = differs or (i > 0 and not np.array_equal(mine[k - 1]["xw"][i], default[k - 1]["xw"][i]))
    assert differs and ticks[0] + 1 < K   # (the default swing gain gives other bits: the record took the instance's own)


# ------------------------------------------------------------------ the state rules
def test_state_rules():
    lib = capi.load()
    p = DL._params(go1_params)
    B = 3
    sh = streams_host(DL.rough_streams(p, B, 3))
    bound = C.c_double(-1.0)
    INVALID, ORDER, OK = capi.DEKF_ERR_INVALID, capi.DEKF_ERR_ORDER, capi.DEKF_OK

    def state(est):
        """(smoothing handle, the bound)"""
        capi.check(lib.dekf_get_innovation_gate(est.h, C.byref(bound), None, capi.DEKF_HOST))
        return est.solve_kernel_name().endswith("_smooth"), bound.value

    # on = 1 needs a gating handle: not an ADMM, KF or foot-state handle, a direct handle, an innovation handle without a bound
    for est in (BatchedEstimator(p, B), BatchedEstimator(DL._params(go1_params, est_type=1), B),
                BatchedEstimator(DL._params(go1_params, leg_odom_type=1), B, solver="direct"),
                BatchedEstimator(p, B, solver="direct"), BatchedEstimator(p, B, solver="direct", innovation=True)):
        assert lib.dekf_set_gate_smoother(est.h, 1) == INVALID
        assert lib.dekf_set_gate_smoother(est.h, 0) == OK
        est.close()
    # ... with the smoother off; off on a plain smoothing handle leaves it a smoothing handle
    est = BatchedEstimator(p, B, solver="direct", smoother=True, innovation=True)
    assert lib.dekf_set_gate_smoother(est.h, 1) == INVALID
    assert lib.dekf_set_gate_smoother(est.h, 0) == OK and state(est) == (True, 0.0)
    est.close()
    with pytest.raises(capi.DekfError):
        BatchedEstimator(p, B, solver="direct", smoother=True, innovation=True, innovation_gate=100.0, gate_smoother=True)
    est = BatchedEstimator(p, B, solver="direct", innovation=True, innovation_gate=100.0)
    for bad in (-1, 2):
        assert lib.dekf_set_gate_smoother(est.h, bad) == INVALID
    assert state(est) == (False, 100.0)
    with pytest.raises(capi.DekfError):
        est.window()
    assert lib.dekf_set_gate_smoother(est.h, 1) == OK and lib.dekf_set_gate_smoother(est.h, 1) == OK      # idempotent
    assert state(est) == (True, 100.0)
    # while the option is on
    assert lib.dekf_set_smoother(est.h, 1) == INVALID and state(est) == (True, 100.0)
    assert lib.dekf_set_window_cross(est.h, 1) == INVALID
    assert lib.dekf_set_innovation_gate(est.h, 120.0) == OK and state(est) == (True, 120.0)               # the bound changes
    assert lib.dekf_set_gate_smoother(est.h, 0) == OK and state(est) == (False, 120.0)                    # off: the gate stays
    assert lib.dekf_set_gate_smoother(est.h, 1) == OK
    assert lib.dekf_set_smoother(est.h, 0) == OK and state(est) == (False, 120.0)                         # both off, the gate stays
    assert lib.dekf_set_smoother(est.h, 1) == INVALID                                                     # (a gating handle again)
    assert lib.dekf_set_gate_smoother(est.h, 1) == OK
    assert lib.dekf_set_innovation_gate(est.h, 0.0) == OK and state(est) == (False, 0.0)                  # gate, option, smoother off
    assert lib.dekf_set_smoother(est.h, 1) == OK and lib.dekf_set_window_cross(est.h, 1) == OK            # (a plain smoothing handle)
    assert lib.dekf_set_window_cross(est.h, 0) == OK and lib.dekf_set_smoother(est.h, 0) == OK
    assert lib.dekf_set_innovation_gate(est.h, 100.0) == OK and lib.dekf_set_gate_smoother(est.h, 1) == OK
    capi.check(lib.dekf_set_innovation(est.h, 0))                                                         # everything off
    assert state(est) == (False, 0.0)
    capi.check(lib.dekf_set_innovation(est.h, 1))
    assert state(est) == (False, 0.0) and lib.dekf_set_gate_smoother(est.h, 1) == INVALID
    assert lib.dekf_set_innovation_gate(est.h, 100.0) == OK and lib.dekf_set_gate_smoother(est.h, 1) == OK
    capi.check(lib.dekf_set_solver(est.h, capi.DEKF_SOLVER_ADMM))                                         # everything off
    capi.check(lib.dekf_set_solver(est.h, capi.DEKF_SOLVER_DIRECT))
    assert state(est) == (False, 0.0)
    capi.check(lib.dekf_set_innovation(est.h, 1))
    assert lib.dekf_set_innovation_gate(est.h, 100.0) == OK and lib.dekf_set_gate_smoother(est.h, 1) == OK
    # a running handle
    est.push_stream_step(sh, 0)
    est.step(0)
    assert lib.dekf_set_gate_smoother(est.h, 0) == ORDER and lib.dekf_set_gate_smoother(est.h, 1) == ORDER
    est.push_stream_step(sh, 1)
    est.step(1)
    assert est.window()[0] == 2 and state(est) == (True, 100.0)
    est.reset()
    assert state(est) == (True, 100.0)                                                                    # the setting survives
    assert lib.dekf_set_gate_smoother(est.h, 0) == OK and state(est) == (False, 100.0)                    # right after dekf_reset
    for k in range(2):
        est.push_stream_step(sh, k)
        est.step(k)
    assert np.isfinite(est.innovation()["nis"]).all()
    est.close()


# ------------------------------------------------------------------ snapshots
def test_snapshot_round_trip_and_a_refused_load():
    """instance 1 of the Go1 case, saved before tick 22 on a handle with the option, goes on in slot 0 of another such handle (of two
    robots, before its tick 3) with the bits of its source, window included, through gated ticks; a plain gating handle refuses the blob"""
    p, B, K, sub, s = GL.case_streams("go1", gpu=True)
    gate, N, T0, D0, after = GL.CASES["go1"][2], p.N, 22, 3, 20
    ref = case_run("go1", "low")[0]
    assert any(ref[k - 1]["gated"][1].any() for k in range(T0, T0 + after))
    blobs = []
    GS.run_gpu(p, s, B, T0 + 1, gate, before=lambda k, e: blobs.append(e.save_instances([1])) if k == T0 else None)
    s_own = DL.rough_streams(p, 2, D0 + after, seed_shift=11)
    sm = SL.migrated_streams(s_own, D0, s, T0, [(1, 0)], after)
    dst = GS.make_est(p, 2, gate)
    got = [None] + GS.run_gpu(p, sm, 2, D0 + after, gate, est=dst,
                              before=lambda k, e: e.load_instances([0], blobs[0]) if k == D0 else None)[0]
    for i in range(after):
        _assert_instance(got[D0 + i], 0, ref[T0 + i - 1], 1, N, OUTPUTS + ("gated",), ("moved", i))
    plain = BatchedEstimator(p, 2, solver="direct", innovation=True, innovation_gate=gate)
    smooth = BatchedEstimator(p, 2, solver="direct", smoother=True, innovation=True)
    for est in (plain, smooth):
        with pytest.raises(capi.DekfError):
            est.load_instances([0], blobs[0])
        est.close()
