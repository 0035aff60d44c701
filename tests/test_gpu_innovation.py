"""The innovation statistics of a direct handle on the GPU (dekf_set_innovation / dekf_get_innovation, BatchedEstimator(innovation=True)
and .innovation()): every tick of the smallest shapes that reach the four kernels against the oracle's window QP with the newest Meas
rows made free, with the limits of innov_lib; everything else the handle returns to the bit against the same handle without the
option; the five arrays to the bit across the smoother and cross options, the batch, a reset and the two kinds of pointer; restart,
pause and parameter table on one handle; the status codes."""
import ctypes as C

import numpy as np
import pytest

import direct_lib as DL
import epoch_lib as EL
import innov_lib as IL
import instance_params_lib as PL
import pause_lib as PZ
from decentralized_ekf_mhe_amd import capi, go1_params
from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host

pytestmark = pytest.mark.gpu


def _equal(a, b, keys, what):
    assert len(a) == len(b), what
    for i, (ra, rb) in enumerate(zip(a, b)):
        for key in keys:
            assert np.array_equal(ra[key], rb[key], equal_nan=True), (what, i + 1, key)


# ------------------------------------------------------------------ accuracy
MUST_HOLD = {"go1": ("flight", "mixed", "vo"), "cassie": ("flight", "mixed", "vo"), "tripod": ("flight", "mixed"), "pogox": ("flight",)}


@pytest.mark.parametrize("name", list(IL.GPU_CASES))
def test_every_tick_against_the_oracle(name):
    """Go1 B = 6, 48 ticks (k_mhe_innov_4: window fill, full windows, a flight phase, VO equality rows), Cassie B = 2, 48 ticks, the
    tripod B = 2, 24 ticks, PogoX B = 2, 12 ticks: every tick of the oracle instances within the limits the lane-sequential build set"""
    mk, B, K, sub, _ = IL.GPU_CASES[name]
    p, s, refs = IL.case_reference(name, gpu=True)
    got, _ = IL.gpu_case_run(name)
    worst, seen = {}, set()
    for b in sub:
        for k in range(1, K):
            g, r = IL.instance(got[k - 1], b), refs[b][k]
            assert got[k - 1]["status"][b] == capi.DEKF_SOLVE_OK
            e = IL.errors(g, r)
            worst = {key: max(v, worst.get(key, 0.0)) for key, v in e.items()}
            seen.add(IL.contact_kind(s, k, b))
            if r["vo"] > 0:
                seen.add("vo")
    print(name, {key: f"{v:.2e}" for key, v in worst.items()}, sorted(seen))
    IL.assert_within_limits(worst, name)
    for b in range(B):
        for k in range(1, K):
            IL.check_identities(IL.instance(got[k - 1], b), p.num_legs, (name, b, k))
    assert set(MUST_HOLD[name]) <= seen, (MUST_HOLD[name], seen)


# ------------------------------------------------------------------ bit identities, Go1 B = 6
OUTPUTS = ("x", "v_b", "status", "iters", "cov")


@pytest.mark.parametrize("variant", ["plain", "cross"])
def test_every_other_output_keeps_its_bits(variant):
    """x, v_b, status, iters and Cov(x_T), and with smoother and cross on the window and cross arrays, of a handle with the option
    against the same handle without it; and the solve kernel is the same one"""
    on, names_on = IL.gpu_case_run("go1", variant, True)
    off, names_off = IL.gpu_case_run("go1", variant, False)
    assert names_on == names_off == ("k_mhe_solve_direct_4_n20" + EL.SIBLING_SUFFIX[variant],) * 2
    _equal(on, off, OUTPUTS + (("K", "xw", "cw", "l1", "zn") if variant == "cross" else ()), variant)


def test_the_five_arrays_do_not_depend_on_smoother_or_cross():
    plain, _ = IL.gpu_case_run("go1", "plain")
    assert all(np.isfinite(r[key]).all() for r in plain for key in IL.KEYS)
    for variant in ("smooth", "cross"):
        _equal(IL.gpu_case_run("go1", variant)[0], plain, IL.KEYS, variant)


def test_the_five_arrays_do_not_depend_on_the_batch():
    """B = 6 against the first six of B = 70"""
    mk, B, K, _, _ = IL.GPU_CASES["go1"]
    p, s = IL.big_streams()
    big = IL.run_gpu(p, s, IL.BIG, K)[0]
    small, _ = IL.gpu_case_run("go1", "plain")
    for i, (ra, rb) in enumerate(zip(big, small)):
        for key in IL.KEYS + OUTPUTS:
            assert np.array_equal(ra[key][:B], rb[key]), (i + 1, key)


def test_reset_and_rerun_is_a_fresh_handle():
    """the setting survives dekf_reset; the getter answers DEKF_ERR_ORDER from the reset to the next update"""
    mk, B, K, _, _ = IL.GPU_CASES["go1"]
    p, s = IL.gpu_streams("go1")
    first, _, est = IL.run_gpu(p, s, B, 30, close=False)
    est.reset()
    lib = capi.load()
    nis = np.zeros(B)
    assert lib.dekf_get_innovation(est.h, None, None, C.c_void_p(nis.ctypes.data), None, None, capi.DEKF_HOST) == capi.DEKF_ERR_ORDER
    again = IL.run_gpu(p, s, B, 30, est=est)[0]
    fresh, _ = IL.gpu_case_run("go1", "plain")
    _equal(first, fresh[:29], IL.KEYS + OUTPUTS, "first run")
    _equal(again, fresh[:29], IL.KEYS + OUTPUTS, "after the reset")


def test_host_and_device_pointers_null_pointers_and_one_timed_launch():
    import torch
    lib = capi.load()
    p, s = IL.gpu_streams("go1")
    B, L = 6, p.num_legs
    nm = 3 * L
    est = BatchedEstimator(p, B, solver="direct", innovation=True)
    est.timing_enable(2)
    sh = streams_host(s)
    shapes = dict(innov=(B, nm), innov_cov=(B, nm, nm), nis=(B,), nis_leg=(B, L), loglik=(B,))
    for k in range(24):
        est.push_stream_step(sh, k)
        est.step(k)
        if k not in (1, 7, 23):
            continue
        host = est.innovation()
        dev = {key: torch.full(shapes[key], DL.FILL, dtype=torch.float64, device="cuda") for key in IL.KEYS}
        torch.cuda.synchronize()
        capi.check(lib.dekf_get_innovation(est.h, *[C.c_void_p(dev[key].data_ptr()) for key in IL.KEYS], capi.DEKF_DEVICE))
        est.sync()
        for i, key in enumerate(IL.KEYS):
            assert np.array_equal(dev[key].cpu().numpy(), host[key]), (k, key)
            one = np.full(shapes[key], DL.FILL)       # any pointer may be NULL: this array alone
            args = [None] * 5
            args[i] = C.c_void_p(one.ctypes.data)
            capi.check(lib.dekf_get_innovation(est.h, *args, capi.DEKF_HOST))
            assert np.array_equal(one, host[key]), (k, key)
        capi.check(lib.dekf_get_innovation(est.h, None, None, None, None, None, capi.DEKF_HOST))
    # timing class 2 brackets the solve and the innovation kernel as one launch: one pair per update
    assert est.timing_read()["solve"][1] == 23
    est.close()


# ------------------------------------------------------------------ restart, pause and parameter table on one handle
def test_restart_pause_and_parameter_table_on_one_handle():
    """Go1, B = 4, 30 ticks.  Instance 1 is restarted before step 5: NaN at step 5, then the bits of a fresh handle fed the samples from
    step 5.  Instance 2 is paused for steps 8 to 11: frozen, then the bits of a handle that never saw those steps.  Instance 3 is on a
    second noise set: the bits of a handle created with it.  Instance 0 is untouched."""
    p = DL._params(go1_params)
    B, K = 4, 30
    s = DL.rough_streams(p, B, K)
    sets = PL.param_sets(p)
    est = BatchedEstimator(p, B, solver="direct", innovation=True)
    kernel = "k_mhe_solve_direct_4_n20"
    assert est.solve_kernel_name() == kernel
    est.set_instance_params(sets, [0, 0, 0, 1])
    assert est.solve_kernel_name() == kernel + "_pp"
    sh = streams_host(s)
    got = [None]
    for k in range(K):
        if k == 5:
            est.reset_instances(np.array([0, 1, 0, 0], np.int32))
        if k == 8:
            est.set_active(np.array([1, 1, 0, 1], np.int32))
        if k == 12:
            est.set_active(np.ones(B, np.int32))
        est.push_stream_step(sh, k)
        est.step(k)
        if k:
            got.append(dict(IL.gpu_record(est), **est.innovation()))
    assert est.solve_kernel_name(True) == est.solve_kernel_name(False) == kernel + "_pp"
    est.close()
    keys = IL.KEYS + ("x", "status", "cov")
    whole = IL.run_gpu(p, s, B, K)[0]                                   # instance 0: never named
    for k in range(1, K):
        for key in keys:
            assert np.array_equal(got[k][key][0], whole[k - 1][key][0]), (k, key)
    # instance 1: NaN from the restart until its first solve, then a fresh handle's bits
    assert all(np.isnan(got[5][key][1]).all() for key in IL.KEYS)
    assert all(np.isfinite(got[k][key][1]).all() for k in (4, 6) for key in IL.KEYS)
    fresh = IL.run_gpu(p, EL.slice_streams(s, 5), B, K - 5)[0]
    for k in range(6, K):
        for key in keys:
            assert np.array_equal(got[k][key][1], fresh[k - 6][key][1]), (k, key)
    # instance 2: frozen over steps 8 .. 11, then the log with those steps cut out
    life = tuple(k for k in range(K) if not 8 <= k < 12)
    cut = IL.run_gpu(p, PZ.cut_streams(s, life), B, len(life))[0]
    for k in range(1, K):
        ref = got[7] if 8 <= k < 12 else cut[life.index(k) - 1]
        for key in keys:
            assert np.array_equal(got[k][key][2], ref[key][2]), (k, key)
    # instance 3: a handle created with its set
    other = IL.run_gpu(PL.param_set(p, 1), s, B, K)[0]
    differs = False
    for k in range(1, K):
        for key in keys:
            assert np.array_equal(got[k][key][3], other[k - 1][key][3]), (k, key)
        differs = differs or not np.array_equal(got[k]["loglik"][3], whole[k - 1]["loglik"][3])
    assert differs   # (the second set scores differently on the same log: what the number is for)


# ------------------------------------------------------------------ the status codes
def test_status_codes():
    lib = capi.load()
    p = DL._params(go1_params)
    B = 3
    sh = streams_host(DL.rough_streams(p, B, 3))
    nis = np.zeros(B)

    def get(est):
        return lib.dekf_get_innovation(est.h, None, None, C.c_void_p(nis.ctypes.data), None, None, capi.DEKF_HOST)

    # ADMM, KF and foot-state handles are outside the interface
    for est in (BatchedEstimator(p, B), BatchedEstimator(DL._params(go1_params, est_type=1), B),
                BatchedEstimator(DL._params(go1_params, leg_odom_type=1), B, solver="direct")):
        assert lib.dekf_set_innovation(est.h, 1) == capi.DEKF_ERR_INVALID
        assert lib.dekf_set_innovation(est.h, 0) == capi.DEKF_OK
        assert get(est) == capi.DEKF_ERR_INVALID
        est.close()
    with pytest.raises(capi.DekfError):
        BatchedEstimator(p, B, innovation=True)
    est = BatchedEstimator(p, B, solver="direct")
    kernel = est.solve_kernel_name()
    for on in (2, -1):
        assert lib.dekf_set_innovation(est.h, on) == capi.DEKF_ERR_INVALID
    assert get(est) == capi.DEKF_ERR_INVALID                               # a handle without the option
    assert lib.dekf_set_innovation(est.h, 1) == capi.DEKF_OK
    assert est.solve_kernel_name() == kernel == "k_mhe_solve_direct_4_n20"  # the solve kernel is the same one
    assert get(est) == capi.DEKF_ERR_ORDER                                 # before the first update
    est.push_stream_step(sh, 0)
    est.step(0)
    assert get(est) == capi.DEKF_ERR_ORDER
    assert lib.dekf_set_innovation(est.h, 0) == capi.DEKF_ERR_ORDER        # not on a running handle
    est.push_stream_step(sh, 1)
    est.step(1)
    assert get(est) == capi.DEKF_OK and np.isfinite(nis).all()
    est.reset()
    assert get(est) == capi.DEKF_ERR_ORDER                                 # the setting survives, the results do not
    # dekf_set_solver(ADMM) switches the option off; going back to direct does not switch it on again
    capi.check(lib.dekf_set_solver(est.h, capi.DEKF_SOLVER_ADMM))
    assert get(est) == capi.DEKF_ERR_INVALID
    capi.check(lib.dekf_set_solver(est.h, capi.DEKF_SOLVER_DIRECT))
    assert get(est) == capi.DEKF_ERR_INVALID
    # any combination with the smoother and the cross-covariances
    capi.check(lib.dekf_set_innovation(est.h, 1))
    capi.check(lib.dekf_set_smoother(est.h, 1))
    capi.check(lib.dekf_set_window_cross(est.h, 1))
    capi.check(lib.dekf_set_smoother(est.h, 0))
    for k in range(2):
        est.push_stream_step(sh, k)
        est.step(k)
    assert get(est) == capi.DEKF_OK and np.isfinite(nis).all()
    est.close()
