"""Restarting single instances of a direct handle on the GPU (dekf_reset_instances / dekf_get_instance_ticks,
BatchedEstimator.reset_instances / instance_ticks): every life of a restarted instance against a fresh handle on the log sliced from
its restart tick, every untouched instance against the run without restarts, on every getter the contract names, to the bit; the local
ticks and the window getters' steps; the kernels the handle launches; an instance poisoned by a NaN sample brought back by a restart;
the error codes, host and device masks, the all-zero mask, dekf_reset."""
import ctypes as C

import numpy as np
import pytest

import direct_lib as DL
import epoch_lib as EL
from decentralized_ekf_mhe_amd import capi, go1_params
from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host

pytestmark = pytest.mark.gpu


def check_schedule(name, variant):
    """the shape's GPU schedule: lives, untouched instances, local ticks, steps and kernel names"""
    mk, B, K, kernel = EL.GPU_SHAPES[name]
    p, s = EL.gpu_streams(name)
    resets = EL.GPU_RESETS[name]
    got, names, _ = EL.run_gpu(p, s, B, K, variant, resets)
    sibling, twin = kernel + EL.SIBLING_SUFFIX[variant], kernel + EL.TWIN_SUFFIX[variant]
    assert names[0] == (sibling, sibling) and all(n == (twin, twin) for n in names[1:]) and len(names) == 1 + len(resets)
    plain = EL.gpu_fresh(name, variant, 0)
    for b in range(B):
        first = min([T0 for T0 in resets if b in resets[T0]] + [K])
        EL.assert_gpu_life_equal(got, plain, b, 0, first, p.N, "untouched")
    assert len(EL.untouched(resets, B)) >= 2
    for b, T0, end in EL.lives(resets, K):
        EL.assert_gpu_life_equal(got, EL.gpu_fresh(name, variant, T0), b, T0, end, p.N, "life")
        assert got[T0]["status"][b] == capi.DEKF_SOLVE_NONE and np.isnan(got[T0]["cov"][b]).all()
        assert got[end - 1]["status"][b] == capi.DEKF_SOLVE_OK
    # *steps is the largest window of the batch: the untouched instances' here
    assert all(r["K"] == min(k + 1, p.N) for k, r in enumerate(got) if "K" in r)
    return got


# ------------------------------------------------------------------ Go1, the three variants
@pytest.mark.parametrize("variant", list(DL.VARIANTS))
def test_go1_lives_and_untouched_instances(variant):
    """B = 6, 100 ticks: an odd instance restarted before tick 5 and again before tick 12 (inside its own fill), an even one before tick
    30, and that one together with another before tick 45 (full windows with VO equality rows)"""
    got = check_schedule("go1", variant)
    assert got[11]["ticks"].tolist() == [11, 11, 11, 6, 11, 11] and got[99]["ticks"].tolist() == [99, 99, 54, 87, 54, 99]


# ------------------------------------------------------------------ other shapes
@pytest.mark.parametrize("variant", ["plain", "cross"])
@pytest.mark.parametrize("name", ["tripod", "go1_foot"])
def test_other_shapes_one_restart_in_the_fill_and_one_in_full_windows(name, variant):
    """the generic run-time-K kernel (tripod, N = 12, B = 6) and ns = 21 (Go1 with foot states, B = 4)"""
    check_schedule(name, variant)


# ------------------------------------------------------------------ the motivating case
def test_poisoned_instance_restarted_while_its_neighbours_keep_their_bits():
    """direct_lib.poisoned_runs' poison (a NaN accelerometer sample on instance 2 at tick 26) reaches the instance's arrival cost: it
    stays DEKF_SOLVE_NUMERIC.  Restarted alone before tick 40 it is DEKF_SOLVE_OK from tick 41 on with the bits of a fresh handle from
    tick 40; every neighbour keeps the bits of the clean run throughout"""
    p = DL._params(go1_params)
    B, K, bad, t_bad, T0, variant = 6, 60, 2, 26, 40, "cross"
    s = DL.rough_streams(p, B, K)
    sp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    sp["accel"][t_bad, bad, 0] = np.nan
    clean = EL.run_gpu(p, s, B, K, variant)[0]
    got = EL.run_gpu(p, sp, B, K, variant, {T0: [bad]})[0]
    fresh = EL.run_gpu(p, EL.slice_streams(sp, T0), B, K - T0, variant)[0]
    assert all(got[k]["status"][bad] == capi.DEKF_SOLVE_NUMERIC for k in range(t_bad, T0))
    assert got[T0]["status"][bad] == capi.DEKF_SOLVE_NONE
    assert all(got[k]["status"][bad] == capi.DEKF_SOLVE_OK for k in range(T0 + 1, K))
    EL.assert_gpu_life_equal(got, fresh, bad, T0, K, p.N, "restarted")
    for b in range(B):
        if b != bad:
            EL.assert_gpu_life_equal(got, clean, b, 0, K, p.N, "neighbour")
            assert all(got[k]["status"][b] == capi.DEKF_SOLVE_OK for k in range(1, K))


# ------------------------------------------------------------------ the API
def test_error_codes():
    lib = capi.load()
    p = DL._params(go1_params)
    B = 4
    m = np.array([0, 1, 0, 0], np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    sh = streams_host(DL.rough_streams(p, B, 3))

    def started(est):
        for k in range(2):
            est.push_stream_step(sh, k)
            est.step(k)
        return est

    # an ADMM handle, a KF handle, a pipelined handle
    for est in (BatchedEstimator(p, B), BatchedEstimator(DL._params(go1_params, est_type=1), B),
                BatchedEstimator(DL._params(go1_params, solve_pipeline=1), B)):
        started(est)
        assert lib.dekf_reset_instances(est.h, ptr(m), capi.DEKF_HOST) == capi.DEKF_ERR_INVALID
        t = np.full(B, -7, np.int32)
        assert lib.dekf_get_instance_ticks(est.h, ptr(t), capi.DEKF_HOST) == capi.DEKF_OK and t.tolist() == [1] * B
        est.close()
    est = BatchedEstimator(p, B, solver="direct")
    t = np.full(B, -7, np.int32)
    assert lib.dekf_reset_instances(est.h, ptr(m), capi.DEKF_HOST) == capi.DEKF_ERR_ORDER          # before dekf_initialize
    assert lib.dekf_get_instance_ticks(est.h, ptr(t), capi.DEKF_HOST) == capi.DEKF_ERR_ORDER and t.tolist() == [-7] * B
    started(est)
    assert lib.dekf_reset_instances(est.h, None, capi.DEKF_HOST) == capi.DEKF_ERR_INVALID          # null mask
    assert lib.dekf_get_instance_ticks(est.h, None, capi.DEKF_HOST) == capi.DEKF_ERR_INVALID
    for v in (2, -1):                                                                              # a mask entry other than 0 or 1
        assert lib.dekf_reset_instances(est.h, ptr(np.array([0, 1, v, 0], np.int32)), capi.DEKF_HOST) == capi.DEKF_ERR_INVALID
    # none of the refused calls did anything: no instance restarted, the kernel is the sibling
    assert est.instance_ticks().tolist() == [1] * B and est.solve_kernel_name() == "k_mhe_solve_direct_4_n20"
    est.reset_instances(m)
    assert est.instance_ticks().tolist() == [1, -1, 1, 1] and est.solve_kernel_name() == "k_mhe_solve_direct_4_n20_ep"
    est.close()


def test_host_and_device_masks_give_the_same_bits():
    mk, B, K, _ = EL.GPU_SHAPES["go1"]
    p, s = EL.gpu_streams("go1")
    host = EL.run_gpu(p, s, B, 50, "cross", EL.GPU_RESETS["go1"])[0]
    dev = EL.run_gpu(p, s, B, 50, "cross", EL.GPU_RESETS["go1"], device_mask=True)[0]
    for k in range(50):
        assert sorted(host[k]) == sorted(dev[k])
        for key in host[k]:
            if key not in EL.WINDOW_KEYS:
                assert np.array_equal(host[k][key], dev[k][key], equal_nan=True), (k, key)
                continue
            for b in range(B):     # (an instance's entries beyond its own window are not specified)
                n = EL.window_lengths(key, EL.local_K(int(host[k]["ticks"][b]), p.N))
                assert np.array_equal(host[k][key][b, :n], dev[k][key][b, :n]), (k, key, b)


def test_all_zero_mask_changes_nothing():
    """bits and dekf_solve_kernel_name: an all-zero mask before the first real call (host and device), and one after it"""
    import torch
    mk, B, K, kernel = EL.GPU_SHAPES["go1"]
    p, s = EL.gpu_streams("go1")
    seen = []

    def poke(est, k):
        if k in (3, 25, 50):
            before = est.solve_kernel_name()
            est.reset_instances(np.zeros(B, np.int32))
            z = torch.zeros(B, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            est.reset_instances(z)
            assert est.solve_kernel_name() == before
            seen.append(before)

    got = EL.run_gpu(p, s, B, 60, "smooth", poke=poke)[0]
    assert seen == [kernel + "_smooth"] * 3
    plain = EL.gpu_fresh("go1", "smooth", 0)
    for b in range(B):
        EL.assert_gpu_life_equal(got, plain, b, 0, 60, p.N, "all-zero mask")
    seen.clear()
    got = EL.run_gpu(p, s, B, 60, "smooth", {30: [4]}, poke=poke)[0]
    assert seen == [kernel + "_smooth"] * 2 + [kernel + "_smooth_ep"]
    EL.assert_gpu_life_equal(got, EL.gpu_fresh("go1", "smooth", 30), 4, 30, 60, p.N, "life")
    for b in (0, 1, 2, 3, 5):
        EL.assert_gpu_life_equal(got, plain, b, 0, 60, p.N, "untouched")


def test_reset_and_rerun_is_a_fresh_handle():
    """dekf_reset clears every epoch: the handle launches the siblings again and gives the bits of the run without restarts"""
    mk, B, K, kernel = EL.GPU_SHAPES["go1"]
    p, s = EL.gpu_streams("go1")
    _, names, est = EL.run_gpu(p, s, B, 50, "cross", EL.GPU_RESETS["go1"], close=False)
    assert names[-1][0] == kernel + "_smooth_cross_ep"
    est.reset()
    again, names, _ = EL.run_gpu(p, s, B, 50, "cross", est=est)
    assert names == [(kernel + "_smooth_cross",) * 2]
    plain = EL.gpu_fresh("go1", "cross", 0)
    for b in range(B):
        EL.assert_gpu_life_equal(again, plain, b, 0, 50, p.N, "reset and re-run")
