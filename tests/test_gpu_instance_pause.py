"""Pausing single instances of a direct handle on the GPU (dekf_set_active / dekf_get_active, BatchedEstimator.set_active / active):
every life of every instance against a fresh handle that never hears of the interface, on the log cut down to the ticks at which the
instance ran; every paused tick against the last tick that ran; instances that are never named against the run without pauses; on
every getter the contract names and on dekf_get_instance_ticks, to the bit.  The kernels the handle launches, host and device masks,
the error codes, dekf_get_active, dekf_reset, a handle with a parameter table, VO samples pushed for a paused instance."""
import ctypes as C

import numpy as np
import pytest

import direct_lib as DL
import epoch_lib as EL
import instance_params_lib as PL
import pause_lib as PZ
from decentralized_ekf_mhe_amd import capi, go1_params
from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host

pytestmark = pytest.mark.gpu


def check_schedule(name, variant, stray=False):
    """the shape's schedule (pause_lib.gpu_schedule): lives, frozen ticks, instances never named, local ticks, steps, kernel names"""
    mk, B, K, kernel = PZ.GPU_SHAPES[name]
    p, s = EL.gpu_streams(name)
    schedule = PZ.gpu_schedule(B, K)
    got, names, _ = PZ.run_gpu(p, s, B, K, variant, schedule, stray=stray)
    sibling, twin = kernel + EL.SIBLING_SUFFIX[variant], kernel + EL.TWIN_SUFFIX[variant]
    assert names[0] == (sibling, sibling) and all(n == (twin, twin) for n in names[1:]) and len(names) == 1 + len(schedule)
    lives = PZ.check_against_cut_logs(got, lambda life: PZ.gpu_fresh(name, variant, life), schedule, B, K, p.N, PZ.GPU_KEYS, (name, variant))
    named = {b for ev in schedule.values() for b in list(ev.get("reset", ())) + [i for i, a in enumerate(ev.get("active", ())) if not a]}
    assert len(named) < B and all((b, tuple(range(K))) in lives for b in range(B) if b not in named)
    # *steps is the largest window of the batch, paused instances counted with the one they stand at
    assert all(r["K"] == r["Kmax"] for r in got if "K" in r)
    for k, r in enumerate(got):
        want = np.ones(B, np.int32)
        for t in sorted(schedule):
            if t <= k and "reset" in schedule[t]:
                want[list(schedule[t]["reset"])] = 1
            if t <= k and "active" in schedule[t]:
                want = np.array(schedule[t]["active"], np.int32)
        assert r["active"].tolist() == want.tolist(), (k, r["active"], want)
    return got


# ------------------------------------------------------------------ Go1, the three variants
@pytest.mark.parametrize("variant", list(DL.VARIANTS))
def test_go1_lives_frozen_ticks_and_untouched_instances(variant):
    """B = 6, 100 ticks, pause_lib.cpu_schedule (pauses inside the fill, from the fill into full windows, in full windows with VO rows; a
    paused instance restarted; a restart and a pause in one gap; an instance never resumed) and two instances paused together"""
    got = check_schedule("go1", variant)
    assert got[26]["ticks"].tolist() == [26, 9, 26, 26, 26, 26] and got[40]["ticks"].tolist() == [40, 23, 40, 33, 29, 40]
    assert got[99]["ticks"].tolist() == [81, 15, 99, 92, 88, 99] and got[99]["active"].tolist() == [0, 1, 1, 1, 1, 1]
    assert [got[k]["ticks"][1] for k in (65, 66, 80, 83, 84)] == [42, 0, -1, -1, 0]


# ------------------------------------------------------------------ other shapes
@pytest.mark.parametrize("variant", ["plain", "cross"])
@pytest.mark.parametrize("name", ["tripod", "go1_foot"])
def test_other_shapes(name, variant):
    """the generic run-time-K kernel (tripod, N = 12, B = 6) and ns = 21 (Go1 with foot states, B = 4), 60 ticks"""
    check_schedule(name, variant)


def test_vo_pushed_for_a_paused_instance_is_dropped():
    """a made-up VO sample (interval and orientation pose) pushed for the paused instances at every tick of every pause: the references,
    which never see it, still give every bit"""
    check_schedule("go1_foot", "smooth", stray=True)


# ------------------------------------------------------------------ the API
def test_error_codes_and_get_active():
    lib = capi.load()
    p = DL._params(go1_params)
    B = 4
    m = np.array([1, 0, 1, 1], np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    sh = streams_host(DL.rough_streams(p, B, 3))

    def started(est):
        for k in range(2):
            est.push_stream_step(sh, k)
            est.step(k)
        return est

    # an ADMM handle, a KF handle, a pipelined handle: no pausing, and dekf_get_active answers all ones
    for est in (BatchedEstimator(p, B), BatchedEstimator(DL._params(go1_params, est_type=1), B),
                BatchedEstimator(DL._params(go1_params, solve_pipeline=1), B)):
        started(est)
        assert lib.dekf_set_active(est.h, ptr(m), capi.DEKF_HOST) == capi.DEKF_ERR_INVALID
        a = np.full(B, -7, np.int32)
        assert lib.dekf_get_active(est.h, ptr(a), capi.DEKF_HOST) == capi.DEKF_OK and a.tolist() == [1] * B
        est.close()
    est = BatchedEstimator(p, B, solver="direct")
    a = np.full(B, -7, np.int32)
    assert lib.dekf_set_active(est.h, ptr(m), capi.DEKF_HOST) == capi.DEKF_ERR_ORDER          # before dekf_initialize
    assert lib.dekf_get_active(est.h, ptr(a), capi.DEKF_HOST) == capi.DEKF_ERR_ORDER and a.tolist() == [-7] * B
    started(est)
    assert lib.dekf_set_active(est.h, None, capi.DEKF_HOST) == capi.DEKF_ERR_INVALID          # null array
    assert lib.dekf_get_active(est.h, None, capi.DEKF_HOST) == capi.DEKF_ERR_INVALID
    for v in (2, -1):                                                                         # an entry other than 0 or 1
        assert lib.dekf_set_active(est.h, ptr(np.array([1, 0, v, 1], np.int32)), capi.DEKF_HOST) == capi.DEKF_ERR_INVALID
    # none of the refused calls did anything; a mask of ones on a handle that never paused leaves the kernel names as they are
    kernel = "k_mhe_solve_direct_4_n20"
    assert est.active().tolist() == [1] * B and est.solve_kernel_name() == kernel
    est.set_active(np.ones(B, np.int32))
    assert (est.solve_kernel_name(True), est.solve_kernel_name(False)) == (kernel, kernel)
    est.set_active(m)
    assert est.active().tolist() == m.tolist() and est.instance_ticks().tolist() == [1] * B
    assert (est.solve_kernel_name(True), est.solve_kernel_name(False)) == (kernel + "_ep", kernel + "_ep")
    # the device forms of both calls
    import torch
    d = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    capi.check(lib.dekf_get_active(est.h, C.c_void_p(d.data_ptr()), capi.DEKF_DEVICE))
    assert d.cpu().tolist() == m.tolist()
    est.push_stream_step(sh, 2)
    est.step(2)
    assert est.instance_ticks().tolist() == [2, 1, 2, 2]
    # dekf_reset_instances on a paused instance makes it active
    est.reset_instances(np.array([0, 1, 0, 0], np.int32))
    assert est.active().tolist() == [1] * B and est.instance_ticks().tolist() == [2, -1, 2, 2]
    est.close()


def test_host_and_device_masks_give_the_same_bits():
    mk, B, K, _ = PZ.GPU_SHAPES["go1"]
    p, s = EL.gpu_streams("go1")
    schedule = PZ.gpu_schedule(B, K)
    host = PZ.run_gpu(p, s, B, 70, "cross", schedule)[0]
    dev = PZ.run_gpu(p, s, B, 70, "cross", schedule, device_mask=True)[0]
    for k in range(70):
        assert sorted(host[k]) == sorted(dev[k])
        for key in host[k]:
            if key not in EL.WINDOW_KEYS:
                assert np.array_equal(host[k][key], dev[k][key], equal_nan=True), (k, key)
                continue
            for b in range(B):     # (an instance's entries beyond its own window are not specified)
                n = EL.window_lengths(key, EL.local_K(int(host[k]["ticks"][b]), p.N))
                assert np.array_equal(host[k][key][b, :n], dev[k][key][b, :n]), (k, key, b)


def test_reset_and_rerun_is_a_fresh_handle():
    """dekf_reset makes every instance active: the handle launches the siblings again and gives the bits of the run without pauses"""
    mk, B, K, kernel = PZ.GPU_SHAPES["go1"]
    p, s = EL.gpu_streams("go1")
    got, names, est = PZ.run_gpu(p, s, B, 55, "cross", PZ.gpu_schedule(B, K), close=False)
    assert names[-1][0] == kernel + "_smooth_cross_ep" and got[-1]["active"].tolist() == [0, 1, 1, 1, 1, 1]
    est.reset()
    again, names, _ = PZ.run_gpu(p, s, B, 55, "cross", est=est)
    assert names == [(kernel + "_smooth_cross",) * 2]
    plain = PZ.gpu_fresh("go1", "cross", tuple(range(K)))
    for b in range(B):
        PZ.assert_cut_life_equal(again, plain, b, tuple(range(55)), p.N, PZ.GPU_KEYS, "reset and re-run")
        assert all(r["active"][b] == 1 for r in again)


def test_parameter_table_one_paused_instance_on_its_own_noise_set():
    """a handle with a parameter table launches the _pp twins before and after the pause; the paused instance (on set 1) equals a uniform
    handle created with set 1 on the cut log, its neighbours uniform handles with their sets on the whole log"""
    mk, B, set_of, kernel = PL.GPU_SHAPES["go1"]
    p, s = PL.gpu_streams("go1")
    K, variant, b = PL.K_LOG, "cross", 1
    sets = PL.param_sets(p)
    schedule = {20: dict(active=PZ._mask(B, {b})), 31: dict(active=PZ._mask(B, ()))}
    got, names, _ = PZ.run_gpu(p, s, B, K, variant, schedule, stray=True, sets=sets, set_of=set_of)
    assert all(n == (kernel + PL.TWIN_SUFFIX[variant],) * 2 for n in names) and len(names) == 3
    life = tuple(k for k in range(K) if not 20 <= k < 31)
    fresh = EL.run_gpu(PL.param_set(p, set_of[b]), PZ.cut_streams(s, life), B, len(life), variant)[0]
    PZ.assert_cut_life_equal(got, fresh, b, life, p.N, PZ.GPU_KEYS, "paused, set 1")
    for k in range(20, 31):
        PZ.assert_frozen(got, b, k, 19, p.N, PZ.GPU_KEYS, "paused, set 1")
    for o in range(B):
        if o != b:
            PZ.assert_cut_life_equal(got, PL.gpu_uniform("go1", variant, set_of[o]), o, tuple(range(K)), p.N, PZ.GPU_KEYS, "neighbour")
