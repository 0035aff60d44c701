"""dekf_set_instance_params on a two-rate handle on the GPU (EKF 500 Hz, MHE 200 Hz), through the C ABI.

On tworate_lib's 1 ms event grid a restart may fall anywhere between two updates, with EKF ticks of the handle behind the last update.
A restarted instance takes a set as long as IT has not ticked since ITS restart, whatever the handle ticked before: the schedule with
a table, every life against a fresh uniform handle created with the life's set and driven from the restart's ms, to the bit; and the
ordering rule per instance."""
import ctypes as C
import functools

import numpy as np
import pytest

import instance_params_lib as PL
import tworate_lib as TL
from decentralized_ekf_mhe_amd import capi
from decentralized_ekf_mhe_amd.params import DekfParams
from test_gpu_tworate_reset import SHAPES

pytestmark = pytest.mark.gpu
H = 16


@pytest.mark.parametrize("name,variant", [("go1", "plain"), ("go1", "cross"), ("go1_foot", "cross")])
def test_restarted_instances_take_another_set_between_two_updates(name, variant):
    """the table SET_OF from ms 0; every restart of tworate_lib.RESETS gives its instances ANOTHER set (NEW_SETS).  The restart before
    ms 63 lies behind an EKF tick of the handle (ms 62) that followed the last update (ms 60)"""
    B, kernel = SHAPES[name]
    p, s, n_grid = TL.streams(name, H, B)
    set_of = TL.SET_OF[:B]
    got, names = TL.run_gpu(name, H, B, variant, set_of=set_of, resets=TL.RESETS, new_sets=TL.NEW_SETS)
    twin = kernel + PL.TWIN_SUFFIX[variant]
    assert names == [(twin, twin)] * (1 + len(TL.RESETS))
    for b in range(B):
        first = min([g for g in TL.RESETS if b in TL.RESETS[g]] + [n_grid])
        TL.assert_gpu_life_equal(got, TL.gpu_fresh(name, H, B, variant, 0, set_of[b]), b, 0, first, p.N, "untouched")
    now = dict(enumerate(set_of))
    lives = TL.lives(TL.RESETS, n_grid)
    assert len(lives) == 6
    for b, g0, g_end in lives:       # (in the order of the restarts)
        k = TL.NEW_SETS[g0][b]
        assert k != now[b]
        now[b] = k
        TL.assert_gpu_life_equal(got, TL.gpu_fresh(name, H, B, variant, g0, k), b, g0, g_end, p.N, "life on set %d" % k)
        T0, T1 = TL.first_step(g0), TL.first_step(g0) + TL.steps_of(g0, g_end) - 1
        assert got[T0]["status"][b] == capi.DEKF_SOLVE_NONE and got[T1]["status"][b] == capi.DEKF_SOLVE_OK
    # the sets matter on this grid
    a, c = TL.gpu_fresh(name, H, B, variant, 226, 1), TL.gpu_fresh(name, H, B, variant, 226, 2)
    for key in ("x", "quat", "cov"):
        assert not np.array_equal(a[-1][key], c[-1][key]), key


# ------------------------------------------------------------------ the ordering rule, per instance
NAME, VARIANT, B = "go1", "plain", 4


def _raw_set(est, sets, so):
    """dekf_set_instance_params' own status"""
    arr = (DekfParams * len(sets))(*[q.copy() for q in sets])
    so = np.ascontiguousarray(so, np.int32)
    return capi.load().dekf_set_instance_params(est.h, C.cast(arr, C.c_void_p), len(sets), C.c_void_p(so.ctypes.data))


@functools.lru_cache(maxsize=None)
def _sets():
    return PL.param_sets(TL.streams(NAME, H, B)[0])


def test_set_after_an_ekf_tick_of_the_handle_but_none_of_the_instance():
    """dekf_update (ms 60), dekf_ekf_step (ms 62), dekf_reset_instances(1), dekf_set_instance_params(1 -> set 2) on a handle that had no
    table: DEKF_OK, although the handle has ticked since its last update: instance 1 has not since its restart.  Its life is the
    fresh handle created with set 2 and driven from ms 63; every other instance keeps the bits of the run without restarts"""
    p, s, n_grid = TL.streams(NAME, H, B)
    sets, seen = _sets(), []

    def poke(dev):
        seen.append(_raw_set(dev.est, sets, [-1, 2, -1, -1]))
        seen.append(dev.est.solve_kernel_name())
        seen.append(bytes(dev.est.instance_params(1)) == bytes(sets[2]) and bytes(dev.est.instance_params(0)) == bytes(sets[0]))

    got, _ = TL.run_gpu(NAME, H, B, VARIANT, resets={63: [1]}, pokes={63: poke})
    assert seen == [capi.DEKF_OK, SHAPES[NAME][1] + "_pp", True]
    TL.assert_gpu_life_equal(got, TL.gpu_fresh(NAME, H, B, VARIANT, 63, 2), 1, 63, n_grid, p.N, "life on set 2")
    plain = TL.gpu_fresh(NAME, H, B, VARIANT)
    TL.assert_gpu_life_equal(got, plain, 1, 0, 63, p.N, "before the restart")
    for b in (0, 2, 3):
        TL.assert_gpu_life_equal(got, plain, b, 0, n_grid, p.N, "untouched")


def test_restarted_instance_that_has_ticked_since_is_refused():
    """instance 1 restarted before ms 63; after its first EKF tick (ms 64) it no longer takes a set: DEKF_ERR_ORDER, and nothing is
    applied: the handle keeps its kernels and its parameters, and the life stays the fresh handle's with the handle's own set"""
    p, s, n_grid = TL.streams(NAME, H, B)
    sets, seen = _sets(), []

    def poke(dev):
        seen.append(_raw_set(dev.est, sets, [-1, 2, -1, -1]))
        seen.append(dev.est.solve_kernel_name())
        seen.append(all(bytes(dev.est.instance_params(b)) == bytes(sets[0]) for b in range(B)))

    got, _ = TL.run_gpu(NAME, H, B, VARIANT, resets={63: [1]}, pokes={65: poke})   # (ms 65: behind the tick of ms 64, before the timer)
    assert seen == [capi.DEKF_ERR_ORDER, SHAPES[NAME][1] + "_ep", True]
    TL.assert_gpu_life_equal(got, TL.gpu_fresh(NAME, H, B, VARIANT, 63), 1, 63, n_grid, p.N, "life")
    plain = TL.gpu_fresh(NAME, H, B, VARIANT)
    for b in (0, 2, 3):
        TL.assert_gpu_life_equal(got, plain, b, 0, n_grid, p.N, "untouched")


def test_two_restarts_in_one_gap_are_told_apart():
    """between the updates of ms 60 and 65: instance 1 restarted before ms 61, the EKF tick of ms 62, instance 2 restarted before ms 63.
    Instance 2 may take a set, instance 1 may not, and a call that names both is refused whole"""
    p, s, n_grid = TL.streams(NAME, H, B)
    sets, seen = _sets(), []

    def poke(dev):
        seen.append(_raw_set(dev.est, sets, [-1, 1, 2, -1]))       # names instance 1: nothing is applied, not to instance 2 either
        seen.append(dev.est.solve_kernel_name())
        seen.append(_raw_set(dev.est, sets, [-1, 1, -1, -1]))
        seen.append(_raw_set(dev.est, sets, [-1, -1, 2, -1]))
        seen.append(dev.est.solve_kernel_name())
        seen.append([bytes(dev.est.instance_params(b)) == bytes(sets[k]) for b, k in enumerate([0, 0, 2, 0])])

    got, _ = TL.run_gpu(NAME, H, B, VARIANT, resets={61: [1], 63: [2]}, pokes={63: poke})
    kernel = SHAPES[NAME][1]
    assert seen == [capi.DEKF_ERR_ORDER, kernel + "_ep", capi.DEKF_ERR_ORDER, capi.DEKF_OK, kernel + "_pp", [True] * 4]
    TL.assert_gpu_life_equal(got, TL.gpu_fresh(NAME, H, B, VARIANT, 61), 1, 61, n_grid, p.N, "instance 1, the handle's own set")
    TL.assert_gpu_life_equal(got, TL.gpu_fresh(NAME, H, B, VARIANT, 63, 2), 2, 63, n_grid, p.N, "instance 2 on set 2")
    plain = TL.gpu_fresh(NAME, H, B, VARIANT)
    for b in (0, 3):
        TL.assert_gpu_life_equal(got, plain, b, 0, n_grid, p.N, "untouched")
