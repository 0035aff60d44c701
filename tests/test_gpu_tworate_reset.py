"""dekf_reset_instances on a two-rate handle on the GPU (EKF 500 Hz, MHE 200 Hz: go1_params() as it ships), through the C ABI.

Every lock-step test ticks the EKF once per update, so the two epochs of a restart (t0: the handle's MHE step, c0: its EKF tick count)
are equal there and the C boundary could pass one for the other unnoticed.  On tworate_lib's 1 ms event grid 2 or 3 EKF ticks lie
between two updates and a restart may fall anywhere between them: every life against a fresh handle driven from the restart's ms,
every getter, to the bit; the kernels the handle launches; host and device masks; and two instances against the fp64 oracle driven by
the same events (exact optimum of its window QP, inverse of its KKT matrix)."""
import functools

import numpy as np
import pytest

import direct_lib as DL
import epoch_lib as EL
import tworate_lib as TL
from decentralized_ekf_mhe_amd import capi

pytestmark = pytest.mark.gpu
# name: (B, direct kernel)
SHAPES = {"go1": (6, "k_mhe_solve_direct_4_n20"), "go1_foot": (4, "k_mhe_solve_direct_foot_4")}
# ekf_history 16: the rewind ring wraps ten times in a run and more than twice in a restarted life (256: the default, never wraps)
CASES = [("go1", "plain", 16), ("go1", "cross", 16), ("go1_foot", "cross", 16), ("go1", "plain", 256)]


@functools.lru_cache(maxsize=None)
def scheduled(name, variant, H, device_mask=False):
    """the shape's handle over the grid with tworate_lib.RESETS, once per process"""
    return TL.run_gpu(name, H, SHAPES[name][0], variant, resets=TL.RESETS, device_mask=device_mask)


@pytest.mark.parametrize("name,variant,H", CASES)
def test_every_life_is_a_fresh_handle_started_at_its_restart(name, variant, H):
    B, kernel = SHAPES[name]
    p, s, n_grid = TL.streams(name, H, B)
    assert (p.ekf_rate, p.rate, p.ekf_history) == (500, 200, H)
    got, names = scheduled(name, variant, H)
    sibling, twin = kernel + EL.SIBLING_SUFFIX[variant], kernel + EL.TWIN_SUFFIX[variant]
    assert names[0] == (sibling, sibling) and names[1:] == [(twin, twin)] * len(TL.RESETS)
    assert len(got) == TL.N_MHE
    plain = TL.gpu_fresh(name, H, B, variant)
    for b in range(B):
        first = min([g for g in TL.RESETS if b in TL.RESETS[g]] + [n_grid])
        TL.assert_gpu_life_equal(got, plain, b, 0, first, p.N, "untouched")
    assert EL.untouched(TL.RESETS, B) == list(range(3, B))
    lives = TL.lives(TL.RESETS, n_grid)
    assert len(lives) == 6
    # a VO pose straddles a restart: the one event at which a wrong EKF epoch changes bits (tworate_lib.RESETS)
    assert sum(len(TL.straddling_poses(s, b, g0, g_end)) for b, g0, g_end in lives) >= 1
    for b, g0, g_end in lives:
        TL.assert_gpu_life_equal(got, TL.gpu_fresh(name, H, B, variant, g0), b, g0, g_end, p.N, "life")
        T0, T1 = TL.first_step(g0), TL.first_step(g0) + TL.steps_of(g0, g_end) - 1
        assert got[T0]["status"][b] == capi.DEKF_SOLVE_NONE and np.isnan(got[T0]["cov"][b]).all()
        assert got[T1]["status"][b] == capi.DEKF_SOLVE_OK
        # the two epochs of this restart differ (EKF ticks before ms g0 against timer events before it)
        assert TL.ekf_ticks(0, g0) != T0
    if H == 16:
        assert sum(TL.ekf_ticks(g0, g_end) >= 2 * H for _, g0, g_end in lives) >= 3
    assert all(r["K"] == min(T + 1, p.N) for T, r in enumerate(got) if "K" in r)   # (*steps: the untouched instances' window)
    assert got[-1]["ticks"].tolist()[:4] == [23, 42, 23, 69]


def test_host_and_device_masks_give_the_same_bits():
    name, variant, H = "go1", "cross", 16
    B = SHAPES[name][0]
    p = TL.streams(name, H, B)[0]
    (host, names_h), (dev, names_d) = scheduled(name, variant, H), scheduled(name, variant, H, True)
    assert names_h == names_d and len(host) == len(dev)
    for T in range(len(host)):
        assert sorted(host[T]) == sorted(dev[T])
        for key in host[T]:
            if key not in EL.WINDOW_KEYS:
                assert np.array_equal(host[T][key], dev[T][key], equal_nan=True), (T, key)
                continue
            for b in range(B):     # (an instance's entries beyond its own window are not specified)
                n = EL.window_lengths(key, EL.local_K(int(host[T]["ticks"][b]), p.N))
                assert np.array_equal(host[T][key][b, :n], dev[T][key][b, :n]), (T, key, b)


@pytest.mark.parametrize("variant", ["plain", "cross"])
def test_restarted_and_untouched_instance_against_the_oracle(variant):
    """Go1 at ekf_history 16, instance 1 (restarted before ms 63 and 132) and instance 3 (never), every life of each: the oracle's
    orientation filter and estimator driven by the life's events from its first ms.  At every MHE step the quaternion within 1e-9
    (test_gpu_configs._multirate_case's bound), x_T within direct_lib.XREL / XABS per 3-block of the exact optimum of the oracle's window
    QP, Cov(x_T) within direct_lib.CREL of the inverse of its KKT matrix.  The oracle's history is unbounded: no pose of these logs
    reaches back further than the 16-deep ring (asserted), so it stays the reference of the wrapped ring too.
    Measured on an MI355X, plain and cross alike: quaternion 2.2e-16 / 1.1e-16, x_T 0.0027 / 0.0053 of the bound, Cov(x_T) 1.1e-10 /
    9.5e-11 for instances 1 / 3"""
    name, H = "go1", 16
    B = SHAPES[name][0]
    p, s, n_grid = TL.streams(name, H, B)
    got, _ = scheduled(name, variant, H)
    ns = p.dim_state
    for b, lives in ((1, [(0, 63), (63, 132), (132, n_grid)]), (3, [(0, n_grid)])):
        worst_q, worst_x, worst_c, replays = 0.0, 0.0, 0.0, 0
        for g0, g_end in lives:
            n, deepest = TL.oracle_replays(p, s, b, g0, g_end)
            assert n >= 1 and deepest < H, (b, g0, n, deepest)
            replays += n
            ref = TL.oracle_life(name, H, B, b, g0, g_end)
            T0 = TL.first_step(g0)
            assert len(ref) == TL.steps_of(g0, g_end)
            for j, (q, x, Cx) in enumerate(ref):
                g = got[T0 + j]
                assert g["ticks"][b] == j
                worst_q = max(worst_q, float(np.abs(g["quat"][b] - q).max()))
                if j:
                    assert g["status"][b] == capi.DEKF_SOLVE_OK, (b, g0, j)
                    worst_x = max(worst_x, DL.block_err(g["x"][b], x, DL.blocks3(ns), DL.XREL, DL.XABS))
                    worst_c = max(worst_c, DL.cov_err(g["cov"][b], Cx))
        print(f"[{variant}, instance {b}] {replays} replays; quaternion {worst_q:.3g} (bound 1e-9), x_T {worst_x:.3g} x (1e-8 rel + 1e-10), "
              f"Cov(x_T) {worst_c:.3g} (bound {DL.CREL:g}, units of sqrt(C_ii C_jj))")
        assert worst_q < 1e-9
        assert worst_x <= 1.0
        assert worst_c <= DL.CREL
