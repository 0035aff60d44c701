"""Restarting single instances of a direct handle (dekf_reset_instances / dekf_get_instance_ticks, csrc/mhe_epoch_core.h) without a GPU.

ABI: the two calls are declared, exported and bound, refuse a null handle and compile as C99, while the ABI version and dekf_params
stay what they were; the thirty _ep twins sit at their siblings' design point.
Core: the lane-sequential build of the epoch cores (tests/hostsim/epoch_hostsim.cpp) over 100-tick rough_streams logs with four
restarts: every life equals, to the bit, a fresh simulation (the harness WITHOUT epochs) of the log sliced from its restart tick, and
an instance equals the run without restarts until its first one.  Two lives are also held against the oracle on the sliced log."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import direct_lib as DL
import epoch_lib as EL
import tworate_lib as TL
from decentralized_ekf_mhe_amd import capi, go1_params

SYMBOLS = ("dekf_reset_instances", "dekf_get_instance_ticks")


# ------------------------------------------------------------------ 1: the C boundary
def test_header_declares_both_calls():
    hdr = DL.header()
    assert re.search(r"dekf_status\s+dekf_reset_instances\s*\(\s*dekf_handle\s+h\s*,\s*const\s+int\s*\*\s*mask\s*,\s*dekf_mem\s+where\s*\)\s*;", hdr)
    assert re.search(r"dekf_status\s+dekf_get_instance_ticks\s*\(\s*dekf_handle\s+h\s*,\s*int\s*\*\s*ticks\s*,\s*dekf_mem\s+where\s*\)\s*;", hdr)
    assert re.search(r"#define\s+DEKF_ABI_VERSION\s+4\b", hdr)


def test_library_exports_and_binding_lists_them():
    DL.check_exports_and_binding(SYMBOLS)
    for name in SYMBOLS:
        assert capi.PROTOTYPES[name] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int])


def test_abi_version_and_params_layout_unchanged():
    DL.check_abi_version_and_params_layout()


def test_null_handle_is_invalid():
    lib = capi.load()
    m = (C.c_int * 4)(0, 1, 0, 0)
    t = (C.c_int * 4)(-7, -7, -7, -7)
    for where in (capi.DEKF_HOST, capi.DEKF_DEVICE):
        assert lib.dekf_reset_instances(None, C.cast(m, C.c_void_p), where) == capi.DEKF_ERR_INVALID
        assert lib.dekf_get_instance_ticks(None, C.cast(t, C.c_void_p), where) == capi.DEKF_ERR_INVALID
    assert list(t) == [-7] * 4


def test_header_compiles_as_c99_with_the_instance_calls(tmp_path):
    DL.check_c99_client(tmp_path, "instance_client",
                        "    int mask[2] = {1, 0}, ticks[2] = {-7, -7};\n"
                        "    dekf_status a = dekf_reset_instances((dekf_handle)0, mask, DEKF_HOST);\n"
                        "    dekf_status b = dekf_get_instance_ticks((dekf_handle)0, ticks, DEKF_HOST);\n"
                        '    printf("reset %d ticks %d first %d abi %d\\n", (int)a, (int)b, ticks[0], DEKF_ABI_VERSION);\n',
                        f"reset {capi.DEKF_ERR_INVALID} ticks {capi.DEKF_ERR_INVALID} first -7 abi 4")


# ------------------------------------------------------------------ 2: the epoch cores, lane-sequential
@pytest.mark.parametrize("variant", list(DL.VARIANTS))
@pytest.mark.parametrize("name", list(EL.CPU_SHAPES))
def test_every_life_is_a_fresh_simulation_of_the_sliced_log(name, variant):
    mk, B = EL.CPU_SHAPES[name]
    p, K, resets = mk(), EL.K_LOG, EL.CPU_RESETS[name]
    s = DL.rough_streams(p, B, K)
    keys = EL.SIM_KEYS + ("pri_res", "dua_res")
    got = EL.run_epoch_sim(p, s, B, K, variant, resets)
    plain = EL.run_fresh_sim(p, s, B, K, variant)
    # until its first restart an instance is an untouched one: the run without restarts, every tick
    for b in range(B):
        first = min([T0 for T0 in resets if b in resets[T0]] + [K])
        EL.assert_life_equal(got, plain, b, 0, first, p.N, keys, "untouched")
    n_lives = 0
    for b, T0, end in EL.lives(resets, K):
        fresh = EL.run_fresh_sim(p, EL.slice_streams(s, T0), B, end - T0, variant)
        EL.assert_life_equal(got, fresh, b, T0, end, p.N, keys, "life")
        assert (got[T0]["status"][b], got[T0]["ticks"][b]) == (capi.DEKF_SOLVE_NONE, 0)
        assert np.isnan(got[T0]["cov"][b]).all() and not np.isnan(got[T0 + 1]["cov"][b]).any()
        assert got[end - 1]["status"][b] == capi.DEKF_SOLVE_OK and got[end - 1]["ticks"][b] == end - 1 - T0
        n_lives += 1
    assert n_lives == 4
    # the restart before tick 12 fell inside the instance's own window fill, the one before tick 45 behind a full window
    assert got[11]["ticks"][resets[12][0]] == 6 < p.N - 1 <= got[44]["ticks"][resets[45][0]]


def test_go1_restart_before_tick_45_leaves_a_window_with_vo_equality_rows():
    """the Go1 schedule's last restart hits an even instance whose full window holds VO equality rows (the oracle's own count)"""
    mk, B = EL.CPU_SHAPES["go1"]
    p = mk()
    s = DL.rough_streams(p, B, EL.K_LOG)
    (_, _, _, _, nv), = DL.kkt_reference(p, s, EL.CPU_RESETS["go1"][45][0], {44}, solve=False, invert=False)
    assert nv > 0


def test_epoch_with_nothing_restarted_is_the_plain_harness():
    """every epoch 0: the epoch cores, tick 0 included, leave what hs_initialize / hs_update_direct_cross leave"""
    p = DL._params(go1_params)
    B, K = 2, 30
    s = DL.rough_streams(p, B, K)
    got, plain = EL.run_epoch_sim(p, s, B, K, "cross", {}), EL.run_fresh_sim(p, s, B, K, "cross")
    for b in range(B):
        EL.assert_life_equal(got, plain, b, 0, K, p.N, EL.SIM_KEYS, "no restart")


def test_fold_keeps_the_local_count_modulo_the_history_and_whether_it_is_full():
    """dekf_ekf_step folds its tick count at 2^30 to H + count % H; fold_epoch gives every instance the epoch that keeps the local count
    modulo H and whether it has reached H: all that ekf_tick takes from it"""
    L = EL.epoch_hostsim()
    for H in (4, 7, 256):
        old = 1 << 30
        new = H + old % H
        for local in (0, 1, H - 1, H, H + 1, 2 * H + 3, 12345, old - 5, old):
            c0 = old - local
            c1 = L.hs_fold_epoch(c0, old, new, H)
            after = new - c1
            assert 0 <= after < 2 * H and after % H == local % H and (after >= H) == (local >= H), (H, local, after)
            if local < H:
                assert after == local
        # a second fold, epochs that the first one made negative included
        for c1 in (-(H - 1), 0, H):
            local = old - c1
            after = new - L.hs_fold_epoch(c1, old, new, H)
            assert after % H == local % H and after >= H


# ------------------------------------------------------------------ 2b: the two rates (EKF 500 Hz, MHE 200 Hz)
@pytest.mark.parametrize("name,H", [("go1", 256), ("go1", 16), ("tripod", 16)])
def test_two_rate_lives_are_fresh_simulations_started_at_their_restart(name, H):
    """tworate_lib's event grid and schedule, variant cross (which writes every array), B = 4: restarts with EKF ticks behind the last
    update, with a VO pose that straddles the restart, directly behind an update, inside the instance's own fill on an EKF-tick ms,
    and of two instances from full windows.  2
    or 3 EKF ticks lie between two updates, so the two epochs of a restart differ: a core that took one for the other, or the C
    boundary's order of them, shows here and in no lock-step test.  At ekf_history 16 the rewind ring of a restarted life wraps"""
    B, variant = 4, "cross"
    p, s, n_grid = TL.streams(name, H, B)
    assert (p.ekf_rate, p.rate, p.ekf_history) == (500, 200, H)
    keys = EL.SIM_KEYS + ("pri_res", "dua_res")
    got = TL.run_epoch_sim(name, H, B, variant, TL.RESETS)
    plain = TL.cpu_fresh(name, H, B, variant)
    assert len(got) == len(plain) == TL.N_MHE
    assert EL.untouched(TL.RESETS, B) == [3]
    for b in range(B):
        first = min([g for g in TL.RESETS if b in TL.RESETS[g]] + [n_grid])
        TL.assert_life_equal(got, plain, b, 0, first, p.N, keys, "untouched")
    lives = TL.lives(TL.RESETS, n_grid)
    assert len(lives) == 6
    differ, wrapped, straddled = 0, 0, 0
    for b, g0, g_end in lives:
        TL.assert_life_equal(got, TL.cpu_fresh(name, H, B, variant, g0), b, g0, g_end, p.N, keys, "life")
        straddled += len(TL.straddling_poses(s, b, g0, g_end))
        T0 = TL.first_step(g0)
        # the epochs the harness holds: the step of the life's first timer event, and the EKF ticks of the handle before ms g0
        assert (got[T0]["t0"][b], got[T0]["c0"][b]) == (T0, TL.ekf_ticks(0, g0)), (b, g0)
        assert (got[T0]["status"][b], got[T0]["ticks"][b]) == (capi.DEKF_SOLVE_NONE, 0)
        assert np.isnan(got[T0]["cov"][b]).all() and not np.isnan(got[T0 + 1]["cov"][b]).any()
        differ += got[T0]["c0"][b] != got[T0]["t0"][b]
        wrapped += TL.ekf_ticks(g0, g_end) >= 2 * H
        # the oracle's filter rewinds inside the life: the restarted instance's ring is read back, never deeper than the ring
        replays, deepest = TL.oracle_replays(p, s, b, g0, g_end)
        assert replays >= 1 and deepest < 16, (b, g0, replays, deepest)
    assert differ == 6
    assert wrapped >= (3 if H == 16 else 0)
    assert straddled >= 1      # (the event at which a wrong EKF epoch changes bits: tworate_lib.RESETS)
    # ms 226 fell behind full windows; ms 132 at instance 1's local step 13: inside its own fill at N = 20, just behind it at N = 12
    assert got[26]["ticks"][1] == 13 and p.N - 1 <= got[45]["ticks"][0]
    assert (13 < p.N - 1) == (name == "go1")


# ------------------------------------------------------------------ 3: against the oracle
@pytest.mark.parametrize("b,T0", [(4, 30), (2, 45)])
def test_life_against_the_oracle_on_the_sliced_log(b, T0):
    """a restarted instance against the exact optimum of the oracle's window QP and the inverse of its KKT matrix, the oracle fed the
    log from the restart tick on: x_T and Cov(x_T), every window state and its covariance, the cross-covariances"""
    p = DL._params(go1_params)
    B, K, ns, N = 6, EL.K_LOG, 9, 20
    ticks = [1, 10, 19, 20, 40, 54]
    s = DL.rough_streams(p, B, K)
    got = EL.run_epoch_sim(p, s, B, K, "cross", {30: [4], 45: [2]})
    sl = EL.slice_streams(s, T0)
    worst_x, worst_c, worst_w, worst_wc, worst_1, worst_n, vo = 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, {}
    for j, x, Ki, xo, nv in DL.kkt_reference(p, sl, b, set(ticks)):
        g = got[T0 + j]
        Kb = min(j + 1, N)
        assert g["ticks"][b] == j and g["status"][b] == capi.DEKF_SOLVE_OK and len(xo) == Kb
        X = np.array([x[o:o + ns] for o in xo])
        idx = np.concatenate([np.arange(o, o + ns) for o in xo])
        Cf = Ki[np.ix_(idx, idx)].reshape(Kb, ns, Kb, ns).transpose(0, 2, 1, 3)
        Cv = np.array([Cf[k, k] for k in range(Kb)])
        worst_x = max(worst_x, DL.block_err(g["x"][b], X[-1], DL.blocks3(ns), DL.XREL, DL.XABS))
        worst_c = max(worst_c, DL.cov_err(g["cov"][b], Cv[-1]))
        ex, ec, _ = DL.window_errors(g["xw"][b, :Kb], g["cw"][b, :Kb], X, Cv, ns)
        e1, en = DL.cross_errors(g["l1"][b, :Kb - 1], g["zn"][b, :Kb], Cf)
        worst_w, worst_wc, worst_1, worst_n = max(worst_w, ex), max(worst_wc, ec), max(worst_1, e1), max(worst_n, en)
        vo[j] = nv
    print(f"[instance {b}, T0 = {T0}] x_T {worst_x:.3g} x (1e-8 rel + 1e-10), Cov(x_T) {worst_c:.3g}; window x {worst_w:.3g} x, cov {worst_wc:.3g}; "
          f"lag-one {worst_1:.3g}, to-newest {worst_n:.3g} (covariances in units of sqrt(C_ii C_jj)); VO equality rows by local tick: {vo}")
    assert sorted(vo) == ticks
    assert vo[40] > 0 and vo[54] > 0, "the windows at local ticks 40 and 54 hold no VO equality row"
    assert worst_x <= 1.0 and worst_w <= 1.0
    assert max(worst_c, worst_wc, worst_1, worst_n) <= DL.CREL


# ------------------------------------------------------------------ 4: resource remarks
@pytest.mark.parametrize("variant", list(DL.VARIANTS))
def test_epoch_twins_at_their_siblings_design_point(variant):
    """every direct kernel's _ep twin against the kernel it wraps: no spills, no scratch, no static LDS, an occupancy class not below
    the sibling's (or still above what the kernel's LDS admits)"""
    DL.check_twins_at_their_design_point(EL.SIBLING_SUFFIX[variant], EL.TWIN_SUFFIX[variant])


# ------------------------------------------------------------------ 5: sanitizers
ASAN_MAIN = r"""
#include "epoch_hostsim.cpp"
#include <cmath>
#include <cstdio>
// synthetic sensors as direct_lib.ASAN_DRIVER's, VO on every sixth step; B = 3, instance 1 restarted in its window fill (before tick 5),
// again inside its second fill (before tick 9) and, with instance 2, from full windows (before tick N + 9); instance 0 never
static int run(int L, int nj, int N, int steps, int ft, int form) {
    dekf_params p; default_params(&p); p.ekf_rate = 200; p.num_legs = L; p.joints_per_leg = nj; p.N = N; p.leg_odom_type = ft; p.arrival_cost_form = form;
    const int ns = 9 + 3 * L * ft, B = 3;
    void* h = hs_create(&p, B);
    if (!h) return 1;
    void* e = hs_epochs_create(B);
    std::vector<double> t(B), acc(3 * B), gy(3 * B), pf(3 * L * B), J(3 * L * nj * B), qd(L * nj * B), c(L * B), cov((size_t)B * ns * ns, NAN);
    std::vector<int> mask(B, 1), ticks(B); std::vector<double> tp(B), tn(B), dp(3 * B), q(4 * B);
    std::vector<double> xw, cw, l1, zn;
    int bad = 0;
    for (int T = 0; T < steps; ++T) {
        if (T == 5 || T == 9) { const int m[3] = {0, 1, 0}; hs_reset_instances(h, e, m, cov.data()); }
        if (T == N + 9) { const int m[3] = {0, 1, 1}; hs_reset_instances(h, e, m, cov.data()); }
        for (int b = 0; b < B; ++b) {
            t[b] = 0.005 * T + 1e-5 * b;
            acc[3*b] = 0.1; acc[3*b+1] = -0.05; acc[3*b+2] = 9.8; gy[3*b] = 0.01; gy[3*b+1] = 0.02; gy[3*b+2] = 0.2;
            for (int i = 0; i < 3 * L; ++i) pf[3*L*b + i] = 0.1 * (i % 3) - 0.25;
            for (int i = 0; i < 3 * L * nj; ++i) J[3*L*nj*b + i] = (i % (nj + 1) == 0) ? 0.2 : 0.03 * ((i + T) % 5);
            for (int i = 0; i < L * nj; ++i) qd[L*nj*b + i] = 0.1 * ((i + T) % 7) - 0.3;
            for (int i = 0; i < L; ++i) c[L*b + i] = ((T / 5 + i) % 2) ? 1.0 : 0.0;
            tp[b] = 0.005 * (T - 7); tn[b] = 0.005 * (T - 1); dp[3*b] = 0.003; dp[3*b+1] = 0; dp[3*b+2] = 0;
            q[4*b] = 1; q[4*b+1] = q[4*b+2] = q[4*b+3] = 0;
        }
        hs_push_imu(h, t.data(), acc.data(), gy.data());
        hs_push_leg(h, pf.data(), J.data(), qd.data(), c.data());
        if (T > 8 && T % 6 == 0) hs_push_vo(h, mask.data(), tp.data(), tn.data(), dp.data(), tn.data(), q.data());
        hs_ekf_step_epoch(h, e);
        // the four window buffers at exactly their contract sizes, the guard behind every instance's K_b written entries checked
        xw.assign((size_t)B * N * ns, -7.0);
        cw.assign((size_t)B * N * ns * ns, -7.0);
        l1.assign((size_t)B * (N - 1) * ns * ns, -7.0);
        zn.assign((size_t)B * N * ns * ns, -7.0);
        hs_update_direct_cross_epoch(h, e, T, cov.data(), xw.data(), cw.data(), l1.data(), zn.data());
        hs_instance_ticks(e, T, ticks.data());
        for (int b = 0; b < B; ++b) {
            const int K = ticks[b] < 1 ? 0 : (ticks[b] + 1 < N ? ticks[b] + 1 : N);
            for (int k = 0; k < N; ++k) {
                for (int i = 0; i < ns; ++i) { const double v = xw[((size_t)b * N + k) * ns + i]; bad += k < K ? !std::isfinite(v) : v != -7.0; }
                for (int i = 0; i < ns * ns; ++i) {
                    const double v = cw[((size_t)b * N + k) * ns * ns + i], z = zn[((size_t)b * N + k) * ns * ns + i];
                    bad += k < K ? !std::isfinite(v) : v != -7.0;
                    bad += k < K ? !std::isfinite(z) : z != -7.0;
                    if (k < N - 1) { const double w = l1[((size_t)b * (N - 1) + k) * ns * ns + i]; bad += k < K - 1 ? !std::isfinite(w) : w != -7.0; }
                }
            }
            for (int i = 0; i < ns * ns; ++i) bad += K ? !std::isfinite(cov[(size_t)b * ns * ns + i]) : !std::isnan(cov[(size_t)b * ns * ns + i]);
        }
    }
    std::vector<double> x(ns * B); std::vector<int> st(B);
    hs_get(h, x.data(), nullptr, nullptr, nullptr, st.data(), nullptr, nullptr);
    std::printf("L=%d nj=%d N=%d leg_odom_type=%d arrival_cost_form=%d: status %d %d %d ticks %d %d %d, %d bad entries\n", L, nj, N, ft, form,
                st[0], st[1], st[2], ticks[0], ticks[1], ticks[2], bad);
    const bool ticks_ok = ticks[0] == steps - 1 && ticks[1] == steps - 1 - (N + 9) && ticks[2] == ticks[1];
    hs_epochs_destroy(e);
    hs_destroy(h);
    return st[0] == 1 && st[1] == 1 && st[2] == 1 && bad == 0 && ticks_ok ? 0 : 2;
}
// The two rates on a 1 ms grid: sensors and one EKF tick on every even ms, the update on every 5th, VO on every 30th from ms 40 on, at a
// history of 8 samples (the ring wraps in every life).  Instance 1 restarted before ms 63 (an EKF tick lies between the update of ms 60
// and the restart) and before ms 132 (on an EKF-tick ms, in its own fill), instances 1 and 2 before ms 5 N + 46; instance 0 never
static int run_two_rate(int L, int nj, int N, int steps, int ft, int form) {
    dekf_params p; default_params(&p); p.ekf_rate = 500; p.rate = 200; p.ekf_history = 8; p.num_legs = L; p.joints_per_leg = nj; p.N = N; p.leg_odom_type = ft; p.arrival_cost_form = form;
    const int ns = 9 + 3 * L * ft, B = 3, last = 5 * N + 46;
    void* h = hs_create(&p, B);
    if (!h) return 1;
    void* e = hs_epochs_create(B);
    std::vector<double> t(B), acc(3 * B), gy(3 * B), pf(3 * L * B), J(3 * L * nj * B), qd(L * nj * B), c(L * B), cov((size_t)B * ns * ns, NAN);
    std::vector<int> mask(B, 1), ticks(B, 0); std::vector<double> tp(B), tn(B), dp(3 * B), q(4 * B);
    std::vector<double> xw, cw, l1, zn;
    int bad = 0;
    for (int i = 0; i < 5 * (steps - 1) + 1; ++i) {
        if (i == 63 || i == 132) { const int m[3] = {0, 1, 0}; hs_reset_instances(h, e, m, cov.data()); }
        if (i == last) { const int m[3] = {0, 1, 1}; hs_reset_instances(h, e, m, cov.data()); }
        if (i > 39 && i % 30 == 10) {
            for (int b = 0; b < B; ++b) {
                tp[b] = 0.001 * (i - 42); tn[b] = 0.001 * (i - 9); dp[3*b] = 0.003; dp[3*b+1] = 0; dp[3*b+2] = 0;
                q[4*b] = 1; q[4*b+1] = q[4*b+2] = q[4*b+3] = 0;
            }
            hs_push_vo(h, mask.data(), tp.data(), tn.data(), dp.data(), tn.data(), q.data());
        }
        if (i % 2 == 0) {
            const int T = i / 5;
            for (int b = 0; b < B; ++b) {
                t[b] = 0.001 * i + 1e-5 * b;
                acc[3*b] = 0.1; acc[3*b+1] = -0.05; acc[3*b+2] = 9.8; gy[3*b] = 0.01; gy[3*b+1] = 0.02; gy[3*b+2] = 0.2;
                for (int k = 0; k < 3 * L; ++k) pf[3*L*b + k] = 0.1 * (k % 3) - 0.25;
                for (int k = 0; k < 3 * L * nj; ++k) J[3*L*nj*b + k] = (k % (nj + 1) == 0) ? 0.2 : 0.03 * ((k + T) % 5);
                for (int k = 0; k < L * nj; ++k) qd[L*nj*b + k] = 0.1 * ((k + T) % 7) - 0.3;
                for (int k = 0; k < L; ++k) c[L*b + k] = ((T / 5 + k) % 2) ? 1.0 : 0.0;
            }
            hs_push_imu(h, t.data(), acc.data(), gy.data());
            hs_push_leg(h, pf.data(), J.data(), qd.data(), c.data());
            hs_ekf_step_epoch(h, e);
        }
        if (i % 5) continue;
        const int T = i / 5;
        xw.assign((size_t)B * N * ns, -7.0);
        cw.assign((size_t)B * N * ns * ns, -7.0);
        l1.assign((size_t)B * (N - 1) * ns * ns, -7.0);
        zn.assign((size_t)B * N * ns * ns, -7.0);
        hs_update_direct_cross_epoch(h, e, T, cov.data(), xw.data(), cw.data(), l1.data(), zn.data());
        hs_instance_ticks(e, T, ticks.data());
        for (int b = 0; b < B; ++b) {
            const int K = ticks[b] < 1 ? 0 : (ticks[b] + 1 < N ? ticks[b] + 1 : N);
            for (int k = 0; k < N; ++k) {
                for (int j = 0; j < ns; ++j) { const double v = xw[((size_t)b * N + k) * ns + j]; bad += k < K ? !std::isfinite(v) : v != -7.0; }
                for (int j = 0; j < ns * ns; ++j) {
                    const double v = cw[((size_t)b * N + k) * ns * ns + j], z = zn[((size_t)b * N + k) * ns * ns + j];
                    bad += k < K ? !std::isfinite(v) : v != -7.0;
                    bad += k < K ? !std::isfinite(z) : z != -7.0;
                    if (k < N - 1) { const double w = l1[((size_t)b * (N - 1) + k) * ns * ns + j]; bad += k < K - 1 ? !std::isfinite(w) : w != -7.0; }
                }
            }
            for (int j = 0; j < ns * ns; ++j) bad += K ? !std::isfinite(cov[(size_t)b * ns * ns + j]) : !std::isnan(cov[(size_t)b * ns * ns + j]);
        }
    }
    std::vector<double> x(ns * B); std::vector<int> st(B);
    hs_get(h, x.data(), nullptr, nullptr, nullptr, st.data(), nullptr, nullptr);
    std::printf("two rates, L=%d nj=%d N=%d leg_odom_type=%d arrival_cost_form=%d: status %d %d %d ticks %d %d %d, %d bad entries\n", L, nj, N, ft, form,
                st[0], st[1], st[2], ticks[0], ticks[1], ticks[2], bad);
    const int T1 = ((last > 132 ? last : 132) + 4) / 5, T2 = (last + 4) / 5;   // (N = 6: ms 132 is instance 1's last restart)
    const bool ticks_ok = ticks[0] == steps - 1 && ticks[1] == steps - 1 - T1 && ticks[2] == steps - 1 - T2;
    hs_epochs_destroy(e);
    hs_destroy(h);
    return st[0] == 1 && st[1] == 1 && st[2] == 1 && bad == 0 && ticks_ok ? 0 : 2;
}
int main() {
    return run(4, 3, 20, 50, 0, 0) | run(4, 3, 20, 44, 1, 0) | run(2, 5, 6, 30, 1, 1) | run_two_rate(4, 3, 20, 40, 0, 0) | run_two_rate(2, 5, 6, 30, 1, 1);
}
"""


def test_epoch_cores_clean_under_asan_ubsan(tmp_path):
    """a stand-alone program over epoch_hostsim.cpp under AddressSanitizer + UBSan (CPU build, as direct_lib.check_clean_under_asan_ubsan
    builds its driver): restarts in the window fill and from full windows, Go1 and foot states (both arrival-cost forms); and the two
    rates on a 1 ms grid with restarts that are not aligned with an update, at a history of 8 samples"""
    src = tmp_path / "epoch_driver.cpp"
    src.write_text(ASAN_MAIN)
    exe = tmp_path / "epoch_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-DDEKF_HOSTSIM", "-w", "-I", DL.HOSTSIM, "-o", str(exe), str(src)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
