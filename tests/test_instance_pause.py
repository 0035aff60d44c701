"""Pausing single instances of a direct handle (dekf_set_active / dekf_get_active, csrc/mhe_pause_core.h) without a GPU.

ABI: the two calls are declared, exported and bound, refuse a null handle and compile as C99, while the ABI version and dekf_params
stay what they were.
Core: the lane-sequential build of the pause cores (tests/hostsim/pause_hostsim.cpp) over 100-tick rough_streams logs under
pause_lib.cpu_schedule: every life of every instance equals, to the bit, a simulation WITHOUT this interface (direct_lib.DirectSim) of
the log cut down to the ticks at which the instance ran; while it is paused every output keeps its bits; an instance that is never
named equals the run without pauses.  The conditions on the reference (DEKF_SOLVE_OK on every compared tick, VO equality rows in a
compared window behind a resume) are asserted on the reference alone.
Arithmetic: a pause, folds of the handle's EKF tick count while paused, and the resume, around the history depth H.
Resources: the new kernels against their siblings, every other kernel against the table of the commit before this interface."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import direct_lib as DL
import epoch_lib as EL
import pause_lib as PZ
import tworate_lib as TL
from decentralized_ekf_mhe_amd import capi

SYMBOLS = ("dekf_set_active", "dekf_get_active")


# ------------------------------------------------------------------ 1: the C boundary
def test_header_declares_both_calls():
    hdr = DL.header()
    assert re.search(r"dekf_status\s+dekf_set_active\s*\(\s*dekf_handle\s+h\s*,\s*const\s+int\s*\*\s*active\s*,\s*dekf_mem\s+where\s*\)\s*;", hdr)
    assert re.search(r"dekf_status\s+dekf_get_active\s*\(\s*dekf_handle\s+h\s*,\s*int\s*\*\s*active\s*,\s*dekf_mem\s+where\s*\)\s*;", hdr)
    assert re.search(r"#define\s+DEKF_ABI_VERSION\s+4\b", hdr)
    assert "switched off" not in hdr.replace("switched off: dekf_set_active", "")   # struck from the lists of what is not offered


def test_library_exports_and_binding_lists_them():
    DL.check_exports_and_binding(SYMBOLS)
    for name in SYMBOLS:
        assert capi.PROTOTYPES[name] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int])


def test_abi_version_and_params_layout_unchanged():
    DL.check_abi_version_and_params_layout()


def test_null_handle_is_invalid():
    lib = capi.load()
    m = (C.c_int * 4)(1, 0, 1, 1)
    a = (C.c_int * 4)(-7, -7, -7, -7)
    for where in (capi.DEKF_HOST, capi.DEKF_DEVICE):
        assert lib.dekf_set_active(None, C.cast(m, C.c_void_p), where) == capi.DEKF_ERR_INVALID
        assert lib.dekf_get_active(None, C.cast(a, C.c_void_p), where) == capi.DEKF_ERR_INVALID
    assert list(a) == [-7] * 4


def test_header_compiles_as_c99_with_the_pause_calls(tmp_path):
    DL.check_c99_client(tmp_path, "pause_client",
                        "    int mask[2] = {1, 0}, active[2] = {-7, -7};\n"
                        "    dekf_status a = dekf_set_active((dekf_handle)0, mask, DEKF_HOST);\n"
                        "    dekf_status b = dekf_get_active((dekf_handle)0, active, DEKF_HOST);\n"
                        '    printf("set %d get %d first %d abi %d\\n", (int)a, (int)b, active[0], DEKF_ABI_VERSION);\n',
                        f"set {capi.DEKF_ERR_INVALID} get {capi.DEKF_ERR_INVALID} first -7 abi 4")


# ------------------------------------------------------------------ 2: the pause cores, lane-sequential
def _run(name, variant, stray=False):
    mk, B = PZ.CPU_SHAPES[name]
    p, s = PZ.cpu_streams(name)
    return p, s, B, PZ.run_pause_sim(p, s, B, PZ.K_LOG, variant, PZ.cpu_schedule(B), stray)


@pytest.mark.parametrize("variant", list(DL.VARIANTS))
@pytest.mark.parametrize("name", list(PZ.CPU_SHAPES))
def test_every_life_is_a_simulation_of_the_cut_log(name, variant):
    """x, v_b, quaternion, p_vo, status, solver info, the EKF covariance, Cov(x_T), the arrival cost and the first K_b window and cross
    entries, array_equal, at every tick an instance ran; frozen bits at every tick it did not"""
    p, s, B, got = _run(name, variant)
    K, N = PZ.K_LOG, p.N
    lives = PZ.check_against_cut_logs(got, lambda life: PZ.cpu_fresh(name, variant, life), PZ.cpu_schedule(B), B, K, N, PZ.SIM_KEYS, name)
    by = {b: [life for bb, life in lives if bb == b] for b in range(B)}
    # instance 1: its first life runs over both pauses (inside the fill; from the fill into full windows) up to tick 59; restarted
    # while paused, it is a fresh run on the log from tick 66; restarted and paused in one gap, a fresh run from its resume at tick 84
    first = tuple(k for k in range(60) if not (5 <= k < 9 or 14 <= k < 27))
    assert by[1] == [first, tuple(range(66, 80)), tuple(range(84, K))]
    assert got[8]["ticks"][1] == 4 and got[9]["ticks"][1] == 5 < N - 1           # paused and resumed inside the window fill
    assert got[26]["ticks"][1] == 9 < N - 1 <= got[26]["ticks"][0] == 26           # the handle has full windows, the instance has not
    assert got[59]["ticks"][1] == len(first) - 1 >= N - 1                        # ... and went on into full windows
    assert [got[k]["ticks"][1] for k in (65, 66, 79, 80, 83, 84)] == [len(first) - 1, 0, 13, -1, -1, 0]
    assert got[84]["status"][1] == capi.DEKF_SOLVE_NONE and got[85]["status"][1] == capi.DEKF_SOLVE_OK
    assert (got[84]["t0"][1], got[84]["c0"][1]) == (84, 84)
    # instance 0: one life, paused from and into full windows, and never resumed from tick 90 on: frozen bits to the end
    assert by[0] == [tuple(k for k in range(90) if not 50 <= k < 58)]
    assert got[57]["ticks"][0] == 49 and got[58]["ticks"][0] == 50 and got[K - 1]["ticks"][0] == 81
    assert got[K - 1]["active"].tolist()[:2] == [0, 1]
    sentinel = PZ.pause_hostsim().hs_epoch_paused_sentinel()
    assert got[K - 1]["t0"][0] == got[K - 1]["c0"][0] == sentinel == 2 ** 31 - 2 ** 16
    # an instance whose mask entry never changes: the run without pauses, at every tick
    for b in range(2, B):
        assert by[b] == [tuple(range(K))]


@pytest.mark.parametrize("name", list(PZ.CPU_SHAPES))
def test_reference_windows_behind_the_resume_hold_vo_equality_rows(name):
    """a condition on the reference alone (the oracle on the cut log): the windows that instance 0's reference solves behind the resume
    of tick 58 hold VO equality rows.  (Its own tick 50 stands where the log's tick 58 does)"""
    p, s = PZ.cpu_streams(name)
    life = tuple(k for k in range(90) if not 50 <= k < 58)
    nv = PZ.vo_equality_rows(p, s, 0, life, 52)
    print(f"{name}: {nv} VO equality rows in the reference's window at its tick 52")
    assert nv > 0


def test_vo_pushed_for_a_paused_instance_changes_nothing():
    """a VO sample (interval and orientation pose) pushed for the paused instances at every tick of every pause: the run's bits at every
    tick, of every instance, are those of the run without the stray samples"""
    _, _, B, clean = _run("go1", "cross")
    _, _, _, got = _run("go1", "cross", stray=True)
    for k in range(PZ.K_LOG):
        for key in clean[k]:
            assert np.array_equal(got[k][key], clean[k][key], equal_nan=True), (k, key)


def test_an_unchanged_mask_changes_nothing():
    mk, B = PZ.CPU_SHAPES["go1"]
    p, s = PZ.cpu_streams("go1")
    sim = PZ.PauseSim(p, B, "plain")
    for k in range(3):
        sim.feed(s, k)
        sim.step(k)
    assert sim.set_active([1] * B) == 0 and sim.epochs()[0].tolist() == [0] * B
    assert sim.set_active([1, 0, 1]) == 1 and sim.set_active([1, 0, 1]) == 0
    assert sim.active().tolist() == [1, 0, 1] and sim.ticks(2).tolist() == [2, 2, 2]


# ------------------------------------------------------------------ 3: the arithmetic around the history depth and across a fold
@pytest.mark.parametrize("H", [4, 7, 16, 256])
def test_pause_and_resume_keep_the_local_count_around_the_history_depth_and_across_a_fold(H):
    """what ekf_tick takes from its count is the value modulo H and whether it has reached H.  An instance paused at a local count
    around H keeps both over the pause, whatever the handle counts meanwhile and however often it folds its count; the sentinel on
    the device survives the fold; the epoch of the resume stays within 2 H of the handle's count"""
    L = PZ.pause_hostsim()
    sentinel = L.hs_epoch_paused_sentinel()
    out = (C.c_int * 4)()
    for c0 in (0, 37, -(H - 1)):
        for local in (0, 1, H - 1, H, H + 1, 2 * H + 3, 12345, (1 << 30) - 50):
            if c0 + local < 0:     # (a negative epoch is a folded one: the handle's count is H or more)
                continue
            for later, folds in ((c0 + local + 9, 0), (1 << 30, 1), (1 << 30, 2)):
                L.hs_pause_fold_resume(c0, c0 + local, later, folds, H, out)
                dev_c0, stored, now, new_c0 = list(out)
                after = now - new_c0
                assert dev_c0 == sentinel and stored == local, (H, c0, local, folds)
                assert after % H == local % H and (after >= H) == (local >= H), (H, c0, local, folds, after)
                assert 0 <= after < 2 * H or after == local, (H, c0, local, after)
                if local < H:
                    assert after == local
                assert -2 * H < new_c0 <= now


# ------------------------------------------------------------------ 4: the two rates (EKF 500 Hz, MHE 200 Hz)
@pytest.mark.parametrize("name,H", [("go1", 256), ("go1", 16)])
def test_two_rate_pauses_against_the_cut_grid(name, H):
    """tworate_lib's event grid, variant cross, B = 4.  2 or 3 EKF ticks lie between two updates, so the two stored clocks of a pause
    differ; at ekf_history 16 the handle's ticks wrap the rewind ring during instance 1's pause"""
    B, variant = 4, "cross"
    p0 = TL.SHAPES[name](H)
    p, s, got, refs, pauses = PZ.two_rate_run(name, H, B, lambda: PZ.PauseDev(PZ.PauseSim(p0, B, variant)),
                                              lambda: TL.SimDev(DL.DirectSim(p0, B, variant)))
    assert (p.ekf_rate, p.rate, p.ekf_history) == (500, 200, H)
    PZ.check_two_rate(p, got, refs, TL.cpu_fresh(name, H, B, variant), pauses, B, PZ.SIM_KEYS)
    (_, a0, r0), (_, a1, r1), _ = pauses
    # instance 0 ticked at ms 62 and then stood still: 32 EKF ticks and 13 updates behind it at the pause, the same at the resume
    T_resume = TL.first_step(r0)
    assert got[12]["ticks"][0] == 12 == got[T_resume - 1]["ticks"][0] and got[T_resume]["ticks"][0] == 13
    # (a stored count of H or more comes back as H + count % H: all that ekf_tick takes from it)
    assert got[T_resume]["t0"][0] == T_resume - 13 and got[T_resume]["c0"][0] == TL.ekf_ticks(0, r0) - (32 if H > 32 else H + 32 % H)
    assert got[T_resume]["t0"][0] != got[T_resume]["c0"][0]
    # the pose that arrives at the ms of the resume was stamped while the instance was paused, and is not dropped
    assert s["vo_mask"][r0, 0] and s["imu_t"][a0 + 1, 0] <= s["vo_t_pose"][r0, 0] < s["imu_t"][r0 - 1, 0]
    assert H > 16 or TL.ekf_ticks(a1, r1) >= H


# ------------------------------------------------------------------ 5: resource remarks
NEW_KERNELS = {"k_ekf_tick_act": "k_ekf_tick_ep", "k_ekf_tick_act_pp": "k_ekf_tick_pp", "k_mhe_assemble_act": "k_mhe_assemble_ep",
               "k_mhe_assemble_act_pp": "k_mhe_assemble_pp", "k_latch_vo_act": "k_latch_vo", "k_fold_epochs_act": "k_fold_epochs"}
BEFORE = os.path.join(DL.ROOT, "tests", "golden", "resource_usage_before_pause.json")


def test_new_kernels_have_no_scratch_beyond_their_siblings():
    table, static_lds = DL.usage_table()
    for new, sibling in NEW_KERNELS.items():
        assert new in table and sibling in table, new
        n, u = table[new], table[sibling]
        print(new, n, "sibling", u)
        assert n["scratch"] <= u["scratch"] and n["spill"] <= u["spill"] and n["occupancy"] >= u["occupancy"], (new, n, u)
        assert static_lds[new] == static_lds[sibling], (new, static_lds[new], static_lds[sibling])


def test_every_kernel_from_before_keeps_its_entry():
    """the compiler's account of every kernel of the commit before this interface (tests/golden/resource_usage_before_pause.json:
    test_resource_usage.parse_usage of that build's libdekf_resource_usage.txt) against this build's: the same names with the same
    registers, spills, scratch and occupancy, and nothing added but the six kernels above"""
    table, _ = DL.usage_table()
    before = json.load(open(BEFORE))
    assert len(before) > 200
    moved = {k: (before[k], table.get(k)) for k in before if table.get(k) != before[k]}
    assert not moved, moved
    assert sorted(set(table) - set(before)) == sorted(NEW_KERNELS)


# ------------------------------------------------------------------ 6: sanitizers
ASAN_MAIN = r"""
#include "pause_hostsim.cpp"
#include <cmath>
#include <cstdio>
// synthetic sensors as test_instance_reset.ASAN_MAIN's, VO on every sixth step for every instance (paused ones included: dropped).
// B = 3: instance 1 paused over ticks 5 .. 8 (inside its fill) and from tick N + 8 on (full windows), restarted while paused before
// tick N + 12; instance 2 restarted and paused in one gap before tick 7, resumed before tick 11, paused for good before tick steps - 4;
// instance 0 never named.  The books are checked against the ticks the schedule implies
static int run(int L, int nj, int N, int steps, int ft, int form) {
    dekf_params p; default_params(&p); p.ekf_rate = 200; p.num_legs = L; p.joints_per_leg = nj; p.N = N; p.leg_odom_type = ft; p.arrival_cost_form = form;
    const int ns = 9 + 3 * L * ft, B = 3;
    void* h = hs_create(&p, B);
    if (!h) return 1;
    void* e = hs_epochs_create(B);
    void* z = hs_pauses_create(B);
    std::vector<double> t(B), acc(3 * B), gy(3 * B), pf(3 * L * B), J(3 * L * nj * B), qd(L * nj * B), c(L * B), cov((size_t)B * ns * ns, NAN);
    std::vector<int> mask(B, 1), ticks(B), act(B); std::vector<double> tp(B), tn(B), dp(3 * B), q(4 * B);
    std::vector<double> xw((size_t)B * N * ns, -7.0), cw((size_t)B * N * ns * ns, -7.0), l1((size_t)B * (N - 1) * ns * ns, -7.0), zn((size_t)B * N * ns * ns, -7.0);
    int bad = 0, ran[3] = {0, 0, 0};
    for (int T = 0; T < steps; ++T) {
        if (T == 5) { const int m[3] = {1, 0, 1}; hs_set_active(h, e, z, m); }
        if (T == 7) { const int r[3] = {0, 0, 1}; hs_reset_instances_pause(h, e, z, r, cov.data()); ran[2] = 0; const int m[3] = {1, 0, 0}; hs_set_active(h, e, z, m); }
        if (T == 9) { const int m[3] = {1, 1, 0}; hs_set_active(h, e, z, m); }
        if (T == 11) { const int m[3] = {1, 1, 1}; hs_set_active(h, e, z, m); }
        if (T == N + 8) { const int m[3] = {1, 0, 1}; hs_set_active(h, e, z, m); }
        if (T == N + 12) { const int r[3] = {0, 1, 0}; hs_reset_instances_pause(h, e, z, r, cov.data()); ran[1] = 0; }
        if (T == steps - 4) { const int m[3] = {1, 1, 0}; hs_set_active(h, e, z, m); }
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
        if (T > 8 && T % 6 == 0) hs_push_vo_pause(h, e, mask.data(), tp.data(), tn.data(), dp.data(), tn.data(), q.data());
        hs_ekf_step_pause(h, e);
        hs_update_direct_cross_pause(h, e, T, cov.data(), xw.data(), cw.data(), l1.data(), zn.data());
        hs_instance_ticks_pause(e, z, T, ticks.data());
        hs_get_active(z, act.data());
        for (int b = 0; b < B; ++b) {
            ran[b] += act[b];
            bad += ticks[b] != ran[b] - 1;
            // the persistent window stores: an instance's K_b entries finite, everything behind the largest K_b it ever had untouched
            const int K = ticks[b] < 1 ? 0 : (ticks[b] + 1 < N ? ticks[b] + 1 : N);
            for (int k = 0; k < K; ++k) {
                for (int i = 0; i < ns; ++i) bad += !std::isfinite(xw[((size_t)b * N + k) * ns + i]);
                for (int i = 0; i < ns * ns; ++i) {
                    bad += !std::isfinite(cw[((size_t)b * N + k) * ns * ns + i]) + !std::isfinite(zn[((size_t)b * N + k) * ns * ns + i]);
                    if (k < K - 1) bad += !std::isfinite(l1[((size_t)b * (N - 1) + k) * ns * ns + i]);
                }
            }
            for (int i = 0; i < ns * ns; ++i) bad += K ? !std::isfinite(cov[(size_t)b * ns * ns + i]) : !std::isnan(cov[(size_t)b * ns * ns + i]);
        }
    }
    std::vector<double> x(ns * B); std::vector<int> st(B);
    hs_get(h, x.data(), nullptr, nullptr, nullptr, st.data(), nullptr, nullptr);
    std::printf("L=%d nj=%d N=%d leg_odom_type=%d arrival_cost_form=%d: status %d %d %d ticks %d %d %d, %d bad entries\n", L, nj, N, ft, form,
                st[0], st[1], st[2], ticks[0], ticks[1], ticks[2], bad);
    const bool ticks_ok = ticks[0] == steps - 1 && ticks[1] == steps - 1 - (N + 12) && ticks[2] == steps - 4 - 11 - 1;
    hs_pauses_destroy(z);
    hs_epochs_destroy(e);
    hs_destroy(h);
    return st[0] == 1 && st[1] == 1 && st[2] == 1 && bad == 0 && ticks_ok ? 0 : 2;
}
int main() {
    int out[4];
    hs_pause_fold_resume(-7, 12352 - 7, 1 << 30, 2, 8, out);
    if (out[0] != hs_epoch_paused_sentinel() || out[1] != 12352 || (out[2] - out[3]) % 8 != 12352 % 8) return 3;
    return run(4, 3, 20, 50, 0, 0) | run(4, 3, 20, 44, 1, 0) | run(2, 5, 6, 30, 1, 1);
}
"""


def test_pause_cores_clean_under_asan_ubsan(tmp_path):
    """a stand-alone program over pause_hostsim.cpp under AddressSanitizer + UBSan (CPU build, run directly): pauses in the window fill
    and in full windows, a paused instance restarted, a restart and a pause in one gap, an instance never resumed; Go1 and foot states
    (both arrival-cost forms); the pause, fold and resume arithmetic"""
    src = tmp_path / "pause_driver.cpp"
    src.write_text(ASAN_MAIN)
    exe = tmp_path / "pause_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-DDEKF_HOSTSIM", "-w", "-I", DL.HOSTSIM, "-o", str(exe), str(src)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
