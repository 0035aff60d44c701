"""Noise parameters per instance of a direct handle (dekf_set_instance_params / dekf_get_instance_params, csrc/mhe_params_core.h) without a
GPU.

ABI: the two calls are declared, exported and bound, refuse a null handle and compile as C99, while the ABI version and dekf_params stay
what they were; the thirty _pp twins sit at their siblings' design point.
Core: the lane-sequential build of the parameter cores (tests/hostsim/params_hostsim.cpp) over 60-tick rough_streams logs: every
instance equals, to the bit, the same instance of the uniform harness (no table, no epochs) created with its set; a restarted instance
that takes a new set equals a fresh uniform run with that set on the sliced log; one run is held against the oracle with the sets'
parameters; the factored host derivation gives fill_cfg's doubles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import direct_lib as DL
import epoch_lib as EL
import instance_params_lib as PL
import tworate_lib as TL
from decentralized_ekf_mhe_amd import capi
from decentralized_ekf_mhe_amd.params import DekfParams

SYMBOLS = ("dekf_set_instance_params", "dekf_get_instance_params")
KEYS = EL.SIM_KEYS + ("pri_res", "dua_res")


# ------------------------------------------------------------------ 1: the C boundary
def test_header_declares_both_calls():
    hdr = DL.header()
    assert re.search(r"dekf_status\s+dekf_set_instance_params\s*\(\s*dekf_handle\s+h\s*,\s*const\s+dekf_params\s*\*\s*sets\s*,\s*int\s+nsets\s*,"
                     r"\s*const\s+int\s*\*\s*set_of\s*\)\s*;", hdr)
    assert re.search(r"dekf_status\s+dekf_get_instance_params\s*\(\s*dekf_handle\s+h\s*,\s*int\s+b\s*,\s*dekf_params\s*\*\s*out\s*\)\s*;", hdr)
    assert re.search(r"#define\s+DEKF_ABI_VERSION\s+4\b", hdr)
    for f in PL.NOISE_FIELDS:      # the header lists every per-instance field
        assert re.search(r"\b" + f + r"\b", hdr.split("noise parameters per instance")[1]), f


def test_library_exports_and_binding_lists_them():
    DL.check_exports_and_binding(SYMBOLS)
    assert capi.PROTOTYPES["dekf_set_instance_params"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p])
    assert capi.PROTOTYPES["dekf_get_instance_params"] == (C.c_int, [C.c_void_p, C.c_int, C.POINTER(DekfParams)])


def test_abi_version_and_params_layout_unchanged():
    DL.check_abi_version_and_params_layout()


def test_null_handle_is_invalid():
    lib = capi.load()
    p = DekfParams()
    lib.dekf_default_params(C.byref(p))
    before = bytes(p)
    so = (C.c_int * 2)(0, 0)
    assert lib.dekf_set_instance_params(None, C.cast(C.byref(p), C.c_void_p), 1, C.cast(so, C.c_void_p)) == capi.DEKF_ERR_INVALID
    assert lib.dekf_set_instance_params(None, None, 0, None) == capi.DEKF_ERR_INVALID
    assert lib.dekf_get_instance_params(None, 0, C.byref(p)) == capi.DEKF_ERR_INVALID
    assert bytes(p) == before


def test_header_compiles_as_c99_with_the_parameter_calls(tmp_path):
    DL.check_c99_client(tmp_path, "params_client",
                        "    dekf_params p;\n    int set_of[2] = {0, -1};\n"
                        "    dekf_status a, b;\n"
                        "    dekf_default_params(&p);\n"
                        "    a = dekf_set_instance_params((dekf_handle)0, &p, 1, set_of);\n"
                        "    b = dekf_get_instance_params((dekf_handle)0, 0, &p);\n"
                        '    printf("set %d get %d N %d abi %d\\n", (int)a, (int)b, p.N, DEKF_ABI_VERSION);\n',
                        f"set {capi.DEKF_ERR_INVALID} get {capi.DEKF_ERR_INVALID} N 20 abi 4")


# ------------------------------------------------------------------ 2: the parameter sets
@pytest.mark.parametrize("name", list(PL.CPU_SHAPES))
def test_sets_change_every_noise_field_and_nothing_else(name):
    p, _ = PL.cpu_streams(name)
    s0, s1, s2 = PL.param_sets(p)
    assert bytes(s0) == bytes(p)
    for a, b in ((s0, s1), (s0, s2), (s1, s2)):
        assert sorted(PL.changed_fields(a, b)) == sorted(PL.NOISE_FIELDS)
    for k, sk in ((1, s1), (2, s2)):
        for f in PL.NOISE_FIELDS[:-1]:
            r = np.array(list(getattr(sk, f))) / np.array(list(getattr(s0, f)))
            assert ((r >= 0.25) & (r <= 4.0)).all(), (k, f, r)
        assert abs(np.linalg.norm(list(sk.ekf_quaternion_init)) - 1.0) < 1e-15


@pytest.mark.parametrize("name", list(PL.CPU_SHAPES))
def test_uniform_runs_solve_every_tick_and_differ_between_sets(name):
    """the conditions on the sets: every tick of every uniform run ends DEKF_SOLVE_OK, and the runs of any two sets differ in x_mhe, in
    the EKF quaternion and in Cov(x_T) on the same log"""
    uni = [PL.cpu_uniform(name, "plain", k) for k in range(3)]
    for k in range(3):
        assert all((r["status"] == capi.DEKF_SOLVE_OK).all() for r in uni[k][1:]), k
    for a, b in ((0, 1), (0, 2), (1, 2)):
        for key in ("x", "quat", "cov"):
            assert not np.array_equal(uni[a][-1][key], uni[b][-1][key]), (a, b, key)


# ------------------------------------------------------------------ 3: the parameter cores, lane-sequential
@pytest.mark.parametrize("variant", list(DL.VARIANTS))
@pytest.mark.parametrize("name", list(PL.CPU_SHAPES))
def test_every_instance_is_the_uniform_run_with_its_set(name, variant):
    _, B, set_of = PL.CPU_SHAPES[name]
    p, s = PL.cpu_streams(name)
    got = PL.run_params_sim(p, s, B, PL.K_LOG, variant, PL.param_sets(p), set_of)
    for b in range(B):
        EL.assert_life_equal(got, PL.cpu_uniform(name, variant, set_of[b]), b, 0, PL.K_LOG, p.N, KEYS, "set %d" % set_of[b])
    assert all((r["status"] == capi.DEKF_SOLVE_OK).all() for r in got[1:])


def test_minus_one_leaves_an_instance_and_a_second_call_overrides_what_it_names():
    name, variant = "go1", "plain"
    _, B, _ = PL.CPU_SHAPES[name]
    p, s = PL.cpu_streams(name)
    sets = PL.param_sets(p)
    sim = PL.ParamsSim(p, B, variant)
    assert sim.set_params(sets, [1, -1, 2]) == 0      # instance 1 stays on the handle's own set (set 0)
    assert sim.set_params(sets, [-1, -1, 1]) == 0     # instance 2 again, instance 0 keeps set 1
    out = []
    for k in range(30):
        sim.feed(s, k)
        sim.step(k)
        out.append(dict(EL._record(sim, sim.cov), ticks=sim.ticks(k)))
    for b, k in enumerate([1, 0, 1]):
        EL.assert_life_equal(out, PL.cpu_uniform(name, variant, k), b, 0, 30, p.N, KEYS, "set %d" % k)


def test_a_set_that_differs_in_another_field_is_refused():
    """same_but_noise (host_common.h), which dekf_set_instance_params applies to every set: a change of ANY field that is not a noise
    field is refused, a change of any noise field accepted; and fill_cfg's positivity of the foot stds holds for every set"""
    p = DL._params(PL.go1_params, leg_odom_type=1)
    sim = PL.ParamsSim(p, 1)
    for f, _ in DekfParams._fields_:
        q = p.copy()
        v = getattr(q, f)
        if hasattr(v, "__len__"):
            v[len(v) - 1] = v[len(v) - 1] * 1.5 + 0.125
        else:
            setattr(q, f, v + 1)
        assert PL.changed_fields(p, q) == [f]
        assert sim.set_params([q], [0]) == (0 if f in PL.NOISE_FIELDS else 1), f
    for f in ("foot_slide_std", "foot_init_std", "foot_swing_std"):
        q = p.copy()
        getattr(q, f)[1] = 0.0
        assert sim.set_params([q], [0]) == 1, f


# ------------------------------------------------------------------ 4: restart with a new set
@pytest.mark.parametrize("variant", ["plain", "cross"])
def test_restarted_instance_with_a_new_set_is_a_fresh_run_with_that_set(variant):
    """epoch_lib's Go1 schedule on the 60-tick log: instance 1 restarted before ticks 5 and 12 and instance 0 before tick 45 keep
    their sets; instance 2, restarted before tick 30, takes a NEW set (2 for 1).  Every life equals the fresh uniform run with its
    set on the log sliced from its restart; until its first restart an instance is the uniform run with its first set"""
    name = "go1"
    _, B, set_of = PL.CPU_SHAPES[name]
    p, s = PL.cpu_streams(name)
    resets, K = EL.CPU_RESETS[name], PL.K_LOG
    got = PL.run_params_sim(p, s, B, K, variant, PL.param_sets(p), set_of, resets, {30: {2: 2}})
    now = {0: set_of[0], 1: set_of[1], 2: 2}
    assert set_of[2] != 2
    for b in range(B):
        first = min(T0 for T0 in resets if b in resets[T0])
        EL.assert_life_equal(got, PL.cpu_uniform(name, variant, set_of[b]), b, 0, first, p.N, KEYS, "untouched")
    lives = EL.lives(resets, K)
    assert len(lives) == 4
    for b, T0, end in lives:
        EL.assert_life_equal(got, PL.cpu_uniform(name, variant, now[b], T0), b, T0, end, p.N, KEYS, "life")
        assert (got[T0]["status"][b], got[T0]["ticks"][b]) == (capi.DEKF_SOLVE_NONE, 0)
        assert got[end - 1]["status"][b] == capi.DEKF_SOLVE_OK


def test_two_rate_restarted_instances_take_another_set():
    """tworate_lib's event grid and schedule (EKF 500 Hz, MHE 200 Hz: the two epochs of a restart differ) at ekf_history 16, Go1
    cross, B = 4 on the table SET_OF: every restarted instance takes ANOTHER set at its restart and equals, to the bit, a fresh
    uniform simulation created with that set and started at the restart's ms; until its first restart an instance is the uniform
    run with its first set, the untouched instance throughout"""
    name, H, B, variant = "go1", 16, 4, "cross"
    p, s, n_grid = TL.streams(name, H, B)
    set_of = TL.SET_OF[:B]
    got = TL.run_params_sim(name, H, B, variant, set_of, TL.RESETS, TL.NEW_SETS)
    for b in range(B):
        first = min([g for g in TL.RESETS if b in TL.RESETS[g]] + [n_grid])
        TL.assert_life_equal(got, TL.cpu_fresh(name, H, B, variant, 0, set_of[b]), b, 0, first, p.N, KEYS, "untouched")
    now = dict(enumerate(set_of))
    lives = TL.lives(TL.RESETS, n_grid)
    assert len(lives) == 6 and sum(len(TL.straddling_poses(s, b, g0, g_end)) for b, g0, g_end in lives) >= 1
    for b, g0, g_end in lives:       # (in the order of the restarts)
        k = TL.NEW_SETS[g0][b]
        assert k != now[b]
        now[b] = k
        TL.assert_life_equal(got, TL.cpu_fresh(name, H, B, variant, g0, k), b, g0, g_end, p.N, KEYS, "life on set %d" % k)
        T0 = TL.first_step(g0)
        assert (got[T0]["t0"][b], got[T0]["c0"][b]) == (T0, TL.ekf_ticks(0, g0)) and got[T0]["c0"][b] != got[T0]["t0"][b]
        assert (got[T0]["status"][b], got[T0]["ticks"][b]) == (capi.DEKF_SOLVE_NONE, 0)
        assert got[T0 + TL.steps_of(g0, g_end) - 1]["status"][b] == capi.DEKF_SOLVE_OK
    assert max(TL.ekf_ticks(g0, g_end) for _, g0, g_end in lives) >= 2 * H
    # the sets matter on this grid: the life of instance 1 from ms 132 differs from the default set's in x, the quaternion and Cov(x_T)
    a, c = TL.cpu_fresh(name, H, B, variant, 226, 1), TL.cpu_fresh(name, H, B, variant, 226, 2)
    for key in ("x", "quat", "cov"):
        assert not np.array_equal(a[-1][key], c[-1][key]), key


# ------------------------------------------------------------------ 5: against the oracle
@pytest.mark.parametrize("b", [0, 2])
def test_instance_against_the_oracle_with_its_set(b):
    """Go1, B = 3, set_of = [2, 0, 1]: an instance on a non-default set against the exact optimum of the oracle's window QP and the
    inverse of its KKT matrix, the oracle run with THAT set's parameters: x within XREL / XABS and the covariances within CREL of
    direct_lib.  The even instances carry the 30 Hz camera: their windows hold VO equality rows from tick 40"""
    name = "go1"
    _, B, set_of = PL.CPU_SHAPES[name]
    p, s = PL.cpu_streams(name)
    ns, N, ticks = p.dim_state, p.N, [1, 19, 20, 40, 54]
    assert set_of[b] != 0 and b % 2 == 0
    got = PL.run_params_sim(p, s, B, PL.K_LOG, "cross", PL.param_sets(p), set_of)
    worst_x, worst_c, worst_w, worst_wc, worst_1, worst_n, vo = 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, {}
    for j, x, Ki, xo, nv in DL.kkt_reference(PL.param_set(p, set_of[b]), s, b, set(ticks)):
        g = got[j]
        Kb = min(j + 1, N)
        assert g["status"][b] == capi.DEKF_SOLVE_OK and len(xo) == Kb
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
    print(f"[instance {b}, set {set_of[b]}] x_T {worst_x:.3g} x (1e-8 rel + 1e-10), Cov(x_T) {worst_c:.3g}; window x {worst_w:.3g} x, "
          f"cov {worst_wc:.3g}; lag-one {worst_1:.3g}, to-newest {worst_n:.3g}; VO equality rows by tick: {vo}")
    assert sorted(vo) == ticks
    assert vo[40] > 0 and vo[54] > 0, "the windows at ticks 40 and 54 hold no VO equality row"
    assert worst_x <= 1.0 and worst_w <= 1.0
    assert max(worst_c, worst_wc, worst_1, worst_n) <= DL.CREL


# ------------------------------------------------------------------ 6: the host derivation
@pytest.mark.parametrize("name", list(PL.CPU_SHAPES))
def test_fill_noise_gives_fill_cfgs_doubles(name):
    """fill_cfg on the handle's parameters followed by fill_noise on a set (what dekf_set_instance_params puts into the tables) is, byte
    for byte, the DevCfg fill_cfg gives for a handle created with the set"""
    L = PL.params_hostsim()
    p, _ = PL.cpu_streams(name)
    a, b = (C.c_ubyte * 4096)(), (C.c_ubyte * 4096)()
    for k, q in enumerate(PL.param_sets(p)):
        n = L.hs_cfg_bytes(C.byref(p), C.byref(q), 5, 0, a)
        assert 0 < n <= 4096 and L.hs_cfg_bytes(C.byref(p), C.byref(q), 5, 1, b) == n
        assert bytes(a)[:n] == bytes(b)[:n], k
        if k:
            L.hs_cfg_bytes(C.byref(p), C.byref(p), 5, 0, b)
            assert bytes(a)[:n] != bytes(b)[:n]
    assert L.hs_ekf_table_len() == 18


# ------------------------------------------------------------------ 7: resource remarks
@pytest.mark.parametrize("variant", list(DL.VARIANTS))
def test_parameter_twins_at_their_siblings_design_point(variant):
    """every direct kernel's _pp twin against the epoch twin it extends: no spills, no scratch, no static LDS, an occupancy class not
    below the sibling's (or still above what the kernel's LDS admits)"""
    DL.check_twins_at_their_design_point(EL.TWIN_SUFFIX[variant], PL.TWIN_SUFFIX[variant])
    table, _ = DL.usage_table()
    for n, _, _ in DL.KERNELS:
        t, u = table[n + PL.TWIN_SUFFIX[variant]], table[n + EL.TWIN_SUFFIX[variant]]
        assert -(-t["vgprs"] // 8) <= -(-u["vgprs"] // 8), (n, t, u)      # the sibling's VGPR class (granule 8): the table costs scalar registers


# ------------------------------------------------------------------ 8: sanitizers
ASAN_MAIN = r"""
#include "params_hostsim.cpp"
#include <cmath>
#include <cstdio>
// synthetic sensors as direct_lib.ASAN_DRIVER's, VO on every sixth step; B = 3 on three sets (instance 1 on the Sim's own), instance 1
// restarted in its window fill (before tick 5) and, with instance 2, from full windows (before tick N + 9), instance 2 then on a new set
static int run(int L, int nj, int N, int steps, int ft, int form) {
    dekf_params p; default_params(&p); p.ekf_rate = 200; p.num_legs = L; p.joints_per_leg = nj; p.N = N; p.leg_odom_type = ft; p.arrival_cost_form = form;
    dekf_params sets[2] = {p, p};
    for (int i = 0; i < 3; ++i) { sets[0].accel_bias_std[i] *= 2.0; sets[0].vo_p_std[i] *= 0.5; sets[0].ekf_process_std[i] *= 3.0; sets[0].foot_slide_std[i] *= 2.0; }
    for (int i = 0; i < nj; ++i) { sets[1].joint_velocity_std[i] *= 0.5 + 0.25 * i; sets[1].joint_position_std[i] *= 1.5; }
    for (int i = 0; i < 4; ++i) sets[1].ekf_init_std[i] *= 2.0;
    const int ns = 9 + 3 * L * ft, B = 3;
    void* h = hs_create(&p, B);
    if (!h) return 1;
    void* e = hs_epochs_create(B);
    void* tb = hs_tables_create(h);
    { const int so[3] = {0, -1, 1}; if (hs_set_instance_params(h, tb, &p, sets, 2, so)) return 1; }
    std::vector<double> t(B), acc(3 * B), gy(3 * B), pf(3 * L * B), J(3 * L * nj * B), qd(L * nj * B), c(L * B), cov((size_t)B * ns * ns, NAN);
    std::vector<int> mask(B, 1), ticks(B); std::vector<double> tp(B), tn(B), dp(3 * B), q(4 * B);
    std::vector<double> xw, cw, l1, zn;
    int bad = 0;
    for (int T = 0; T < steps; ++T) {
        if (T == 5) { const int m[3] = {0, 1, 0}; hs_reset_instances_pp(h, e, tb, m, cov.data()); }
        if (T == N + 9) {
            const int m[3] = {0, 1, 1}, so[3] = {-1, -1, 0};
            hs_reset_instances_pp(h, e, tb, m, cov.data());
            if (hs_set_instance_params(h, tb, &p, sets, 2, so)) return 1;
        }
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
        hs_ekf_step_pp(h, e, tb);
        // the four window buffers at exactly their contract sizes, the guard behind every instance's K_b written entries checked
        xw.assign((size_t)B * N * ns, -7.0);
        cw.assign((size_t)B * N * ns * ns, -7.0);
        l1.assign((size_t)B * (N - 1) * ns * ns, -7.0);
        zn.assign((size_t)B * N * ns * ns, -7.0);
        hs_update_direct_cross_pp(h, e, tb, T, cov.data(), xw.data(), cw.data(), l1.data(), zn.data());
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
    hs_tables_destroy(tb);
    hs_epochs_destroy(e);
    hs_destroy(h);
    return st[0] == 1 && st[1] == 1 && st[2] == 1 && bad == 0 && ticks_ok ? 0 : 2;
}
// (Go1 with foot states in covariance form: 34 steps as in direct_lib.ASAN_DRIVER.  On these synthetic sensors that form loses
// definiteness at steps 35 to 39 once a noise constant moves, in the uniform harness created with the set just the same)
int main() { return run(4, 3, 20, 50, 0, 0) | run(4, 3, 20, 34, 1, 0) | run(2, 5, 6, 30, 1, 1); }
"""


def test_parameter_cores_clean_under_asan_ubsan(tmp_path):
    """a stand-alone program over params_hostsim.cpp under AddressSanitizer + UBSan (CPU build, with the compile line and options of
    direct_lib.check_clean_under_asan_ubsan, whose driver is tied to direct_hostsim.cpp): a table, restarts in the window fill and from
    full windows, a new set for a restarted instance, Go1 and foot states (both arrival-cost forms)"""
    src = tmp_path / "params_driver.cpp"
    src.write_text(ASAN_MAIN)
    exe = tmp_path / "params_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-DDEKF_HOSTSIM", "-w", "-I", DL.HOSTSIM, "-o", str(exe), str(src)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
