"""The window cross-covariances of the direct smoother (dekf_set_window_cross / dekf_get_window_cross, csrc/mhe_direct_core.h: CROSS)
without a GPU.

ABI: the two calls are declared, exported and bound, refuse a null handle and compile as C99, while the ABI version and dekf_params
stay what they were; the C++ shim compiles with robot_params::windowCross_; the ten _smooth_cross twins sit at their design point.
Core: the lane-sequential build of the CROSS instantiation (tests/hostsim/direct_hostsim.cpp: hs_update_direct_cross) on the records and
the input snapshot that the assemble step leaves: EVERY written block of cov_lag1 and cov_newest, every checked tick, against the
matching off-diagonal block of the inverse of the oracle QP's KKT matrix (direct_lib.cross_reference: window_reference's construction,
for every pair of window states), in units of sqrt(Cov(x_a)_ii Cov(x_b)_jj) and inside CREL; the two bit identities of the new arrays;
everything the SMOOTH core writes unchanged to the bit; without VO rows the Kalman smoother's cross-covariances."""
import ctypes as C
import re

import numpy as np
import pytest

from decentralized_ekf_mhe_amd import capi, cassie_params, go1_params
from decentralized_ekf_mhe_amd.estimator import relative_cov
from decentralized_ekf_mhe_amd.streams import make_streams
from direct_lib import (CORE_CASES, CREL, FILL, _params, build_shim, check_abi_version_and_params_layout, check_c99_client,
                        check_clean_under_asan_ubsan, check_exports_and_binding, check_shim_usage, check_twins_at_their_design_point,
                        cross_errors, cross_reference, header, own_arrival, rough_streams, run_direct_sim)

SYMBOLS = ("dekf_set_window_cross", "dekf_get_window_cross")


# ------------------------------------------------------------------ 1: the C boundary
def test_header_declares_both_calls():
    hdr = header()
    assert re.search(r"dekf_status\s+dekf_set_window_cross\s*\(\s*dekf_handle\s+h\s*,\s*int\s+on\s*\)\s*;", hdr)
    assert re.search(r"dekf_status\s+dekf_get_window_cross\s*\(\s*dekf_handle\s+h\s*,\s*int\s*\*\s*steps\s*,\s*double\s*\*\s*cov_lag1\s*,\s*"
                     r"double\s*\*\s*cov_newest\s*,\s*dekf_mem\s+where\s*\)\s*;", hdr)
    assert re.search(r"#define\s+DEKF_ABI_VERSION\s+4\b", hdr)
    assert "Not part of this interface: the lag-one" not in hdr


def test_library_exports_and_binding_lists_them():
    check_exports_and_binding(SYMBOLS)
    assert capi.PROTOTYPES["dekf_set_window_cross"] == (C.c_int, [C.c_void_p, C.c_int])
    assert capi.PROTOTYPES["dekf_get_window_cross"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])


def test_abi_version_and_params_layout_unchanged():
    check_abi_version_and_params_layout()


def test_null_handle_is_invalid():
    lib = capi.load()
    for on in (0, 1, 2):
        assert lib.dekf_set_window_cross(None, on) == capi.DEKF_ERR_INVALID
    k = C.c_int(-7)
    x = (C.c_double * 81)()
    assert lib.dekf_get_window_cross(None, C.cast(C.byref(k), C.c_void_p), C.cast(x, C.c_void_p), None, capi.DEKF_HOST) == capi.DEKF_ERR_INVALID
    assert k.value == -7


def test_header_compiles_as_c99_with_the_cross_calls(tmp_path):
    check_c99_client(tmp_path, "cross_client",
                     "    double lag1[81], newest[81];\n"
                     "    int steps = 0;\n"
                     "    dekf_status a = dekf_set_window_cross((dekf_handle)0, 1);\n"
                     "    dekf_status b = dekf_get_window_cross((dekf_handle)0, &steps, lag1, newest, DEKF_HOST);\n"
                     '    printf("set %d get %d steps %d abi %d\\n", (int)a, (int)b, steps, DEKF_ABI_VERSION);\n',
                     f"set {capi.DEKF_ERR_INVALID} get {capi.DEKF_ERR_INVALID} steps 0 abi 4")


def test_shim_compiles_with_window_cross(tmp_path):
    check_shim_usage(build_shim(tmp_path, "cross"))


def test_cross_twins_at_their_design_point():
    """every direct kernel has its _smooth_cross twin in the product build; no spills, no scratch, no static LDS (the dynamic LDS is
    DirectScratch::len for all three, so the twins keep the LDS residency of DESIGN.md section 4.8); and the twin's occupancy class
    (wavefronts per SIMD as far as registers go) is not below its _smooth sibling's, or is still above what the kernel's LDS admits (the
    rule of test_smoothing_twins_at_their_design_point, one twin further)"""
    check_twins_at_their_design_point("_smooth", "_smooth_cross")


# ------------------------------------------------------------------ 2: the core, lane-sequential
def check_identities(g, b):
    """what holds to the bit inside one cross window, and what stays unwritten"""
    Kw = g["K"]
    assert np.array_equal(g["zn"][b, Kw - 1], g["cw"][b, Kw - 1])     # Z_{K-1} = P_{K-1}
    assert np.array_equal(g["zn"][b, Kw - 2], g["l1"][b, Kw - 2])     # Z_{K-2} = T1' P_{K-1} = W_{K-2}: one product, the same operands
    assert (g["l1"][b, Kw - 1:] == FILL).all() and (g["zn"][b, Kw:] == FILL).all()
    assert np.isfinite(g["l1"][b, :Kw - 1]).all() and np.isfinite(g["zn"][b, :Kw]).all()


@pytest.mark.parametrize("name", list(CORE_CASES))
def test_core_every_cross_block_is_a_block_of_the_kkt_inverse(name):
    mk, B, K, ticks = CORE_CASES[name]
    p = mk()
    s = rough_streams(p, B, K)
    got = run_direct_sim(p, s, B, K, set(ticks), "cross")
    smooth = run_direct_sim(p, s, B, K, set(ticks), "smooth")
    N = p.N
    worst_1, worst_n, vo_eq = 0.0, 0.0, 0
    for b in range(B):
        arrival = own_arrival(p, got, ticks, b)
        ref = cross_reference(p, s, b, set(ticks))
        ref_own = cross_reference(p, s, b, {k for k in ticks if k >= N}, arrival=arrival) if arrival else {}
        for k in ticks:
            Cf, nv = ref_own.get(k, ref[k])
            g, Kw = got[k], got[k]["K"]
            assert Kw == min(k + 1, N) == Cf.shape[0]
            assert g["status"][b] == capi.DEKF_SOLVE_OK
            # everything the SMOOTH core writes: the same bits, the unwritten tail included
            for key in ("x", "v_b", "status", "iters", "cov", "xw", "cw"):
                assert np.array_equal(g[key], smooth[k][key]), (k, key)
            check_identities(g, b)
            e1, en = cross_errors(g["l1"][b, :Kw - 1], g["zn"][b, :Kw], Cf)
            worst_1, worst_n, vo_eq = max(worst_1, e1), max(worst_n, en), vo_eq + nv
    print(f"[{name}] every cross block: worst lag-one error {worst_1:.3g}, worst to-newest error {worst_n:.3g} (units of "
          f"sqrt(Cov(x_a)_ii Cov(x_b)_jj)); VO equality rows in the checked windows: {vo_eq}")
    assert vo_eq > 0, "no checked window holds a VO equality row"
    assert worst_1 <= CREL
    assert worst_n <= CREL


@pytest.mark.parametrize("name,maker", [("go1", lambda: _params(go1_params)), ("cassie", lambda: _params(cassie_params))])
def test_core_without_vo_every_cross_block(name, maker):
    """no VO row (make_streams(vo=False)): the cross-covariances of the fixed-interval Kalman smoother on the window"""
    p = maker()
    B, K = 2, 2 * p.N + 5
    ticks = [3, p.N - 1, p.N, p.N + 7, K - 1]
    s = make_streams(p, B, K, vo=False)
    got = run_direct_sim(p, s, B, K, set(ticks), "cross")
    worst_1, worst_n = 0.0, 0.0
    for b in range(B):
        ref = cross_reference(p, s, b, set(ticks))
        for k in ticks:
            Cf, nv = ref[k]
            assert nv == 0
            Kw = got[k]["K"]
            check_identities(got[k], b)
            e1, en = cross_errors(got[k]["l1"][b, :Kw - 1], got[k]["zn"][b, :Kw], Cf)
            worst_1, worst_n = max(worst_1, e1), max(worst_n, en)
    print(f"[{name}, no VO] every cross block: worst lag-one error {worst_1:.3g}, worst to-newest error {worst_n:.3g}")
    assert worst_1 <= CREL
    assert worst_n <= CREL


def test_relative_cov_is_the_covariance_of_the_difference():
    """relative_cov on the reference's own blocks of one full go1 window against Cov(x_T - x_k) = D Cov D' formed from the full inverse
    (D = [.. -I .. I]); the cancellation is against the marginals, so the error is stated in the marginals' scale, as CREL is"""
    p = _params(go1_params)
    B, K = 1, 48
    s = rough_streams(p, B, K)
    (Cf, nv), = cross_reference(p, s, 0, {K - 1}).values()
    Kw, ns = Cf.shape[0], p.dim_state
    assert Kw == p.N and nv > 0
    cov_win = np.array([Cf[k, k] for k in range(Kw)])
    cov_newest = np.array([Cf[k, Kw - 1] for k in range(Kw)])
    full = Cf.transpose(0, 2, 1, 3).reshape(Kw * ns, Kw * ns)
    worst = 0.0
    for k in range(Kw):
        D = np.zeros((ns, Kw * ns))
        D[:, (Kw - 1) * ns:] += np.eye(ns)
        D[:, k * ns:(k + 1) * ns] -= np.eye(ns)
        want = D @ full @ D.T
        got = relative_cov(cov_win, cov_newest, k)
        dT, dk = np.sqrt(np.diagonal(Cf[Kw - 1, Kw - 1])), np.sqrt(np.diagonal(Cf[k, k]))
        scale = np.maximum(dT, dk)
        worst = max(worst, float((np.abs(got - want) / (scale[:, None] * scale[None, :])).max()))
    print(f"relative_cov against D Cov D' over one go1 window: worst {worst:.3g} of the marginals' scale")
    assert worst <= CREL
    # a batch axis in front works the same
    assert np.array_equal(relative_cov(cov_win[None], cov_newest[None], 3)[0], relative_cov(cov_win, cov_newest, 3))


def test_cross_core_clean_under_asan_ubsan(tmp_path):
    """the CROSS core under AddressSanitizer + UBSan (CPU build): Go1 and foot states (both arrival-cost forms) through window fill,
    marginalisation and VO rows, the four window buffers exactly as large as the contract says"""
    check_clean_under_asan_ubsan(tmp_path, "cross_driver", "std::vector<double> xw, cw, l1, zn;", r"""
        // All four window buffers are allocated at exactly their contract sizes ([B][N][...], lag-one [B][N-1][...]) and the guard behind
        // the written entries is checked, so that an index past the window is caught by the sanitizer or by the guard.
        xw.assign((size_t)B * N * ns, -7.0);
        cw.assign((size_t)B * N * ns * ns, -7.0);
        l1.assign((size_t)B * (N - 1) * ns * ns, -7.0);
        zn.assign((size_t)B * N * ns * ns, -7.0);
        hs_update_direct_cross(h, T, cov.data(), xw.data(), cw.data(), l1.data(), zn.data());
        const int K = T + 1 < N ? T + 1 : N;
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < N; ++k) {
                for (int i = 0; i < ns; ++i) { const double v = xw[((size_t)b * N + k) * ns + i]; bad += k < K ? !std::isfinite(v) : v != -7.0; }
                for (int i = 0; i < ns * ns; ++i) {
                    const double v = cw[((size_t)b * N + k) * ns * ns + i], z = zn[((size_t)b * N + k) * ns * ns + i];
                    bad += k < K ? !std::isfinite(v) : v != -7.0;
                    bad += k < K ? !std::isfinite(z) : z != -7.0;
                    if (k < N - 1) { const double w = l1[((size_t)b * (N - 1) + k) * ns * ns + i]; bad += k < K - 1 ? !std::isfinite(w) : w != -7.0; }
                }
            }""", r'std::printf("lag1=%g newest=%g, %d bad window entries\n", l1[0], zn[0], bad);')
