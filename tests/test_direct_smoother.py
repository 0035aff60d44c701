"""The window smoother of the direct MHE solve (dekf_set_smoother / dekf_get_window, csrc/mhe_direct_core.h: SMOOTH) without a GPU.

ABI: the two calls are declared, exported and bound, refuse a null handle and compile as C99, while the ABI version and dekf_params
stay what they were; the C++ shim compiles with robot_params::smoothWindow_; the ten smoothing twins sit at their design point.
Core: the lane-sequential build of the SMOOTH instantiation (tests/hostsim/direct_hostsim.cpp: hs_update_direct_smooth) on the records
and the input snapshot that the assemble step leaves: EVERY block of the window, every checked tick, against the exact optimum of the
oracle's QP (ref_numpy.kkt_exact) and the diagonal blocks of the inverse of that QP's KKT matrix (direct_lib.window_reference), inside
test_direct_solve.py's yardstick; the newest block bit-equal to what the non-smoothing core returns; without VO rows against the same
references."""
import ctypes as C
import re

import numpy as np
import pytest

from decentralized_ekf_mhe_amd import capi, cassie_params, go1_params
from decentralized_ekf_mhe_amd.streams import make_streams
from direct_lib import (CORE_CASES, CREL, FILL, _params, build_shim, check_abi_version_and_params_layout, check_c99_client,
                        check_clean_under_asan_ubsan, check_exports_and_binding, check_shim_usage, check_twins_at_their_design_point,
                        header, own_arrival, rough_streams, run_direct_sim, window_errors, window_reference)

SYMBOLS = ("dekf_set_smoother", "dekf_get_window")


# ------------------------------------------------------------------ 1: the C boundary
def test_header_declares_both_calls():
    hdr = header()
    assert re.search(r"dekf_status\s+dekf_set_smoother\s*\(\s*dekf_handle\s+h\s*,\s*int\s+on\s*\)\s*;", hdr)
    assert re.search(r"dekf_status\s+dekf_get_window\s*\(\s*dekf_handle\s+h\s*,\s*int\s*\*\s*steps\s*,\s*double\s*\*\s*x_win\s*,\s*double\s*\*\s*"
                     r"cov_win\s*,\s*dekf_mem\s+where\s*\)\s*;", hdr)
    assert re.search(r"#define\s+DEKF_ABI_VERSION\s+4\b", hdr)


def test_library_exports_and_binding_lists_them():
    check_exports_and_binding(SYMBOLS)
    assert capi.PROTOTYPES["dekf_set_smoother"] == (C.c_int, [C.c_void_p, C.c_int])
    assert capi.PROTOTYPES["dekf_get_window"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])


def test_abi_version_and_params_layout_unchanged():
    check_abi_version_and_params_layout()


def test_null_handle_is_invalid():
    lib = capi.load()
    for on in (0, 1, 2):
        assert lib.dekf_set_smoother(None, on) == capi.DEKF_ERR_INVALID
    k = C.c_int(-7)
    x = (C.c_double * 9)()
    assert lib.dekf_get_window(None, C.cast(C.byref(k), C.c_void_p), C.cast(x, C.c_void_p), None, capi.DEKF_HOST) == capi.DEKF_ERR_INVALID
    assert k.value == -7


def test_header_compiles_as_c99_with_the_smoother_calls(tmp_path):
    check_c99_client(tmp_path, "smoother_client",
                     "    double x[9], cov[81];\n"
                     "    int steps = 0;\n"
                     "    dekf_status a = dekf_set_smoother((dekf_handle)0, 1);\n"
                     "    dekf_status b = dekf_get_window((dekf_handle)0, &steps, x, cov, DEKF_HOST);\n"
                     '    printf("set %d get %d steps %d abi %d\\n", (int)a, (int)b, steps, DEKF_ABI_VERSION);\n',
                     f"set {capi.DEKF_ERR_INVALID} get {capi.DEKF_ERR_INVALID} steps 0 abi 4")


def test_shim_compiles_with_smooth_window(tmp_path):
    check_shim_usage(build_shim(tmp_path, "smooth"))


def test_smoothing_twins_at_their_design_point():
    """every direct kernel has its _smooth twin in the product build; no spills, no scratch, no static LDS (the
    dynamic LDS is DirectScratch::len for both, so the twins keep the LDS residency of section 4.8); and the twin's occupancy class
    (wavefronts per SIMD as far as registers go) is not below its non-smoothing twin's — or, where it is (k_mhe_solve_direct_foot_1_smooth:
    7 against 8, over the scalar registers), it is still above what the kernel's LDS admits, which then decides the residency of both"""
    check_twins_at_their_design_point("", "_smooth")


# ------------------------------------------------------------------ 2: the core, lane-sequential
@pytest.mark.parametrize("name", list(CORE_CASES))
def test_core_every_window_block_is_the_exact_optimum_of_the_oracle_qp(name):
    mk, B, K, ticks = CORE_CASES[name]
    p = mk()
    s = rough_streams(p, B, K)
    got = run_direct_sim(p, s, B, K, set(ticks), "smooth")
    plain = run_direct_sim(p, s, B, K, set(ticks))
    ns, N = p.dim_state, p.N
    worst_x, worst_c, worst_blk, vo_eq = 0.0, 0.0, None, 0
    for b in range(B):
        arrival = own_arrival(p, got, ticks, b)
        ref = window_reference(p, s, b, set(ticks))
        ref_own = window_reference(p, s, b, {k for k in ticks if k >= N}, arrival=arrival) if arrival else {}
        for k in ticks:
            X, Cv, nv = ref_own.get(k, ref[k])
            g, Kw = got[k], got[k]["K"]
            assert Kw == min(k + 1, N) == len(X)
            assert g["status"][b] == capi.DEKF_SOLVE_OK
            # everything the non-smoothing core writes: the same bits; the newest block of the window: those bits again
            for key in ("x", "v_b", "status", "iters", "cov"):
                assert np.array_equal(g[key], plain[k][key]), (k, key)
            assert np.array_equal(g["xw"][b, Kw - 1], plain[k]["x"][b]), k
            assert np.array_equal(g["cw"][b, Kw - 1], plain[k]["cov"][b]), k
            assert (g["xw"][b, Kw:] == FILL).all() and (g["cw"][b, Kw:] == FILL).all(), k
            cw = g["cw"][b, :Kw]
            assert np.array_equal(cw[:Kw - 1], np.swapaxes(cw[:Kw - 1], -1, -2)), k   # symmetric, both triangles
            ex, ec, blk = window_errors(g["xw"][b, :Kw], cw, X, Cv, ns)
            if ex > worst_x:
                worst_blk = (k, blk, Kw)
            worst_x, worst_c, vo_eq = max(worst_x, ex), max(worst_c, ec), vo_eq + nv
    print(f"[{name}] every window block: worst x error {worst_x:.3g} x (1e-8 rel + 1e-10) at (tick, block, K) = {worst_blk}; worst "
          f"covariance error {worst_c:.3g} sqrt(C_ii C_jj); VO equality rows in the checked windows: {vo_eq}")
    assert vo_eq > 0, "no checked window holds a VO equality row"
    assert worst_x <= 1.0
    assert worst_c <= CREL


@pytest.mark.parametrize("name,maker", [("go1", lambda: _params(go1_params)), ("cassie", lambda: _params(cassie_params))])
def test_core_without_vo_every_window_block(name, maker):
    """no VO row (make_streams(vo=False)): the fixed-interval Kalman smoother on the window; every block against the same references"""
    p = maker()
    B, K = 2, 2 * p.N + 5
    ticks = [3, p.N - 1, p.N, p.N + 7, K - 1]
    s = make_streams(p, B, K, vo=False)
    got = run_direct_sim(p, s, B, K, set(ticks), "smooth")
    worst_x, worst_c = 0.0, 0.0
    for b in range(B):
        ref = window_reference(p, s, b, set(ticks))
        for k in ticks:
            X, Cv, nv = ref[k]
            assert nv == 0
            Kw = got[k]["K"]
            ex, ec, _ = window_errors(got[k]["xw"][b, :Kw], got[k]["cw"][b, :Kw], X, Cv, p.dim_state)
            worst_x, worst_c = max(worst_x, ex), max(worst_c, ec)
    print(f"[{name}, no VO] every window block: worst x error {worst_x:.3g} x, worst covariance error {worst_c:.3g}")
    assert worst_x <= 1.0
    assert worst_c <= CREL


def test_smooth_core_clean_under_asan_ubsan(tmp_path):
    """the SMOOTH core under AddressSanitizer + UBSan (CPU build): Go1 and foot states (both arrival-cost forms) through window fill,
    marginalisation and VO rows, the window buffers exactly as large as the contract says"""
    check_clean_under_asan_ubsan(tmp_path, "smooth_driver", "std::vector<double> xw, cw;", r"""
        // The window buffers are allocated at exactly [B][N][...] and the guard behind the K written entries is checked, so that an
        // index past the window is caught by the sanitizer or by the guard.
        xw.assign((size_t)B * N * ns, -7.0);
        cw.assign((size_t)B * N * ns * ns, -7.0);
        hs_update_direct_smooth(h, T, cov.data(), xw.data(), cw.data());
        const int K = T + 1 < N ? T + 1 : N;
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < N; ++k) {
                for (int i = 0; i < ns; ++i) { const double v = xw[((size_t)b * N + k) * ns + i]; bad += k < K ? !std::isfinite(v) : v != -7.0; }
                for (int i = 0; i < ns * ns; ++i) { const double v = cw[((size_t)b * N + k) * ns * ns + i]; bad += k < K ? !std::isfinite(v) : v != -7.0; }
            }""", r'std::printf("oldest v=%g cov00=%g, %d bad window entries\n", xw[3], cw[0], bad);')
