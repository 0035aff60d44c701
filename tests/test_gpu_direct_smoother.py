"""The window smoother of the direct MHE solve on the GPU (dekf_set_smoother / dekf_get_window, BatchedEstimator(solver="direct",
smoother=True)): every block of every checked window against the exact optimum of the oracle's QP and the diagonal blocks of the
inverse of its KKT matrix (direct_lib.window_reference, test_direct_solve.py's yardstick), past the tick where VO rows turn
into equalities; the bit identities with the non-smoothing handle, batch independence, reset, host and device pointers; the call-order
contract; an instance poisoned by a NaN sample; the C++ shim."""
import ctypes as C

import numpy as np
import pytest

from decentralized_ekf_mhe_amd import capi, go1_params
from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host
from direct_lib import (CASES, CREL, _params, block_err, blocks3, build_shim, case_run, check_reset_rerun, check_window_pointers,
                        poisoned_runs, rough_streams, run, shim_rows, shim_twin, sub_streams, window_errors, window_reference)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 6: every window block, every checked tick
@pytest.mark.parametrize("name", list(CASES))
def test_every_window_block_is_the_exact_optimum_of_the_oracle_qp(name):
    p, s, keep, r = case_run(name, "smooth")
    _, B, K, sub, every, kernel = CASES[name]
    assert r["kernel"] == (kernel + "_smooth", kernel + "_smooth")
    ticks = [int(k) for k in r["ticks"] if k >= 1]
    assert (r["st"][1:] == capi.DEKF_SOLVE_OK).all() and (r["it"][1:] == 0).all() and np.isnan(r["pri"][1:]).all()
    ns, N = p.dim_state, p.N
    info_form = p.leg_odom_type == 1 and p.arrival_cost_form == 1
    wx, wc, wxi, wci, vo_eq, where = 0.0, 0.0, 0.0, 0.0, 0, None
    assert {b % 2 for b in sub} == {0, 1} or info_form   # fast-camera (even) and slow-camera (odd) instances
    for b in sub:
        ref = window_reference(p, s, b, set(ticks))
        for i, k in enumerate(ticks):
            X, Cv, nv = ref[k]
            Kw = int(r["K"][i])
            assert Kw == min(k + 1, N) == len(X)
            xw, cw = r["xw"][i][keep.index(b)], r["cw"][i][keep.index(b)]
            assert xw.shape == (Kw, ns) and cw.shape == (Kw, ns, ns)
            assert np.array_equal(cw[:Kw - 1], np.swapaxes(cw[:Kw - 1], -1, -2)), (b, k)   # symmetric, both triangles
            vo_eq += nv
            if info_form and k >= N:
                # arrival_cost_form 1 on full windows: the allowances test_gpu_direct_solve.py gives this case (the information-form
                # arrival cost differs from the oracle's covariance form by rounding: an input of the solve, not the solve; the
                # lane-sequential build holds the solve to the tight yardstick given its own arrival cost, test_direct_smoother.py),
                # now for every block of the window
                for j in range(Kw):
                    assert block_err(xw[j], X[j], blocks3(9), 1e-4, 1e-6) <= 1.0, (b, k, j)
                    assert block_err(xw[j], X[j], blocks3(ns)[3:], 1e-4, 1e-6) <= 3.0, (b, k, j)
                ex, ec, _ = window_errors(xw, cw, X, Cv, ns)
                wxi, wci = max(wxi, ex), max(wci, ec)
                continue
            ex, ec, blk = window_errors(xw, cw, X, Cv, ns)
            if ex > wx:
                where = (b, k, blk, Kw)
            wx, wc = max(wx, ex), max(wc, ec)
    print(f"[{name}] every window block: worst x error {wx:.3g} x (1e-8 rel + 1e-10) at (instance, tick, block, K) = {where}, covariance "
          f"{wc:.3g} sqrt(C_ii C_jj); VO equality rows in the checked windows: {vo_eq}"
          + (f"; arrival_cost_form 1 full windows: x {wxi:.3g} x, covariance {wci:.3g}" if info_form else ""))
    assert vo_eq > 0, "no checked window holds a VO equality row"
    assert wx <= 1.0
    assert wc <= CREL
    assert wci <= 1e-3


# ------------------------------------------------------------------ 7: bit identities
@pytest.mark.parametrize("name", ["go1_832", "go1_foot", "pogox_n100"])
def test_smoother_on_equals_smoother_off_and_newest_block_equals_x_mhe(name):
    p, s, keep, on = case_run(name, "smooth")
    _, _, _, off = case_run(name, "plain")
    for key in ("x", "vb", "st", "it", "cov", "ticks"):
        assert np.array_equal(on[key], off[key]), key
    assert np.array_equal(np.isnan(on["pri"]), np.isnan(off["pri"]))
    for i, k in enumerate(int(k) for k in on["ticks"] if k >= 1):
        Kw = int(on["K"][i])
        assert Kw == min(k + 1, p.N)
        assert np.array_equal(on["xw"][i][:, Kw - 1], on["x"][i + 1][keep]), k
        assert np.array_equal(on["cw"][i][:, Kw - 1], on["cov"][i][keep]), k


def test_same_window_bits_at_b6_and_b832():
    p, s, keep, big = case_run("go1_832", "smooth")
    _, B, K, _, every, _ = CASES["go1_832"]
    assert keep[:6] == list(range(6))
    small = run(p, sub_streams(s, list(range(6)), B), 6, K, smoother=True, every=every)
    for key in ("x", "vb", "st", "cov"):
        assert np.array_equal(small[key], big[key][:, :6]), key
    assert np.array_equal(small["K"], big["K"])
    for i in range(len(small["K"])):
        assert np.array_equal(small["xw"][i], big["xw"][i][:6]), i
        assert np.array_equal(small["cw"][i], big["cw"][i][:6]), i


def test_reset_rerun_reproduces_the_window_bits():
    check_reset_rerun("smooth", ("xw", "cw"))


def test_host_and_device_pointers_agree_and_entries_past_k_are_untouched():
    check_window_pointers(cross=False)


# ------------------------------------------------------------------ 8: contract
def test_call_order_and_refusals():
    lib = capi.load()
    p = _params(go1_params)
    ns, N = p.dim_state, p.N
    xw, cw = np.zeros((2, N, ns)), np.zeros((2, N, ns, ns))
    kk = C.c_int(-3)

    def get(est):
        return lib.dekf_get_window(est.h, C.byref(kk), xw.ctypes.data, cw.ctypes.data, capi.DEKF_HOST)

    est = BatchedEstimator(p, 2)
    assert lib.dekf_set_smoother(est.h, 1) == capi.DEKF_ERR_INVALID                          # an ADMM handle
    assert lib.dekf_set_smoother(est.h, 0) == capi.DEKF_OK
    assert get(est) == capi.DEKF_ERR_INVALID
    assert lib.dekf_set_solver(est.h, capi.DEKF_SOLVER_DIRECT) == capi.DEKF_OK
    assert get(est) == capi.DEKF_ERR_INVALID                                                 # direct, but no smoother
    assert est.solve_kernel_name(True) == "k_mhe_solve_direct_4_n20"
    for on in (2, -1):
        assert lib.dekf_set_smoother(est.h, on) == capi.DEKF_ERR_INVALID
    assert lib.dekf_set_solver(est.h, 2) == capi.DEKF_ERR_INVALID                            # (the accepted solver values did not change)
    assert lib.dekf_set_smoother(est.h, 1) == capi.DEKF_OK
    assert est.solve_kernel_name(True) == est.solve_kernel_name(False) == "k_mhe_solve_direct_4_n20_smooth"
    assert get(est) == capi.DEKF_ERR_ORDER                                                   # before the first update
    assert kk.value == -3
    s = rough_streams(p, 2, N + 3)
    sh = streams_host(s)
    est.push_stream_step(sh, 0)
    est.step(0)
    assert lib.dekf_set_smoother(est.h, 0) == capi.DEKF_ERR_ORDER
    assert lib.dekf_set_smoother(est.h, 1) == capi.DEKF_ERR_ORDER
    assert get(est) == capi.DEKF_ERR_ORDER                                                   # initialize is not an update
    for k in range(1, N + 3):
        est.push_stream_step(sh, k)
        est.step(k)
        assert get(est) == capi.DEKF_OK
        assert kk.value == min(k + 1, N)                                                     # through the window fill and beyond
    assert est.launch_info()["solve_workgroups"] == 2
    est.reset()                                                                              # the setting survives, the window does not
    assert est.solve_kernel_name(True) == "k_mhe_solve_direct_4_n20_smooth"
    assert get(est) == capi.DEKF_ERR_ORDER
    # back to ADMM: the smoother goes with the direct solve, and does not come back by itself
    assert lib.dekf_set_solver(est.h, capi.DEKF_SOLVER_ADMM) == capi.DEKF_OK
    assert est.solve_kernel_name(True) == "k_mhe_solve_r3_4_n20"
    assert get(est) == capi.DEKF_ERR_INVALID
    assert lib.dekf_set_smoother(est.h, 1) == capi.DEKF_ERR_INVALID
    assert lib.dekf_set_solver(est.h, capi.DEKF_SOLVER_DIRECT) == capi.DEKF_OK
    assert est.solve_kernel_name(True) == "k_mhe_solve_direct_4_n20"
    assert get(est) == capi.DEKF_ERR_INVALID
    est.close()
    # a KF handle; the Python layer
    est = BatchedEstimator(_params(go1_params, est_type=1), 2)
    assert lib.dekf_set_smoother(est.h, 1) == capi.DEKF_ERR_INVALID
    assert get(est) == capi.DEKF_ERR_INVALID
    est.close()
    with pytest.raises(capi.DekfError) as e:
        BatchedEstimator(p, 2, smoother=True)
    assert e.value.status == capi.DEKF_ERR_INVALID


def test_kernel_name_names_the_smoothing_twin():
    for name, (mk, *_, kernel) in CASES.items():
        est = BatchedEstimator(mk(), 2, solver="direct", smoother=True)
        assert est.solve_kernel_name(True) == est.solve_kernel_name(False) == kernel + "_smooth", name
        est.close()


# ------------------------------------------------------------------ 9: a NaN sample
def test_nan_sample_poisons_only_its_own_window():
    p, sp, B, K, _, pois = poisoned_runs("smooth", ("xw", "cw"))
    plain = run(p, sp, B, K)                     # the same poisoned log without the smoother: the same bits in everything it writes
    for key in ("x", "vb", "st", "cov"):
        assert np.array_equal(pois[key], plain[key], equal_nan=True), key


# ------------------------------------------------------------------ the C++ shim
def test_shim_smooth_window_equals_batched_estimator(tmp_path):
    p = _params(go1_params)
    K = 30
    s, quats, rows = shim_rows(build_shim(tmp_path, "smooth"), tmp_path, p, K)
    for k, est in shim_twin(p, s, quats, K, "smooth"):
        row = rows[k]
        Kw, xw, cw = est.window()
        assert np.array_equal(row[0:9], est.get()["x"][0]), k        # (the shim prints %.17g: a double round-trips exactly)
        assert int(row[93]) == Kw == min(k + 1, p.N), k
        win = row[94:94 + 90 * Kw].reshape(Kw, 90)
        assert np.array_equal(win[:, :9], xw[0]), k
        assert np.array_equal(win[:, 9:].reshape(Kw, 9, 9), cw[0]), k
