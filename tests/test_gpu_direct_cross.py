"""The window cross-covariances of the direct smoother on the GPU (dekf_set_window_cross / dekf_get_window_cross,
BatchedEstimator(solver="direct", smoother=True, cross=True)): every written block of cov_lag1 and cov_newest of every checked window
against the matching off-diagonal block of the inverse of the oracle QP's KKT matrix (direct_lib.cross_reference), past the
tick where VO rows turn into equalities; the bit identities with the option off and inside the new arrays, batch independence, reset,
host and device pointers; the call-order contract; an instance poisoned by a NaN sample; the C++ shim."""
import ctypes as C

import numpy as np
import pytest

from decentralized_ekf_mhe_amd import capi, go1_params
from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, relative_cov, streams_host
from direct_lib import CROSS_CASES as CASES
from direct_lib import (CREL, _params, build_shim, case_run, check_reset_rerun, check_window_pointers, cross_errors, cross_reference,
                        poisoned_runs, rough_streams, run, shim_rows, shim_twin, sub_streams)

pytestmark = pytest.mark.gpu


def check_identities(r, i):
    """read tick i of a run: the two bit identities of the new arrays, all instances"""
    Kw = int(r["K"][i])
    assert np.array_equal(r["zn"][i][:, Kw - 1], r["cw"][i][:, Kw - 1]), i
    assert np.array_equal(r["zn"][i][:, Kw - 2], r["l1"][i][:, Kw - 2]), i


# ------------------------------------------------------------------ every cross block, every checked tick
@pytest.mark.parametrize("name", list(CASES))
def test_every_cross_block_is_a_block_of_the_kkt_inverse(name):
    p, s, _, r = case_run(name, "cross")
    _, B, K, sub, every, kernel = CASES[name]
    assert r["kernel"] == (kernel + "_smooth_cross", kernel + "_smooth_cross")
    ticks = [int(k) for k in r["ticks"] if k >= 1]
    assert (r["st"][1:] == capi.DEKF_SOLVE_OK).all()
    ns, N = p.dim_state, p.N
    info_form = p.leg_odom_type == 1 and p.arrival_cost_form == 1
    w1, wn, w1i, wni, vo_eq = 0.0, 0.0, 0.0, 0.0, 0
    for b in sub:
        ref = cross_reference(p, s, b, set(ticks))
        for i, k in enumerate(ticks):
            Cf, nv = ref[k]
            Kw = int(r["K"][i])
            assert Kw == min(k + 1, N) == Cf.shape[0]
            l1, zn = r["l1"][i][b], r["zn"][i][b]
            assert l1.shape == (Kw - 1, ns, ns) and zn.shape == (Kw, ns, ns)
            vo_eq += nv
            e1, en = cross_errors(l1, zn, Cf)
            if info_form and k >= N:
                # arrival_cost_form 1 on full windows: the information-form arrival cost differs from the oracle's covariance form by
                # rounding (an input of the solve, not the solve: DESIGN.md section 4.8); the covariance allowance of
                # test_gpu_direct_solve.py for this case.  The lane-sequential build holds these windows to CREL given their own
                # arrival cost (test_direct_cross.py)
                w1i, wni = max(w1i, e1), max(wni, en)
                continue
            w1, wn = max(w1, e1), max(wn, en)
    print(f"[{name}] every cross block: worst lag-one error {w1:.3g}, worst to-newest error {wn:.3g} (units of sqrt(Cov(x_a)_ii "
          f"Cov(x_b)_jj)); VO equality rows in the checked windows: {vo_eq}"
          + (f"; arrival_cost_form 1 full windows: lag-one {w1i:.3g}, to-newest {wni:.3g}" if info_form else ""))
    assert vo_eq > 0, "no checked window holds a VO equality row"
    assert w1 <= CREL and wn <= CREL
    assert w1i <= 1e-3 and wni <= 1e-3


# ------------------------------------------------------------------ bit identities
@pytest.mark.parametrize("name", ["go1", "go1_foot", "pogox_n100"])
def test_cross_on_equals_cross_off_and_the_new_arrays_agree_with_each_other(name):
    p, s, _, on = case_run(name, "cross")
    _, B, K, _, every, kernel = CASES[name]
    off = run(p, s, B, K, smoother=True, every=every)
    assert off["kernel"] == (kernel + "_smooth", kernel + "_smooth")
    for key in ("x", "vb", "st", "it", "cov", "ticks", "K"):
        assert np.array_equal(on[key], off[key]), key
    assert len(on["K"]) == len(on["ticks"]) - 1
    for i in range(len(on["K"])):
        assert np.array_equal(on["xw"][i], off["xw"][i]), i
        assert np.array_equal(on["cw"][i], off["cw"][i]), i
        check_identities(on, i)
        assert np.isfinite(on["l1"][i]).all() and np.isfinite(on["zn"][i]).all(), i
    # the use it is for: Cov(x_T - x_0) of the last window is a covariance, far below the sum of the marginals where position is unobservable
    rel = relative_cov(on["cw"][-1], on["zn"][-1], 0)
    assert (np.diagonal(rel, axis1=-2, axis2=-1) >= 0).all()


def test_same_cross_bits_at_b6_and_b70():
    p = _params(go1_params)
    B, K = 70, 48
    s = rough_streams(p, B, K)
    big = run(p, s, B, K, smoother=True, cross=True, every=3, keep=list(range(6)))
    small = run(p, sub_streams(s, list(range(6)), B), 6, K, smoother=True, cross=True, every=3)
    for key in ("x", "vb", "st", "cov"):
        assert np.array_equal(small[key], big[key][:, :6]), key
    assert np.array_equal(small["K"], big["K"])
    for i in range(len(small["K"])):
        for key in ("xw", "cw", "l1", "zn"):
            assert np.array_equal(small[key][i], big[key][i]), (key, i)


def test_reset_rerun_reproduces_the_cross_bits():
    check_reset_rerun("cross", ("xw", "cw", "l1", "zn"))


def test_host_and_device_pointers_agree_and_entries_past_k_are_untouched():
    check_window_pointers(cross=True)


# ------------------------------------------------------------------ contract
def test_call_order_and_refusals():
    lib = capi.load()
    p = _params(go1_params)
    ns, N = p.dim_state, p.N
    l1, zn = np.zeros((2, N - 1, ns, ns)), np.zeros((2, N, ns, ns))
    kk = C.c_int(-3)
    twin = "k_mhe_solve_direct_4_n20"

    def get(est):
        return lib.dekf_get_window_cross(est.h, C.byref(kk), l1.ctypes.data, zn.ctypes.data, capi.DEKF_HOST)

    est = BatchedEstimator(p, 2)
    assert lib.dekf_set_window_cross(est.h, 1) == capi.DEKF_ERR_INVALID                      # an ADMM handle
    assert lib.dekf_set_window_cross(est.h, 0) == capi.DEKF_OK
    assert get(est) == capi.DEKF_ERR_INVALID
    assert lib.dekf_set_solver(est.h, capi.DEKF_SOLVER_DIRECT) == capi.DEKF_OK
    assert lib.dekf_set_window_cross(est.h, 1) == capi.DEKF_ERR_INVALID                      # direct, but no smoother
    assert lib.dekf_set_smoother(est.h, 1) == capi.DEKF_OK
    assert get(est) == capi.DEKF_ERR_INVALID                                                 # smoother, but not the option
    assert est.solve_kernel_name(True) == twin + "_smooth"
    for on in (2, -1):
        assert lib.dekf_set_window_cross(est.h, on) == capi.DEKF_ERR_INVALID
    assert lib.dekf_set_window_cross(est.h, 1) == capi.DEKF_OK
    assert est.solve_kernel_name(True) == est.solve_kernel_name(False) == twin + "_smooth_cross"
    assert get(est) == capi.DEKF_ERR_ORDER                                                   # before the first update
    assert kk.value == -3
    # the smoother off takes the option with it, and back on does not bring it back
    assert lib.dekf_set_smoother(est.h, 0) == capi.DEKF_OK
    assert est.solve_kernel_name(True) == twin
    assert get(est) == capi.DEKF_ERR_INVALID
    assert lib.dekf_set_smoother(est.h, 1) == capi.DEKF_OK
    assert est.solve_kernel_name(True) == twin + "_smooth"
    assert get(est) == capi.DEKF_ERR_INVALID
    assert lib.dekf_set_window_cross(est.h, 1) == capi.DEKF_OK
    s = rough_streams(p, 2, N + 3)
    sh = streams_host(s)
    est.push_stream_step(sh, 0)
    est.step(0)
    assert lib.dekf_set_window_cross(est.h, 0) == capi.DEKF_ERR_ORDER
    assert lib.dekf_set_window_cross(est.h, 1) == capi.DEKF_ERR_ORDER
    assert get(est) == capi.DEKF_ERR_ORDER                                                   # initialize is not an update
    for k in range(1, N + 3):
        est.push_stream_step(sh, k)
        est.step(k)
        assert get(est) == capi.DEKF_OK
        assert kk.value == min(k + 1, N)                                                     # through the window fill and beyond
    est.reset()                                                                              # the setting survives, the arrays do not
    assert est.solve_kernel_name(True) == twin + "_smooth_cross"
    assert get(est) == capi.DEKF_ERR_ORDER
    assert lib.dekf_set_window_cross(est.h, 0) == capi.DEKF_OK                               # right after reset: allowed
    assert est.solve_kernel_name(True) == twin + "_smooth"
    assert lib.dekf_set_window_cross(est.h, 1) == capi.DEKF_OK
    # back to ADMM: the option goes with the direct solve, and neither the solver nor the smoother brings it back
    assert lib.dekf_set_solver(est.h, capi.DEKF_SOLVER_ADMM) == capi.DEKF_OK
    assert est.solve_kernel_name(True) == "k_mhe_solve_r3_4_n20"
    assert get(est) == capi.DEKF_ERR_INVALID
    assert lib.dekf_set_window_cross(est.h, 1) == capi.DEKF_ERR_INVALID
    assert lib.dekf_set_solver(est.h, capi.DEKF_SOLVER_DIRECT) == capi.DEKF_OK
    assert est.solve_kernel_name(True) == twin
    assert lib.dekf_set_smoother(est.h, 1) == capi.DEKF_OK
    assert est.solve_kernel_name(True) == twin + "_smooth"
    assert get(est) == capi.DEKF_ERR_INVALID
    est.close()
    # a KF handle; the Python layer: cross implies nothing else
    est = BatchedEstimator(_params(go1_params, est_type=1), 2)
    assert lib.dekf_set_window_cross(est.h, 1) == capi.DEKF_ERR_INVALID
    assert get(est) == capi.DEKF_ERR_INVALID
    est.close()
    for kw in (dict(cross=True), dict(solver="direct", cross=True)):
        with pytest.raises(capi.DekfError) as e:
            BatchedEstimator(p, 2, **kw)
        assert e.value.status == capi.DEKF_ERR_INVALID


def test_kernel_name_names_the_cross_twin():
    for name, (mk, *_, kernel) in CASES.items():
        est = BatchedEstimator(mk(), 2, solver="direct", smoother=True, cross=True)
        assert est.solve_kernel_name(True) == est.solve_kernel_name(False) == kernel + "_smooth_cross", name
        est.close()


# ------------------------------------------------------------------ a NaN sample
def test_nan_sample_poisons_only_its_own_cross_arrays():
    poisoned_runs("cross", ("l1", "zn"))


# ------------------------------------------------------------------ the C++ shim
def test_shim_cross_arrays_equal_batched_estimator(tmp_path):
    p = _params(go1_params)
    K = 30
    s, quats, rows = shim_rows(build_shim(tmp_path, "cross"), tmp_path, p, K)
    for k, est in shim_twin(p, s, quats, K, "cross"):
        row = rows[k]
        Kw, xw, cw = est.window()
        Kc, l1, zn = est.window_cross()
        assert np.array_equal(row[0:9], est.get()["x"][0]), k        # (the shim prints %.17g: a double round-trips exactly)
        assert int(row[12]) == Kw == Kc == min(k + 1, p.N), k
        o = 13
        for j in range(Kw):
            assert np.array_equal(row[o:o + 81].reshape(9, 9), cw[0, j]), (k, j)
            assert np.array_equal(row[o + 81:o + 162].reshape(9, 9), zn[0, j]), (k, j)
            o += 162
            if j + 1 < Kw:
                assert np.array_equal(row[o:o + 81].reshape(9, 9), l1[0, j]), (k, j)
                o += 81
        assert o + 1 == len(row), k                                   # (solver_iters_ closes the line)
