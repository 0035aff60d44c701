"""The direct MHE solve on the GPU (dekf_set_solver(h, DEKF_SOLVER_DIRECT), BatchedEstimator(solver="direct")): every checked tick
against the exact optimum of the oracle's QP and the covariance against the inverse of its KKT matrix (direct_lib.exact_reference),
past the tick where VO rows turn into equalities, the Kalman-filter identity without VO, the distance of the cold ADMM oracle from the optimum (a record), batch
independence, defaults and reset, the call-order contract, an instance poisoned by a NaN sample, the C++ shim and the kernel name."""
import numpy as np
import pytest

import oracle_lib as O
import ref_numpy as RN
from decentralized_ekf_mhe_amd import capi, cassie_params, go1_params
from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host
from decentralized_ekf_mhe_amd.streams import make_streams
from direct_lib import (CASES, CREL, XABS, XREL, _params, block_err, blocks3, build_shim, case_run, check_reset_rerun, cov_err,
                        exact_reference, poisoned_runs, rough_streams, run, shim_rows, shim_twin, sub_streams, tripod_params)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 3: exactness, every checked tick
@pytest.mark.parametrize("name", list(CASES))
def test_direct_is_the_exact_optimum_of_the_oracle_qp(name):
    p, s, _, r = case_run(name, "plain")
    _, B, K, sub, every, kernel = CASES[name]
    assert r["kernel"] == (kernel, kernel)
    ticks = [int(k) for k in r["ticks"] if k >= 1]
    assert (r["st"][1:] == capi.DEKF_SOLVE_OK).all() and (r["it"][1:] == 0).all() and np.isnan(r["pri"][1:]).all()
    ns, N = p.dim_state, p.N
    info_form = p.leg_odom_type == 1 and p.arrival_cost_form == 1
    wx, wc, wxi, wci, vo_eq = 0.0, 0.0, 0.0, 0.0, 0
    for b in sub:
        ref = exact_reference(p, s, b, set(ticks))
        for i, k in enumerate(ticks):
            xr, Cr, nv = ref[k]
            x, Cm = r["x"][i + 1, b], r["cov"][i, b]
            vo_eq += nv
            if info_form and k >= N:
                # arrival_cost_form 1 on full windows: the information-form arrival cost differs from the oracle's covariance form by
                # rounding (the lane-sequential build shows the solve exact given its own arrival cost, test_direct_solve.py): x is held
                # to the foot-state allowances of test_foot_states.py (1 x base, 3 x feet of the ADMM yardstick), the covariance to its
                # measured worst case with a margin of about 3
                assert block_err(x, xr, blocks3(9), 1e-4, 1e-6) <= 1.0, (b, k)
                assert block_err(x, xr, blocks3(ns)[3:], 1e-4, 1e-6) <= 3.0, (b, k)
                wxi, wci = max(wxi, block_err(x, xr, blocks3(ns), XREL, XABS)), max(wci, cov_err(Cm, Cr))
                continue
            wx = max(wx, block_err(x, xr, blocks3(ns), XREL, XABS))
            wc = max(wc, cov_err(Cm, Cr))
    print(f"[{name}] worst x error {wx:.3g} x (1e-8 rel + 1e-10), covariance {wc:.3g} sqrt(C_ii C_jj); VO equality rows in the checked "
          f"windows: {vo_eq}" + (f"; arrival_cost_form 1 full windows: x {wxi:.3g} x, covariance {wci:.3g}" if info_form else ""))
    assert vo_eq > 0, "no checked window holds a VO equality row"
    assert wx <= 1.0
    assert wc <= CREL
    assert wci <= 1e-3


def test_direct_without_vo_is_the_kalman_filter():
    """KA1 on the device: x_T and Cov(x_T) of a direct handle equal the numpy Kalman filter's state and covariance"""
    p = _params(go1_params)
    B, K = 4, 3 * p.N + 5
    s = make_streams(p, B, K, vo=False)
    est = BatchedEstimator(p, B, solver="direct")
    sh = streams_host(s)
    xs, covs, quats = [], [], []
    for k in range(K):
        est.push_stream_step(sh, k)
        est.step(k)
        o = est.get()
        quats.append(o["quat"].copy())
        xs.append(o["x"].copy())
        covs.append(est.mhe_cov() if k else None)
    est.close()
    quats = np.array(quats)
    for b in range(B):
        xk, Ck = RN.kalman_filter(p, s, b, quats[:, b])
        for k in range(1, K):
            for blk in blocks3(9):
                rel = np.abs(xs[k][b][blk] - xk[k][blk]).max() / max(np.abs(xk[k][blk]).max(), 1e-6)
                assert rel < 1e-7, (b, k, blk, rel)
            assert cov_err(covs[k][b], Ck[k]) <= CREL, (b, k)


# ------------------------------------------------------------------ 4: the cold ADMM oracle's distance from the optimum (a record)
RECORD_CASES = {
    "go1": (lambda: _params(go1_params), 8, 45),
    "cassie": (lambda: _params(cassie_params), 6, 45),
    "tripod": (lambda: tripod_params(), 6, 40),
    "go1_foot": (lambda: _params(go1_params, leg_odom_type=1), 6, 45),
}


@pytest.mark.parametrize("name", list(RECORD_CASES))
def test_direct_against_the_cold_admm_oracle(name):
    """How far the reference's own ADMM output (the cold CPU oracle, eps 1e-6) lies from the exact optimum, every tick, in units of the
    ADMM yardstick (1e-4 rel + 1e-6 per 3-block): a record of the ADMM iterate's own error, not the pin (the exactness test above is).
    Warm start measured 2.1 x (9 states) / 8.3 x (foot-state base states) against the same oracle.  test_oracle_mhe.py
    (test_admm_vs_exact_with_vo_ka2) bounds the oracle's distance from the optimum by 5 x in the first steps after VO rows switch on;
    the measured worst cases are printed and asserted against that bound."""
    mk, B, K = RECORD_CASES[name]
    p = mk()
    s = rough_streams(p, B, K)
    r = run(p, s, B, K)
    x_ref, vb_ref, _, _ = O.run_streams(p, s, nthreads=8)
    x, xr = r["x"][1:], x_ref[1:]
    if p.leg_odom_type == 1:
        eb, ef = block_err(x, xr, blocks3(9), 1e-4, 1e-6), block_err(x, xr, blocks3(p.dim_state)[3:], 1e-4, 1e-6)
        print(f"[{name}] cold ADMM oracle against the direct optimum: base {eb:.2f} x, feet {ef:.2f} x the yardstick")
        assert eb <= 10.0 and ef <= 10.0
    else:
        e = block_err(x, xr, blocks3(9), 1e-4, 1e-6)
        print(f"[{name}] cold ADMM oracle against the direct optimum: {e:.2f} x the yardstick")
        assert e <= 5.0


# ------------------------------------------------------------------ 5: batch independence
def test_same_bits_at_b6_and_b832():
    p, s, _, big = case_run("go1_832", "plain")
    _, B, K, _, every, _ = CASES["go1_832"]
    small = run(p, sub_streams(s, list(range(6)), B), 6, K, every=every)
    for key in ("x", "vb", "st", "cov"):
        assert np.array_equal(small[key], big[key][:, :6]), key


# ------------------------------------------------------------------ 6: defaults and reset
def test_explicit_admm_equals_default_handle():
    p = _params(go1_params)
    B, K = 8, 30
    s = rough_streams(p, B, K)
    default = run(p, s, B, K, solver="admm", every=3)
    est = BatchedEstimator(p, B)
    assert est.lib.dekf_set_solver(est.h, capi.DEKF_SOLVER_ADMM) == capi.DEKF_OK
    sh = streams_host(s)
    xs = []
    for k in range(K):
        est.push_stream_step(sh, k)
        est.step(k)
        if k % 3 == 0 or k == K - 1:
            xs.append(est.get()["x"])
    assert est.solve_kernel_name(True) == default["kernel"][0]
    est.close()
    assert np.array_equal(np.array(xs), default["x"])


def test_reset_rerun_equals_fresh_direct_handle():
    check_reset_rerun("plain")


# ------------------------------------------------------------------ 7: contract
def test_call_order_and_refusals():
    lib = capi.load()
    p = _params(go1_params)
    cov = np.zeros((2, 9, 9))
    cp = cov.ctypes.data
    est = BatchedEstimator(p, 2)
    assert lib.dekf_set_solver(est.h, 2) == capi.DEKF_ERR_INVALID
    assert lib.dekf_set_solver(est.h, -1) == capi.DEKF_ERR_INVALID
    assert lib.dekf_get_mhe_cov(est.h, cp, capi.DEKF_HOST) == capi.DEKF_ERR_INVALID        # ADMM handle
    assert lib.dekf_set_solver(est.h, capi.DEKF_SOLVER_DIRECT) == capi.DEKF_OK
    assert lib.dekf_set_warm_start(est.h, 1) == capi.DEKF_ERR_INVALID                       # warm start on a direct handle
    assert lib.dekf_set_warm_start(est.h, 0) == capi.DEKF_OK
    assert lib.dekf_get_mhe_cov(est.h, cp, capi.DEKF_HOST) == capi.DEKF_ERR_ORDER          # before the first update
    s = rough_streams(p, 2, 4)
    sh = streams_host(s)
    est.push_stream_step(sh, 0)
    est.step(0)
    assert lib.dekf_set_solver(est.h, capi.DEKF_SOLVER_ADMM) == capi.DEKF_ERR_ORDER
    assert lib.dekf_get_mhe_cov(est.h, cp, capi.DEKF_HOST) == capi.DEKF_ERR_ORDER          # initialize is not an update
    est.push_stream_step(sh, 1)
    est.step(1)
    assert lib.dekf_get_mhe_cov(est.h, cp, capi.DEKF_HOST) == capi.DEKF_OK
    assert np.all(np.linalg.eigvalsh(cov) > 0)
    assert est.launch_info()["solve_workgroups"] == 2                                       # one wavefront per instance
    est.reset()                                                                              # the setting survives, the store does not
    assert est.solve_kernel_name(True) == "k_mhe_solve_direct_4_n20"
    assert lib.dekf_get_mhe_cov(est.h, cp, capi.DEKF_HOST) == capi.DEKF_ERR_ORDER
    assert lib.dekf_set_solver(est.h, capi.DEKF_SOLVER_ADMM) == capi.DEKF_OK
    assert est.solve_kernel_name(True) == "k_mhe_solve_r3_4_n20"
    assert lib.dekf_get_mhe_cov(est.h, cp, capi.DEKF_HOST) == capi.DEKF_ERR_INVALID
    est.close()
    # a warm handle, a polishing handle, a pipelined handle and a KF handle are refused
    est = BatchedEstimator(p, 2, warm_start=True)
    assert lib.dekf_set_solver(est.h, capi.DEKF_SOLVER_DIRECT) == capi.DEKF_ERR_INVALID
    est.close()
    for kw in (dict(polish=1), dict(solve_pipeline=1), dict(est_type=1)):
        with pytest.raises(capi.DekfError) as e:
            BatchedEstimator(_params(go1_params, **kw), 2, solver="direct")
        assert e.value.status == capi.DEKF_ERR_INVALID, kw
    est = BatchedEstimator(_params(go1_params, est_type=1), 2)
    assert lib.dekf_get_mhe_cov(est.h, cp, capi.DEKF_HOST) == capi.DEKF_ERR_INVALID
    est.close()


def test_nan_sample_poisons_only_its_own_instance():
    poisoned_runs("plain")


# ------------------------------------------------------------------ 8: the C++ shim
def test_shim_direct_equals_batched_estimator(tmp_path):
    p = _params(go1_params)
    K = 40
    s, quats, rows = shim_rows(build_shim(tmp_path, "plain"), tmp_path, p, K)
    for k, est in shim_twin(p, s, quats, K, "plain"):
        o = est.get()
        assert np.array_equal(rows[k][0:9], o["x"][0]), k        # (the shim prints %.17g: a double round-trips exactly)
        assert np.array_equal(rows[k][9:12], o["v_b"][0]), k
        assert np.array_equal(rows[k][12:93].reshape(9, 9), est.mhe_cov()[0]), k


# ------------------------------------------------------------------ 9: kernel name
def test_solve_kernel_name_names_the_direct_kernel():
    for name, (mk, *_, kernel) in CASES.items():
        est = BatchedEstimator(mk(), 2, solver="direct")
        assert est.solve_kernel_name(True) == est.solve_kernel_name(False) == kernel, name
        est.close()
