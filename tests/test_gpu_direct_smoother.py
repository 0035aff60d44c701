"""The window smoother of the direct MHE solve on the GPU (dekf_set_smoother / dekf_get_window, BatchedEstimator(solver="direct",
smoother=True)): every block of every checked window against the exact optimum of the oracle's QP and the diagonal blocks of the
inverse of its KKT matrix (test_direct_smoother.window_reference, test_direct_solve.py's yardstick), past the tick where VO rows turn
into equalities; the bit identities with the non-smoothing handle, batch independence, reset, host and device pointers; the call-order
contract; an instance poisoned by a NaN sample; the C++ shim."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from decentralized_ekf_mhe_amd import capi, go1_params
from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host
from decentralized_ekf_mhe_amd.streams import make_streams
from test_direct_smoother import FILL, build_shim_smooth, window_errors, window_reference
from test_direct_solve import CREL, XABS, XREL, _params, block_err, blocks3, cov_err, rough_streams
from test_gpu_direct_solve import CASES, case_run, run, sub_streams

pytestmark = pytest.mark.gpu


def run_smooth(p, s, B, K, every=1, reset_rerun=False, keep=None):
    """x, v_b, status, Cov(x_T) and the window (K, x_win, cov_win of the instances `keep`, default all) of a smoothing handle at the read
    ticks (every `every`-th tick and the last); the window from tick 1 on"""
    est = BatchedEstimator(p, B, solver="direct", smoother=True)
    sh = streams_host(s)
    keep = list(range(B)) if keep is None else keep
    res = []
    for _ in range(2 if reset_rerun else 1):
        out = {k: [] for k in ("x", "vb", "st", "it", "pri", "cov", "ticks", "K", "xw", "cw")}
        for k in range(K):
            est.push_stream_step(sh, k)
            est.step(k)
            if k % every == 0 or k == K - 1:
                o, info = est.get(), est.solver_info()
                out["x"].append(o["x"]); out["vb"].append(o["v_b"]); out["st"].append(o["status"]); out["it"].append(info["iters"])
                out["pri"].append(info["pri_res"]); out["ticks"].append(k)
                if k:
                    out["cov"].append(est.mhe_cov())
                    Kw, xw, cw = est.window()
                    out["K"].append(Kw); out["xw"].append(xw[keep]); out["cw"].append(cw[keep])
        r = {k: (v if k in ("xw", "cw") else np.array(v)) for k, v in out.items()}
        r["kernel"] = (est.solve_kernel_name(True), est.solve_kernel_name(False))
        res.append(r)
        if reset_rerun:
            est.reset()
    est.close()
    return res if reset_rerun else res[0]


@functools.lru_cache(maxsize=None)
def smooth_case_run(name):
    mk, B, K, sub, every, kernel = CASES[name]
    p = mk()
    s = rough_streams(p, B, K)
    keep = sorted(set(sub) | set(range(min(B, 6))))
    return p, s, keep, run_smooth(p, s, B, K, every=every, keep=keep)


# ------------------------------------------------------------------ 6: every window block, every checked tick
@pytest.mark.parametrize("name", list(CASES))
def test_every_window_block_is_the_exact_optimum_of_the_oracle_qp(name):
    p, s, keep, r = smooth_case_run(name)
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
    p, s, keep, on = smooth_case_run(name)
    _, _, off = case_run(name)
    for key in ("x", "vb", "st", "it", "cov", "ticks"):
        assert np.array_equal(on[key], off[key]), key
    assert np.array_equal(np.isnan(on["pri"]), np.isnan(off["pri"]))
    for i, k in enumerate(int(k) for k in on["ticks"] if k >= 1):
        Kw = int(on["K"][i])
        assert Kw == min(k + 1, p.N)
        assert np.array_equal(on["xw"][i][:, Kw - 1], on["x"][i + 1][keep]), k
        assert np.array_equal(on["cw"][i][:, Kw - 1], on["cov"][i][keep]), k


def test_same_window_bits_at_b6_and_b832():
    p, s, keep, big = smooth_case_run("go1_832")
    _, B, K, _, every, _ = CASES["go1_832"]
    assert keep[:6] == list(range(6))
    small = run_smooth(p, sub_streams(s, list(range(6)), B), 6, K, every=every)
    for key in ("x", "vb", "st", "cov"):
        assert np.array_equal(small[key], big[key][:, :6]), key
    assert np.array_equal(small["K"], big["K"])
    for i in range(len(small["K"])):
        assert np.array_equal(small["xw"][i], big["xw"][i][:6]), i
        assert np.array_equal(small["cw"][i], big["cw"][i][:6]), i


def test_reset_rerun_reproduces_the_window_bits():
    p = _params(go1_params)
    B, K = 8, 30
    s = rough_streams(p, B, K)
    a, b = run_smooth(p, s, B, K, every=3, reset_rerun=True)
    fresh = run_smooth(p, s, B, K, every=3)
    for other in (a, b):
        for key in ("x", "vb", "st", "cov", "K"):
            assert np.array_equal(other[key], fresh[key]), key
        for i in range(len(fresh["K"])):
            assert np.array_equal(other["xw"][i], fresh["xw"][i]) and np.array_equal(other["cw"][i], fresh["cw"][i]), i


def test_host_and_device_pointers_agree_and_entries_past_k_are_untouched():
    import torch
    lib = capi.load()
    p = _params(go1_params)
    B, ns, N = 5, p.dim_state, p.N
    s = rough_streams(p, B, N + 4)
    est = BatchedEstimator(p, B, solver="direct", smoother=True)
    sh = streams_host(s)
    for k in range(N + 4):
        est.push_stream_step(sh, k)
        est.step(k)
        if k not in (1, 7, N - 2, N - 1, N + 3):
            continue
        Kw = min(k + 1, N)
        xh, ch = np.full((B, N, ns), FILL), np.full((B, N, ns, ns), FILL)
        kh = C.c_int(0)
        assert lib.dekf_get_window(est.h, C.byref(kh), xh.ctypes.data, ch.ctypes.data, capi.DEKF_HOST) == capi.DEKF_OK
        assert kh.value == Kw
        assert (xh[:, Kw:] == FILL).all() and (ch[:, Kw:] == FILL).all(), k
        assert np.isfinite(xh[:, :Kw]).all() and np.isfinite(ch[:, :Kw]).all(), k
        xd = torch.full((B, N, ns), FILL, dtype=torch.float64, device="cuda")
        cd = torch.full((B, N, ns, ns), FILL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        kd = C.c_int(0)
        assert lib.dekf_get_window(est.h, C.byref(kd), xd.data_ptr(), cd.data_ptr(), capi.DEKF_DEVICE) == capi.DEKF_OK
        est.sync()
        assert kd.value == Kw
        assert np.array_equal(xd.cpu().numpy(), xh) and np.array_equal(cd.cpu().numpy(), ch), k
        # any of the three pointers may be NULL
        x2 = np.full((B, N, ns), FILL)
        assert lib.dekf_get_window(est.h, None, x2.ctypes.data, None, capi.DEKF_HOST) == capi.DEKF_OK
        assert np.array_equal(x2, xh)
        c2 = np.full((B, N, ns, ns), FILL)
        assert lib.dekf_get_window(est.h, None, None, c2.ctypes.data, capi.DEKF_HOST) == capi.DEKF_OK
        assert np.array_equal(c2, ch)
        k3 = C.c_int(0)
        assert lib.dekf_get_window(est.h, C.byref(k3), None, None, capi.DEKF_HOST) == capi.DEKF_OK and k3.value == Kw
        # window() hands out the K written entries
        Kp, xp, cp = est.window()
        assert Kp == Kw and np.array_equal(xp, xh[:, :Kw]) and np.array_equal(cp, ch[:, :Kw])
    est.close()


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
    p = _params(go1_params)
    B, K, bad, t_bad = 6, 34, 2, 26
    s = rough_streams(p, B, K)
    clean = run_smooth(p, s, B, K)
    sp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    sp["accel"][t_bad, bad, 0] = np.nan
    pois = run_smooth(p, sp, B, K)
    plain = run(p, sp, B, K)                     # the same poisoned log without the smoother: the same bits in everything it writes
    others = [b for b in range(B) if b != bad]
    for key in ("x", "vb", "st", "cov"):
        assert np.array_equal(pois[key][:, others], clean[key][:, others]), key
        assert np.array_equal(pois[key], plain[key], equal_nan=True), key
    assert np.array_equal(pois["K"], clean["K"])
    assert (clean["st"][1:] == capi.DEKF_SOLVE_OK).all()
    assert pois["st"][t_bad, bad] == capi.DEKF_SOLVE_NUMERIC
    n_numeric = 0
    for i in range(len(clean["K"])):
        assert np.array_equal(pois["xw"][i][others], clean["xw"][i][others]), i
        assert np.array_equal(pois["cw"][i][others], clean["cw"][i][others]), i
        assert np.isfinite(clean["xw"][i]).all() and np.isfinite(clean["cw"][i]).all(), i
        if pois["st"][i + 1, bad] == capi.DEKF_SOLVE_NUMERIC:     # (read tick i + 1: the window arrays start at tick 1)
            n_numeric += 1
            assert np.isnan(pois["xw"][i][bad]).all() and np.isnan(pois["cw"][i][bad]).all(), i
    assert n_numeric >= 1


# ------------------------------------------------------------------ the C++ shim
def test_shim_smooth_window_equals_batched_estimator(tmp_path):
    exe = build_shim_smooth(tmp_path)
    p = _params(go1_params)
    K = 30
    s = make_streams(p, 1, K)
    quats = O.run_streams(p, s)[2][:, 0]
    log = np.zeros((K, 81))
    for k in range(K):
        log[k, 0] = s["imu_t"][k, 0]
        log[k, 1:4], log[k, 4:7], log[k, 7:11] = s["accel"][k, 0], s["gyro"][k, 0], quats[k]
        log[k, 11:23] = s["p_foot"][k, 0].ravel()
        log[k, 23:59] = s["J"][k, 0].ravel()
        log[k, 59:71] = s["qdot"][k, 0].ravel()
        log[k, 71:75] = s["contact"][k, 0]
        if s["vo_mask"][k, 0]:
            log[k, 75], log[k, 76], log[k, 77], log[k, 78:81] = 1.0, s["vo_t_pre"][k, 0], s["vo_t_now"][k, 0], s["vo_dp"][k, 0]
    path = tmp_path / "log.bin"
    log.tofile(path)
    r = subprocess.run([exe, str(path), str(K)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows = [[float(v) for v in line.split()[1:]] for line in r.stdout.strip().splitlines()]
    est = BatchedEstimator(p, 1, solver="direct", smoother=True)
    sh = streams_host(s)
    for k in range(K):
        est.push_stream_step(sh, k)
        est.push_quaternion(np.ascontiguousarray(quats[k][None, :]))
        est.update(k) if k else est.initialize()
        if k:
            row = np.array(rows[k])
            Kw, xw, cw = est.window()
            assert np.array_equal(row[0:9], est.get()["x"][0]), k        # (the shim prints %.17g: a double round-trips exactly)
            assert int(row[93]) == Kw == min(k + 1, p.N), k
            win = row[94:94 + 90 * Kw].reshape(Kw, 90)
            assert np.array_equal(win[:, :9], xw[0]), k
            assert np.array_equal(win[:, 9:].reshape(Kw, 9, 9), cw[0]), k
    est.close()
