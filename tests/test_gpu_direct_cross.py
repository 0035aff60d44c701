"""The window cross-covariances of the direct smoother on the GPU (dekf_set_window_cross / dekf_get_window_cross,
BatchedEstimator(solver="direct", smoother=True, cross=True)): every written block of cov_lag1 and cov_newest of every checked window
against the matching off-diagonal block of the inverse of the oracle QP's KKT matrix (test_direct_cross.cross_reference), past the
tick where VO rows turn into equalities; the bit identities with the option off and inside the new arrays, batch independence, reset,
host and device pointers; the call-order contract; an instance poisoned by a NaN sample; the C++ shim."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from decentralized_ekf_mhe_amd import capi, go1_params, pogox_params
from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, relative_cov, streams_host
from decentralized_ekf_mhe_amd.streams import make_streams
from test_direct_cross import build_shim_cross, cross_errors, cross_reference
from test_direct_smoother import FILL
from test_direct_solve import CREL, _params, rough_streams
from test_gpu_direct_solve import sub_streams

pytestmark = pytest.mark.gpu


def run_cross(p, s, B, K, every=1, reset_rerun=False, keep=None, cross=True):
    """x, v_b, status, Cov(x_T), the window and (cross) the cross-covariances (K, x_win, cov_win, lag1, newest of the instances `keep`,
    default all) of a smoothing handle with or without the option, at the read ticks (every `every`-th tick and the last); the window
    arrays from tick 1 on"""
    est = BatchedEstimator(p, B, solver="direct", smoother=True, cross=cross)
    sh = streams_host(s)
    keep = list(range(B)) if keep is None else keep
    res = []
    lists = ("xw", "cw", "l1", "zn")
    for _ in range(2 if reset_rerun else 1):
        out = {k: [] for k in ("x", "vb", "st", "it", "cov", "ticks", "K") + lists}
        for k in range(K):
            est.push_stream_step(sh, k)
            est.step(k)
            if k % every == 0 or k == K - 1:
                o, info = est.get(), est.solver_info()
                out["x"].append(o["x"]); out["vb"].append(o["v_b"]); out["st"].append(o["status"]); out["it"].append(info["iters"])
                out["ticks"].append(k)
                if k:
                    out["cov"].append(est.mhe_cov())
                    Kw, xw, cw = est.window()
                    out["K"].append(Kw); out["xw"].append(xw[keep]); out["cw"].append(cw[keep])
                    if cross:
                        Kc, l1, zn = est.window_cross()
                        assert Kc == Kw and l1.shape[1] == Kw - 1 and zn.shape[1] == Kw
                        out["l1"].append(l1[keep]); out["zn"].append(zn[keep])
        r = {k: (v if k in lists else np.array(v)) for k, v in out.items()}
        r["kernel"] = (est.solve_kernel_name(True), est.solve_kernel_name(False))
        res.append(r)
        if reset_rerun:
            est.reset()
    est.close()
    return res if reset_rerun else res[0]


# name: (params, B, ticks, instances checked, every, kernel).  The smallest shapes that take every path: Go1 is the _4_n20 twin with the
# fast (even) and the slow (odd) camera; go1_foot has ns = 21, several entries per lane and the blocks that bound LDS; PogoX is the
# run-time horizon with a 99-step chain of Z.  The foot-state references are KKT systems ~2 200 wide (every 8th tick, which still
# takes the window fill, full windows and, from tick 40 on, VO equality rows), PogoX's ~3 900 wide (every 10th, one instance).
CASES = {
    "go1": (lambda: _params(go1_params), 6, 48, [0, 1], 1, "k_mhe_solve_direct_4_n20"),
    "go1_foot": (lambda: _params(go1_params, leg_odom_type=1), 4, 48, [0, 1], 8, "k_mhe_solve_direct_foot_4"),
    "pogox_n100": (lambda: _params(pogox_params), 2, 111, [0], 10, "k_mhe_solve_direct_1"),
    "go1_foot_info": (lambda: _params(go1_params, leg_odom_type=1, arrival_cost_form=1), 2, 48, [0], 8, "k_mhe_solve_direct_foot_4"),
}


@functools.lru_cache(maxsize=None)
def cross_case_run(name):
    mk, B, K, sub, every, kernel = CASES[name]
    p = mk()
    s = rough_streams(p, B, K)
    return p, s, run_cross(p, s, B, K, every=every)


def check_identities(r, i):
    """read tick i of a run: the two bit identities of the new arrays, all instances"""
    Kw = int(r["K"][i])
    assert np.array_equal(r["zn"][i][:, Kw - 1], r["cw"][i][:, Kw - 1]), i
    assert np.array_equal(r["zn"][i][:, Kw - 2], r["l1"][i][:, Kw - 2]), i


# ------------------------------------------------------------------ every cross block, every checked tick
@pytest.mark.parametrize("name", list(CASES))
def test_every_cross_block_is_a_block_of_the_kkt_inverse(name):
    p, s, r = cross_case_run(name)
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
    p, s, on = cross_case_run(name)
    _, B, K, _, every, kernel = CASES[name]
    off = run_cross(p, s, B, K, every=every, cross=False)
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
    big = run_cross(p, s, B, K, every=3, keep=list(range(6)))
    small = run_cross(p, sub_streams(s, list(range(6)), B), 6, K, every=3)
    for key in ("x", "vb", "st", "cov"):
        assert np.array_equal(small[key], big[key][:, :6]), key
    assert np.array_equal(small["K"], big["K"])
    for i in range(len(small["K"])):
        for key in ("xw", "cw", "l1", "zn"):
            assert np.array_equal(small[key][i], big[key][i]), (key, i)


def test_reset_rerun_reproduces_the_cross_bits():
    p = _params(go1_params)
    B, K = 8, 30
    s = rough_streams(p, B, K)
    a, b = run_cross(p, s, B, K, every=3, reset_rerun=True)
    fresh = run_cross(p, s, B, K, every=3)
    for other in (a, b):
        for key in ("x", "vb", "st", "cov", "K"):
            assert np.array_equal(other[key], fresh[key]), key
        for i in range(len(fresh["K"])):
            for key in ("xw", "cw", "l1", "zn"):
                assert np.array_equal(other[key][i], fresh[key][i]), (key, i)


def test_host_and_device_pointers_agree_and_entries_past_k_are_untouched():
    import torch
    lib = capi.load()
    p = _params(go1_params)
    B, ns, N = 5, p.dim_state, p.N
    s = rough_streams(p, B, N + 4)
    est = BatchedEstimator(p, B, solver="direct", smoother=True, cross=True)
    sh = streams_host(s)
    for k in range(N + 4):
        est.push_stream_step(sh, k)
        est.step(k)
        if k not in (1, 7, N - 2, N - 1, N + 3):
            continue
        Kw = min(k + 1, N)
        lh, zh = np.full((B, N - 1, ns, ns), FILL), np.full((B, N, ns, ns), FILL)
        kh = C.c_int(0)
        assert lib.dekf_get_window_cross(est.h, C.byref(kh), lh.ctypes.data, zh.ctypes.data, capi.DEKF_HOST) == capi.DEKF_OK
        assert kh.value == Kw
        assert (lh[:, Kw - 1:] == FILL).all() and (zh[:, Kw:] == FILL).all(), k
        assert np.isfinite(lh[:, :Kw - 1]).all() and np.isfinite(zh[:, :Kw]).all(), k
        ld = torch.full((B, N - 1, ns, ns), FILL, dtype=torch.float64, device="cuda")
        zd = torch.full((B, N, ns, ns), FILL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        kd = C.c_int(0)
        assert lib.dekf_get_window_cross(est.h, C.byref(kd), ld.data_ptr(), zd.data_ptr(), capi.DEKF_DEVICE) == capi.DEKF_OK
        est.sync()
        assert kd.value == Kw
        assert np.array_equal(ld.cpu().numpy(), lh) and np.array_equal(zd.cpu().numpy(), zh), k
        # any of the three pointers may be NULL
        l2 = np.full((B, N - 1, ns, ns), FILL)
        assert lib.dekf_get_window_cross(est.h, None, l2.ctypes.data, None, capi.DEKF_HOST) == capi.DEKF_OK
        assert np.array_equal(l2, lh)
        z2 = np.full((B, N, ns, ns), FILL)
        assert lib.dekf_get_window_cross(est.h, None, None, z2.ctypes.data, capi.DEKF_HOST) == capi.DEKF_OK
        assert np.array_equal(z2, zh)
        k3 = C.c_int(0)
        assert lib.dekf_get_window_cross(est.h, C.byref(k3), None, None, capi.DEKF_HOST) == capi.DEKF_OK and k3.value == Kw
        # window_cross() hands out the written entries
        Kp, lp, zp = est.window_cross()
        assert Kp == Kw and np.array_equal(lp, lh[:, :Kw - 1]) and np.array_equal(zp, zh[:, :Kw])
    est.close()


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
    p = _params(go1_params)
    B, K, bad, t_bad = 6, 34, 2, 26
    s = rough_streams(p, B, K)
    clean = run_cross(p, s, B, K)
    sp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    sp["accel"][t_bad, bad, 0] = np.nan      # (the smoother test's input: poisoned data, no fault)
    pois = run_cross(p, sp, B, K)
    others = [b for b in range(B) if b != bad]
    for key in ("x", "vb", "st", "cov"):
        assert np.array_equal(pois[key][:, others], clean[key][:, others]), key
    assert np.array_equal(pois["K"], clean["K"])
    assert (clean["st"][1:] == capi.DEKF_SOLVE_OK).all()
    assert pois["st"][t_bad, bad] == capi.DEKF_SOLVE_NUMERIC
    n_numeric = 0
    for i in range(len(clean["K"])):
        for key in ("l1", "zn"):
            assert np.array_equal(pois[key][i][others], clean[key][i][others]), (key, i)
            assert np.isfinite(clean[key][i]).all(), (key, i)
        if pois["st"][i + 1, bad] == capi.DEKF_SOLVE_NUMERIC:     # (read tick i + 1: the window arrays start at tick 1)
            n_numeric += 1
            assert np.isnan(pois["l1"][i][bad]).all() and np.isnan(pois["zn"][i][bad]).all(), i
    assert n_numeric >= 1


# ------------------------------------------------------------------ the C++ shim
def test_shim_cross_arrays_equal_batched_estimator(tmp_path):
    exe = build_shim_cross(tmp_path)
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
    est = BatchedEstimator(p, 1, solver="direct", smoother=True, cross=True)
    sh = streams_host(s)
    for k in range(K):
        est.push_stream_step(sh, k)
        est.push_quaternion(np.ascontiguousarray(quats[k][None, :]))
        est.update(k) if k else est.initialize()
        if k:
            row = np.array(rows[k])
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
    est.close()
