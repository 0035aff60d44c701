"""Warm start (dekf_set_warm_start, BatchedEstimator(warm_start=True)) on the GPU: every tick against the cold CPU oracle with the
yardstick of test_gpu_parity.py (per 3-block |gpu - oracle|_inf <= 1e-4 |oracle|_inf + 1e-6), against the exact optimum of the
oracle's QP, the per-instance warm/cold decision, bit-identity with a cold run where the contract says cold, bit-identity across
kernel families and batch sizes, reset, call-order errors, polishing, and an instance poisoned by a NaN sample."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import ref_numpy as RN
from decentralized_ekf_mhe_amd import capi, cassie_params, go1_params, pogox_params
from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host
from direct_lib import _params, rough_streams, tripod_params

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-6


def block_err(x, ref, blocks):
    worst = 0.0
    for blk in blocks:
        num = np.abs(x[..., blk] - ref[..., blk]).max(axis=-1)
        den = RTOL * np.abs(ref[..., blk]).max(axis=-1) + ATOL
        worst = max(worst, float((num / den).max()))
    return worst


def base_blocks():
    return [slice(0, 3), slice(3, 6), slice(6, 9)]


def foot_blocks(L):
    return [slice(9 + 3 * i, 12 + 3 * i) for i in range(L)]


def run(p, s, B, K, warm, every=1, reset_rerun=False, on_step=None):
    """x, v_b, status, iters, warm_status at the read ticks (every `every`-th tick and the last)"""
    est = BatchedEstimator(p, B, warm_start=warm)
    sh = streams_host(s)
    reps = 2 if reset_rerun else 1
    res = []
    for _ in range(reps):
        xs, vbs, sts, its, ws, ps = [], [], [], [], [], []
        for k in range(K):
            est.push_stream_step(sh, k)
            est.step(k)
            if on_step:
                on_step(k, est)
            if k % every == 0 or k == K - 1:
                o, info = est.get(), est.solver_info()
                xs.append(o["x"]); vbs.append(o["v_b"]); sts.append(o["status"]); its.append(info["iters"])
                ps.append(info["polish_status"]); ws.append(est.warm_status())
        res.append(dict(x=np.array(xs), vb=np.array(vbs), st=np.array(sts), it=np.array(its), warm=np.array(ws), pol=np.array(ps),
                        kernel=est.lib.dekf_solve_kernel_name(est.h, 1)))
        if reset_rerun:
            est.reset()
            if warm:
                capi.check(est.lib.dekf_set_warm_start(est.h, 1))
    est.close()
    return res if reset_rerun else res[0]


def check_warm_pattern(r, N, ks):
    """0 on every window-fill tick and on the first full one, 1 afterwards (every solve here ends OK)"""
    for i, k in enumerate(ks):
        want = 1 if k >= N else 0
        assert (r["warm"][i] == want).all(), (k, r["warm"][i])


def full_iters(r, ks, N):
    sel = [i for i, k in enumerate(ks) if k >= N]
    return r["it"][sel].astype(float)


# ------------------------------------------------------------------ 1 + 3: parity with the cold oracle at every tick, and warm is warm
CASES = {
    # name: (params, B, K, oracle instances, expected full-window kernel)
    "go1_r3_832": (lambda: _params(go1_params), 832, 45, [0, 1, 2, 3, 768, 769, 770, 831], "k_mhe_solve_r3_4_n20"),
    "cassie": (lambda: _params(cassie_params), 6, 45, None, "k_mhe_solve_r3_2_n20"),
    "pogox_rr": (lambda: _params(pogox_params, N=100), 4, 125, None, "k_mhe_solve_rr_1"),
    "go1_r4": (lambda: _params(go1_params, solve_workgroups_per_cu=4), 600, 45, [0, 5, 300, 599], "k_mhe_solve_r4_4_n20"),
    "tripod_generic": (lambda: tripod_params(), 6, 40, None, None),
    "go1_foot": (lambda: _params(go1_params, leg_odom_type=1), 6, 45, None, None),
}


@functools.lru_cache(maxsize=None)
def case_runs(name):
    mk, B, K, sub, kernel = CASES[name]
    p = mk()
    s = rough_streams(p, B, K)
    warm = run(p, s, B, K, True)
    cold = run(p, s, B, K, False)
    idx = list(range(B)) if sub is None else sub
    so = {k: (np.ascontiguousarray(v[:, idx]) if isinstance(v, np.ndarray) and v.ndim >= 2 and v.shape[1] == B else v) for k, v in s.items()}
    x_ref, vb_ref, _, _ = O.run_streams(p, so, nthreads=8)
    return p, s, warm, cold, idx, x_ref, vb_ref


@pytest.mark.parametrize("name", list(CASES))
def test_warm_parity_with_cold_oracle_every_tick(name):
    p, s, warm, cold, idx, x_ref, vb_ref = case_runs(name)
    K, N = s["imu_t"].shape[0], p.N
    kernel = CASES[name][4]
    if kernel:  # (a warm handle launches the full-window kernel's warm twin, solve_kernels.def)
        assert warm["kernel"].decode() == kernel + "_warm" and cold["kernel"].decode() == kernel
    assert (warm["st"][1:] == capi.DEKF_SOLVE_OK).all()
    x = warm["x"][:, idx]
    # Window-fill ticks and the first full window are the cold solve: the yardstick of test_gpu_parity.py as it is.  A warm solve stops
    # at the first termination check that meets eps 1e-6 (iteration 25 in 94 % of the Go1 solves), where the cold oracle, started from
    # zero, runs to 75: both are OSQP-converged iterates of the same QP, within eps of its optimum from opposite sides, so they differ by
    # up to about twice what either differs from the optimum.  Measured: 1.46-2.09 x the per-block yardstick on the 9-state shapes, 8.3 x
    # on the base states of leg_odom_type 1 (whose own cold contract is 1 x base, 3 x feet).  The exact optimum is the arbiter:
    # test_warm_matches_exact_optimum_of_oracle_qp holds the warm iterate to 1 x of it.
    cold_ticks = slice(1, N)
    warm_ticks = slice(N, None)
    if p.leg_odom_type == 1:
        eb, ef = block_err(x[warm_ticks], x_ref[warm_ticks], base_blocks()), block_err(x[warm_ticks], x_ref[warm_ticks], foot_blocks(p.num_legs))
        print(f"[{name}] warm ticks against the cold oracle: base {eb:.2f} x, feet {ef:.2f} x the yardstick")
        assert block_err(x[cold_ticks], x_ref[cold_ticks], base_blocks()) <= 1.0
        assert block_err(x[cold_ticks], x_ref[cold_ticks], foot_blocks(p.num_legs)) <= 3.0
        assert eb <= 12.0 and ef <= 12.0
    else:
        eb = block_err(x[warm_ticks], x_ref[warm_ticks], base_blocks())
        print(f"[{name}] warm ticks against the cold oracle: {eb:.2f} x the yardstick")
        assert block_err(x[cold_ticks], x_ref[cold_ticks], base_blocks()) <= 1.0
        assert eb <= 3.0
        assert np.abs(warm["vb"][1:, idx] - vb_ref[1:]).max() <= 3 * (RTOL * np.abs(vb_ref).max() + ATOL)
    ks = list(range(K))
    check_warm_pattern(warm, N, ks)
    assert (cold["warm"] == 0).all()
    wi, ci = full_iters(warm, ks, N), full_iters(cold, ks, N)
    print(f"[{name}] full-window mean iterations: warm {wi.mean():.2f} cold {ci.mean():.2f}; "
          f"warm histogram {dict(zip(*np.unique(wi, return_counts=True)))}")
    assert wi.mean() < ci.mean()


# ------------------------------------------------------------------ 4: window-fill ticks and the first full one are the cold bits
@pytest.mark.parametrize("name", ["go1_r3_832", "pogox_rr", "tripod_generic", "go1_foot"])
def test_window_fill_ticks_equal_cold_run(name):
    p, s, warm, cold, *_ = case_runs(name)
    n = p.N  # ticks 0 .. N - 1: window fill and the first full window
    for key in ("x", "vb", "st", "it"):
        assert np.array_equal(warm[key][:n], cold[key][:n]), key


# ------------------------------------------------------------------ 2: against the exact optimum of the oracle's QP
def test_warm_matches_exact_optimum_of_oracle_qp():
    p = _params(go1_params)
    B, K = 4, 34
    s = rough_streams(p, B, K)
    warm = run(p, s, B, K, True)
    nm, ns = 3 * p.num_legs, p.dim_state
    for b in range(B):
        pipe = O.Pipe(p)
        for k in range(K):
            pipe.feed(s, k, b)
            pipe.step(k)
            if k >= p.N + 1 and k % 4 == 1:
                H, g, A, l, u = pipe.est.qp()
                xs = RN.kkt_exact(H, g, A, l, u)[0]
                exact = xs[len(xs) - ns - nm:len(xs) - nm]
                assert block_err(warm["x"][k, b], exact, base_blocks()) <= 1.0, (b, k)


# ------------------------------------------------------------------ 5: the same bits from every kernel family and batch size
def _warm_x(p, s, B, K):
    r = run(p, s, B, K, True, every=5)
    assert (r["warm"][-1] == 1).all()
    return r


def test_warm_families_are_bit_identical():
    K = 45
    go1 = _params(go1_params)
    s = rough_streams(go1, 832, K)
    r3 = _warm_x(go1, s, 832, K)
    assert r3["kernel"].decode() == "k_mhe_solve_r3_4_n20_warm"
    r2 = _warm_x(_params(go1_params, solve_workgroups_per_cu=2), s, 832, K)
    assert r2["kernel"].decode() == "k_mhe_solve_ll_4_n20"
    r4 = _warm_x(_params(go1_params, solve_workgroups_per_cu=4), s, 832, K)
    assert r4["kernel"].decode() == "k_mhe_solve_r4_4_n20_warm"
    for other in (r2, r4):
        for key in ("x", "vb", "st", "it"):
            assert np.array_equal(r3[key], other[key]), key
    # B = 1 against B = 832 for the same robot (instance 5 of the fleet)
    s1 = {k: (v[:, 5:6] if isinstance(v, np.ndarray) and v.ndim >= 2 and v.shape[1] == 832 else v) for k, v in s.items()}
    s1["vo_any"] = s1["vo_mask"].any(axis=1)
    one = _warm_x(go1, s1, 1, K)
    assert np.array_equal(one["x"][:, 0], r3["x"][:, 5]) and np.array_equal(one["it"][:, 0], r3["it"][:, 5])
    # PogoX: rows in registers (rr) against the generic kernel (cap of one workgroup per CU)
    pg = _params(pogox_params, N=100)
    sp = rough_streams(pg, 4, 125)
    rr = _warm_x(pg, sp, 4, 125)
    assert rr["kernel"].decode() == "k_mhe_solve_rr_1_warm"
    gg = _warm_x(_params(pogox_params, N=100, solve_workgroups_per_cu=1), sp, 4, 125)
    assert not gg["kernel"].decode().startswith("k_mhe_solve_rr_1")
    for key in ("x", "vb", "st", "it"):
        assert np.array_equal(rr[key], gg[key]), key


# ------------------------------------------------------------------ 6: reset and errors
def test_reset_rerun_equals_fresh_warm_handle():
    p = _params(go1_params)
    B, K = 8, 32
    s = rough_streams(p, B, K)
    a, b = run(p, s, B, K, True, every=4, reset_rerun=True)
    fresh = run(p, s, B, K, True, every=4)
    for key in ("x", "st", "it", "warm"):
        assert np.array_equal(a[key], fresh[key]), key
        assert np.array_equal(b[key], fresh[key]), key


def test_warm_start_call_order_and_invalid_handles():
    lib = capi.load()
    p = _params(go1_params)
    est = BatchedEstimator(p, 2)
    assert lib.dekf_set_warm_start(est.h, 2) == capi.DEKF_ERR_INVALID
    assert lib.dekf_set_warm_start(est.h, 1) == capi.DEKF_OK
    assert lib.dekf_set_warm_start(est.h, 0) == capi.DEKF_OK
    est.ekf_step()
    est.initialize()
    assert lib.dekf_set_warm_start(est.h, 1) == capi.DEKF_ERR_ORDER
    est.reset()
    assert lib.dekf_set_warm_start(est.h, 1) == capi.DEKF_OK
    est.close()
    with pytest.raises(capi.DekfError) as e:
        BatchedEstimator(_params(go1_params, est_type=1), 2, warm_start=True)
    assert e.value.status == capi.DEKF_ERR_INVALID
    with pytest.raises(capi.DekfError) as e:
        BatchedEstimator(_params(go1_params, solve_pipeline=1), 2, warm_start=True)
    assert e.value.status == capi.DEKF_ERR_INVALID
    # never enabled: every solve reports cold
    est = BatchedEstimator(p, 3)
    assert (est.warm_status() == 0).all()
    est.close()


# ------------------------------------------------------------------ 7: polishing
def test_warm_with_polishing_matches_oracle():
    p = _params(go1_params, polish=1)
    B, K = 6, 40
    s = rough_streams(p, B, K)
    warm = run(p, s, B, K, True)
    x_ref, _, _, _ = O.run_streams(p, s, nthreads=8)
    assert (warm["st"][1:] == capi.DEKF_SOLVE_OK).all()
    assert block_err(warm["x"][1:], x_ref[1:], base_blocks()) <= 1.0
    check_warm_pattern(warm, p.N, list(range(K)))
    assert np.isin(warm["pol"][1:], (1, -1)).all()      # polishing ran on every solved tick, as it does cold


# ------------------------------------------------------------------ 8: a poisoned instance never seeds a warm start
def test_nan_sample_never_seeds_a_warm_start():
    p = _params(go1_params)
    B, K, bad, t_bad = 6, 34, 2, 26
    s = rough_streams(p, B, K)
    clean = run(p, s, B, K, True)
    sp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    sp["accel"][t_bad, bad, 0] = np.nan
    pois = run(p, sp, B, K, True)
    others = [b for b in range(B) if b != bad]
    for key in ("x", "vb", "st", "it", "warm"):
        assert np.array_equal(pois[key][:, others], clean[key][:, others]), key
    assert pois["st"][t_bad, bad] != capi.DEKF_SOLVE_OK
    assert pois["warm"][t_bad + 1, bad] == 0
    # a tick whose solve was not OK / MAX_ITER with a finite iterate seeds nothing
    for k in range(t_bad, K - 1):
        if not np.isin(pois["st"][k, bad], (capi.DEKF_SOLVE_OK, capi.DEKF_SOLVE_MAX_ITER)):
            assert pois["warm"][k + 1, bad] == 0, k
