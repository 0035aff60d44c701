"""The three-workgroup solve kernels (`k_mhe_solve_r3_*`, mhe_admm_core.h: admm_chunk_r3) start their block-tridiagonal chain UNDER the
workers' x-column phase: the solve wavefront computes the x columns of the three outermost blocks at either end of the window itself
(xends_regs_load, XendsHooks::load / finish), the workers' tiles leave those 54 entries out, and the barrier "xs complete" sits inside the unrolled forward legs,
between step 1 and the operand prefetch of step 2 (sweeps_one_wave, before_step2).

Same operations on the same operands, so the contract is BIT identity, at every tick and on every output, with the kernels that do not
run admm_chunk_r3: the two-workgroup kernels (`solve_workgroups_per_cu = 2`: `_ll_` / `_lg_`, all four wavefronts through every phase)
and the four-per-CU kernels (`= 4`: `_r4_`, their own chunk with the barrier in front of the chain).  A `= 4` handle launches `_r4_`
only where that offers more slots than two workgroups per CU do (dekf_capi.hip: take_full_window) — below that it launches `_r3_`
itself and the comparison with it says nothing; the last two tests therefore size their batch from the device so that `_r4_` really
runs, on plain Go1 and with short chunks.
The reference's solve: MheSrb.cpp:340-349 (OSQP), set up per tick by MheSrb.cpp:272-338."""
import numpy as np
import pytest

from decentralized_ekf_mhe_amd import cassie_params, go1_params
from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_to_device
from decentralized_ekf_mhe_amd.streams import make_streams
from test_gpu_parity import _params

pytestmark = pytest.mark.gpu
OUT_KEYS = ("x", "v_b", "quat", "status")
INFO_KEYS = ("iters", "rho_updates", "pri_res", "dua_res", "polish_status")


def _identical_every_tick(p, B, K, r3_name, other_name, warm=False, r4_runs=False):
    """the same logs through a handle without a cap (r3), one capped at two workgroups per CU and one with cap 4"""
    sd = streams_to_device(make_streams(p, B, K))
    ests = []
    for cap in (0, 2, 4):
        q = p.copy()
        q.solve_workgroups_per_cu = cap
        ests.append(BatchedEstimator(q, B, warm_start=warm))
    names = [e.solve_kernel_name(True) for e in ests]
    assert names[0] == r3_name and names[1] == other_name, names
    assert "_r4_" in names[2] if r4_runs else names[2] in (r3_name, r3_name.replace("_r3_", "_r4_")), names
    iters = []
    for k in range(K):
        outs = []
        for e in ests:
            e.push_stream_step(sd, k)
            e.step(k)
            outs.append((e.get(), e.solver_info()))
        (o3, i3) = outs[0]
        for name, (o, i) in zip(names[1:], outs[1:]):
            for key in OUT_KEYS:
                assert np.array_equal(o3[key], o[key]), (k, key, name)
            for key in INFO_KEYS:
                assert np.array_equal(i3[key], i[key]), (k, key, name)
        iters.append(i3["iters"].copy())
    for e in ests:
        e.close()
    return np.array(iters)


@pytest.mark.parametrize("maker,r3_name,other_name", [(go1_params, "k_mhe_solve_r3_4_n20", "k_mhe_solve_ll_4_n20"),
                                                     (cassie_params, "k_mhe_solve_r3_2_n20", "k_mhe_solve_lg_2_n20")], ids=["go1", "cassie"])
def test_r3_gives_the_bits_of_the_other_kernels(maker, r3_name, other_name):
    """70 distinct logs (more than one wavefront of instances), window fill + 30 full windows with vision intervals in the window;
    Cassie's 40 Meas blocks give the workers another tile map"""
    p = _params(maker)
    it = _identical_every_tick(p, 70, p.N + 30, r3_name, other_name)
    assert it[p.N:].min() >= 25


@pytest.mark.parametrize("cap,adapt", [(40, 1), (60, 0)])
def test_short_chunks_keep_the_barriers_matched(cap, adapt):
    """chunks of 15 and of 10 iterations (the cap is no multiple of the termination check / there is no rho adaptation): the barrier
    inside the chain is executed once per iteration by every wavefront, however short the chunk"""
    p = _params(go1_params, max_qp_iter=cap, adapt_rho=adapt)
    it = _identical_every_tick(p, 70, p.N + 30, "k_mhe_solve_r3_4_n20", "k_mhe_solve_ll_4_n20")
    assert it[p.N:].max() == cap


def test_polishing_twin():
    p = _params(go1_params, polish=1)
    _identical_every_tick(p, 70, p.N + 30, "k_mhe_solve_r3_4_n20_pol", "k_mhe_solve_ll_4_n20_pol")


def test_warm_start_twin():
    p = _params(go1_params)
    _identical_every_tick(p, 70, p.N + 30, "k_mhe_solve_r3_4_n20_warm", "k_mhe_solve_ll_4_n20", warm=True)


@pytest.mark.parametrize("B", [1, 3])
def test_fewer_workgroups_than_a_cu_holds(B):
    """one workgroup alone on its CU, which gets no second instance from the queue; three workgroups: at most one CU's worth"""
    p = _params(go1_params)
    _identical_every_tick(p, B, p.N + 30, "k_mhe_solve_r3_4_n20", "k_mhe_solve_ll_4_n20")


def _smallest_batch_that_runs_r4(p):
    """the smallest batch at which a handle with cap 4 launches the four-per-CU kernel: a few instances more than two workgroups per
    CU hold"""
    probe = BatchedEstimator(p, 1)
    B = 2 * probe.launch_info()["compute_units"] + 8
    probe.close()
    return B


def test_r3_gives_the_bits_of_r4_where_r4_runs():
    p = _params(go1_params)
    _identical_every_tick(p, _smallest_batch_that_runs_r4(p), p.N + 12, "k_mhe_solve_r3_4_n20", "k_mhe_solve_ll_4_n20", r4_runs=True)


@pytest.mark.parametrize("cap,adapt", [(40, 1), (60, 0)])
def test_short_chunks_give_the_bits_of_r4_where_r4_runs(cap, adapt):
    """the chunks of 15 and of 10 iterations against the kernel whose barrier "xs complete" still stands in front of the chain"""
    p = _params(go1_params, max_qp_iter=cap, adapt_rho=adapt)
    it = _identical_every_tick(p, _smallest_batch_that_runs_r4(p), p.N + 12, "k_mhe_solve_r3_4_n20", "k_mhe_solve_ll_4_n20", r4_runs=True)
    assert it[p.N:].max() == cap
