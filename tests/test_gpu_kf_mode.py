"""est_type 1 on the device (k_kf_initialize / k_kf_update), every leg count, every tick, covariance included, against the oracle
(tests/kf_lib.py; the lane-sequential twin of these checks is tests/test_kf_mode.py).  Two branches of kf_core.h exist in the device build
only and run nowhere else: kf_predict's C <- A C A' on the matrix core (v_mfma_f64_16x16x4_f64 over zero-padded 9 x 9 tiles, in-place
overwrite of C), taken with 9 states, and kf_correct's register-resident Gauss-Jordan gj_columns<3 L> of H C H' + C_meas, one
instantiation per leg count.  dekf_get_kf_cov is the first branch's one direct output.

9 states: the two references agree to 3e-15, so x, v_b and the covariance are held to the project's KF tolerance of 1e-9 — a wrong lane
map, a lost G C G' term, a stale read of C after the in-place store or a wrong column count are orders above it.
Foot states (generic predict in LDS, gj_columns<3 L>): the covariance-form filter amplifies rounding by ~1e10, two correct fp64
implementations differ by ~1e-2 in C; the device is held to 10 x the spread between oracle and numpy on the same ticks.

Measured on an MI355X (worst over 3 instances x 130 ticks, against the oracle):
  9 states     x / v_b / covariance  L = 1: 1.9e-16 / 2.2e-16 / 1.4e-15   L = 2: 4.4e-16 / 4.4e-16 / 2.0e-15
                                     L = 3: 3.3e-16 / 3.6e-16 / 3.3e-15   L = 4: 3.3e-16 / 3.1e-16 / 3.0e-15   asymmetry <= 2.0e-15
  foot states  x 0.37 / 2.0 / 1.05 / 0.93 x the tolerance at L = 1 .. 4; covariance over the references' spread 1.8 / 1.9 / 1.2 / 1.9
               (full) and 3.1 / 6.6 / 1.0 / 1.9 (base 9 x 9 block)"""
import ctypes as C

import numpy as np
import pytest

import kf_lib as KF

pytestmark = pytest.mark.gpu
KF_TOL = 1e-9      # as in test_gpu_parity.py::test_kf_mode_matches_oracle


@pytest.mark.parametrize("shape", list(KF.SHAPES))
def test_nine_states_every_leg_count_every_tick(shape):
    """the matrix-core predict and gj_columns<3>, <6>, <9>, <12>"""
    p, s, orc, ref = KF.case(shape, 0)
    got = KF.gpu_run(p, s)
    assert np.abs(got["quat"] - orc["quat"]).max() < 1e-9
    KF.check_nine_states(shape, got, tol_x=KF_TOL, tol_vb=KF_TOL, tol_cov=KF_TOL, who="gpu")


@pytest.mark.parametrize("shape", list(KF.SHAPES))
def test_foot_states_every_leg_count_every_tick(shape):
    """the generic predict in LDS and gj_columns<3 L> at ns = 12, 15, 18, 21"""
    p, s, orc, ref = KF.case(shape, 1)
    got = KF.gpu_run(p, s)
    assert got["cov"].shape == (KF.K, KF.B, p.dim_state, p.dim_state)
    assert np.abs(got["quat"] - orc["quat"]).max() < 1e-9
    assert np.isfinite(got["cov"]).all()
    KF.check_foot_states(shape, got, who="gpu")


def _placed(p, one, batch, positions, nsteps):
    """a batch of different logs with instance 0 of `one` copied to `positions`"""
    s = KF.streams(p, batch, nsteps, first_instance=7)
    for key, v in s.items():
        if isinstance(v, np.ndarray) and v.shape[:2] == (nsteps, batch):
            for pos in positions:
                v[:, pos] = one[key][:, 0]
    return s


@pytest.mark.parametrize("foot", [0, 1], ids=["nine-states", "foot-states"])
def test_an_instance_computes_the_same_bits_wherever_it_sits(foot):
    """one log alone (B = 1), at positions 0, 17 and 36 of B = 37 and at position 64 of B = 65, the other instances on other logs: x, v_b
    and the covariance agree bit for bit at every tick — nothing of an instance depends on its block index or its neighbours"""
    p = KF.params("go1", foot)
    nsteps = 40                                    # the ring wraps six times, flight from tick 25 on
    one = KF.streams(p, 1, nsteps)
    alone = KF.gpu_run(p, one)
    assert np.abs(alone["cov"]).max() > 0 and np.abs(alone["v_b"][1:]).max() > 1e-3
    for batch, positions in ((37, (0, 17, 36)), (65, (64,))):
        s = _placed(p, one, batch, positions, nsteps)
        got = KF.gpu_run(p, s)
        others = [b for b in range(batch) if b not in positions]
        assert not np.array_equal(got["x"][:, others[0]], alone["x"][:, 0])          # the neighbours do run other logs
        for pos in positions:
            for key in ("x", "v_b", "quat", "cov"):
                assert np.array_equal(got[key][:, pos], alone[key][:, 0]), (batch, pos, key)


@pytest.mark.parametrize("foot", [0, 1], ids=["nine-states", "foot-states"])
def test_kf_cov_device_pointer_equals_host_pointer(foot):
    """dekf_get_kf_cov into a device tensor (as test_gpu_configs.py::test_ekf_cov_device_pointer_equals_host_pointer)"""
    import torch
    from decentralized_ekf_mhe_amd import capi
    from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host
    p = KF.params("go1", foot)
    batch, nsteps, ns = 37, 12, p.dim_state
    s = streams_host(KF.streams(p, batch, nsteps))
    est = BatchedEstimator(p, batch)
    for k in range(nsteps):
        est.push_stream_step(s, k)
        est.step(k)
    host = est.kf_cov()
    dev = torch.full((batch, ns, ns), float("nan"), dtype=torch.float64, device="cuda")
    # the fill runs on torch's stream and the handle's own stream is non-blocking: the tensor must be complete before the getter copies
    # into it in the handle's stream order, or the fill can land on top of the copy
    torch.cuda.synchronize()
    capi.check(est.lib.dekf_get_kf_cov(est.h, C.c_void_p(dev.data_ptr()), capi.DEKF_DEVICE))
    est.sync()
    est.close()
    assert host.shape == (batch, ns, ns) and np.isfinite(host).all()
    assert np.array_equal(dev.cpu().numpy(), host)
    assert KF.asymmetry(host) <= KF_TOL and (np.einsum("bii->bi", host) > 0).all()
    assert len({host[b].tobytes() for b in range(batch)}) == batch                    # every instance its own covariance


@pytest.mark.parametrize("shape,foot", [("go1", 0), ("cassie", 1)])
def test_reset_and_rerun_reproduce_the_bits(shape, foot):
    from decentralized_ekf_mhe_amd.estimator import BatchedEstimator
    p = KF.params(shape, foot)
    nsteps = 40
    s = KF.streams(p, KF.B, nsteps)
    est = BatchedEstimator(p, KF.B)
    first = KF.gpu_run(p, s, est)
    est.reset()
    second = KF.gpu_run(p, s, est)
    est.close()
    assert np.abs(first["v_b"][1:]).max() > 1e-3 and not first["v_b"][0].any()
    for key in ("x", "v_b", "quat", "cov"):
        assert np.array_equal(first[key], second[key]), key
