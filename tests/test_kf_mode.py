"""est_type 1 (kf_core.h) at every leg count, every tick, covariance included: the lane-sequential build of the device cores against the
oracle, both against ref_numpy's textbook filter (tests/kf_lib.py).  The log wraps the record ring about twenty times and sends
instances through a flight phase and an all-stance phase.  The same checks run on the real wavefronts — where kf_predict takes the
matrix-core branch and kf_correct the register-resident Gauss-Jordan — in tests/test_gpu_kf_mode.py.

Measured here (3 instances x 130 ticks per shape, worst over shapes):
  9 states     x 3.9e-16, covariance 3.3e-15 against the oracle; oracle against numpy 1.3e-15; asymmetry 1.6e-15; smallest eigenvalue
               of the symmetrised covariance >= 0.6 of its smallest diagonal entry
  foot states  x 0.34 x the tolerance; covariance 3.0e-2 (full) / 1.9e-5 (base 9 x 9 block) against the oracle, where oracle and
               numpy differ by 1.3e-2 / 1.3e-5: the covariance-form filter amplifies rounding by ~1e10 once a foot has swung
               (test_foot_states.py::test_kf_with_foot_states_and_its_conditioning), so the yardstick is the references' own spread"""
import numpy as np
import pytest

import kf_lib as KF


@pytest.mark.parametrize("shape", list(KF.SHAPES))
def test_nine_states_every_tick_three_ways(shape):
    p, s, orc, ref = KF.case(shape, 0)
    got = KF.hostsim_run(p, s)
    assert np.abs(got["quat"] - orc["quat"]).max() < 1e-12
    KF.check_nine_states(shape, got, tol_x=1e-12, tol_vb=1e-12, tol_cov=1e-12, who="hostsim")
    # the numpy filter holds hostsim as it holds the oracle
    assert KF.cov_err(got["cov"], ref["cov"]) <= 1e-12 and KF.x_err(got["x"], ref["x"]) <= 1e-12


@pytest.mark.parametrize("shape", list(KF.SHAPES))
def test_foot_states_every_tick_within_the_references_spread(shape):
    p, s, orc, ref = KF.case(shape, 1)
    got = KF.hostsim_run(p, s)
    assert got["cov"].shape == (KF.K, KF.B, p.dim_state, p.dim_state) and p.dim_state == 9 + 3 * p.num_legs
    KF.check_foot_states(shape, got, who="hostsim")
    # against the numpy filter: the same allowance (hostsim is one more implementation of the recursion)
    spread_full = KF.cov_err(orc["cov"], ref["cov"])
    assert KF.cov_err(got["cov"], ref["cov"]) <= 10.0 * spread_full
    assert np.isfinite(got["cov"]).all() and KF.asymmetry(got["cov"]) <= 1e-12


def test_the_log_exercises_what_it_claims():
    """the ring wraps, the flight and all-stance phases are there, and the flight phase is felt by the covariance"""
    p, s, orc, ref = KF.case("go1", 0)
    assert KF.K // (p.N + 1) >= 20
    c = s["contact"]
    assert not c[25:55, 0].any() and c[60:85, 1].all() and not c[90:93, 2].any() and c[24, 0].any() and not c[59, 1].all()
    v_var = orc["cov"][:, :, 3, 3]
    assert (np.diff(v_var[25:55, 0]) > 0).all()        # no foot on the ground: the velocity is dead-reckoned, its variance grows
    assert v_var[54, 0] > v_var[24, 0]
