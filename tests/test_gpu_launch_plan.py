"""What a handle launches, frozen: the solve kernel's symbol for full windows and for window-fill ticks (dekf_solve_kernel_name) and its
grid (dekf_launch_info) of every configuration below, at a batch that fills no slot (4) and at one that fills all of them (4096: the grid
is the kernel's slots, not the batch), against tests/golden/launch_plan.json.  The fixture is a record of what the library decided
BEFORE its variant tables and its launch description were folded into one place (tools/record_launch_plan.py wrote it on an MI355X), so
it is no mirror of the code under test.  The direct variants are also restarted (dekf_reset_instances: the epoch twins) and reset (back
to the siblings)."""
import json
import os

import numpy as np
import pytest

import direct_lib as DL
from decentralized_ekf_mhe_amd import capi, cassie_params, go1_params, pogox_params
from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plan.json")
BATCHES = (4, 4096)
MAKERS = {"go1": go1_params, "cassie": cassie_params, "pogox": pogox_params}
# (name, shape, dekf_params fields, BatchedEstimator options, setters called afterwards)
CONFIGS = [
    ("go1", "go1", {}, {}, []),
    ("go1_cap2", "go1", dict(solve_workgroups_per_cu=2), {}, []),
    ("go1_cap4", "go1", dict(solve_workgroups_per_cu=4), {}, []),
    ("go1_polish", "go1", dict(polish=1), {}, []),
    ("go1_warm", "go1", {}, dict(warm_start=True), []),
    ("go1_warm_polish", "go1", dict(polish=1), dict(warm_start=True), []),
    ("go1_warm_cap4", "go1", dict(solve_workgroups_per_cu=4), dict(warm_start=True), []),
    ("go1_warm_off_again", "go1", {}, dict(warm_start=True), [("dekf_set_warm_start", 0)]),
    ("cassie", "cassie", {}, {}, []),
    ("pogox", "pogox", {}, {}, []),
    ("go1_foot", "go1", dict(leg_odom_type=1), {}, []),
    ("go1_pipelined", "go1", dict(solve_pipeline=1), {}, []),
    ("go1_kf", "go1", dict(est_type=1), {}, []),
    ("direct_plain", "go1", {}, dict(solver="direct"), []),
    ("direct_smooth", "go1", {}, dict(solver="direct", smoother=True), []),
    ("direct_cross", "go1", {}, dict(solver="direct", smoother=True, cross=True), []),
    ("direct_smoother_off_after_cross", "go1", {}, dict(solver="direct", smoother=True, cross=True), [("dekf_set_smoother", 0)]),
    ("direct_back_to_admm", "go1", {}, dict(solver="direct", smoother=True, cross=True), [("dekf_set_solver", capi.DEKF_SOLVER_ADMM)]),
]
BY_NAME = {c[0]: c[1:] for c in CONFIGS}
RESTARTED = ("direct_plain", "direct_smooth", "direct_cross")  # at batch 4: also restarted and reset
CASES = [(c[0], B) for c in CONFIGS for B in BATCHES]


def plan(est):
    return [est.solve_kernel_name(True), est.solve_kernel_name(False), est.launch_info()["solve_workgroups"]]


def observe(name, B):
    """{"created": plan} of the configuration at batch B; the restarted ones at batch 4 add "restarted" and "reset" """
    shape, fields, options, setters = BY_NAME[name]
    p = DL._params(MAKERS[shape], **fields)
    est = BatchedEstimator(p, B, **options)
    try:
        for setter, arg in setters:
            capi.check(getattr(est.lib, setter)(est.h, arg))
        seen = {"created": plan(est)}
        if name in RESTARTED and B == 4:
            sh = streams_host(DL.rough_streams(p, B, 5))

            def steps(ks):
                for k in ks:
                    est.push_stream_step(sh, k)
                    est.step(k)

            steps(range(3))  # dekf_initialize and two updates
            assert plan(est) == seen["created"]
            est.reset_instances(np.array([0, 1, 0, 0], np.int32))
            seen["restarted"] = plan(est)
            steps(range(3, 5))
            out = est.get()
            assert np.isfinite(out["x"]).all() and (out["status"] == capi.DEKF_SOLVE_OK).all(), out["status"]
            est.reset()
            seen["reset"] = plan(est)
        return seen
    finally:
        est.close()


def compute_units():
    est = BatchedEstimator(go1_params(), 4)
    try:
        return est.launch_info()["compute_units"]
    finally:
        est.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    have = compute_units()
    if have != g["compute_units"]:
        pytest.skip(f"this device has {have} compute units, {os.path.basename(GOLDEN)} was recorded on one with {g['compute_units']}: "
                    "the grids are not comparable")
    return g


def test_the_fixture_covers_every_case():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert sorted(g["plans"]) == sorted(f"{name}/{B}" for name, B in CASES)


@pytest.mark.parametrize("name,B", CASES, ids=[f"{name}-{B}" for name, B in CASES])
def test_launch_plan(golden, name, B):
    seen = observe(name, B)
    want = golden["plans"][f"{name}/{B}"]
    print(name, B, seen)
    assert seen == want
    if name in RESTARTED and B == 4:  # (what the fixture itself must say: the epoch twins, and the siblings again)
        assert [n + "_ep" for n in want["created"][:2]] == want["restarted"][:2] and want["reset"] == want["created"]
    if name == "go1_kf":
        assert seen["created"][:2] == [None, None]
