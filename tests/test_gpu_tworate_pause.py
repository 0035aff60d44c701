"""Pausing single instances of a two-rate direct handle on the GPU (EKF 500 Hz, MHE 200 Hz: tworate_lib's event grid) under
pause_lib.two_rate_pauses: a pause behind an EKF tick of its gap, resumed on the ms at which a VO pose stamped during the pause
arrives; a pause directly behind an update; an instance never resumed.  Every paused instance against a fresh handle driven over the
grid without its paused ms, every other instance against the handle that runs the whole grid, on every getter, to the bit."""
import pytest

import direct_lib as DL
import pause_lib as PZ
import tworate_lib as TL
from decentralized_ekf_mhe_amd.estimator import BatchedEstimator

pytestmark = pytest.mark.gpu


class GpuPauseDev(TL.GpuDev):
    """tworate_lib.GpuDev with dekf_set_active, and dekf_get_active in every record"""

    def set_active(self, mask):
        import numpy as np
        self.est.set_active(np.ascontiguousarray(mask, np.int32))
        self.names.append((self.est.solve_kernel_name(True), self.est.solve_kernel_name(False)))

    def record(self, T):
        return dict(super().record(T), active=self.est.active())


@pytest.mark.parametrize("variant", ["plain", "cross"])
def test_two_rate_pauses_against_the_cut_grid(variant):
    name, H, B = "go1", 256, 6
    p0 = TL.SHAPES[name](H)
    made = []

    def dev(cls):
        made.append(cls(BatchedEstimator(p0, B, solver="direct", **DL.VARIANTS[variant]), variant))
        return made[-1]

    try:
        p, s, got, refs, pauses = PZ.two_rate_run(name, H, B, lambda: dev(GpuPauseDev), lambda: dev(TL.GpuDev))
    finally:
        for d in made:
            d.est.close()
    PZ.check_two_rate(p, got, refs, TL.gpu_fresh(name, H, B, variant), pauses, B, PZ.GPU_KEYS)
    kernel = "k_mhe_solve_direct_4_n20"
    sibling, twin = kernel + PZ.EL.SIBLING_SUFFIX[variant], kernel + PZ.EL.TWIN_SUFFIX[variant]
    assert made[0].names[0] == (sibling, sibling) and made[0].names[1:] == [(twin, twin)] * 5
    (_, a0, r0), _, _ = pauses
    T_resume = TL.first_step(r0)
    assert got[T_resume - 1]["ticks"][0] == 12 and got[T_resume]["ticks"][0] == 13 and got[-1]["active"].tolist() == [1, 1, 0, 1, 1, 1]
