// TEST INFRASTRUCTURE ONLY.  innov_hostsim.cpp (unchanged) plus the lane-sequential build of the gate core
// (decentralized_ekf_mhe_amd/csrc/mhe_gate_core.h) behind the plain direct solve and the innovation core: what dekf_update launches on
// a gating handle.  Built as libgate_hostsim.so by tests/gate_lib.py.
#include "innov_hostsim.cpp"

#include "../../decentralized_ekf_mhe_amd/csrc/mhe_gate_core.h"

extern "C" {
// hs_update_direct, then the innovation core and the gate core on every instance, as k_mhe_innov_gate_<L> runs them.  The arrays of
// hs_update_direct_innov, and gated [B][L].  nis_leg_max: the bound (> 0).  leg_odom_type 0 only (returns 1 otherwise, nothing runs)
int hs_update_direct_innov_gate(void* hv, int T, double nis_leg_max, double* cov, double* innov, double* innov_cov, double* nis,
                                double* nis_leg, double* loglik, int* gated) {
    Sim* h = (Sim*)hv;
    if (h->c.ft) return 1;
    update_direct<false, false>(h, T, cov);
    InnovStore out;
    out.nu = innov;
    out.S = innov_cov;
    out.nis = nis;
    out.nis_leg = nis_leg;
    out.loglik = loglik;
    GateStore gs;
    gs.nis_leg_max = nis_leg_max;
    gs.gated = gated;
    std::vector<double> sm((size_t)GateScratch::len(h->c.L), 0.0);
    const int slot = T % h->c.wcap;  // the newest record: (kstart + K - 1) % wcap
#define GATE(LEGS)                                                                                  \
    {                                                                                               \
        const bool solved = innovation_t<LEGS>(h->c, h->s, b, slot, cov, out, sm.data());           \
        gate_t<LEGS>(h->c, h->c, h->s, b, slot, cov, out, gs, solved, sm.data());                   \
    }
    for (int b = 0; b < h->c.B; ++b) {
        switch (h->c.L) {
            case 1: GATE(1) break;
            case 2: GATE(2) break;
            case 3: GATE(3) break;
            default: GATE(4) break;
        }
    }
#undef GATE
    return 0;
}

// the Q_m words of step T's window record, [B][6 L]: every leg's packed 3 x 3 block
void hs_get_record_qm(void* hv, int T, double* qm) {
    Sim* h = (Sim*)hv;
    const int n = 6 * h->c.L;
    for (int b = 0; b < h->c.B; ++b) {
        const double* r = h->s.rec + ((size_t)b * h->c.wcap + T % h->c.wcap) * h->c.rec;
        for (int i = 0; i < n; ++i) qm[(size_t)n * b + i] = r[Rec::qm(h->c.nm) + i];
    }
}
}  // extern "C"
