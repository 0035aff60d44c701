// TEST INFRASTRUCTURE ONLY.  direct_hostsim.cpp (unchanged) plus the lane-sequential build of the innovation core
// (decentralized_ekf_mhe_amd/csrc/mhe_innov_core.h) behind the plain direct solve: what dekf_update launches on an innovation handle.
// Built as libinnov_hostsim.so by tests/innov_lib.py.
#include "direct_hostsim.cpp"

#include "../../decentralized_ekf_mhe_amd/csrc/mhe_innov_core.h"

extern "C" {
// hs_update_direct, then the innovation core on every instance: innov [B][nm], innov_cov [B][nm][nm], nis [B], nis_leg [B][L],
// loglik [B].  leg_odom_type 0 only (returns 1 otherwise, and nothing runs)
int hs_update_direct_innov(void* hv, int T, double* cov, double* innov, double* innov_cov, double* nis, double* nis_leg, double* loglik) {
    Sim* h = (Sim*)hv;
    if (h->c.ft) return 1;
    update_direct<false, false>(h, T, cov);
    InnovStore out;
    out.nu = innov;
    out.S = innov_cov;
    out.nis = nis;
    out.nis_leg = nis_leg;
    out.loglik = loglik;
    std::vector<double> sm((size_t)InnovScratch::len(h->c.L), 0.0);
    const int slot = T % h->c.wcap;  // the newest record: (kstart + K - 1) % wcap
    for (int b = 0; b < h->c.B; ++b) {
        switch (h->c.L) {
            case 1: innovation_t<1>(h->c, h->s, b, slot, cov, out, sm.data()); break;
            case 2: innovation_t<2>(h->c, h->s, b, slot, cov, out, sm.data()); break;
            case 3: innovation_t<3>(h->c, h->s, b, slot, cov, out, sm.data()); break;
            default: innovation_t<4>(h->c, h->s, b, slot, cov, out, sm.data()); break;
        }
    }
    return 0;
}
}  // extern "C"
