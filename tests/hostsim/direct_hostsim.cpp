// TEST INFRASTRUCTURE ONLY.  hostsim.cpp (unchanged) plus the lane-sequential build of the direct solve core
// (decentralized_ekf_mhe_amd/csrc/mhe_direct_core.h), built as libdirect_hostsim.so by tests/test_direct_solve.py.
#include "hostsim.cpp"

#include "../../decentralized_ekf_mhe_amd/csrc/mhe_direct_core.h"

extern "C" {
// update(T) of a direct handle: the assemble step of hs_update, then the direct core in place of the ADMM solve (what dekf_update
// launches on a direct handle).  cov: [B][ns][ns], Cov(x_T) of every instance.
void hs_update_direct(void* hv, int T, double* cov) {
    Sim* h = (Sim*)hv;
    std::vector<double> sm((size_t)DirectScratch::len(h->c.ns), 0.0);
    const int kstart = T - h->c.N + 1 > 0 ? T - h->c.N + 1 : 0, K = T - kstart + 1;
    for (int b = 0; b < h->c.B; ++b) {
        assemble_update(h->c, h->s, b, T, h->pushes, h->lds.data());
        if (h->c.ft) {
            switch (h->c.L) {
                case 1: direct_solve_t<1, 1>(h->c, h->s, b, kstart, K, sm.data(), cov); break;
                case 2: direct_solve_t<2, 1>(h->c, h->s, b, kstart, K, sm.data(), cov); break;
                case 3: direct_solve_t<3, 1>(h->c, h->s, b, kstart, K, sm.data(), cov); break;
                default: direct_solve_t<4, 1>(h->c, h->s, b, kstart, K, sm.data(), cov); break;
            }
        } else {
            switch (h->c.L) {
                case 1: direct_solve_t<1, 0>(h->c, h->s, b, kstart, K, sm.data(), cov); break;
                case 2: direct_solve_t<2, 0>(h->c, h->s, b, kstart, K, sm.data(), cov); break;
                case 3: direct_solve_t<3, 0>(h->c, h->s, b, kstart, K, sm.data(), cov); break;
                default: direct_solve_t<4, 0>(h->c, h->s, b, kstart, K, sm.data(), cov); break;
            }
        }
    }
    h->pushes++;
}
}  // extern "C"
