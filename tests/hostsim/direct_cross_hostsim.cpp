// TEST INFRASTRUCTURE ONLY.  direct_smooth_hostsim.cpp (unchanged) plus the lane-sequential build of the direct core's CROSS instantiation
// (decentralized_ekf_mhe_amd/csrc/mhe_direct_core.h: the window cross-covariances), built as libdirect_cross_hostsim.so by
// tests/test_direct_cross.py.
#include "direct_smooth_hostsim.cpp"

extern "C" {
// update(T) of a cross handle: hs_update_direct_smooth with the CROSS core.  cov, x_win and cov_win as there; cov_lag1: [B][N-1][ns][ns],
// the core's T1 store itself, of which the K - 1 first entries end as Cov(x_k, x_{k+1}); cov_newest: [B][N][ns][ns], of which the
// K = min(T + 1, N) first entries receive Cov(x_k, x_T).
void hs_update_direct_cross(void* hv, int T, double* cov, double* x_win, double* cov_win, double* cov_lag1, double* cov_newest) {
    Sim* h = (Sim*)hv;
    const int ns = h->c.ns, N = h->c.N;
    std::vector<double> sm((size_t)DirectScratch::len(ns), 0.0);
    DirectWindow w;
    w.x = x_win;
    w.cov = cov_win;
    w.t1 = cov_lag1;
    DirectCross x;
    x.newest = cov_newest;
    const int kstart = T - N + 1 > 0 ? T - N + 1 : 0, K = T - kstart + 1;
    for (int b = 0; b < h->c.B; ++b) {
        assemble_update(h->c, h->s, b, T, h->pushes, h->lds.data());
        if (h->c.ft) {
            switch (h->c.L) {
                case 1: direct_solve_t<1, 1, true, true>(h->c, h->s, b, kstart, K, sm.data(), cov, w, x); break;
                case 2: direct_solve_t<2, 1, true, true>(h->c, h->s, b, kstart, K, sm.data(), cov, w, x); break;
                case 3: direct_solve_t<3, 1, true, true>(h->c, h->s, b, kstart, K, sm.data(), cov, w, x); break;
                default: direct_solve_t<4, 1, true, true>(h->c, h->s, b, kstart, K, sm.data(), cov, w, x); break;
            }
        } else {
            switch (h->c.L) {
                case 1: direct_solve_t<1, 0, true, true>(h->c, h->s, b, kstart, K, sm.data(), cov, w, x); break;
                case 2: direct_solve_t<2, 0, true, true>(h->c, h->s, b, kstart, K, sm.data(), cov, w, x); break;
                case 3: direct_solve_t<3, 0, true, true>(h->c, h->s, b, kstart, K, sm.data(), cov, w, x); break;
                default: direct_solve_t<4, 0, true, true>(h->c, h->s, b, kstart, K, sm.data(), cov, w, x); break;
            }
        }
    }
    h->pushes++;
}
}  // extern "C"
