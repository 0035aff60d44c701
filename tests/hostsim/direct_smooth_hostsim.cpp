// TEST INFRASTRUCTURE ONLY.  direct_hostsim.cpp (unchanged) plus the lane-sequential build of the direct core's SMOOTH instantiation
// (decentralized_ekf_mhe_amd/csrc/mhe_direct_core.h: the window smoother), built as libdirect_smooth_hostsim.so by
// tests/test_direct_smoother.py.
#include "direct_hostsim.cpp"

extern "C" {
// update(T) of a smoothing direct handle: hs_update_direct with the SMOOTH core.  cov: [B][ns][ns]; x_win: [B][N][ns] and cov_win:
// [B][N][ns][ns], of which the K = min(T + 1, N) first window positions are written (0 the oldest step).
void hs_update_direct_smooth(void* hv, int T, double* cov, double* x_win, double* cov_win) {
    Sim* h = (Sim*)hv;
    const int ns = h->c.ns, N = h->c.N;
    std::vector<double> sm((size_t)DirectScratch::len(ns), 0.0);
    std::vector<double> t1((size_t)h->c.B * (N - 1) * ns * ns, 0.0);
    DirectWindow w;
    w.x = x_win;
    w.cov = cov_win;
    w.t1 = t1.data();
    const int kstart = T - N + 1 > 0 ? T - N + 1 : 0, K = T - kstart + 1;
    for (int b = 0; b < h->c.B; ++b) {
        assemble_update(h->c, h->s, b, T, h->pushes, h->lds.data());
        if (h->c.ft) {
            switch (h->c.L) {
                case 1: direct_solve_t<1, 1, true>(h->c, h->s, b, kstart, K, sm.data(), cov, w); break;
                case 2: direct_solve_t<2, 1, true>(h->c, h->s, b, kstart, K, sm.data(), cov, w); break;
                case 3: direct_solve_t<3, 1, true>(h->c, h->s, b, kstart, K, sm.data(), cov, w); break;
                default: direct_solve_t<4, 1, true>(h->c, h->s, b, kstart, K, sm.data(), cov, w); break;
            }
        } else {
            switch (h->c.L) {
                case 1: direct_solve_t<1, 0, true>(h->c, h->s, b, kstart, K, sm.data(), cov, w); break;
                case 2: direct_solve_t<2, 0, true>(h->c, h->s, b, kstart, K, sm.data(), cov, w); break;
                case 3: direct_solve_t<3, 0, true>(h->c, h->s, b, kstart, K, sm.data(), cov, w); break;
                default: direct_solve_t<4, 0, true>(h->c, h->s, b, kstart, K, sm.data(), cov, w); break;
            }
        }
    }
    h->pushes++;
}
}  // extern "C"
