// TEST INFRASTRUCTURE ONLY.  hostsim.cpp (unchanged) plus the lane-sequential build of the direct solve core
// (decentralized_ekf_mhe_amd/csrc/mhe_direct_core.h) in its three instantiations: plain, SMOOTH (the window smoother) and CROSS (the
// window cross-covariances).  Built as libdirect_hostsim.so by tests/direct_lib.py.
#include "hostsim.cpp"

#include "../../decentralized_ekf_mhe_amd/csrc/mhe_direct_core.h"

// update(T) of a direct handle: the assemble step of hs_update, then the direct core in place of the ADMM solve (what dekf_update
// launches on a direct handle)
template <bool SMOOTH, bool CROSS>
static void update_direct(Sim* h, int T, double* cov, DirectWindow w = DirectWindow(), DirectCross x = DirectCross()) {
    std::vector<double> sm((size_t)DirectScratch::len(h->c.ns), 0.0);
    const int kstart = T - h->c.N + 1 > 0 ? T - h->c.N + 1 : 0, K = T - kstart + 1;
#define DIRECT_SOLVE(LEGS, FEET) direct_solve_t<LEGS, FEET, SMOOTH, CROSS>(h->c, h->s, b, kstart, K, sm.data(), cov, w, x)
    for (int b = 0; b < h->c.B; ++b) {
        assemble_update(h->c, h->s, b, T, h->pushes, h->lds.data());
        if (h->c.ft) {
            switch (h->c.L) {
                case 1: DIRECT_SOLVE(1, 1); break;
                case 2: DIRECT_SOLVE(2, 1); break;
                case 3: DIRECT_SOLVE(3, 1); break;
                default: DIRECT_SOLVE(4, 1); break;
            }
        } else {
            switch (h->c.L) {
                case 1: DIRECT_SOLVE(1, 0); break;
                case 2: DIRECT_SOLVE(2, 0); break;
                case 3: DIRECT_SOLVE(3, 0); break;
                default: DIRECT_SOLVE(4, 0); break;
            }
        }
    }
#undef DIRECT_SOLVE
    h->pushes++;
}

extern "C" {
// cov: [B][ns][ns], Cov(x_T) of every instance.
void hs_update_direct(void* hv, int T, double* cov) { update_direct<false, false>((Sim*)hv, T, cov); }

// hs_update_direct with the SMOOTH core.  x_win: [B][N][ns] and cov_win: [B][N][ns][ns], of which the K = min(T + 1, N) first window
// positions are written (0 the oldest step).  The core's T1 store is private to the call.
void hs_update_direct_smooth(void* hv, int T, double* cov, double* x_win, double* cov_win) {
    Sim* h = (Sim*)hv;
    std::vector<double> t1((size_t)h->c.B * (h->c.N - 1) * h->c.ns * h->c.ns, 0.0);
    DirectWindow w;
    w.x = x_win;
    w.cov = cov_win;
    w.t1 = t1.data();
    update_direct<true, false>(h, T, cov, w);
}

// hs_update_direct_smooth with the CROSS core.  cov_lag1: [B][N-1][ns][ns], the core's T1 store itself, of which the K - 1 first entries
// end as Cov(x_k, x_{k+1}); cov_newest: [B][N][ns][ns], of which the K first entries receive Cov(x_k, x_T).
void hs_update_direct_cross(void* hv, int T, double* cov, double* x_win, double* cov_win, double* cov_lag1, double* cov_newest) {
    DirectWindow w;
    w.x = x_win;
    w.cov = cov_win;
    w.t1 = cov_lag1;
    DirectCross x;
    x.newest = cov_newest;
    update_direct<true, true>((Sim*)hv, T, cov, w, x);
}
}  // extern "C"
