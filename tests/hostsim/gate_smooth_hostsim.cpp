// TEST INFRASTRUCTURE ONLY.  gate_hostsim.cpp (unchanged) plus the lane-sequential build of the window correction of a gating handle
// that smooths (decentralized_ekf_mhe_amd/csrc/mhe_gate_window_core.h) behind the SMOOTH direct solve, the innovation core and the
// gate core: what dekf_update launches on a handle with dekf_set_gate_smoother.  Built as libgate_smooth_hostsim.so by
// tests/gate_smooth_lib.py.
#include "gate_hostsim.cpp"

#include "../../decentralized_ekf_mhe_amd/csrc/mhe_gate_window_core.h"

extern "C" {
// hs_update_direct_smooth, then the innovation core on every instance and, with nis_leg_max > 0, the gate core and the window
// correction, as k_mhe_innov_gate_<L>_smooth runs them (nis_leg_max == 0: a smoothing innovation handle without the gate; gated is
// then not touched).  The arrays of hs_update_direct_innov_gate, and x_win [B][N][ns], cov_win [B][N][ns][ns] of which the
// K = min(T + 1, N) first window positions are written.  The T1 store is private to the call.  leg_odom_type 0 only (returns 1
// otherwise, nothing runs)
int hs_update_direct_smooth_innov_gate(void* hv, int T, double nis_leg_max, double* cov, double* x_win, double* cov_win, double* innov,
                                       double* innov_cov, double* nis, double* nis_leg, double* loglik, int* gated) {
    Sim* h = (Sim*)hv;
    if (h->c.ft) return 1;
    std::vector<double> t1((size_t)h->c.B * (h->c.N - 1) * h->c.ns * h->c.ns, 0.0);
    DirectWindow win;
    win.x = x_win;
    win.cov = cov_win;
    win.t1 = t1.data();
    update_direct<true, false>(h, T, cov, win);
    InnovStore out;
    out.nu = innov;
    out.S = innov_cov;
    out.nis = nis;
    out.nis_leg = nis_leg;
    out.loglik = loglik;
    GateStore gs;
    gs.nis_leg_max = nis_leg_max;
    gs.gated = gated;
    std::vector<double> sm((size_t)GateWindowScratch::len(h->c.L), 0.0);
    const int kstart = T - h->c.N + 1 > 0 ? T - h->c.N + 1 : 0, K = T - kstart + 1;
    const int slot = T % h->c.wcap;  // the newest record: (kstart + K - 1) % wcap
#define GATE_SMOOTH(LEGS)                                                                            \
    {                                                                                               \
        const bool solved = innovation_t<LEGS>(h->c, h->s, b, slot, cov, out, sm.data());           \
        bool corrected = false;                                                                     \
        if (nis_leg_max > 0.0 && gate_t<LEGS>(h->c, h->c, h->s, b, slot, cov, out, gs, solved, sm.data(), &corrected)) \
            gate_window_t<LEGS>(h->c, b, K, corrected, win, sm.data());                             \
    }
    for (int b = 0; b < h->c.B; ++b) {
        switch (h->c.L) {
            case 1: GATE_SMOOTH(1) break;
            case 2: GATE_SMOOTH(2) break;
            case 3: GATE_SMOOTH(3) break;
            default: GATE_SMOOTH(4) break;
        }
    }
#undef GATE_SMOOTH
    return 0;
}

// gate_window_t of instance b over K window steps behind a correction that FAILED (gate_t's DEKF_SOLVE_NUMERIC path, which no valid
// input of the harness reaches): x_win [B][N][ns] and cov_win [B][N][ns][ns] as above, the scratch and the T1 store zeroed
void hs_gate_window_failed(void* hv, int b, int K, double* x_win, double* cov_win) {
    Sim* h = (Sim*)hv;
    std::vector<double> t1((size_t)h->c.B * (h->c.N - 1) * h->c.ns * h->c.ns, 0.0);
    DirectWindow win;
    win.x = x_win;
    win.cov = cov_win;
    win.t1 = t1.data();
    std::vector<double> sm((size_t)GateWindowScratch::len(h->c.L), 0.0);
    switch (h->c.L) {
        case 1: gate_window_t<1>(h->c, b, K, false, win, sm.data()); break;
        case 2: gate_window_t<2>(h->c, b, K, false, win, sm.data()); break;
        case 3: gate_window_t<3>(h->c, b, K, false, win, sm.data()); break;
        default: gate_window_t<4>(h->c, b, K, false, win, sm.data()); break;
    }
}
}  // extern "C"
