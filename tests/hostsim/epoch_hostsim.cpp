// TEST INFRASTRUCTURE ONLY.  direct_hostsim.cpp (unchanged) plus the lane-sequential build of the epoch cores
// (decentralized_ekf_mhe_amd/csrc/mhe_epoch_core.h): what a direct handle launches once dekf_reset_instances has restarted an instance.
// Built as libepoch_hostsim.so by tests/epoch_lib.py.
#include "direct_hostsim.cpp"

#include "../../decentralized_ekf_mhe_amd/csrc/mhe_epoch_core.h"

// the epochs of a Sim: t0 | c0 as the handle keeps them on the device
struct Epochs {
    std::vector<int> t0, c0;
};

// update(T) of a direct handle with epochs, T = 0 included (every instance at epoch 0 then takes the initialise path): per instance the
// assemble step, the direct core on its local window and, as dekf_update launches it beside the solve, the arrival cost of step T + 1
template <bool SMOOTH, bool CROSS>
static void update_direct_epoch(Sim* h, Epochs* ep, int T, double* cov, DirectWindow w = DirectWindow(), DirectCross x = DirectCross()) {
    std::vector<double> sm((size_t)DirectScratch::len(h->c.ns), 0.0);
#define DIRECT_SOLVE(LEGS, FEET) direct_solve_t<LEGS, FEET, SMOOTH, CROSS>(h->c, h->s, b, kstart, K, sm.data(), cov, w, x)
    for (int b = 0; b < h->c.B; ++b) {
        assemble_epoch(h->c, h->s, b, T, h->pushes, ep->t0.data(), h->lds.data());
        int kstart, K;
        if (direct_window_epoch(h->c, T, ep->t0[b], kstart, K)) {
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
        if (h->c.N >= 2) marginalize_early_epoch(h->c, h->s, b, T + 1, ep->t0.data(), h->lds.data());
    }
#undef DIRECT_SOLVE
    h->pushes++;
}

extern "C" {
void* hs_epochs_create(int B) {
    Epochs* ep = new Epochs();
    ep->t0.assign((size_t)B, 0);
    ep->c0.assign((size_t)B, 0);
    return ep;
}
void hs_epochs_destroy(void* ev) { delete (Epochs*)ev; }

// dekf_reset_instances between update(T0 - 1) and the pushes of step T0: mask [B], cov [B][ns][ns] the handle's Cov(x_T) store
void hs_reset_instances(void* hv, void* ev, const int* mask, double* cov) {
    Sim* h = (Sim*)hv;
    Epochs* ep = (Epochs*)ev;
    for (int b = 0; b < h->c.B; ++b)
        if (mask[b]) reset_instance(h->c, h->s, b, cov, ep->t0.data(), ep->c0.data(), h->pushes, h->ekf_count);
}
void hs_ekf_step_epoch(void* hv, void* ev) {
    Sim* h = (Sim*)hv;
    for (int b = 0; b < h->c.B; ++b) ekf_tick_epoch(h->c, h->s, b, h->ekf_count, ((Epochs*)ev)->c0.data());
    h->ekf_count++;
}
// the local step of every instance at the handle's step T
void hs_instance_ticks(void* ev, int T, int* ticks) {
    Epochs* ep = (Epochs*)ev;
    for (size_t b = 0; b < ep->t0.size(); ++b) ticks[b] = T - ep->t0[b];
}
// the two epoch arrays as they stand ([B] each)
void hs_epochs_copy(void* ev, int* t0, int* c0) {
    Epochs* ep = (Epochs*)ev;
    for (size_t b = 0; b < ep->t0.size(); ++b) { t0[b] = ep->t0[b]; c0[b] = ep->c0[b]; }
}
// hs_update_direct* (direct_hostsim.cpp) with epochs
void hs_update_direct_epoch(void* hv, void* ev, int T, double* cov) { update_direct_epoch<false, false>((Sim*)hv, (Epochs*)ev, T, cov); }
void hs_update_direct_smooth_epoch(void* hv, void* ev, int T, double* cov, double* x_win, double* cov_win) {
    Sim* h = (Sim*)hv;
    std::vector<double> t1((size_t)h->c.B * (h->c.N - 1) * h->c.ns * h->c.ns, 0.0);
    DirectWindow w;
    w.x = x_win;
    w.cov = cov_win;
    w.t1 = t1.data();
    update_direct_epoch<true, false>(h, (Epochs*)ev, T, cov, w);
}
void hs_update_direct_cross_epoch(void* hv, void* ev, int T, double* cov, double* x_win, double* cov_win, double* cov_lag1, double* cov_newest) {
    DirectWindow w;
    w.x = x_win;
    w.cov = cov_win;
    w.t1 = cov_lag1;
    DirectCross x;
    x.newest = cov_newest;
    update_direct_epoch<true, true>((Sim*)hv, (Epochs*)ev, T, cov, w, x);
}
// the host's fold of its EKF tick count (dekf_ekf_step) as the epochs see it
int hs_fold_epoch(int c0, int count_old, int count_new, int H) { return fold_epoch(c0, count_old, count_new, H); }
}  // extern "C"
