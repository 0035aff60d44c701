// TEST INFRASTRUCTURE ONLY.  params_hostsim.cpp (unchanged) plus the lane-sequential build of the pause cores
// (decentralized_ekf_mhe_amd/csrc/mhe_pause_core.h): what a direct handle launches once dekf_set_active has paused an instance, and the
// host's books of the pauses as dekf_capi.hip keeps them, through the same functions.  Built as libpause_hostsim.so by tests/pause_lib.py.
#include "params_hostsim.cpp"

#include "../../decentralized_ekf_mhe_amd/csrc/mhe_pause_core.h"

// the books of a Sim: who runs, and the next local step and local EKF count of who does not.  (Epochs is the device's image: the
// sentinel while an instance is paused.)
struct Pauses {
    std::vector<int> active, step, count;
};

// update(T) of a direct handle that has paused an instance: update_direct_epoch with the assemble that skips a paused one; the solve
// and the arrival cost ahead of time are the epoch cores as they are
template <bool SMOOTH, bool CROSS>
static void update_direct_pause(Sim* h, Epochs* ep, int T, double* cov, DirectWindow w = DirectWindow(), DirectCross x = DirectCross()) {
    std::vector<double> sm((size_t)DirectScratch::len(h->c.ns), 0.0);
#define DIRECT_SOLVE(LEGS, FEET) direct_solve_t<LEGS, FEET, SMOOTH, CROSS>(h->c, h->s, b, kstart, K, sm.data(), cov, w, x)
    for (int b = 0; b < h->c.B; ++b) {
        assemble_active(h->c, h->s, b, T, h->pushes, ep->t0.data(), h->lds.data());
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
void* hs_pauses_create(int B) {
    Pauses* pz = new Pauses();
    pz->active.assign((size_t)B, 1);
    pz->step.assign((size_t)B, 0);
    pz->count.assign((size_t)B, 0);
    return pz;
}
void hs_pauses_destroy(void* pv) { delete (Pauses*)pv; }

// dekf_set_active between update(T0 - 1) and update(T0): active [B], the whole mask.  Returns how many entries changed
int hs_set_active(void* hv, void* ev, void* pv, const int* active) {
    Sim* h = (Sim*)hv;
    Epochs* ep = (Epochs*)ev;
    Pauses* pz = (Pauses*)pv;
    int n = 0;
    for (int b = 0; b < h->c.B; ++b)
        n += set_active_instance(b, active[b], pz->active.data(), pz->step.data(), pz->count.data(), ep->t0.data(), ep->c0.data(), h->pushes,
                                 h->ekf_count, h->c.ekf_hist);
    return n;
}
void hs_get_active(void* pv, int* active) {
    Pauses* pz = (Pauses*)pv;
    for (size_t b = 0; b < pz->active.size(); ++b) active[b] = pz->active[b];
}
// dekf_reset_instances on a handle that keeps books: a restarted instance is active
void hs_reset_instances_pause(void* hv, void* ev, void* pv, const int* mask, double* cov) {
    Sim* h = (Sim*)hv;
    Epochs* ep = (Epochs*)ev;
    Pauses* pz = (Pauses*)pv;
    for (int b = 0; b < h->c.B; ++b) {
        if (!mask[b]) continue;
        reset_instance(h->c, h->s, b, cov, ep->t0.data(), ep->c0.data(), h->pushes, h->ekf_count);
        restart_instance(b, pz->active.data(), ep->t0.data(), ep->c0.data(), h->pushes, h->ekf_count);
    }
}
// dekf_push_vo of such a handle: a sample for a paused instance is dropped
void hs_push_vo_pause(void* hv, void* ev, const int* mask, const double* t_pre, const double* t_now, const double* dp, const double* t_pose,
                      const double* q_vo) {
    Sim* h = (Sim*)hv;
    for (int b = 0; b < h->c.B; ++b)
        if (mask[b]) latch_vo_active(h->s, b, ((Epochs*)ev)->t0.data(), t_pre, t_now, dp, t_pose, q_vo);
}
void hs_ekf_step_pause(void* hv, void* ev) {
    Sim* h = (Sim*)hv;
    for (int b = 0; b < h->c.B; ++b) ekf_tick_active(h->c, h->s, b, h->ekf_count, ((Epochs*)ev)->c0.data());
    h->ekf_count++;
}
// the local step of every instance at the handle's step T, a paused one's frozen
void hs_instance_ticks_pause(void* ev, void* pv, int T, int* ticks) {
    Epochs* ep = (Epochs*)ev;
    Pauses* pz = (Pauses*)pv;
    for (size_t b = 0; b < ep->t0.size(); ++b) ticks[b] = instance_tick((int)b, T, pz->active.data(), pz->step.data(), ep->t0.data());
}
// hs_update_direct*_epoch (epoch_hostsim.cpp) of a handle that has paused an instance
void hs_update_direct_pause(void* hv, void* ev, int T, double* cov) { update_direct_pause<false, false>((Sim*)hv, (Epochs*)ev, T, cov); }
void hs_update_direct_smooth_pause(void* hv, void* ev, int T, double* cov, double* x_win, double* cov_win) {
    Sim* h = (Sim*)hv;
    std::vector<double> t1((size_t)h->c.B * (h->c.N - 1) * h->c.ns * h->c.ns, 0.0);
    DirectWindow w;
    w.x = x_win;
    w.cov = cov_win;
    w.t1 = t1.data();
    update_direct_pause<true, false>(h, (Epochs*)ev, T, cov, w);
}
void hs_update_direct_cross_pause(void* hv, void* ev, int T, double* cov, double* x_win, double* cov_win, double* cov_lag1, double* cov_newest) {
    DirectWindow w;
    w.x = x_win;
    w.cov = cov_win;
    w.t1 = cov_lag1;
    DirectCross x;
    x.newest = cov_newest;
    update_direct_pause<true, true>((Sim*)hv, (Epochs*)ev, T, cov, w, x);
}

// The host's arithmetic alone, on one instance with epochs (t0, c0) = (0, c0) of a handle at EKF tick count `count`, history depth H:
// the instance is paused at `count`, the handle counts on to `later` and is folded `folds` times on the way (dekf_ekf_step's fold at
// count_old = later: count_new = H + later % H, each time), then the instance resumes.  out[0]: the device's c0 while paused, after the
// folds (the sentinel); out[1]: the local count stored; out[2]: the handle's count at the resume; out[3]: the c0 of the resume
void hs_pause_fold_resume(int c0, int count, int later, int folds, int H, int* out) {
    int active = 1, step = 0, cnt = 0, t0 = 0;
    set_active_instance(0, 0, &active, &step, &cnt, &t0, &c0, 7, count, H);
    int now = later;
    for (int i = 0; i < folds; ++i) {
        const int folded = H + now % H;
        c0 = fold_epoch_active(c0, now, folded, H);
        now = folded;
    }
    out[0] = c0;
    out[1] = cnt;
    out[2] = now;
    set_active_instance(0, 1, &active, &step, &cnt, &t0, &c0, 7, now, H);
    out[3] = c0;
}
int hs_epoch_paused_sentinel(void) { return DEKF_EPOCH_PAUSED; }
}  // extern "C"
