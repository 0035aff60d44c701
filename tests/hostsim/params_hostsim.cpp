// TEST INFRASTRUCTURE ONLY.  epoch_hostsim.cpp (unchanged) plus the lane-sequential build of the parameter cores
// (decentralized_ekf_mhe_amd/csrc/mhe_params_core.h): what a direct handle launches once dekf_set_instance_params has given it a table.
// Built as libparams_hostsim.so by tests/instance_params_lib.py.
#include "epoch_hostsim.cpp"

#include "../../decentralized_ekf_mhe_amd/csrc/mhe_params_core.h"

// the two tables of a Sim as the handle keeps them on the device: pc [B] DevCfg, pe [PpEkf::len][B]
struct Tables {
    std::vector<DevCfg> pc;
    std::vector<double> pe;
};

// update(T) of a direct handle with a table, T = 0 included: update_direct_epoch with the parameter cores
template <bool SMOOTH, bool CROSS>
static void update_direct_pp(Sim* h, Epochs* ep, Tables* tb, int T, double* cov, DirectWindow w = DirectWindow(), DirectCross x = DirectCross()) {
    std::vector<double> sm((size_t)DirectScratch::len(h->c.ns), 0.0);
#define DIRECT_SOLVE(LEGS, FEET) direct_solve_t<LEGS, FEET, SMOOTH, CROSS>(tb->pc[b], h->s, b, kstart, K, sm.data(), cov, w, x)
    for (int b = 0; b < h->c.B; ++b) {
        assemble_pp(tb->pc.data(), h->s, b, T, h->pushes, ep->t0.data(), h->lds.data());
        int kstart, K;
        if (direct_window_epoch(tb->pc[b], T, ep->t0[b], kstart, K)) {
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
        if (h->c.N >= 2) marginalize_early_pp(tb->pc.data(), h->s, b, T + 1, ep->t0.data(), h->lds.data());
    }
#undef DIRECT_SOLVE
    h->pushes++;
}

extern "C" {
// the tables of a Sim, every instance on the Sim's own constants
void* hs_tables_create(void* hv) {
    Sim* h = (Sim*)hv;
    const size_t B = (size_t)h->c.B;
    Tables* tb = new Tables();
    tb->pc.assign(B, h->c);
    tb->pe.assign(B * PpEkf::len, 0.0);
    for (size_t b = 0; b < B; ++b) pp_pack_ekf(h->c, tb->pe.data(), B, b);
    return tb;
}
void hs_tables_destroy(void* tv) { delete (Tables*)tv; }

// dekf_set_instance_params: the rows of the instances with set_of[b] >= 0 from fill_noise of their set, and their EKF state at the
// set's initial values.  Returns 0, or 1 when a set differs from `own` (the Sim's parameters) in another field or fails check_noise
int hs_set_instance_params(void* hv, void* tv, const dekf_params* own, const dekf_params* sets, int nsets, const int* set_of) {
    Sim* h = (Sim*)hv;
    Tables* tb = (Tables*)tv;
    const size_t B = (size_t)h->c.B;
    for (int k = 0; k < nsets; ++k)
        if (!same_but_noise(sets[k], *own) || check_noise(sets[k])) return 1;
    for (size_t b = 0; b < B; ++b) {
        if (set_of[b] < 0) continue;
        tb->pc[b] = h->c;
        fill_noise(with_noise_of(*own, sets[set_of[b]]), tb->pc[b]);
        pp_pack_ekf(tb->pc[b], tb->pe.data(), B, b);
        ekf_init_pp(h->c, h->s, (int)b, tb->pe.data());
    }
    return 0;
}
void hs_reset_instances_pp(void* hv, void* ev, void* tv, const int* mask, double* cov) {
    Sim* h = (Sim*)hv;
    Epochs* ep = (Epochs*)ev;
    for (int b = 0; b < h->c.B; ++b)
        if (mask[b]) reset_instance_pp(h->c, h->s, b, cov, ep->t0.data(), ep->c0.data(), h->pushes, h->ekf_count, ((Tables*)tv)->pe.data());
}
void hs_ekf_step_pp(void* hv, void* ev, void* tv) {
    Sim* h = (Sim*)hv;
    for (int b = 0; b < h->c.B; ++b) ekf_tick_pp(h->c, h->s, b, h->ekf_count, ((Epochs*)ev)->c0.data(), ((Tables*)tv)->pe.data());
    h->ekf_count++;
}
// hs_update_direct*_epoch (epoch_hostsim.cpp) with a table
void hs_update_direct_pp(void* hv, void* ev, void* tv, int T, double* cov) {
    update_direct_pp<false, false>((Sim*)hv, (Epochs*)ev, (Tables*)tv, T, cov);
}
void hs_update_direct_smooth_pp(void* hv, void* ev, void* tv, int T, double* cov, double* x_win, double* cov_win) {
    Sim* h = (Sim*)hv;
    std::vector<double> t1((size_t)h->c.B * (h->c.N - 1) * h->c.ns * h->c.ns, 0.0);
    DirectWindow w;
    w.x = x_win;
    w.cov = cov_win;
    w.t1 = t1.data();
    update_direct_pp<true, false>(h, (Epochs*)ev, (Tables*)tv, T, cov, w);
}
void hs_update_direct_cross_pp(void* hv, void* ev, void* tv, int T, double* cov, double* x_win, double* cov_win, double* cov_lag1,
                               double* cov_newest) {
    DirectWindow w;
    w.x = x_win;
    w.cov = cov_win;
    w.t1 = cov_lag1;
    DirectCross x;
    x.newest = cov_newest;
    update_direct_pp<true, true>((Sim*)hv, (Epochs*)ev, (Tables*)tv, T, cov, w, x);
}

// the host derivation: out <- the DevCfg of fill_cfg(*p) (mode 0), or of fill_cfg(*own) followed by fill_noise(*p) (mode 1): the
// bytes must be the same.  Returns sizeof(DevCfg), or -1 when fill_cfg refuses
int hs_cfg_bytes(const dekf_params* own, const dekf_params* p, int B, int mode, unsigned char* out) {
    DevCfg c;
    if (fill_cfg(mode ? *own : *p, B, c)) return -1;
    if (mode) fill_noise(*p, c);
    std::memcpy(out, &c, sizeof(c));
    return (int)sizeof(c);
}
int hs_ekf_table_len(void) { return PpEkf::len; }
}  // extern "C"
