// mhe_epoch_core.h — restarting single instances of a direct handle (dekf_reset_instances).
//
// The step T reaches the device cores as a function argument only (ekf_tick's count, assemble_update's T and pushes, marginalize_early's
// T, direct_solve_t's kstart and K), and everything those cores keep is indexed by the instance: the window records at T % wcap, the
// sample stack at pushes % ring, marg_tag, st_dtime, the EKF history at count % H.  So an instance that starts over needs no state of
// its own kind, only its own arguments: with t0[b] the handle's step and c0[b] its EKF tick count at the restart (its epoch; 0 on an
// instance never restarted) every core below is the existing core called with T - t0[b], pushes - t0[b] and count - c0[b].  At local
// step 0 the instance takes the initialise path.  No core changes, so a restarted instance computes, bit for bit, what a fresh handle
// computes from the samples of its restart step on; an instance with epoch 0 computes what it computed.
// What the restart leaves behind in the instance's rings (records, stack entries and history samples of its earlier life) is never
// read: every core reads back only as far as its local arguments reach, exactly as after dekf_reset, which clears none of it either.
//
// The epochs are two int arrays [B] handed to the kernels of a handle that has restarted an instance (kernels.hip: the *_ep kernels);
// DevCfg and DevState do not know them.  Compiles lane-sequentially like the cores it calls (tests/hostsim/epoch_hostsim.cpp).
#pragma once
#include "cfg.h"
#include "ekf_core.h"
#include "mhe_assemble_core.h"
#include "mhe_direct_core.h"

namespace dekf {

// What k_reset_state does for instance b (one lane per instance): EKF state and covariance at their initial values, VO latches, way
// points and the p_vo accumulator cleared, outputs and solver info zeroed, no arrival cost computed ahead.  (k_reset_state adds the
// warm store's tags; a direct handle has no warm store.)
DEKF_FN void reset_state_of(const DevCfg& c, const DevState& s, int b) {
    const size_t B = (size_t)c.B;
    for (int i = 0; i < 4; ++i) { s.ekf_q[i * B + b] = c.ekf_q0[i]; s.quat[4 * (size_t)b + i] = c.ekf_q0[i]; }
    for (int i = 0; i < 16; ++i) s.ekf_P[i * B + b] = (i % 5 == 0) ? c.ekf_P0[i / 5] : 0.0;
    s.vo_flag[b] = 0;
    s.ekf_vo_flag[b] = 0;
    s.wp_count[b] = 0;
    for (int i = 0; i < 3; ++i) s.p_vo[3 * (size_t)b + i] = 0.0;
    for (int i = 0; i < c.ns; ++i) s.x_mhe[(size_t)c.ns * b + i] = 0.0;
    for (int i = 0; i < 3; ++i) s.v_b[3 * (size_t)b + i] = 0.0;
    s.status[b] = DEKF_SOLVE_NONE;
    s.iters[b] = 0;
    s.rho_updates[b] = 0;
    s.polish_status[b] = 0;
    s.pri_res[b] = 0.0;
    s.dua_res[b] = 0.0;
    s.vo_ins_idx[b] = 0;
    s.vo_ins_dtime[b] = 0;
    s.marg_tag[b] = -1;
}

// dekf_reset_instances for instance b (one lane per instance): reset_state_of, its block of Cov(x_T) ([B][ns][ns]) NaN until its first
// solve, and its epoch: the handle's step (next_T) and EKF tick count at the call.
DEKF_FN void reset_instance(const DevCfg& c, const DevState& s, int b, double* cov, int* t0, int* c0, int next_T, int ekf_count) {
    reset_state_of(c, s, b);
    const int ns2 = c.ns * c.ns;
    for (int i = 0; i < ns2; ++i) cov[(size_t)ns2 * b + i] = NAN;
    t0[b] = next_T;
    c0[b] = ekf_count;
}

DEKF_FN void ekf_tick_epoch(const DevCfg& c, const DevState& s, int b, int count, const int* c0) { ekf_tick(c, s, b, count - c0[b]); }

// update(T) of a handle with epochs, in front of the solve: the initialise path at local step 0 (k_mhe_initialize), else assemble_update
DEKF_FN void assemble_epoch(const DevCfg& c, const DevState& s, int b, int T, int pushes, const int* t0, double* sm) {
    const int e = t0[b];  // wave-uniform
    if (T == e) {
        assemble_initialize(c, s, b, sm);
        if (DEKF_LANE() == 0) { s.status[b] = DEKF_SOLVE_NONE; s.iters[b] = 0; }
    } else {
        assemble_update(c, s, b, T - e, pushes - e, sm);
    }
}

// The arrival cost of step T ahead of time.  A fresh handle computes none for its steps 0 and 1 (dekf_initialize launches no
// marginalize_early): neither does a restarted instance for its local ones, whose update(1) then computes the gains of step 0 itself.
DEKF_FN void marginalize_early_epoch(const DevCfg& c, const DevState& s, int b, int T, const int* t0, double* sm) {
    const int Tl = T - t0[b];  // wave-uniform
    if (Tl >= 2) marginalize_early(c, s, b, Tl, sm);
}

// The direct solve's window of instance b at the handle's step T: local (kstart, K) as dekf_update computes them from the local step.
// false at local step 0, where there is no solve and nothing is written.
DEKF_FN bool direct_window_epoch(const DevCfg& c, int T, int e, int& kstart, int& K) {
    const int Tl = T - e;
    kstart = Tl - c.N + 1 > 0 ? Tl - c.N + 1 : 0;
    K = Tl - kstart + 1;
    return Tl >= 1;
}

// The host folds its EKF tick count long before the int overflows (dekf_ekf_step): count_old becomes count_new = H + count_old % H,
// both at least H and equal modulo H, H the history depth.  ekf_tick uses the local count count - c0[b] only modulo H (ring slots) and
// to know whether it has reached H (the ring is full), so the fold gives every instance the epoch that keeps exactly those two: a
// local count below H stays what it is, one of H or more becomes H + local % H.  The new epoch may be negative (down to -H + 1); the
// local count stays in [0, 2^30 + H).
DEKF_HD int fold_epoch(int c0, int count_old, int count_new, int H) {
    const int local = count_old - c0;
    return count_new - (local < H ? local : H + local % H);
}

}  // namespace dekf
