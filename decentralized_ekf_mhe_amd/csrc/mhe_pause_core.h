// mhe_pause_core.h — pausing single instances of a direct handle (dekf_set_active).
//
// The epochs of mhe_epoch_core.h give every instance its own clock: its local step T - t0[b] and its local EKF count count - c0[b].  A
// paused instance is one whose clock stands still, so it needs no state of its own kind either: while instance b is paused the device
// copies of t0[b] and c0[b] hold DEKF_EPOCH_PAUSED, and the host keeps the local step and the local count that come next.  At the
// resuming call the host writes the epochs that make exactly those the next ones (t0 = next_T - step, c0 = ekf_count - count): the
// instance goes on with the local tick and step that would have followed the last ones it ran, on records, stack entries, history
// samples, tags and an arrival cost computed ahead that are all indexed by the local clock and were written by nobody in between.
//
// The sentinel is 2^31 - 2^16.  A handle that has paused an instance runs steps below it (dekf_update refuses the sentinel itself: 124
// days at 200 Hz) and counts below 2^30 + H, so T - t0 lies in [-2^31 + 2^16, -1] and count - c0 below that too: neither difference
// overflows, nor does direct_window_epoch's T - t0 - N + 1 at any horizon, and the kernels that were harmless below a local step of 1 or
// 2 stay as they are: direct_window_epoch returns false (the 90 direct kernels of direct_kernels.def end after their epoch load) and
// marginalize_early_epoch returns.  An EKF tick and an assemble are not harmless at a negative local argument, and a VO latch does
// not know the epochs at all: the cores below are theirs, and a handle launches their kernels (kernels.hip: k_*_act) once it has
// paused an instance.  The arithmetic of the host is here too, so the C ABI and the lane-sequential build
// (tests/hostsim/pause_hostsim.cpp) run the same expressions.
#pragma once
#include "cfg.h"
#include "mhe_epoch_core.h"
#include "mhe_params_core.h"

namespace dekf {

constexpr int DEKF_EPOCH_PAUSED = 0x7fff0000;
DEKF_HD bool epoch_paused(int e) { return e == DEKF_EPOCH_PAUSED; }

// ---- the device cores: what mhe_epoch_core.h and mhe_params_core.h call, or nothing for a paused instance
DEKF_FN void ekf_tick_active(const DevCfg& c, const DevState& s, int b, int count, const int* c0) {
    const int e = c0[b];
    if (!epoch_paused(e)) ekf_tick(c, s, b, count - e);
}
DEKF_FN void ekf_tick_active_pp(const DevCfg& c, const DevState& s, int b, int count, const int* c0, const double* pe) {
    const int e = c0[b];
    if (!epoch_paused(e)) ekf_tick(pp_ekf_cfg(c, pe, b), s, b, count - e);
}
DEKF_FN void assemble_active(const DevCfg& c, const DevState& s, int b, int T, int pushes, const int* t0, double* sm) {
    if (!epoch_paused(t0[b])) assemble_epoch(c, s, b, T, pushes, t0, sm);  // wave-uniform
}
DEKF_FN void assemble_active_pp(const DevCfg* pc, const DevState& s, int b, int T, int pushes, const int* t0, double* sm) {
    if (!epoch_paused(t0[b])) assemble_epoch(pc[b], s, b, T, pushes, t0, sm);
}
// k_latch_vo's body for instance b, whose mask entry is 1: a sample pushed for a paused instance is dropped, the orientation pose too
DEKF_FN void latch_vo_active(const DevState& s, int b, const int* t0, const double* t_pre, const double* t_now, const double* dp,
                             const double* t_pose, const double* q_vo) {
    if (epoch_paused(t0[b])) return;
    s.vo_flag[b] = 1;
    s.vo_tpre[b] = t_pre[b];
    s.vo_tnow[b] = t_now[b];
    for (int i = 0; i < 3; ++i) s.vo_dp[3 * (size_t)b + i] = dp[3 * (size_t)b + i];
    if (q_vo) {
        s.ekf_vo_flag[b] = 1;
        s.ekf_vo_t[b] = t_pose[b];
        for (int i = 0; i < 4; ++i) s.ekf_vo_q[4 * (size_t)b + i] = q_vo[4 * (size_t)b + i];
    }
}

// ---- the host's arithmetic
// what ekf_tick takes from a local count: its value modulo the history depth H and whether it has reached H (fold_epoch)
DEKF_HD int reduced_count(int count, int H) { return count < H ? count : H + count % H; }
// fold_epoch of a handle that has paused an instance: the sentinel stays where it is (the stored local count needs no fold)
DEKF_HD int fold_epoch_active(int c0, int count_old, int count_new, int H) {
    return epoch_paused(c0) ? c0 : fold_epoch(c0, count_old, count_new, H);
}

// dekf_set_active for instance b.  active, step, count, t0, c0: [B] each; t0 | c0 the host's image of the device arrays (the sentinel
// while paused), step | count the next local step and local EKF count of a paused instance.  next_T, ekf_count: the handle's step and
// EKF tick count at the call.  Pausing stores next_T - t0 and ekf_count - c0; resuming writes the epochs that give them back, the
// count reduced as a fold reduces it so that the new c0 is above -2 H whatever the handle has counted meanwhile (it may be negative,
// as after a fold).  true if the entry changed: the call states the whole mask, and an unchanged entry changes nothing.
DEKF_HD bool set_active_instance(int b, int want, int* active, int* step, int* count, int* t0, int* c0, int next_T, int ekf_count, int H) {
    if (want == active[b]) return false;
    if (!want) {
        step[b] = next_T - t0[b];
        count[b] = ekf_count - c0[b];
        t0[b] = DEKF_EPOCH_PAUSED;
        c0[b] = DEKF_EPOCH_PAUSED;
    } else {
        t0[b] = next_T - step[b];
        c0[b] = ekf_count - reduced_count(count[b], H);
    }
    active[b] = want;
    return true;
}
// dekf_reset_instances on instance b: it is active, paused or not, on the epochs reset_instance writes on the device
DEKF_HD void restart_instance(int b, int* active, int* t0, int* c0, int next_T, int ekf_count) {
    active[b] = 1;
    t0[b] = next_T;
    c0[b] = ekf_count;
}
// the local step of instance b at the handle's step T (dekf_get_instance_ticks: T the last update): frozen while it is paused
DEKF_HD int instance_tick(int b, int T, const int* active, const int* step, const int* t0) {
    return active[b] ? T - t0[b] : step[b] - 1;
}
// its local EKF count (dekf_set_instance_params: 0 on an instance that has not ticked since its restart)
DEKF_HD int instance_count(int b, int ekf_count, const int* active, const int* count, const int* c0) {
    return active[b] ? ekf_count - c0[b] : count[b];
}

}  // namespace dekf
