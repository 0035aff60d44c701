// mhe_params_core.h — noise parameters per instance of a direct handle (dekf_set_instance_params).
//
// The noise constants reach the device cores only as fields of the const DevCfg& they are called with (C_*, Q_*, Q_bias_dt2, ekf_C*,
// ekf_P0, ekf_q0: what host_common.h's fill_noise derives from the stds).  So an instance with its own noise needs no core of its own
// kind, only its own argument: every function below calls the existing core (through mhe_epoch_core.h: a handle with a table always
// runs the epoch path, every epoch 0 until an instance restarts) with the instance's own DevCfg.  No core, DevCfg or DevState changes,
// so instance b computes, bit for bit, what a handle created with its set computes.  The tables hold the doubles fill_noise gave for
// the instance's set on the host.
//
// Two tables, by who reads them:
//   MHE  [B] DevCfg, instance-major: the handle's DevCfg with the instance's noise constants, whole.  The assemble, marginalise and
//        solve kernels give an instance a wavefront, so the address of its DevCfg is uniform in the workgroup: through a const
//        __restrict__ pointer the cores' reads of c.* are scalar loads into SGPRs, as they are from the kernel-argument segment, and a
//        read at a lane-dependent index (c.Q_bias_dt2[i - 6], c.C_enc_vel[j]) is a load like any other.  A copy of the handle's
//        DevCfg in registers with the noise fields overwritten is what this replaced: one such index keeps the whole copy in scratch
//        (928 bytes per lane in every direct kernel, 221 spilled VGPRs in the assemble kernel).
//   EKF  [PpEkf::len][B], field-major like the EKF state: k_ekf_tick and the reset kernels give an instance one lane, which copies
//        the handle's DevCfg and overwrites the EKF's constants (all indices constant: the copy lives in registers).
// Compiles lane-sequentially like the cores it calls (tests/hostsim/params_hostsim.cpp).
#pragma once
#include "cfg.h"
#include "mhe_epoch_core.h"

namespace dekf {

// X(field of DevCfg, doubles): the order is the layout of the EKF table's rows
#define DEKF_PP_EKF_FIELDS(X) X(ekf_Cgyro, 3) X(ekf_Caccel, 3) X(ekf_Cvo, 4) X(ekf_P0, 4) X(ekf_q0, 4)
#define DEKF_PP_COUNT_(F, N) +(N)
struct PpEkf {
    static constexpr int len = 0 DEKF_PP_EKF_FIELDS(DEKF_PP_COUNT_);
};
#undef DEKF_PP_COUNT_

// host: instance b's entries of the EKF table from the DevCfg of its set (fill_noise)
DEKF_HD void pp_pack_ekf(const DevCfg& c, double* tab, size_t B, size_t b) {
    int o = 0;
#define DEKF_PP_PACK_(F, N) for (int i = 0; i < (N); ++i) tab[(size_t)(o + i) * B + b] = c.F[i]; o += (N);
    DEKF_PP_EKF_FIELDS(DEKF_PP_PACK_)
#undef DEKF_PP_PACK_
}
// the handle's constants with instance b's EKF noise (pe: the EKF table)
DEKF_FN DevCfg pp_ekf_cfg(const DevCfg& c, const double* pe, int b) {
    DevCfg cc = c;
    const size_t B = (size_t)c.B;
    int o = 0;
#define DEKF_PP_TAKE_(F, N) for (int i = 0; i < (N); ++i) cc.F[i] = pe[(size_t)(o + i) * B + b]; o += (N);
    DEKF_PP_EKF_FIELDS(DEKF_PP_TAKE_)
#undef DEKF_PP_TAKE_
    return cc;
}

// one function per core: the core of mhe_epoch_core.h on the instance's own constants.  pc: the MHE table, pe: the EKF table
DEKF_FN void ekf_tick_pp(const DevCfg& c, const DevState& s, int b, int count, const int* c0, const double* pe) {
    ekf_tick_epoch(pp_ekf_cfg(c, pe, b), s, b, count, c0);
}
DEKF_FN void assemble_pp(const DevCfg* pc, const DevState& s, int b, int T, int pushes, const int* t0, double* sm) {
    assemble_epoch(pc[b], s, b, T, pushes, t0, sm);
}
DEKF_FN void marginalize_early_pp(const DevCfg* pc, const DevState& s, int b, int T, const int* t0, double* sm) {
    marginalize_early_epoch(pc[b], s, b, T, t0, sm);
}
// (the direct solve: direct_solve_t on pc[b], in the kernels' own instantiations)
// dekf_reset and dekf_reset_instances of a handle with a table: every instance's own ekf_q0 / ekf_P0
DEKF_FN void reset_state_pp(const DevCfg& c, const DevState& s, int b, const double* pe) { reset_state_of(pp_ekf_cfg(c, pe, b), s, b); }
DEKF_FN void reset_instance_pp(const DevCfg& c, const DevState& s, int b, double* cov, int* t0, int* c0, int next_T, int ekf_count,
                               const double* pe) {
    reset_instance(pp_ekf_cfg(c, pe, b), s, b, cov, t0, c0, next_T, ekf_count);
}
// dekf_set_instance_params on an instance at local tick 0 or -1: the EKF state at its set's initial quaternion and covariance, as
// reset_state_of writes them
DEKF_FN void ekf_init_pp(const DevCfg& c, const DevState& s, int b, const double* pe) {
    const DevCfg cc = pp_ekf_cfg(c, pe, b);
    const size_t B = (size_t)c.B;
    for (int i = 0; i < 4; ++i) { s.ekf_q[i * B + b] = cc.ekf_q0[i]; s.quat[4 * (size_t)b + i] = cc.ekf_q0[i]; }
    for (int i = 0; i < 16; ++i) s.ekf_P[i * B + b] = (i % 5 == 0) ? cc.ekf_P0[i / 5] : 0.0;
}

}  // namespace dekf
