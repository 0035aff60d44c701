/*
 * dekf.h — C ABI of the batched decentralized EKF + MHE estimator for MI355X.
 *
 * This is the drop-in boundary for ONE hot path of well-robotics/Decentralized_EKF_MHE:
 * the orien_est quaternion EKF and the decentral_legged_est MHE/KF update.  The
 * reference has no FFI; its boundary is the C++ class
 *     DecentralizedEstimation::{initialize, update, reset}
 *         (src/decentral_legged_est/include/decentral_legged_est/DecentralEst.hpp:96-103)
 * and the EKF methods gyro_nonlinear_predict / gyro_nonlinear_correct /
 * vo_nonlinear_correct driven by orien_ekf::timerCallback
 *         (src/orien_est/include/orien_ekf.hpp:79-81, src/orien_est/src/orien_ekf.cpp:77-106).
 * Every entry point below names the reference interface it replaces.  The batch
 * dimension B (independent robot instances; on the GPU the solve gives each one a workgroup of four
 * wavefronts, the EKF one lane, term construction one wavefront) is new.
 *
 * Conventions
 *  - plain pointers + sizes, no C++/torch types; all arrays are instance-major
 *    ([B][...], row-major inside an instance), doubles like the reference's
 *    Eigen::*d / ROS float64 fields.
 *  - every pointer argument is either a HOST or a DEVICE (HBM) pointer, selected
 *    by the `dekf_mem` argument of the call.
 *  - all calls are asynchronous on the handle's HIP stream except dekf_create,
 *    dekf_destroy, dekf_sync and host-side dekf_get.
 *  - nothing throws; every call returns a dekf_status.
 *  - there is NO CPU fallback: dekf_create fails with DEKF_ERR_NO_DEVICE when no
 *    gfx950 device is usable.
 */
#ifndef DEKF_H
#define DEKF_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEKF_ABI_VERSION 4 /* 4: dekf_params.polish_accept_osqp (appended), solve_workgroups_per_cu = 4 selects the four-per-CU kernels;
                            * 3: osqp.polish implemented: dekf_params.polish_refine_iter, dekf_get_polish_status;
                            * 2: dekf_params.solve_workgroups_per_cu, dekf_solve_kernel_name, dekf_launch_info; dim_state-sized rows */
#define DEKF_MAX_LEGS 4
#define DEKF_MAX_JOINTS 8 /* joints per leg */

typedef enum dekf_status {
    DEKF_OK = 0,
    DEKF_ERR_INVALID = 1,    /* bad argument / unsupported configuration */
    DEKF_ERR_NO_DEVICE = 2,  /* no usable HIP device (no CPU fallback exists) */
    DEKF_ERR_HIP = 3,        /* a HIP runtime call failed; see dekf_last_error */
    DEKF_ERR_ORDER = 4,      /* call sequence violated (e.g. update before initialize) */
    DEKF_ERR_COMM = 5        /* RCCL communicator error */
} dekf_status;

typedef enum dekf_mem { DEKF_HOST = 0, DEKF_DEVICE = 1 } dekf_mem;

/*
 * Parameter block.  Field-for-field mirror of `robot_params`
 * (DecentralEst.hpp:18-63; ROS names in EstSub.cpp:123-208, values in
 * go1_example/config/parameters_go1.yaml:1-50) plus the orien_ekf parameters
 * (orien_ekf.cpp:13-25, parameters_go1.yaml:68-75).  Three-element std vectors
 * stay three elements; the per-joint encoder stds are widened to
 * joints_per_leg entries so non-Go1 legs (BASELINE configs 3, 5) can be described.
 */
typedef struct dekf_params {
    /* prior.* */
    double p_init_std[3];
    double v_init_std[3];
    double foot_init_std[3];
    double accel_bias_init_std[3];
    /* process.* */
    double p_process_std[3];
    double accel_input_std[3];
    double gyro_input_std[3];
    double accel_bias_std[3]; /* process.accel_bias_process_std */
    /* leg_odom.* */
    double quaternion_ib[4]; /* w x y z */
    double p_ib[3];
    int num_legs;       /* leg_odom.num_leg */
    int joints_per_leg; /* 3 on Go1 (hard-coded block<3,3> in the reference) */
    int leg_odom_type;  /* 0: foot-velocity measurements, dim_state 9.  1: foot positions are states,
                         * dim_state = 9 + 3 num_legs (21 on Go1), DecentralEst.cpp:20.  How the arrival cost of type 1 is
                         * updated is chosen by `arrival_cost_form` below; its default (0) is the reference's covariance-form
                         * saddle inverse (MheSrb.cpp:527-651).
                         * CONTRACT of type 1: the BASE states (p, v, accel bias: what the node logs and publishes) are inside the
                         * 1e-4 relative tolerance of the reference formula (measured 0.16 x of it over 32 x 2000 ticks); the
                         * FOOT-POSITION states are OUTSIDE that contract: <= 3 x the tolerance (measured 1.83 x; form 1: <= 5 x,
                         * measured 3.24 x).  The reference formula itself moves by 1.5 x the tolerance on those states when its
                         * 33-dim saddle inverse is evaluated in another pivot order (a 1e20 - 1e20 cancellation at every
                         * touch-down, DecentralEst.cpp:432-451, 550-563; MheSrb.cpp:527-651) — INTEGRATION.md section 5. */
    double joint_position_std[DEKF_MAX_JOINTS];
    double joint_velocity_std[DEKF_MAX_JOINTS];
    double foot_slide_std[3];
    double foot_swing_std[3];
    double contact_effort_threshold;
    /* visual_odom.* */
    double vo_p_std[3];
    /* estimation.* */
    int rate;     /* Hz of update(T) calls; dt = 1/rate */
    int N;        /* horizon */
    int est_type; /* 0 MHE, 1 KF */
    /* osqp.* (DecentralEst.cpp:204-217) */
    double rho, alpha, delta, sigma;
    int verbose, adapt_rho, polish, max_qp_iter; /* polish: OSQP's solution polishing after a solved QP (DecentralEst.cpp:207;
                                                   * declared default true, EstSub.cpp:188; parameters_go1.yaml:44 sets false) */
    double rel_tol, abs_tol, prim_tol, dual_tol;
    double time_limit; /* accepted, NOT honoured: runs are deterministic */
    /* OSQP defaults the reference leaves implicit, made explicit here */
    int scaling_iters;            /* 10 */
    int check_termination;        /* 25 */
    int adaptive_rho_interval;    /* OSQP: wall-clock derived; here fixed, default 25 */
    double adaptive_rho_tolerance; /* 5 */
    /* orien_sub.* */
    double ekf_init_std[4];
    double ekf_process_std[3];      /* gyro */
    double ekf_gravity_meas_std[3]; /* accel */
    double ekf_vo_meas_std[4];
    double ekf_quaternion_init[4];  /* w x y z */
    int ekf_rate;                   /* 500 */
    int ekf_history;                /* depth of the rewind ring (reference: unbounded); default 256 = 0.5 s at 500 Hz (an ORB-SLAM3
                                     * relocalisation stall), 55 KB per instance; size it as
                                     * ceil(worst VO pose latency * ekf_rate) + 2, INTEGRATION.md section 5 */
    int polish_refine_iter;         /* OSQP's polish_refine_iter (refinement steps of the polishing solve; OSQP default 3, the
                                     * reference does not set it).  Used when `polish` is on. */
    int arrival_cost_form;          /* leg_odom_type 1 only.  0: the reference's covariance-form saddle inverse
                                     * (MheSrb.cpp:527-651).  1: information form (same arrival cost in exact arithmetic,
                                     * computed from gains only). leg_odom_type 0 always uses the reference form. */
    /* launch tuning (new) */
    int solve_pipeline;             /* 0 (default): every kernel of a step in order on the handle's stream.  1: the MHE solve of
                                     * step T runs on a second stream out of double-buffered inputs and outputs, so the pushes, the
                                     * EKF tick and the term construction of step T + 1 (and then its solve) start while the last
                                     * workgroups of step T's solve are still running; getters wait for the newest solve in stream
                                     * order, so results are bit-identical.  Measured on MI355X, Go1, three-workgroup kernels: +3.4 % at
                                     * B = 4096 (2.21 M against 2.14 M steps/s, round 6), +3 ... +10 % on the other shapes at 1024-4096, -4.5 % at 8192 (EXPERIMENTS.md round 5 section 8): it hides the 0.07 ms of EKF + term
                                     * construction + launch gaps in front of every solve and the partly empty last round.  The two solve streams are created
                                     * at the greatest stream priority (their own hardware-queue class). */
    int solve_workgroups_per_cu;    /* 0: the default residency (3 for full Go1 / Cassie windows when the batch exceeds the 512
                                     * slots of the two-workgroup kernels, 2 for full PogoX windows above 256); 1 or 2: cap — 2
                                     * keeps the two-workgroup solve kernels for full windows too; 4 (round 6, Go1 / Cassie full
                                     * windows, batches above 512): workgroups of THREE wavefronts at four per CU
                                     * (k_mhe_solve_r4_*): +36 / +12 / +7 % at 1024 / 2048 / 3072 robots, +-1 % from 4096 on, where
                                     * the hardware leaves 2-9 % of these workgroups unplaced until others finish
                                     * (profiles/r06_go1_four_per_cu_3waves.txt) — an opt-in for fleets of 800-3000 robots per GPU.
                                     * A launch-tuning knob only: every
                                     * kernel family produces the SAME BITS for a given robot log (since round 5 the iteration phases
                                     * are compiled with floating-point contraction off and explicit fma; tests/test_gpu_configs.py
                                     * holds r3 == ll, r3 == lg and rr == gg with array_equal), so a robot's estimate does not depend
                                     * on the size of the fleet it is batched with. */
    int polish_accept_osqp;         /* osqp.polish only.  0 (default): OSQP's acceptance test for a polished point with its third clause
                                     * made symmetric — `pol_dua < dua && pri < 1e-10 && pol_pri < 1e-10` — so that a polished point never
                                     * trades a primal residual of 1e-11 for one of 1e-7 (this solver's iterates
                                     * reach that clause where OSQP's own do not).  1: polish.c's test verbatim
                                     * (`pol_dua < dua && pri < 1e-10`), for strict OSQP parity. */
} dekf_params;

typedef struct dekf_handle_s* dekf_handle;

/* Fill `p` with go1_example/config/parameters_go1.yaml + OSQP defaults. */
void dekf_default_params(dekf_params* p);

int dekf_abi_version(void);
const char* dekf_last_error(void);
/* hipRuntimeGetVersion() of the HIP runtime this library is bound to (0 if the call fails).  The overlap of consecutive steps
 * (solve_pipeline = 1) and of the look-ahead arrival cost rests on stream scheduling of that runtime; bench.py records it. */
int dekf_hip_runtime_version(void);

/* Replaces: constructing DecentralizedEstimation + orien_ekf for `batch` robots.
 * device = HIP device ordinal; stream = hipStream_t to run on (NULL: own stream). */
dekf_status dekf_create(const dekf_params* p, int batch, int device, void* stream,
                        dekf_handle* out);
dekf_status dekf_destroy(dekf_handle h);
/* Replaces DecentralizedEstimation::reset (DecentralEst.cpp:1011-1015): clears the
 * QP window, the arrival cost, the measurement stacks and the EKF state. */
dekf_status dekf_reset(dekf_handle h);
dekf_status dekf_sync(dekf_handle h);
int dekf_batch(dekf_handle h);
void* dekf_stream(dekf_handle h);

/* ---- sensor latches: the writes the ROS callbacks make into robot_store ---------- */

/* go1Sub::imu_callback / orien_ekf::imu_callback (go1Sub.cpp:30-51, orien_ekf.cpp:62-75):
 * imu_time[B], accel_b[B][3], gyro_b[B][3]. */
dekf_status dekf_push_imu(dekf_handle h, const double* imu_time, const double* accel_b,
                          const double* gyro_b, dekf_mem where);

/* go1Sub::lo_callback outputs (go1Sub.cpp:53-126): p_imu_2_foot[B][L][3],
 * J_imu_2_foot[B][L][3][nj], joint_velocity[B][L][nj], contact[B][L] (0/1). */
dekf_status dekf_push_leg(dekf_handle h, const double* p_imu_2_foot, const double* J_imu_2_foot,
                          const double* joint_velocity, const double* contact, dekf_mem where);

/* Same callback one step earlier: raw Go1 joint_position[B][12],
 * joint_velocity[B][12], foot_force[B][4]; FK, Jacobian and the contact threshold
 * run on the device. Go1 only (num_legs 4, joints_per_leg 3). */
dekf_status dekf_push_go1_joints(dekf_handle h, const double* joint_position,
                                 const double* joint_velocity, const double* foot_force,
                                 dekf_mem where);

/* robotSub::vo_callback (EstSub.cpp:45-56) + orien_ekf::vo_pose_callback
 * (orien_ekf.cpp:48-60): mask[B] (int, 1 = a new VO sample for this instance),
 * t_pre[B], t_now[B], dp_body[B][3] (orb/vo), q_vo[B][4] wxyz and its stamp
 * t_pose[B] (orb/pos). Instances with mask 0 are untouched. */
dekf_status dekf_push_vo(dekf_handle h, const int* mask, const double* t_pre, const double* t_now,
                         const double* dp_body, const double* t_pose, const double* q_vo,
                         dekf_mem where);

/* robotSub::orien_filter_callback (EstSub.cpp:34-43): overrides the orientation the
 * MHE reads with an external quaternion[B][4] wxyz instead of the on-device EKF's. */
dekf_status dekf_push_quaternion(dekf_handle h, const double* quat, dekf_mem where);

/* ---- the hot path ------------------------------------------------------------- */

/* orien_ekf::timerCallback (orien_ekf.cpp:77-106): history push, VO rewind/replay
 * when a VO pose is pending, predict, accel-correct; result feeds the MHE latch. */
dekf_status dekf_ekf_step(dekf_handle h);

/* DecentralizedEstimation::initialize (DecentralEst.cpp:9-150), T = 0. */
dekf_status dekf_initialize(dekf_handle h);
/* DecentralizedEstimation::update(T) (DecentralEst.cpp:152-198), T = 1, 2, ... */
dekf_status dekf_update(dekf_handle h, int T);
/* One estimator-step of the benchmark metric: dekf_ekf_step then
 * (T == 0 ? dekf_initialize : dekf_update(T)). */
dekf_status dekf_step(dekf_handle h, int T);

/* ---- results: the public members read by EstSub.cpp:99-106 ---------------------- */
/* x_mhe[B][dim_state] (x_MHE_ / x_KF_; dim_state = 9 + 3 * leg_odom_type * num_legs: p_s, v_s, accel bias,
 * then the foot positions of leg_odom_type 1), v_b[B][3] (v_MHE_b_ / v_KF_b_), quat[B][4] (EKF
 * quaternion_, wxyz), p_vo[B][3] (p_vo_accmulate_), status[B] (int, see below).
 * Any pointer may be NULL. */
dekf_status dekf_get(dekf_handle h, double* x_mhe, double* v_b, double* quat, double* p_vo,
                     int* status, dekf_mem where);
/* EKF covariance Cov_q_[B][4][4]. */
dekf_status dekf_get_ekf_cov(dekf_handle h, double* cov, dekf_mem where);
/* Per-instance solver diagnostics of the last update: iters[B], rho_updates[B] (int),
 * pri_res[B], dua_res[B] (unscaled OSQP residuals). Any pointer may be NULL. */
dekf_status dekf_get_solver_info(dekf_handle h, int* iters, int* rho_updates, double* pri_res,
                                 double* dua_res, dekf_mem where);
/* Outcome of OSQP's polishing step per instance, polish_status[B] (int; OSQP's info->status_polish): 0 polishing off or the
 * solve did not end OSQP_SOLVED, 1 the polished point replaced the ADMM iterate (pri_res / dua_res are then its residuals),
 * -1 polishing ran and was rejected (the ADMM iterate is returned). */
dekf_status dekf_get_polish_status(dekf_handle h, int* polish_status, dekf_mem where);
/* KF covariance C_KF_[B][dim_state][dim_state] (est_type 1). */
dekf_status dekf_get_kf_cov(dekf_handle h, double* cov, dekf_mem where);

/* ---- warm start (OSQP's warm_start setting; DecentralEst.cpp:204 asks for it) ------------------------------------
 * Adding these two symbols does not change DEKF_ABI_VERSION: dekf_params is untouched, and a caller that never calls them gets
 * exactly the cold-start solves (and bits) of before.
 * dekf_set_warm_start(h, on), on = 0 or 1 (default 0): with 1, a full-window MHE solve starts from the previous tick's solution
 * instead of x = z = y = 0 and rho = `rho`.  Allowed before dekf_initialize or right after dekf_reset (else DEKF_ERR_ORDER);
 * DEKF_ERR_INVALID for a KF handle (est_type 1), a pipelined handle (solve_pipeline 1: solve T + 1 would need solve T's per-instance
 * output while T's last workgroups still run) and any other `on`.  The first enable allocates the per-instance warm store
 * ((n + m + 1) doubles, about 9 KB for Go1).
 * Contract, per instance:
 *  - window-fill ticks (T < N - 1) and the first full window start cold, bit-identical to warm start off;
 *  - a full window starts warm only if the previous tick was a full window whose solve ended DEKF_SOLVE_OK or DEKF_SOLVE_MAX_ITER
 *    with a finite iterate; otherwise cold.  dekf_reset invalidates every store.
 *  - the previous iterate is SHIFTED by one window block (block k takes block k + 1; the entering x and leg slacks make this tick's
 *    new Dyn and Meas rows hold exactly, the entering w, c and duals are 0), not reused index for index as osqp_warm_start would:
 *    the window has slid one step, and index-for-index reuse would pair every block with its neighbour's value.  z = A x on the VO
 *    rows; equality rows start on their bound.  x and y are kept unscaled and rescaled with this tick's Ruiz scaling.
 *  - rho starts at the instance's final rho of the previous solve, clamped to [1e-6, 1e6].
 *  - termination, adaptive rho, max_qp_iter, status codes and polishing are unchanged; dekf_get_solver_info reports the warm counts.
 * dekf_get_warm_status: warm[B] (int) = 1 if the last update's solve started from the shifted previous iterate, 0 if cold.
 * (dekf_solve_kernel_name of a warm handle names the full-window kernel's warm twin where it has one, e.g. k_mhe_solve_r3_4_n20_warm.) */
dekf_status dekf_set_warm_start(dekf_handle h, int on);
dekf_status dekf_get_warm_status(dekf_handle h, int* warm, dekf_mem where);

/* ---- direct solve (opt-in): the exact optimum of the window QP and the covariance of its newest state ---------------
 * Adding these two symbols does not change DEKF_ABI_VERSION: dekf_params is untouched, and a caller that never calls them gets
 * exactly the ADMM solves (and bits) of before.
 * dekf_set_solver(h, solver), solver = DEKF_SOLVER_ADMM (default: the reference's OSQP-style ADMM) or DEKF_SOLVER_DIRECT.  Allowed
 * before dekf_initialize or right after dekf_reset (else DEKF_ERR_ORDER); the setting survives dekf_reset.  DEKF_ERR_INVALID for any
 * other value, a KF handle (est_type 1) and a pipelined handle (solve_pipeline 1), and DEKF_ERR_INVALID for DEKF_SOLVER_DIRECT on a
 * handle with osqp.polish = 1 or with warm start on; dekf_set_warm_start(h, 1) on a direct handle is DEKF_ERR_INVALID too.  Polishing
 * and warm start act on an ADMM iterate, which a direct solve does not have.  The first DEKF_SOLVER_DIRECT allocates the covariance
 * store (B dim_state^2 doubles).
 * Contract of a direct handle, per instance and update (window-fill and full windows alike):
 *  - "exact": x_mhe is the newest state of the minimiser of the window QP with every row whose bounds are finite held as an equality
 *    (every Meas and Dyn row; a VO row once vision has written its bound) and every +-1e30 row free — one forward block elimination
 *    over the window (the Kalman filter on the window when no VO row is an equality), with the arrival cost of the ADMM path.  It
 *    differs from an ADMM handle's x_mhe by the ADMM iterate's own distance from that optimum (within OSQP's eps, not bit-equal);
 *  - v_b as on an ADMM handle, from that x_mhe;
 *  - status DEKF_SOLVE_OK, or DEKF_SOLVE_NUMERIC for a non-positive or non-finite pivot or a non-finite result; iters = rho_updates
 *    = 0, polish_status = 0, and pri_res = dua_res = NaN (no ADMM iterate exists);
 *  - dekf_solve_kernel_name names the direct kernel (k_mhe_solve_direct_*) for both window kinds, dekf_launch_info reports B
 *    workgroups (one wavefront each), timing class 2 brackets the direct launch.
 * dekf_get_mhe_cov: cov[B][dim_state][dim_state] (row-major) = Cov(x_T) = [J^-1]_TT of the last update, J the information matrix of
 * the window's states.  DEKF_ERR_INVALID on an ADMM or KF handle, DEKF_ERR_ORDER before the first update and after dekf_reset until
 * the next update. */
#define DEKF_SOLVER_ADMM 0   /* default: OSQP-style ADMM, the reference's solver */
#define DEKF_SOLVER_DIRECT 1 /* exact optimum of the window QP by one forward block elimination */
dekf_status dekf_set_solver(dekf_handle h, int solver);
dekf_status dekf_get_mhe_cov(dekf_handle h, double* cov, dekf_mem where); /* cov[B][ns][ns], row-major */

/* ---- window smoother (opt-in, direct handles): every state of the window and its covariance -------------------------
 * Adding these two symbols does not change DEKF_ABI_VERSION: dekf_params is untouched, and a caller that never calls them gets
 * exactly the results (and bits) of before.
 * dekf_set_smoother(h, on), on = 0 (default) or 1.  Allowed before dekf_initialize or right after dekf_reset (else DEKF_ERR_ORDER);
 * the setting survives dekf_reset.  DEKF_ERR_INVALID for a null handle, any other `on`, and on = 1 on a handle that is not a direct
 * handle (ADMM, KF).  dekf_set_solver(h, DEKF_SOLVER_ADMM) on a smoothing handle switches the smoother off with the direct solve
 * (going back to DEKF_SOLVER_DIRECT does not switch it on again).  The first enable allocates the stores: N ns + (2 N - 1) ns^2
 * doubles per instance (ns = dim_state; Go1 27 KB, PogoX with N = 100 136 KB, Go1 with foot states 141 KB).
 * A smoothing handle's update runs the backward (Rauch-Tung-Striebel) recursion behind the direct solve's forward elimination, in the
 * same kernel launch, and leaves, per instance, for the K = min(T + 1, N) steps of the window it solved (window-fill and full windows):
 *  - x_win[b][k][:], k = 0 (oldest, step T - K + 1) .. K - 1 (newest, step T): the state blocks of the minimiser of the QP the direct
 *    solve minimises (equality rows held, +-1e30 rows free, the ADMM path's arrival cost);
 *  - cov_win[b][k][:][:] = Cov(x_k) = [J^-1]_kk, row-major and symmetric to the bit for k < K - 1, J the information matrix of the
 *    window's states (the J whose last diagonal block dekf_get_mhe_cov returns);
 *  - x_mhe, v_b, status, solver info and dekf_get_mhe_cov are bit-identical to the same handle with the smoother off; x_win[b][K-1]
 *    is bit-identical to x_mhe[b] and cov_win[b][K-1] to the covariance of dekf_get_mhe_cov;
 *  - an instance whose status is DEKF_SOLVE_NUMERIC gets NaN in all K entries of both arrays; its neighbours are unaffected.
 *  - dekf_solve_kernel_name names the direct kernel's smoothing twin (k_mhe_solve_direct_*_smooth) for both window kinds.
 * dekf_get_window: x_win[B][N][dim_state], cov_win[B][N][dim_state][dim_state]; entries k >= K are not written.  *steps (always a host
 * int*) receives K of the last update.  Any of the three pointers may be NULL.  Host pointers: copy and synchronise, like
 * dekf_get_mhe_cov; device pointers: in stream order.  DEKF_ERR_INVALID on a handle without the smoother, DEKF_ERR_ORDER before the
 * first update and after dekf_reset until the next update.
 * Not part of this interface: the window of an ADMM handle. */
dekf_status dekf_set_smoother(dekf_handle h, int on);
dekf_status dekf_get_window(dekf_handle h, int* steps, double* x_win, double* cov_win, dekf_mem where);

/* ---- window cross-covariances (opt-in, smoothing handles): what ties two states of the window together ---------------
 * Two more additive symbols: DEKF_ABI_VERSION and dekf_params are unchanged, and a caller that never calls them gets exactly the
 * results (and bits) of before.
 * dekf_set_window_cross(h, on), on = 0 (default) or 1.  Call order as for dekf_set_smoother: before dekf_initialize or right after
 * dekf_reset (else DEKF_ERR_ORDER); the setting survives dekf_reset.  DEKF_ERR_INVALID for a null handle, any other `on`, and on = 1
 * on a handle without the smoother.  dekf_set_smoother(h, 0) and dekf_set_solver(h, DEKF_SOLVER_ADMM) switch the option off; switching
 * those back on does not switch it on again.  The first enable allocates the one new store: N ns^2 doubles per instance (Go1 13 KB,
 * Go1 with foot states 71 KB); the lag-one blocks take the place of the smoother's own T1 store.
 * A cross handle's update runs the smoothing kernel's twin (k_mhe_solve_direct_*_smooth_cross, which dekf_solve_kernel_name then names
 * for both window kinds), whose backward pass also leaves, per instance, with K = min(T + 1, N) and J the information matrix of
 * dekf_get_window:
 *  - cov_lag1[b][k][:][:] = Cov(x_k, x_{k+1}) = [J^-1]_{k,k+1}, k = 0 .. K - 2: rows index x_k, columns x_{k+1}, row-major;
 *  - cov_newest[b][k][:][:] = Cov(x_k, x_T) = [J^-1]_{k,K-1}, k = 0 .. K - 1: rows index x_k.  The covariance of the relative motion
 *    follows as Cov(x_T - x_k) = cov_win[K-1] + cov_win[k] - cov_newest[k] - cov_newest[k]';
 *  - x_mhe, v_b, status, solver info, dekf_get_mhe_cov, x_win and cov_win are bit-identical to the same handle with the option off;
 *    cov_newest[b][K-1] is bit-identical to cov_win[b][K-1], and cov_newest[b][K-2] to cov_lag1[b][K-2];
 *  - an instance whose status is DEKF_SOLVE_NUMERIC gets NaN in all written entries of both arrays; its neighbours are unaffected.
 * dekf_get_window_cross: cov_lag1[B][N-1][dim_state][dim_state], cov_newest[B][N][dim_state][dim_state]; entries k >= K - 1 of the
 * first and k >= K of the second are not written.  *steps (always a host int*) receives K of the last update.  Any of the three
 * pointers may be NULL.  Host and device pointers as in dekf_get_window.  DEKF_ERR_INVALID on a handle without the option,
 * DEKF_ERR_ORDER before the first update and after dekf_reset until the next update.
 * Not part of this interface: Cov(x_j, x_k) of other pairs, and the window of an ADMM handle. */
dekf_status dekf_set_window_cross(dekf_handle h, int on);
dekf_status dekf_get_window_cross(dekf_handle h, int* steps, double* cov_lag1, double* cov_newest, dekf_mem where);

/* ---- restarting single instances (direct handles): one robot starts over, the others keep running ----------------------
 * Two more additive symbols: DEKF_ABI_VERSION and dekf_params are unchanged, and a caller that never calls them gets exactly the
 * results (and bits) of before.  dekf_reset clears all B instances and asks for a new dekf_initialize; dekf_reset_instances restarts
 * the instances of a mask (a rebooted robot, an estimator whose arrival cost a NaN sample has poisoned, one environment of a
 * vectorised simulator) while every other instance keeps its window, its arrival cost and every bit of every output.
 * dekf_reset_instances(h, mask, where): mask[B], 1 restarts the instance, 0 leaves it alone; a host or a device pointer (a device mask
 * is copied to the host and waited for: the call checks it).
 *  - When: on an initialised direct handle anywhere between dekf_update(h, T0 - 1) and dekf_update(h, T0).  On a lock-step handle
 *    (one dekf_ekf_step per update) that is before the pushes and the dekf_ekf_step of step T0.  On a two-rate handle (ekf_rate above
 *    rate: several dekf_ekf_step between two updates) the call may come before, between or behind the EKF ticks of that gap: the
 *    ticks before the call belong to the instance's earlier life, the ticks behind it to the new one.  IMU and leg samples are pushed
 *    at least once between the call and dekf_update(h, T0), as before any dekf_initialize.  DEKF_ERR_ORDER before dekf_initialize.  DEKF_ERR_INVALID for a null handle or mask, for a handle that is not a
 *    direct handle (ADMM, KF) or has solve_pipeline = 1, and for a mask entry other than 0 or 1.  The handle's stream waits for what
 *    dekf_reset waits for (solves in flight, the arrival cost computed ahead, readers of v_b) before the instances are cleared.
 *  - A restarted instance is as after dekf_reset: EKF state and covariance at their initial values, VO latches, way points and the
 *    p_vo accumulator cleared, x_mhe and v_b 0, status DEKF_SOLVE_NONE, solver info 0; its block of dekf_get_mhe_cov is NaN until its
 *    first solve.  A sample latched before the call is dropped for it; the samples pushed after the call are its first.
 *  - Its next dekf_ekf_step is its EKF tick 0, however many ticks the handle has run (since its last update too); dekf_update(h, T0)
 *    is its dekf_initialize (first sample, prior as arrival cost, no
 *    solve) and dekf_update(h, T0 + j) its update(j), with a window of K_b = min(j + 1, N) steps.
 *  - From step T0 on every output of the instance (dekf_get, dekf_get_ekf_cov, dekf_get_mhe_cov, dekf_get_solver_info and the first K_b
 *    entries of dekf_get_window and dekf_get_window_cross) is bit-identical to the same instance of a fresh handle that is fed the same
 *    samples and runs the same calls FROM THE CALL on: its first dekf_ekf_step is the first one behind the call, its
 *    dekf_initialize stands where dekf_update(h, T0) does.  The instances outside the mask keep every bit of every output at every later step.
 *  - An all-zero mask changes nothing.  An instance may be restarted again at any later step, inside its own window fill too.
 *  - *steps of dekf_get_window and dekf_get_window_cross becomes the largest K_b of the batch; entries k >= K_b of instance b (k >= K_b - 1
 *    of cov_lag1) are not specified.  The two getters return DEKF_ERR_ORDER while no instance has solved since its restart.
 *  - Until the first call with a non-zero mask the handle launches exactly the kernels it launched before this interface existed.
 *    After it, and until dekf_reset, it launches their epoch twins, which take every instance's own step: dekf_solve_kernel_name then
 *    names k_mhe_solve_direct_*_ep, *_smooth_ep or *_smooth_cross_ep.  dekf_reset clears every epoch: a handle reset and run again is
 *    a fresh handle.
 * dekf_get_instance_ticks(h, ticks, where): ticks[B], the local step of every instance at the last update: T on a handle that never
 * restarted one, T - T0 after a restart before step T0 (-1 between the restart and dekf_update(h, T0)); K_b = min(ticks[b] + 1, N)
 * once ticks[b] >= 1.  Any initialised handle; DEKF_ERR_ORDER before dekf_initialize, DEKF_ERR_INVALID for a null handle or pointer.
 * Not part of this interface: ADMM handles (their launch takes one window length for the batch), KF and pipelined handles.
 * (Parameters per instance: dekf_set_instance_params below; instances that are switched off: dekf_set_active below.) */
dekf_status dekf_reset_instances(dekf_handle h, const int* mask, dekf_mem where);
dekf_status dekf_get_instance_ticks(dekf_handle h, int* ticks, dekf_mem where);

/* ---- noise parameters per instance (direct handles): every robot of a handle its own noise ------------------------------
 * Two more additive symbols: DEKF_ABI_VERSION and dekf_params are unchanged, and a caller that never calls them launches exactly the
 * kernels of before and gets the same bits.  A handle estimates thousands of robots with one dekf_params; with a parameter table
 * every instance has its own NOISE FIELDS (noise tuning: B candidate sets on one log in one launch per tick; a vectorised simulator
 * that draws new sensor-noise levels for a restarted environment; a mixed fleet):
 *     p_init_std v_init_std foot_init_std accel_bias_init_std p_process_std accel_input_std gyro_input_std accel_bias_std
 *     joint_position_std joint_velocity_std foot_slide_std foot_swing_std vo_p_std
 *     ekf_init_std ekf_process_std ekf_gravity_meas_std ekf_vo_meas_std ekf_quaternion_init
 * dekf_set_instance_params(h, sets, nsets, set_of): sets[nsets] and set_of[B] are host pointers; set_of[b] in 0 .. nsets - 1 gives
 * instance b the noise fields of that set, set_of[b] = -1 leaves instance b as it is (on the handle's own parameters if it never took
 * a set).  nsets = 0 with both pointers NULL drops the table: every instance is on the handle's parameters again and the handle
 * launches its former kernels (before the first tick or right after dekf_reset only, else DEKF_ERR_ORDER).
 *  - Every other field of every set must equal the handle's own parameters: structure, rates, N, the osqp.* block,
 *    contact_effort_threshold, p_ib, quaternion_ib, the form switches and launch tuning; else DEKF_ERR_INVALID: a difference is
 *    refused, never ignored.  The positivity that dekf_create asks of the foot stds (leg_odom_type 1) is asked of every set.
 *  - Where: direct handles only.  DEKF_ERR_INVALID for ADMM and KF handles, for solve_pipeline = 1, a null handle, an index outside
 *    -1 .. nsets - 1, nsets < 0, and for pointers that do not go with nsets.  dekf_set_solver(h, DEKF_SOLVER_ADMM) on a handle that
 *    has a table is DEKF_ERR_INVALID: drop the table first.
 *  - When: before the first dekf_ekf_step (since dekf_create or dekf_reset): any instance.  On a running handle only instances whose
 *    local tick (dekf_get_instance_ticks) is -1 and that have not ticked since, i.e. restarted by dekf_reset_instances and before
 *    the next dekf_ekf_step behind THAT restart.  The rule is per instance: EKF ticks of the handle before the restart (a two-rate
 *    handle runs several between two updates) do not count, and of two instances restarted in one gap with a tick between them
 *    only the later one still takes a set.  Any other instance with set_of[b] >= 0 makes the whole call DEKF_ERR_ORDER and nothing is applied: an instance never changes parameters in
 *    mid-life.
 *  - The call rewrites the EKF state of the instances it names to their set's initial quaternion and covariance, and returns when
 *    the table is on the device.
 *  - The table survives dekf_reset, as the other settings do, and dekf_reset_instances: a restarted instance keeps its set until
 *    told otherwise, and both calls write every instance's own initial EKF state.
 *  - From its first tick on every output of instance b (dekf_get, dekf_get_ekf_cov, dekf_get_mhe_cov, dekf_get_solver_info,
 *    dekf_get_window, dekf_get_window_cross) is bit-identical to instance b of a handle created with sets[set_of[b]] (same batch, same
 *    samples); after a restart, to a fresh handle with that set fed the samples from the restart on.  The derived constants are
 *    computed on the host by the expressions dekf_create uses.
 *  - A handle with a table launches the parameter twins of the epoch kernels from its first tick on: dekf_solve_kernel_name names
 *    k_mhe_solve_direct_*_pp, *_smooth_pp or *_smooth_cross_pp.
 * dekf_get_instance_params(h, b, out): the handle's parameters with instance b's noise fields; on any handle (without a table: the
 * handle's own parameters).  DEKF_ERR_INVALID for b outside 0 .. B - 1 or a null pointer.
 * Not part of this interface: ADMM, KF and pipelined handles; structure, rates, horizon, solver settings, contact_effort_threshold
 * or the IMU-to-body transform per instance.  (Instances that are switched off: dekf_set_active below.) */
dekf_status dekf_set_instance_params(dekf_handle h, const dekf_params* sets, int nsets, const int* set_of);
dekf_status dekf_get_instance_params(dekf_handle h, int b, dekf_params* out);

/* ---- pausing single instances (direct handles): one robot stands still, the others keep running -------------------------
 * Two more additive symbols: DEKF_ABI_VERSION and dekf_params are unchanged, and a caller that never calls them launches exactly the
 * kernels of before and gets the same bits.  Without them every instance of a handle ticks, assembles and solves at every step: an
 * environment of a vectorised simulator that is done and waits for the others, or a sweep candidate already ruled out, pays its full
 * solve, and a robot whose link is down keeps estimating from stale latches.
 * dekf_set_active(h, active, where): active[B], 1 runs, 0 is paused; a host or a device pointer (a device array is copied to the host
 * and waited for, as dekf_reset_instances does).  The call states the whole mask; it is not a toggle.
 *  - Where: direct handles only.  DEKF_ERR_INVALID for a null handle or array, for ADMM and KF handles, for solve_pipeline = 1 and for
 *    an entry other than 0 or 1.  DEKF_ERR_ORDER before dekf_initialize.
 *  - When: anywhere between dekf_update(h, T0 - 1) and dekf_update(h, T0).  On a two-rate handle the call may come before, between or
 *    behind the EKF ticks of that gap.  The handle's stream waits for what dekf_reset_instances waits for.
 *  - A paused instance stands still.  Every dekf_ekf_step and dekf_update behind the call skips it: no EKF tick, no term
 *    construction, no arrival cost ahead of time, no solve.  Every getter keeps, to the bit, the values it had at the call: dekf_get,
 *    dekf_get_ekf_cov, dekf_get_mhe_cov, dekf_get_solver_info, its entries of dekf_get_window and dekf_get_window_cross, and its
 *    local step in dekf_get_instance_ticks, which is frozen.  dekf_allgather_vb contributes its frozen v_b.  VO samples pushed for it
 *    (dekf_push_vo with its mask entry 1) are dropped, the orientation pose included.  Its IMU, leg and quaternion latches are
 *    unspecified while it is paused (so is the quaternion of dekf_get on a handle that is fed dekf_push_quaternion).
 *  - Resuming: its next dekf_ekf_step and dekf_update are the local tick and step that would have followed the last ones it ran.
 *    IMU and leg samples are pushed at least once between the resuming call and its next tick or update (the rule of
 *    dekf_reset_instances).  From then on every output of the instance (every getter above, the first K_b window and cross
 *    entries) is bit-identical to the same instance of a handle that was never paused and received, in order, exactly the pushes,
 *    EKF ticks and updates that occurred while the instance was active: the log with the paused steps cut out.
 *  - Instances whose mask entry does not change keep every bit of every output at every later step.  An unchanged mask changes
 *    nothing.
 *  - With restarts: dekf_reset_instances on a paused instance restarts it and makes it active; its new life starts at that call.  A
 *    restarted instance may be paused in the same gap, at local tick -1: its dekf_initialize is then the first update after it
 *    resumes.
 *  - With parameter tables: the rule of dekf_set_instance_params is unchanged and is read on the instance's local tick and local EKF
 *    count, not on the handle's: a restarted instance that is paused before its first tick still takes a set while it is paused.
 *  - dekf_reset makes every instance active: a reset handle is a fresh handle.  Pausing is state, not a setting.
 *  - *steps of dekf_get_window and dekf_get_window_cross is the largest K_b of the batch; paused instances count with the K_b they
 *    stand at.
 *  - Until the first call that pauses an instance the handle launches exactly the kernels it launched before this interface
 *    existed (a mask of ones on such a handle changes nothing).  After it, and until dekf_reset, dekf_solve_kernel_name names the
 *    _ep twins, or the _pp twins on a handle with a parameter table, as after a restart: for a paused instance they end after the
 *    load of its epoch.  Such a handle runs 2^31 - 2^16 steps (124 days at 200 Hz); dekf_update then returns DEKF_ERR_ORDER.
 * dekf_get_active(h, active, where): active[B] as the last dekf_set_active and dekf_reset_instances left it; all ones where the
 * interface was never used.  Any initialised handle; DEKF_ERR_ORDER before dekf_initialize, DEKF_ERR_INVALID for a null handle or
 * pointer.
 * Not part of this interface: ADMM, KF and pipelined handles; a robot that was really away (its clock did not stand still: restart
 * it with dekf_reset_instances, do not resume it). */
dekf_status dekf_set_active(dekf_handle h, const int* active, dekf_mem where);
dekf_status dekf_get_active(dekf_handle h, int* active, dekf_mem where);

/* ---- innovation statistics (opt-in, direct handles): do the newest measurements agree with the estimate? -----------------
 * Two more additive symbols: DEKF_ABI_VERSION and dekf_params are unchanged, and a caller that never calls them launches exactly the
 * kernels of before and gets the same bits.  A direct handle returns an estimate and its covariance; these return the numbers that say
 * whether the newest leg measurement agrees with them: its innovation and innovation covariance, the normalised innovation squared
 * (NIS), whole and per leg, and the predictive log-likelihood of the tick.  Summed over a log, loglik is the score of a noise set
 * (with dekf_set_instance_params: B candidate sets on one log give B scores in one pass, no ground truth needed); nis_leg against its
 * chi-square bound (3 degrees of freedom) is the usual test for a stance foot that slips.
 * dekf_set_innovation(h, on), on = 0 (default) or 1.  Call order as for dekf_set_smoother: before dekf_initialize or right after
 * dekf_reset (else DEKF_ERR_ORDER); the setting survives dekf_reset.  DEKF_ERR_INVALID for a null handle, any other `on`, on = 1 on a
 * handle that is not a direct handle (ADMM, KF) and on = 1 on a handle with leg_odom_type = 1.  dekf_set_solver(h, DEKF_SOLVER_ADMM)
 * switches the option off, as it does the smoother; going back to DEKF_SOLVER_DIRECT does not switch it on again.  The option is
 * independent of dekf_set_smoother and dekf_set_window_cross: any combination is allowed.  The first enable allocates the stores:
 * 3L + 9L^2 + 2 + L doubles per instance, L = num_legs (Go1: 162 doubles).
 * An innovation handle's update launches one small kernel (k_mhe_innov_<L>, or its epoch twin k_mhe_innov_<L>_ep behind an epoch or
 * parameter twin of the direct kernel) behind the direct solve on the same stream; timing class 2 brackets the two as one launch.
 * It leaves, per instance and update that solved (window-fill and full windows alike), for the newest step T, with nm = 3 num_legs:
 *  - x^- and P^-: the newest state and its covariance block of the minimiser of the QP the direct solve minimises WITH THE NEWEST
 *    STEP'S MEAS ROWS MADE FREE, i.e. everything the window knows about x_T except this tick's leg measurement; H and y: those rows'
 *    state coefficients and bound; Q_m: their slacks' cost;
 *  - innov[b][:] = nu = y - H x^-;
 *  - innov_cov[b][:][:] = S = H P^- H' + Q_m^-1, row-major and symmetric to the bit;
 *  - nis[b] = nu' S^-1 nu;
 *  - nis_leg[b][l] = nu_l' (S_ll)^-1 nu_l, from leg l's 3-block of nu and its 3 x 3 diagonal block of S;
 *  - loglik[b] = -1/2 (nis + log det S + nm log 2 pi) = log p(y_T | the rest of the window problem).
 * No second elimination: with P = Cov(x_T) and e = y - H x_T, S^-1 = Q_m - Q_m H P H' Q_m and nu = S Q_m e (Woodbury).
 *  - x_mhe, v_b, status, solver info, dekf_get_mhe_cov, dekf_get_window and dekf_get_window_cross are bit-identical to the same handle
 *    with the option off; dekf_solve_kernel_name is unchanged: the solve kernel is the same one.
 *  - An instance whose status is DEKF_SOLVE_NUMERIC, or whose S^-1 has a pivot that is not positive and finite, gets NaN in all five
 *    arrays.  Its status is not changed; its neighbours are unaffected.
 *  - An instance at its local step 0 (restarted by dekf_reset_instances, at dekf_update(h, T0)) has no solve: it holds NaN from the
 *    dekf_reset_instances call on until its first solve.  A paused instance (dekf_set_active) keeps every bit it had at the pausing call.
 *  - On a handle with a parameter table instance b gives the bits of a handle created with its set; after a restart, of a fresh handle
 *    fed the samples from the restart on.  A robot's five arrays do not depend on the batch it runs in, nor on the smoother or the
 *    cross-covariances being on.
 * dekf_get_innovation: innov[B][nm], innov_cov[B][nm][nm], nis[B], nis_leg[B][num_legs], loglik[B].  Any pointer may be NULL.  Host
 * pointers: copy and synchronise; device pointers: in stream order, like dekf_get_mhe_cov.  DEKF_ERR_INVALID on a handle without the
 * option, DEKF_ERR_ORDER before the first update and after dekf_reset until the next update.
 * Not part of this interface: ADMM and KF handles; handles with foot-position states (leg_odom_type 1: a foot that touches down
 * carries a prior variance of about 1e14 against a measurement variance of about 1e-6, and Q_m - Q_m H P H' Q_m cancels completely);
 * the likelihood of the VO rows (they turn into equalities steps after the fact, so vo_p_std is not scored by this number); and
 * whole-window likelihoods. */
dekf_status dekf_set_innovation(dekf_handle h, int on);
dekf_status dekf_get_innovation(dekf_handle h, double* innov, double* innov_cov, double* nis, double* nis_leg, double* loglik,
                                dekf_mem where);

/* ---- innovation gate (opt-in, innovation handles): take a slipping stance leg out of the solve it has just entered ----------
 * Two more additive symbols: DEKF_ABI_VERSION and dekf_params are unchanged, and a caller that never calls them launches exactly the
 * kernels of before and gets the same bits.  nis_leg against a bound says that a stance foot slips; by then the direct solve has folded
 * the leg's velocity rows into x_mhe, v_b and Cov(x_T) at the stance weight, and the window record keeps that weight for the next N
 * windows and then the arrival cost.  With the gate the library acts on the number, on the device, in the launch that computed it.
 * dekf_set_innovation_gate(h, nis_leg_max): 0 (default) switches the gate off, a positive value is the bound.  There is no default
 * bound: INTEGRATION.md says how to choose one.  Call order as for dekf_set_smoother: before dekf_initialize or right after dekf_reset
 * (else DEKF_ERR_ORDER); the setting survives dekf_reset.  DEKF_ERR_INVALID for a null handle; a value that is negative, NaN or
 * infinite; a positive value on a handle without dekf_set_innovation(h, 1) (which excludes ADMM handles, KF handles and leg_odom_type 1);
 * a positive value on a smoothing handle.  dekf_set_smoother(h, 1) on a gating handle is DEKF_ERR_INVALID too: at a gated tick the
 * backward pass has already run on the ungated block, and x_win[K-1] == x_mhe is promised to the bit; the window of a gating handle is
 * not part of this interface.  dekf_set_innovation(h, 0) and dekf_set_solver(h, DEKF_SOLVER_ADMM) switch the gate off; switching those
 * back on does not switch it on again.  The first enable allocates B * num_legs ints.
 * A gating handle's update launches k_mhe_innov_gate_<L> (or its epoch twin k_mhe_innov_gate_<L>_ep) IN PLACE of k_mhe_innov_<L>[_ep]:
 * the same statistics, then the gate, in one launch; timing class 2 brackets it with the direct solve as before.
 * The rule, per instance and update that solved: leg l is gated iff nis_leg[b][l] > nis_leg_max.  NaN compares false, so an instance
 * whose solve or innovation failed gates nothing; a leg in swing never passes (its NIS is about 1e-14).  In leg_odom_type 0 a leg's
 * contact flag changes exactly one thing in the window problem, the leg's 3 x 3 block of the Meas slack cost Q_m (diag of the swing
 * gain, 1 / foot_swing_std^2, for contact 0).  Gating a leg means "this leg was in swing at this tick":
 *  - the leg's block of the newest window record becomes that swing block, word for word what a contact flag of 0 would have written;
 *    on a handle with a parameter table it is the instance's own foot_swing_std.  Every later window and the arrival cost see it;
 *  - x_mhe, v_b and the instance's block of dekf_get_mhe_cov become the optimum and Cov(x_T) of the window QP with those blocks, by a
 *    rank-3 correction of the posterior (every leg reads the same three velocity states), no second elimination;
 *  - if a pivot of the correction is not positive and finite, or its result is not finite: the record edit stands, the instance's
 *    status becomes DEKF_SOLVE_NUMERIC, x_mhe, v_b and its covariance block are NaN.  The next update solves from the records;
 *  - the five arrays of dekf_get_innovation keep their values: they are those of the ungated problem, the evidence for the decision;
 *  - gated[b][l] = 1 for the legs this update gated, 0 for the others.
 * In bits: a bound so high that it never fires leaves every output equal to the same handle with the gate off.  At every update at
 * which an instance gates nothing, dekf_get, dekf_get_mhe_cov, solver info and the five arrays are bit-identical to those of an
 * innovation handle without the gate that is fed the same log with contact = 0 at every (tick, leg) this instance gated before.  At an
 * update at which it gates, x_mhe, v_b and the covariance agree with that handle to rounding (not to the bit).  A robot's results do
 * not depend on the batch it runs in.
 * dekf_reset zeroes all of gated; dekf_reset_instances zeroes the restarted instances' entries, and from its restart on such an
 * instance gives the bits of a fresh gating handle; a paused instance (dekf_set_active) keeps its gated as it keeps everything else.
 * dekf_get_innovation_gate: *nis_leg_max (host memory, on any handle; 0 = off) and gated[B][num_legs] (ints; all 0 before the first
 * update).  Either pointer may be NULL.  gated on a handle whose gate is off: DEKF_ERR_INVALID.  Host pointer: copy and synchronise;
 * device pointer: in stream order, like dekf_get_mhe_cov.
 * Not part of this interface: a bound per instance; a history of decisions (gated is the last update's); smoothing handles. */
dekf_status dekf_set_innovation_gate(dekf_handle h, double nis_leg_max);
dekf_status dekf_get_innovation_gate(dekf_handle h, double* nis_leg_max, int* gated, dekf_mem where);

/* ---- the window of a gating handle (opt-in, gating handles): carry the gate's correction down the smoothed window ------------
 * One more additive symbol: DEKF_ABI_VERSION and dekf_params are unchanged, and a caller that never calls it launches exactly the
 * kernels of before and gets the same bits.  dekf_set_smoother and dekf_set_innovation_gate refuse each other as the section above
 * says; this call is the exception to it.  Gating a leg at step T changes the newest block's information alone, the smoother's gains
 * of the older steps do not read step T's measurement, and its backward recursion is affine in the newest state and covariance: the
 * gate's rank-3 correction of the posterior runs down the window as a rank-3 correction of every block.
 * dekf_set_gate_smoother(h, 1) needs a gating handle (dekf_set_innovation_gate with a bound > 0, hence a direct innovation handle with
 * leg_odom_type 0) whose smoother is off, else DEKF_ERR_INVALID; after dekf_initialize DEKF_ERR_ORDER (call order as for
 * dekf_set_smoother); DEKF_ERR_INVALID for a null handle and a value other than 0 or 1.  Calling it again is allowed.  The handle
 * becomes a smoothing handle: the first enable allocates the smoother's stores, dekf_solve_kernel_name names the _smooth twin,
 * dekf_get_window works as on any smoothing handle, and the setting survives dekf_reset.  dekf_set_gate_smoother(h, 0) switches the
 * option and the smoother off; the gate stays on.  While the option is on:
 *  - dekf_set_smoother(h, 0) switches both off; dekf_set_smoother(h, 1) stays DEKF_ERR_INVALID;
 *  - dekf_set_innovation_gate(h, 0) switches the gate, the option and the smoother off; a positive value changes the bound (this is
 *    the only smoothing handle on which that call is allowed);
 *  - dekf_set_window_cross(h, 1) is DEKF_ERR_INVALID: its backward pass overwrites the gains this correction reads;
 *  - dekf_set_innovation(h, 0) and dekf_set_solver(h, DEKF_SOLVER_ADMM) switch everything off, as they do without the option.
 * Such a handle's update launches the direct kernel's _smooth twin and, IN PLACE of k_mhe_innov_gate_<L>[_ep], its twin
 * k_mhe_innov_gate_<L>_smooth[_ep]; timing class 2 brackets both as before.
 * The contract, per instance and update.  An instance that gates nothing: the kernel touches nothing but gated, and the window is the
 * smoothing kernel's.  An instance that gates: x_win[b][k] and cov_win[b][k], k = 0 .. K-1, become the state blocks of the optimum of
 * the window QP with the gated legs' swing blocks (the QP whose newest block the gate returns) and their covariances; x_win[b][K-1] is
 * bit-identical to x_mhe[b], cov_win[b][K-1] to the instance's block of dekf_get_mhe_cov, and every cov_win[b][k] is symmetric to the
 * bit.  A failed correction (the gate's DEKF_SOLVE_NUMERIC) gives NaN in all K entries of both arrays, as a failed smoother does.
 * Everything else (x_mhe, v_b, status, solver info, dekf_get_mhe_cov, the five arrays of dekf_get_innovation, gated and the record
 * edit) is bit-identical to the same gating handle without the option.  At every update at which an instance gates nothing, its
 * window too is bit-identical to that of a smoothing innovation handle without the gate fed the log with contact = 0 at every
 * (tick, leg) this instance gated before.  A paused instance keeps every bit; a restarted one behaves as on a smoothing handle and
 * on a gating handle; a parameter table is honoured as the gate honours it.
 * Snapshots: the blob format is unchanged (its header already carries the smoother setting and the bound); a blob of such a handle
 * loads into a handle with the same settings and is refused by any other, as today.
 * Not part of this interface: cross-covariances of a gating handle; ADMM and KF handles; leg_odom_type 1. */
dekf_status dekf_set_gate_smoother(dekf_handle h, int on);

/* ---- snapshots of single instances (direct handles): one robot leaves its slot, its handle, its process -----------------------
 * Three more additive symbols: DEKF_ABI_VERSION and dekf_params are unchanged, and a caller that never calls them launches exactly the
 * kernels of before and gets the same bits.  An instance can be restarted, paused and given its own noise; with these it can also be
 * checkpointed and brought back after a process restart, migrated to another handle, batch size, GPU or rank (dekf_allgather_vb
 * shards a fleet over ranks; this rebalances the shards), and forked: copied into a second slot to run two hypotheses side by side
 * from that point, with the per-tick loglik of dekf_get_innovation as the score between them.
 * A blob is opaque and self-describing: a fixed header (a magic, a format version, a fingerprint, n and the bytes per instance)
 * followed by n contiguous per-instance records in the order of idx.  A record holds the instance's LOCAL step and LOCAL EKF count
 * (the count reduced as a resume stores it), its noise fields as dekf_get_instance_params returns them, and every persistent
 * per-instance array of the handle: latches, EKF state and history, sample stack, window records, arrival cost (the one computed
 * ahead included), tags, outputs, and the handle's optional stores that are allocated: Cov(x_T), the smoother's window stores, the
 * cross store, the five innovation arrays and gated.  The handle's own step, EKF tick count and epochs are never stored, so a record
 * loads into any slot of any compatible handle at any step.  The fingerprint is every field of dekf_params outside the noise fields
 * and every setting: solver, smoother, cross, innovation, the gate and its bound.  A blob is valid for the library build that wrote
 * it; it is not a file format across versions.
 * dekf_snapshot_bytes(h, n): bytes of a blob of n instances of h; 0 on a handle that cannot save (ADMM, KF, pipelined, null) and for
 * n <= 0.  idx[n] is always a host pointer; blob is host or device memory, as `where` says.
 * dekf_save_instances(h, idx, n, blob, bytes, where):
 *  - Where: a direct handle without solve_pipeline.  DEKF_ERR_INVALID on ADMM, KF and pipelined handles; DEKF_ERR_ORDER before
 *    dekf_initialize.
 *  - When: anywhere between dekf_update(h, T0 - 1) and dekf_update(h, T0); on a two-rate handle before, between or behind the EKF
 *    ticks of that gap.  The handle's stream waits for what dekf_reset_instances waits for (the arrival cost computed ahead has
 *    landed before it is copied).  The call returns when the blob is written, host or device.
 *  - Any instance may be saved.  An active one: its current local step and count; a paused one: those it stands at; one restarted
 *    and not yet initialised: local tick -1.
 *  - Saving changes nothing: the handle keeps its kernels (dekf_solve_kernel_name) and every bit of every later output.
 *  - DEKF_ERR_INVALID, with nothing written: a null handle, idx or blob; n <= 0; an index outside 0 .. B - 1; an index named twice;
 *    bytes below dekf_snapshot_bytes(h, n).
 * dekf_load_instances(h, idx, n, blob, bytes, where): where and when as for saving, on an initialised handle.  The header and the
 * records' counters and noise fields of a device blob are copied to the host and waited for, as a device mask is.
 *  - Checks; any failure is DEKF_ERR_INVALID and then NOTHING is applied.  Magic, format version and fingerprint must match; n must
 *    be the blob's n; bytes at least dekf_snapshot_bytes(h, n); the indices as for saving; and the noise fields of record i must
 *    equal, byte for byte, those instance idx[i] has now: the handle's own on a handle without a parameter table, else the slot is
 *    first given the set by dekf_reset_instances, then dekf_set_instance_params.  A difference is refused, never ignored.
 *  - After the load instance idx[i] IS the saved instance, and it is active.  Every getter returns the saved values to the bit:
 *    dekf_get, dekf_get_ekf_cov, dekf_get_mhe_cov, dekf_get_solver_info, its first K_b entries of dekf_get_window and
 *    dekf_get_window_cross, dekf_get_innovation and gated of dekf_get_innovation_gate (a getter that refuses before the handle's first
 *    update still does); dekf_get_instance_ticks returns its local step.  Its epochs are those of a resume: t0 = next step - local
 *    step, which is negative when an old robot loads into a young handle, and c0 = EKF tick count - local count.  A record saved at
 *    local tick -1 loads as a freshly restarted instance: its first update is its dekf_initialize.
 *  - IMU and leg samples are pushed at least once between the load and the instance's next tick or update (the rule of
 *    dekf_reset_instances).  From then on every output of the instance is bit-identical to the source instance on an uninterrupted
 *    handle fed the same samples, ticks and updates in order, whatever the batch size of the destination, the step it stands at, and
 *    whether the blob went through the host.
 *  - Instances not named keep every bit of every output at every later step.
 *  - After the first load the handle launches the epoch twins (_ep, or _pp with a table), exactly as after a restart, until
 *    dekf_reset, which forgets loaded instances like everything else.
 *  - Forking: two indices of one handle may be given copies of one record by two loads of the same blob.
 * Not part of this interface: ADMM, KF and pipelined handles; blobs across library versions; a handle whose parameters outside the
 * noise fields or whose settings differ in any field; changing an instance's noise by loading it. */
size_t dekf_snapshot_bytes(dekf_handle h, int n);
dekf_status dekf_save_instances(dekf_handle h, const int* idx, int n, void* blob, size_t bytes, dekf_mem where);
dekf_status dekf_load_instances(dekf_handle h, const int* idx, int n, const void* blob, size_t bytes, dekf_mem where);

/* status[B] values written by dekf_update */
#define DEKF_SOLVE_NONE 0       /* no solve yet (T = 0) */
#define DEKF_SOLVE_OK 1         /* OSQP_SOLVED */
#define DEKF_SOLVE_MAX_ITER 2   /* OSQP_MAX_ITER_REACHED; iterate still returned, as osqp-eigen does */
#define DEKF_SOLVE_NUMERIC -1   /* non-finite value or zero pivot */

/* ---- measurement (the reference's tic/toc helpers, DecentralEst.cpp:1031-1044) ------- */
/* on = 1: every kernel launch of the hot path is bracketed by HIP events on the handle's stream; on = 2: only the
 * MHE solve launches (class 2) — an event pair costs the stream about 7 us, six of them per step are 1 % of a
 * 2 ms step, so a throughput measurement that only needs the dominant kernel's launch time asks for 2; on = 0: off.  dekf_timing_read synchronises and returns, per kernel class
 * (0 ekf tick, 1 MHE assemble/marginalise [or KF update], 2 MHE ADMM solve, 3 all-gather of v_b), the summed
 * device milliseconds and the number of launches since the last read. */
#define DEKF_TIMING_CLASSES 4 /* (ABI 4: class 3 = the RCCL all-gather of v_b, bracketed on the handle's communication stream in either
                               * timing mode — it is not on the step's critical path) */
dekf_status dekf_timing_enable(dekf_handle h, int on);
dekf_status dekf_timing_read(dekf_handle h, double* ms_sum, int* launches);

/* How the solve kernel is launched on this device: the number of persistent workgroups (each solves
 * ceil(B / solve_workgroups) instances back to back per launch), the compute units and the engine clock in Hz —
 * what a caller needs to turn a launch time into cycles per solve. Any pointer may be NULL. */
dekf_status dekf_launch_info(dekf_handle h, int* solve_workgroups, int* compute_units, double* clock_hz);
/* Name of the solve kernel this handle launches for full windows (full_window != 0) or for the window-fill ticks,
 * e.g. "k_mhe_solve_r3_4_n20": lets a caller match profiler output (rocprofv3 kernel names) to the run. NULL for a
 * KF handle. The string lives as long as the library. */
const char* dekf_solve_kernel_name(dekf_handle h, int full_window);

/* ---- multi-GPU (new: the reference is single-robot) ------------------------------ */
/* All-gather of the fused base velocity over RCCL: every rank contributes its
 * v_b[B][3] and receives v_b_all[world][B][3] (device pointer). The communicator is
 * created from an ncclUniqueId distributed by the caller (torch.distributed, MPI, ...).
 *
 * dekf_allgather_vb is asynchronous twice over: it snapshots v_b in stream order (after
 * the step that produced it) and runs the collective on a second stream owned by the
 * handle, so the exchange of step T overlaps the kernels of step T+1 and a slow rank
 * delays the others by at most one step of slack. v_b_all is complete after dekf_sync,
 * or in stream order after dekf_allgather_wait (which makes dekf_stream() wait for the
 * last all-gather without blocking the host). Use a different v_b_all buffer while the
 * previous one is still being read on another stream. */
#define DEKF_UNIQUE_ID_BYTES 128
dekf_status dekf_comm_unique_id(void* id_out);
dekf_status dekf_comm_init(dekf_handle h, int world, int rank, const void* id);
dekf_status dekf_allgather_vb(dekf_handle h, double* v_b_all_dev);
dekf_status dekf_allgather_wait(dekf_handle h);
/* What the COMMUNICATOR itself says about the exchange (ncclCommCount / ncclCommUserRank of the handle's communicator), not what
 * the caller passed to dekf_comm_init — so that a throughput line can prove how many ranks RCCL really connected.  And a device-side
 * proof of one exchange: every rank contributes its own rank number, dekf_comm_ranks_seen all-gathers them on the communication
 * stream, waits, and writes how many DISTINCT, in-range rank numbers arrived (== world on a working communicator).  Both are
 * collectives over the communicator's ranks where noted.  Any out pointer may be NULL. */
dekf_status dekf_comm_info(dekf_handle h, int* comm_world, int* comm_rank);
dekf_status dekf_comm_ranks_seen(dekf_handle h, int* ranks_seen); /* collective */

#ifdef __cplusplus
}
#endif
#endif /* DEKF_H */
