// dekf_capi.hip — implementation of the C ABI in include/dekf.h on top of the gfx950 kernels.
// No CPU fallback: without a usable HIP device dekf_create fails with DEKF_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dekf.h"
#include "cfg.h"
#include "host_common.h"
#include "kf_core.h"
#include "mhe_assemble_core.h"
#include "mhe_direct_core.h"
#include "mhe_epoch_core.h"
#include "mhe_gate_core.h"
#include "mhe_gate_window_core.h"
#include "mhe_innov_core.h"
#include "mhe_params_core.h"
#include "mhe_pause_core.h"
#include "mhe_snapshot_core.h"
#include "mhe_solve_core.h"

using namespace dekf;

extern "C" {
__global__ void k_ekf_tick(DevCfg c, DevState s, int count);
__global__ void k_mhe_initialize(DevCfg c, DevState s);
__global__ void k_mhe_assemble(DevCfg c, DevState s, int T, int pushes);
__global__ void k_mhe_marginalize_early(DevCfg c, DevState s, int T);
// every solve kernel and its twin with OSQP's polishing step (solve_kernels.def)
#define DEKF_SOLVE_KERNEL(NAME, ...)                                                   \
    __global__ void NAME(DevCfg c, DevState s, int kstart, int K, int gws_len);        \
    __global__ void NAME##_pol(DevCfg c, DevState s, int kstart, int K, int gws_len);  \
    __global__ void NAME##_warm(DevCfg c, DevState s, int kstart, int K, int gws_len); \
    __global__ void NAME##_warm_pol(DevCfg c, DevState s, int kstart, int K, int gws_len);
#include "solve_kernels.def"
// the direct solve kernels: every row of direct_kernels.def in every variant of its list
#define DEKF_DIRECT_DECLARE_(SUFFIX, SMOOTH, CROSS, CLOCK, NAME) __global__ void NAME##SUFFIX(DEKF_DIRECT_PARAMS(SMOOTH, CROSS, CLOCK));
#define DEKF_DIRECT_KERNEL(NAME, ...) DEKF_DIRECT_VARIANTS(DEKF_DIRECT_DECLARE_, NAME)
#include "direct_kernels.def"
// the innovation kernels behind the direct solve (mhe_innov_core.h), one per leg count, and their epoch twins
#define DEKF_INNOV_KERNEL(L)                                                                                          \
    __global__ void k_mhe_innov_##L(DevCfg c, DevState s, int kstart, int K, const double* cov, InnovStore out);      \
    __global__ void k_mhe_innov_##L##_ep(DevCfg c, DevState s, int T, const double* cov, InnovStore out, const int* t0);
DEKF_INNOV_KERNEL(1)
DEKF_INNOV_KERNEL(2)
DEKF_INNOV_KERNEL(3)
DEKF_INNOV_KERNEL(4)
#undef DEKF_INNOV_KERNEL
__global__ void k_innov_nan(DevCfg c, const int* mask, InnovStore out);
// the gate kernels (mhe_gate_core.h): the innovation kernel's body with the gate behind it, one per leg count, and their epoch twins
#define DEKF_GATE_KERNEL(L)                                                                                                       \
    __global__ void k_mhe_innov_gate_##L(DevCfg c, DevState s, int kstart, int K, double* cov, InnovStore out, GateStore gs);     \
    __global__ void k_mhe_innov_gate_##L##_ep(DevCfg c, DevState s, int T, double* cov, InnovStore out, GateStore gs, const int* t0, \
                                              const DevCfg* pc);
DEKF_GATE_KERNEL(1)
DEKF_GATE_KERNEL(2)
DEKF_GATE_KERNEL(3)
DEKF_GATE_KERNEL(4)
#undef DEKF_GATE_KERNEL
// the gate kernels of a smoothing gate handle (mhe_gate_window_core.h): the gate kernel's body with the window correction behind it
#define DEKF_GATE_SMOOTH_KERNEL(L)                                                                                                \
    __global__ void k_mhe_innov_gate_##L##_smooth(DevCfg c, DevState s, int kstart, int K, double* cov, InnovStore out, GateStore gs, \
                                                  DirectWindow win);                                                             \
    __global__ void k_mhe_innov_gate_##L##_smooth_ep(DevCfg c, DevState s, int T, double* cov, InnovStore out, GateStore gs,     \
                                                     const int* t0, const DevCfg* pc, DirectWindow win);
DEKF_GATE_SMOOTH_KERNEL(1)
DEKF_GATE_SMOOTH_KERNEL(2)
DEKF_GATE_SMOOTH_KERNEL(3)
DEKF_GATE_SMOOTH_KERNEL(4)
#undef DEKF_GATE_SMOOTH_KERNEL
__global__ void k_gap();
__global__ void k_kf_initialize(DevCfg c, DevState s);
__global__ void k_kf_update(DevCfg c, DevState s, int pushes);
__global__ void k_latch_vo(DevCfg c, DevState s, const int* mask, const double* t_pre, const double* t_now,
                           const double* dp, const double* t_pose, const double* q_vo);
__global__ void k_reset_state(DevCfg c, DevState s);
// restarting single instances (mhe_epoch_core.h)
__global__ void k_reset_instances(DevCfg c, DevState s, const int* mask, double* cov, int* t0, int* c0, int next_T, int ekf_count);
__global__ void k_fold_epochs(int* c0, int B, int count_old, int count_new, int H);
__global__ void k_ekf_tick_ep(DevCfg c, DevState s, int count, const int* c0);
__global__ void k_mhe_assemble_ep(DevCfg c, DevState s, int T, int pushes, const int* t0);
__global__ void k_mhe_marginalize_early_ep(DevCfg c, DevState s, int T, const int* t0);
// noise parameters per instance (mhe_params_core.h)
__global__ void k_ekf_tick_pp(DevCfg c, DevState s, int count, const int* c0, const double* pe);
__global__ void k_mhe_assemble_pp(DevState s, int T, int pushes, const int* t0, const DevCfg* pc);
__global__ void k_mhe_marginalize_early_pp(DevState s, int T, const int* t0, const DevCfg* pc);
__global__ void k_reset_instances_pp(DevCfg c, DevState s, const int* mask, double* cov, int* t0, int* c0, int next_T, int ekf_count, const double* pe);
__global__ void k_reset_state_pp(DevCfg c, DevState s, const double* pe);
__global__ void k_ekf_init_pp(DevCfg c, DevState s, const int* mask, const double* pe);
// pausing single instances (mhe_pause_core.h)
__global__ void k_ekf_tick_act(DevCfg c, DevState s, int count, const int* c0);
__global__ void k_ekf_tick_act_pp(DevCfg c, DevState s, int count, const int* c0, const double* pe);
__global__ void k_mhe_assemble_act(DevCfg c, DevState s, int T, int pushes, const int* t0);
__global__ void k_mhe_assemble_act_pp(DevState s, int T, int pushes, const int* t0, const DevCfg* pc);
__global__ void k_latch_vo_act(DevCfg c, DevState s, const int* mask, const int* t0, const double* t_pre, const double* t_now,
                               const double* dp, const double* t_pose, const double* q_vo);
__global__ void k_fold_epochs_act(int* c0, int B, int count_old, int count_new, int H);
// snapshots of single instances (mhe_snapshot_core.h)
__global__ void k_save_instances(StateMap m, const int* idx, const SnapBooks* books, unsigned char* recs, size_t rec_bytes);
__global__ void k_load_instances(StateMap m, const int* idx, const unsigned char* recs, size_t rec_bytes);
__global__ void k_ekf_cov_out(DevCfg c, DevState s, double* out);
__global__ void k_latch4(LatchCopy4 a);
__global__ void k_go1_leg_odometry(DevCfg c, DevState s, const double* jp, const double* jv, const double* force,
                                   double thr, double pibx, double piby, double pibz);
}

namespace {
thread_local std::string g_err;

struct RcclApi;  // rccl_dyn.h
}  // namespace
#include "rccl_dyn.h"

namespace { struct SolveKernel; struct DirectKernel; }
struct dekf_handle_s {
    dekf_params prm;
    DevCfg c;
    DevState s;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::vector<void*> blocks;
    // staging for host-side pushes / gets
    void* stage = nullptr;
    size_t stage_bytes = 0;
    // What a step launches is said once, by solve_launch(), from the settings and these fields.  The ADMM solve: the catalogue's row
    // (solve_kernels.def) of the window-fill kernel and its grid ...
    const SolveKernel* solve_entry = nullptr;
    int solve_grid = 0, gws_len = 0;
    // ... and for full windows (K == N) of the shapes that have one, the row of the kernel with more workgroups per CU (kernels.hip),
    // its own grid, workgroup size and LDS size
    const SolveKernel* solve_entry_full = nullptr;
    int solve_grid_full = 0;
    int solve_threads_full = DEKF_SOLVE_THREADS;  // (the four-per-CU kernels: DEKF_R4_THREADS)
    size_t lds_solve_full = 0;
    // dekf_set_solver: DEKF_SOLVER_ADMM (0) or DEKF_SOLVER_DIRECT (1).  A direct handle launches `direct` (one wavefront per instance,
    // a grid of B) wherever an in-order ADMM handle launches its solve, and keeps Cov(x_T) of the last update in mhe_cov ([B][ns][ns])
    int solver = DEKF_SOLVER_ADMM;
    const DirectKernel* direct = nullptr;
    double* mhe_cov = nullptr;
    size_t lds_direct = 0;
    bool mhe_cov_valid = false;  // an update has written mhe_cov since dekf_create / dekf_reset
    // dekf_set_smoother: a smoothing direct handle launches the direct kernel's twin (direct->fn_smooth), which also leaves x_k and
    // Cov(x_k) of every window step in win.x / win.cov (mhe_direct_core.h: DirectWindow); win_steps: K of the last update, 0 before
    // the first one since dekf_create / dekf_reset
    bool smoother = false;
    DirectWindow win;
    int win_steps = 0;
    // dekf_set_window_cross: a cross handle (a smoothing handle with the option) launches direct->fn_cross, whose backward pass turns
    // win.t1's entries into Cov(x_k, x_{k+1}) and leaves Cov(x_k, x_T) in cross_st.newest (mhe_direct_core.h: DirectCross)
    bool cross = false;
    DirectCross cross_st;
    // dekf_set_innovation: an innovation handle launches the innovation kernel of its leg count (mhe_innov_core.h) behind the direct
    // kernel, whichever twin that is, on the same stream; it leaves the five arrays of dekf_get_innovation in innov_st (one block).
    // innov_valid: an update has written them since dekf_create / dekf_reset
    bool innov = false;
    InnovStore innov_st;
    bool innov_valid = false;
    // dekf_set_innovation_gate: a gating handle (gate_st.nis_leg_max > 0; an innovation handle) launches the gate kernel of its leg
    // count (mhe_gate_core.h) in place of the innovation kernel.  gate_st.gated: [B][L] ints, allocated by the first call that
    // switches the gate on, zeroed by dekf_reset and, for the restarted instances, by dekf_reset_instances
    GateStore gate_st;
    // dekf_set_gate_smoother: a gating handle that smooths.  The option switches `smoother` on with it (the handle is a smoothing handle
    // in every other respect) and makes the handle launch the gate kernel's _smooth twin (mhe_gate_window_core.h), which carries the
    // gate's correction down win.x / win.cov with the T1_k the smoothing kernel left in win.t1.  True only with smoother and a bound > 0
    bool gate_smoother = false;
    // dekf_save_instances, dekf_load_instances: the state map (mhe_snapshot_core.h), every persistent per-instance array of `s`
    // (host_common.h: state_map, at dekf_create) and the stores above, each appended where it is allocated
    StateMap snap_map;
    // The per-instance state of a direct handle: what dekf_reset_instances, dekf_set_active and dekf_set_instance_params keep.
    struct Instances {
        // dekf_reset_instances: the epochs (mhe_epoch_core.h).  t0 | c0: [B] ints each on the device (one block), the handle's step
        // and EKF tick count at every instance's last restart (0: never); t0_host: the host's copy of t0 (dekf_get_instance_ticks,
        // the window getters' steps); c0_host: the host's copy of c0 (dekf_set_instance_params: an instance whose c0 is the handle's
        // count has not ticked since its restart), folded with c0.
        int *t0 = nullptr, *c0 = nullptr;
        std::vector<int> t0_host, c0_host;
        // dekf_set_active: pausing single instances (mhe_pause_core.h).  While instance b is paused the device's t0[b] and c0[b], and
        // t0_host[b] and c0_host[b] with them, hold the sentinel, and pz_step[b] | pz_count[b] its next local step and local EKF
        // count; act_host[b]: 1 runs, 0 is paused.  min_t0: the smallest epoch of the active instances (the sentinel: none is);
        // max_frozen: the largest local step at which a paused one stands (-1: none is paused) — bounds() keeps the two.
        std::vector<int> act_host, pz_step, pz_count;
        int min_t0 = 0, max_frozen = -1;
        // dekf_set_instance_params: the noise constants of every instance (mhe_params_core.h).  pp_mhe [B] DevCfg and pp_ekf
        // [PpEkf::len][B] on the device, allocated by the first call that sets a table; inst_prm: the handle's parameters with every
        // instance's noise fields (dekf_get_instance_params)
        DevCfg* pp_mhe = nullptr;
        double* pp_ekf = nullptr;
        std::vector<dekf_params> inst_prm;
        // Since dekf_create / dekf_reset (read through instance_mode()): restarted, an instance has been restarted or paused; paused;
        // table, the handle has a parameter table.  Invariants: paused implies restarted; restarted or table implies that ensure() has
        // run, i.e. that the epoch arrays and the five host vectors exist (every epoch 0 and every instance active until `restarted`).
        bool restarted = false, paused = false, table = false;
        dekf_status ensure(dekf_handle_s* h);  // allocates the epoch arrays, all 0, at the first call that needs them
        void bounds();                         // min_t0 and max_frozen from the host vectors
        dekf_status clear(dekf_handle_s* h);   // dekf_reset: every epoch 0, nobody paused (pausing is state, not a setting); the table survives
    } inst;
    size_t lds_solve = 0, lds_asm = 0, lds_kf = 0;
    int ekf_count = 0, pushes = 0, next_T = 0;
    bool initialized = false;
    // timing: 0 off, 1 every kernel class, 2 only the MHE solve (class 2)
    int timing = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[DEKF_TIMING_CLASSES];
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    // Step pipelining (dekf_params.solve_pipeline): the solve of step T runs on solve_stream[T & 1] out of set T & 1 of the
    // per-solve data (outputs, scratch slabs) and copy T mod 3 of its input snapshot, so the pushes, the EKF tick and the
    // assemble of step T + 1 — and then its solve — start while the last round of step T's persistent workgroups is still
    // running (a launch of B instances on S slots runs ceil(B / S) rounds, the last one partly empty: 4096 on 768 is 5.33).
    bool pipelined = false;
    DevState sp[2];               // sp[0] == s; sp[1]: the second set
    hipStream_t solve_stream[2] = {nullptr, nullptr};
    hipEvent_t ev_asm[2] = {nullptr, nullptr}, ev_solve[2] = {nullptr, nullptr}, ev_mark[2] = {nullptr, nullptr};
    // input snapshots by T mod 3: ev_snap_free[i] is recorded behind the solve that read copy i, the assemble of three steps on waits for it
    hipEvent_t ev_snap_free[3] = {nullptr, nullptr, nullptr};
    bool snap_busy[3] = {false, false, false};
    bool solve_pending[2] = {false, false};
    int last_par = 0;             // set the newest results are in
    // In-order mode: the arrival cost of step T + 1 is computed ahead of time on early_stream (k_mhe_marginalize_early), behind the
    // assemble of step T and beside its solve — i.e. in the slots that solve frees in its partly empty last round — and the assemble
    // of step T + 1 takes it unless a vision interval arrived (cfg.h: DevState::Mp_next).  44 of the 67 us of term construction in
    // front of every solve leave the critical path; results are the same bits.
    hipStream_t early_stream = nullptr;
    hipEvent_t ev_asm_done = nullptr, ev_early_done = nullptr, ev_early_mark = nullptr;
    bool early_pending = false;
    // RCCL: the all-gather runs on its own stream out of a snapshot of v_b, so that it overlaps the next step
    void* comm = nullptr;
    int world = 1, rank = 0;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_vb_ready = nullptr, ev_ag_done = nullptr;
    // pipelined mode: recorded when the all-gather's snapshot copy has READ set i's v_b — what the next solve into set i waits for
    // (one event per set: the solve of step T + 1 must not wait for the copy that follows the solve of step T, or nothing overlaps)
    hipEvent_t ev_vb_read[2] = {nullptr, nullptr};
    bool vb_read_pending[2] = {false, false};
    double* vb_snapshot = nullptr;
    bool ag_pending = false;
};

namespace {

#define HIPCHK(expr)                                                                                       \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) {                                                                            \
            g_err = std::string(#expr) + ": " + hipGetErrorString(e_);                                     \
            return DEKF_ERR_HIP;                                                                           \
        }                                                                                                  \
    } while (0)

dekf_status fail(dekf_status st, const char* msg) {
    g_err = msg;
    return st;
}

// a failed step of an entry point is the entry point's status (the message is in g_err)
#define TRY(expr) do { if (dekf_status st_ = (expr)) return st_; } while (0)

// The solve kernels as dekf_create selects them: every row of solve_kernels.def with its twins, by [warm][polish]
typedef void (*SolveFn)(DevCfg, DevState, int, int, int);
enum class SolveRole { ll, lg, gg, foot_lg, foot_gg, r3, r4, rr };
struct SolveKernel {
    SolveRole role;
    int legs, nfix;  // solve_window_t's L and NFIX (0: run-time horizon)
    bool warm_twin;  // a warm handle launches fn[1][.] (solve_kernels.def: DEKF_WARM_TWIN_<role>); every other row's fn[0][.] carries the warm start
    SolveFn fn[2][2];
    const char* name[2][2];
};
#define DEKF_LEGS_(L, ...) L
#define DEKF_NFIX_(L, FACTOR_LDS, PA_LDS, NFIX, ...) NFIX
#define DEKF_WARM_TWIN_OF_(ROLE) DEKF_WARM_TWIN_##ROLE
#define DEKF_SOLVE_KERNEL(NAME, ROLE, THREADS, WAVES, LOOP, ...)                                                 \
    {SolveRole::ROLE, DEKF_LEGS_(__VA_ARGS__), DEKF_NFIX_(__VA_ARGS__, 0, 0), DEKF_WARM_TWIN_OF_(ROLE) != 0,      \
     {{NAME, NAME##_pol}, {NAME##_warm, NAME##_warm_pol}}, {{#NAME, #NAME "_pol"}, {#NAME "_warm", #NAME "_warm_pol"}}},
const SolveKernel solve_kernels[] = {
#include "solve_kernels.def"
};

// The twin of row k that a handle with these settings launches, picked here and nowhere else.  osqp.polish: the twin with the polishing
// step; warm (dekf_set_warm_start): the twin with the warm start, of a full-window kernel whose register budget left that code out
struct SolveTwin { SolveFn fn; const char* name; };
SolveTwin solve_twin(const SolveKernel* k, bool polish, bool warm) {
    const int w = warm && k->warm_twin, p = polish;
    return {k->fn[w][p], k->name[w][p]};
}

// the kernel of ROLE for L legs: the one compiled for the horizon N if there is one, else the one with a run-time horizon
const SolveKernel* solve_kernel(SolveRole role, int L, int N) {
    const SolveKernel* any = nullptr;
    for (const SolveKernel& k : solve_kernels) {
        if (k.role != role || k.legs != L) continue;
        if (k.nfix == N) return &k;
        if (k.nfix == 0) any = &k;
    }
    return any;
}

// The instance mode of a handle, which says which twin of every kernel it launches ("what a handle launches", below).  The clock is the
// CLOCK of direct_kernels.def's variants.  WINDOW: uniform, the kernels of a handle without per-instance state.  EPOCH: an instance has
// been restarted or paused — the *_ep kernels, every instance on its local step.  PARAM: the handle has a parameter table — the *_pp
// kernels, the epoch kernels with the table as one more argument, with or without a restarted instance (`restarted`).
// paused: an instance has been paused — the *_act kernels where there is one, which skip a paused instance.
enum class Clock { WINDOW, EPOCH, PARAM };
struct InstanceMode { Clock clock; bool restarted, paused; };
InstanceMode instance_mode(const dekf_handle_s* h) {
    const dekf_handle_s::Instances& i = h->inst;
    return {i.table ? Clock::PARAM : (i.restarted ? Clock::EPOCH : Clock::WINDOW), i.restarted, i.paused};
}

// The direct solve kernels as dekf_set_solver selects them: every row of direct_kernels.def with the kernels of its variants
// (DirectVariant: the list's entries; direct_variants[v]: SMOOTH, CROSS and the clock of entry v)
#define DEKF_DIRECT_ENUM_(SUFFIX, ...) dv##SUFFIX,
enum DirectVariant { DEKF_DIRECT_VARIANTS(DEKF_DIRECT_ENUM_) dv_count };
struct DirectVariantInfo { bool smooth, cross; Clock clock; };
#define DEKF_DIRECT_INFO_(SUFFIX, SMOOTH, CROSS, CLOCK, ...) {SMOOTH != 0, CROSS != 0, Clock::CLOCK},
const DirectVariantInfo direct_variants[dv_count] = {DEKF_DIRECT_VARIANTS(DEKF_DIRECT_INFO_)};
struct DirectKernel {
    int legs, ft, nfix;  // direct_solve_t's L and FT; the horizon the row is meant for (0: any)
#define DEKF_DIRECT_FIELD_(SUFFIX, SMOOTH, CROSS, CLOCK, ...) void (*fn##SUFFIX)(DEKF_DIRECT_PARAMS(SMOOTH, CROSS, CLOCK));
    DEKF_DIRECT_VARIANTS(DEKF_DIRECT_FIELD_)  // fn, fn_smooth, ...: every variant's kernel with its own signature
    const char* name[dv_count];  // by DirectVariant
};
#define DEKF_DIRECT_FN_(SUFFIX, SMOOTH, CROSS, CLOCK, NAME) NAME##SUFFIX,
#define DEKF_DIRECT_NAME_(SUFFIX, SMOOTH, CROSS, CLOCK, NAME) #NAME #SUFFIX,
#define DEKF_DIRECT_KERNEL(NAME, L, FT, NFIX) \
    {L, FT, NFIX, DEKF_DIRECT_VARIANTS(DEKF_DIRECT_FN_, NAME) {DEKF_DIRECT_VARIANTS(DEKF_DIRECT_NAME_, NAME)}},
const DirectKernel direct_kernels[] = {
#include "direct_kernels.def"
};

// the direct kernel of the shape: the one meant for the horizon N if there is one, else the one for any horizon
const DirectKernel* direct_kernel(int L, int ft, int N) {
    const DirectKernel* any = nullptr;
    for (const DirectKernel& k : direct_kernels) {
        if (k.legs != L || k.ft != ft) continue;
        if (k.nfix == N) return &k;
        if (k.nfix == 0) any = &k;
    }
    return any;
}

// The innovation kernels as dekf_set_innovation selects them: by leg count, the kernel and its epoch twin
typedef void (*InnovFn)(DevCfg, DevState, int, int, const double*, InnovStore);
typedef void (*InnovEpochFn)(DevCfg, DevState, int, const double*, InnovStore, const int*);
struct InnovKernel { InnovFn fn; InnovEpochFn fn_ep; };
const InnovKernel innov_kernels[DEKF_MAX_LEGS] = {{k_mhe_innov_1, k_mhe_innov_1_ep}, {k_mhe_innov_2, k_mhe_innov_2_ep},
                                                  {k_mhe_innov_3, k_mhe_innov_3_ep}, {k_mhe_innov_4, k_mhe_innov_4_ep}};
// The gate kernels as dekf_set_innovation_gate selects them, in the same way
typedef void (*GateFn)(DevCfg, DevState, int, int, double*, InnovStore, GateStore);
typedef void (*GateEpochFn)(DevCfg, DevState, int, double*, InnovStore, GateStore, const int*, const DevCfg*);
struct GateKernel { GateFn fn; GateEpochFn fn_ep; };
const GateKernel gate_kernels[DEKF_MAX_LEGS] = {{k_mhe_innov_gate_1, k_mhe_innov_gate_1_ep}, {k_mhe_innov_gate_2, k_mhe_innov_gate_2_ep},
                                                {k_mhe_innov_gate_3, k_mhe_innov_gate_3_ep}, {k_mhe_innov_gate_4, k_mhe_innov_gate_4_ep}};
// Their _smooth twins as dekf_set_gate_smoother selects them: the gate kernels' arguments, then the window stores
typedef void (*GateSmoothFn)(DevCfg, DevState, int, int, double*, InnovStore, GateStore, DirectWindow);
typedef void (*GateSmoothEpochFn)(DevCfg, DevState, int, double*, InnovStore, GateStore, const int*, const DevCfg*, DirectWindow);
struct GateSmoothKernel { GateSmoothFn fn; GateSmoothEpochFn fn_ep; };
const GateSmoothKernel gate_smooth_kernels[DEKF_MAX_LEGS] = {{k_mhe_innov_gate_1_smooth, k_mhe_innov_gate_1_smooth_ep},
                                                             {k_mhe_innov_gate_2_smooth, k_mhe_innov_gate_2_smooth_ep},
                                                             {k_mhe_innov_gate_3_smooth, k_mhe_innov_gate_3_smooth_ep},
                                                             {k_mhe_innov_gate_4_smooth, k_mhe_innov_gate_4_smooth_ep}};

// the kernel of its row that a direct handle launches: the variant of the list with the handle's smoother and cross settings and the
// clock of its instance mode
DirectVariant direct_variant(const dekf_handle_s* h) {
    const Clock clock = instance_mode(h).clock;
    const bool cross = h->smoother && h->cross;  // (the cross-covariances are the smoother's)
    for (int v = 0; v < dv_count; ++v)
        if (direct_variants[v].smooth == h->smoother && direct_variants[v].cross == cross && direct_variants[v].clock == clock)
            return (DirectVariant)v;
    return dv_count;  // (not reached: the list has every clock with and without the smoother and its cross-covariances)
}

// The solve launch of a step with a window of K steps: what dekf_update launches, dekf_solve_kernel_name names and dekf_launch_info
// counts.  A function of fields the setters keep: no HIP call, nothing allocated.
struct SolveLaunch {
    const char* name;  // the kernel's symbol
    int grid, threads; size_t lds;
    SolveFn admm;           // the ADMM kernel; null on a direct handle, which launches ...
    DirectVariant variant;  // ... this kernel of its row (h->direct)
    // ... and behind it, on an innovation handle (dekf_set_innovation), the innovation kernel of its leg count (null: none): the epoch
    // twin where the direct kernel's clock is not WINDOW (there is no parameter twin).  One wavefront per instance, a grid of B,
    // lds_innov of LDS
    const InnovKernel* innov;
    size_t lds_innov;
    // ... or, on a gating handle (dekf_set_innovation_gate), the gate kernel of its leg count IN PLACE of the innovation kernel (null:
    // none; `innov` is then null): the same grid, lds_innov of LDS.  The epoch twin takes the parameter table, or null
    const GateKernel* gate;
    // ... or, on a gating handle that smooths (dekf_set_gate_smoother), that kernel's _smooth twin IN PLACE of it (null: none; `gate` is
    // then null): the same grid, lds_innov of LDS, which is then the larger size of the window correction
    const GateSmoothKernel* gate_smooth;
};
SolveLaunch solve_launch(const dekf_handle_s* h, int K) {
    if (h->solver == DEKF_SOLVER_DIRECT) {
        const DirectVariant v = direct_variant(h);
        const bool gate = h->innov && h->gate_st.nis_leg_max > 0.0;
        const bool gate_smooth = gate && h->smoother && h->gate_smoother;
        return {h->direct->name[v], h->c.B, 64, h->lds_direct, nullptr, v, h->innov && !gate ? &innov_kernels[h->c.L - 1] : nullptr,
                (size_t)(gate_smooth ? GateWindowScratch::len(h->c.L) : (gate ? GateScratch::len(h->c.L) : InnovScratch::len(h->c.L))) * sizeof(double),
                gate && !gate_smooth ? &gate_kernels[h->c.L - 1] : nullptr, gate_smooth ? &gate_smooth_kernels[h->c.L - 1] : nullptr};
    }
    const bool full = h->solve_entry_full && K == h->c.N;
    const SolveTwin t = solve_twin(full ? h->solve_entry_full : h->solve_entry, h->c.polish != 0, h->c.warm != 0);
    if (full) return {t.name, h->solve_grid_full, h->solve_threads_full, h->lds_solve_full, t.fn, dv_count, nullptr, 0, nullptr, nullptr};
    return {t.name, h->solve_grid, DEKF_SOLVE_THREADS, h->lds_solve, t.fn, dv_count, nullptr, 0, nullptr, nullptr};
}

// A family of full-window kernels (K == N): the shapes it covers are the rows of its role in solve_kernels.def
struct FullWindowFamily {
    SolveRole role;
    bool eligible;     // the caller's cap on workgroups per CU admits the family
    int threads;       // workgroup size
    size_t lds;        // dynamic LDS of one workgroup (SolveLayout::*_lds_bytes)
    bool (SolveLayout::*fits)(int, size_t) const;
    int max_per_cu;    // workgroups per CU the kernel is compiled for
    bool query;        // true: workgroups per CU from the occupancy query (clamped to max_per_cu and the cap), taken when that is more
                       // than the window-fill kernel's; false: max_per_cu, taken when the grid grows
    const char* ab_grid_env;    // DEKF_AB_KNOBS: another persistent grid
    const char* ab_round5_env;  // DEKF_AB_KNOBS: the round-5 rule, taken only when the grid grows too
};

// makes f the handle's full-window kernel if f's rule takes it (h->solve_grid: the window-fill kernel's grid, per_cu its residency)
bool take_full_window(dekf_handle h, const FullWindowFamily& f, const SolveLayout& lay, int per_cu, int cap, int cus, int batch) {
    const SolveKernel* k = f.eligible && !h->c.ft ? solve_kernel(f.role, h->c.L, h->c.N) : nullptr;
    if (!k) return false;
    const SolveFn fn = solve_twin(k, h->c.polish != 0, false).fn;
    // the kernel's static LDS (reduction scratch of wave.h) counts against the same allocation as the dynamic part
    hipFuncAttributes fa;
    size_t static_lds = 512;
    if (hipFuncGetAttributes(&fa, (const void*)fn) == hipSuccess) static_lds = fa.sharedSizeBytes;
    if (!(lay.*f.fits)(h->c.L, static_lds)) return false;
    if (f.lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.lds);
    int pcf = f.max_per_cu;
    if (f.query) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pcf, (const void*)fn, f.threads, f.lds) != hipSuccess || pcf < 1) pcf = 1;
        if (pcf > f.max_per_cu) pcf = f.max_per_cu;  // the query over-reports: the *_fits rule has decided that max_per_cu fit
        if (cap > 0 && pcf > cap) pcf = cap;
    }
    const long slots = (long)pcf * cus;
    int grid = (int)(slots < batch ? slots : batch);
#ifdef DEKF_AB_KNOBS  // A/B builds only (tools/r4_check.py)
    if (const char* ge = f.ab_grid_env ? getenv(f.ab_grid_env) : nullptr) { const int gv = atoi(ge); if (gv > 0 && gv <= batch) grid = gv; }
#endif
    bool take = f.query ? pcf > per_cu : grid > h->solve_grid;
#ifdef DEKF_AB_KNOBS
    if (f.ab_round5_env && getenv(f.ab_round5_env)) take = take && grid > h->solve_grid;
#endif
    if (!take) return false;
    h->solve_entry_full = k;
    if (k->warm_twin && f.lds > 64 * 1024)  // (the twin a warm handle launches: dekf_set_warm_start)
        (void)hipFuncSetAttribute((const void*)solve_twin(k, h->c.polish != 0, true).fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.lds);
    h->solve_grid_full = grid;
    h->solve_threads_full = f.threads;
    h->lds_solve_full = f.lds;
    return true;
}

dekf_status ensure_stage(dekf_handle h, size_t bytes) {
    if (bytes <= h->stage_bytes) return DEKF_OK;
    if (h->stage) HIPCHK(hipFree(h->stage));
    h->stage = nullptr;
    h->stage_bytes = 0;
    HIPCHK(hipMalloc(&h->stage, bytes));
    h->stage_bytes = bytes;
    return DEKF_OK;
}
// the host array *src -> the staging block at byte offset `at` (after ensure_stage), on the handle's stream; *src becomes its device address
template <class T> dekf_status stage_in(dekf_handle h, size_t at, const T** src, size_t count) {
    T* d = (T*)((char*)h->stage + at);
    HIPCHK(hipMemcpyAsync(d, *src, count * sizeof(T), hipMemcpyHostToDevice, h->stream));
    *src = d;
    return DEKF_OK;
}

// device memory that lives as long as the handle (dekf_destroy frees h->blocks)
template <class T> dekf_status dev_alloc(dekf_handle h, size_t bytes, T** out) {
    HIPCHK(hipMalloc((void**)out, bytes));
    h->blocks.push_back(*out);
    return DEKF_OK;
}

// dst (device) <- src (host or device), n bytes, on the handle's stream
dekf_status put(dekf_handle h, void* dst, const void* src, size_t n, dekf_mem where) {
    if (!src) return fail(DEKF_ERR_INVALID, "null input pointer");
    HIPCHK(hipMemcpyAsync(dst, src, n, where == DEKF_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, h->stream));
    return DEKF_OK;
}
dekf_status fetch(dekf_handle h, void* dst, const void* src, size_t n, dekf_mem where) {
    if (!dst) return DEKF_OK;
    HIPCHK(hipMemcpyAsync(dst, src, n, where == DEKF_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream));
    return DEKF_OK;
}
// the first `width` bytes of each of B rows `pitch` bytes apart, the pitch the same on both sides: the written entries of a window store.
// Full rows are one contiguous copy (hipMemcpy2DAsync with the width equal to the pitch may take another copy path: not measured)
dekf_status fetch_rows(dekf_handle h, void* dst, const void* src, size_t pitch, size_t width, size_t B, dekf_mem where) {
    if (!dst) return DEKF_OK;
    if (width == pitch) return fetch(h, dst, src, B * pitch, where);
    HIPCHK(hipMemcpy2DAsync(dst, pitch, src, pitch, width, B, where == DEKF_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream));
    return DEKF_OK;
}
// the end of a getter: what it copied to the host is there when it returns; device copies stay in stream order
dekf_status host_sync(dekf_handle h, dekf_mem where) {
    if (where == DEKF_HOST) HIPCHK(hipStreamSynchronize(h->stream));
    return DEKF_OK;
}

// up to four device-to-device latches of one push in ONE launch (separate hipMemcpyAsync calls each cost a
// ~5 us blit kernel: seven per step were 0.9 % of the step); host sources still go through hipMemcpyAsync
dekf_status put_many(dekf_handle h, int n, double* const* dst, const double* const* src, const size_t* count, dekf_mem where) {
    for (int i = 0; i < n; ++i) if (!src[i]) return fail(DEKF_ERR_INVALID, "null input pointer");
    if (where == DEKF_HOST) {
        for (int i = 0; i < n; ++i) HIPCHK(hipMemcpyAsync(dst[i], src[i], count[i] * sizeof(double), hipMemcpyHostToDevice, h->stream));
        return DEKF_OK;
    }
    LatchCopy4 a;
    size_t total = 0;
    for (int i = 0; i < 4; ++i) {
        a.dst[i] = i < n ? dst[i] : nullptr;
        a.src[i] = i < n ? src[i] : nullptr;
        total += i < n ? count[i] : 0;
        a.end[i] = total;
    }
    if (total == 0) return DEKF_OK;
    const int blocks = (int)((total + 255) / 256);
    k_latch4<<<blocks < 2048 ? blocks : 2048, 256, 0, h->stream>>>(a);
    HIPCHK(hipGetLastError());
    return DEKF_OK;
}

// the handle's stream waits (no host block) for the solve that produces the newest results; getters then read in stream order
dekf_status await_results(dekf_handle h) {
    if (h->pipelined && h->solve_pending[h->last_par]) HIPCHK(hipStreamWaitEvent(h->stream, h->ev_solve[h->last_par], 0));
    return DEKF_OK;
}

// the handle's stream waits for what a reset would race with: a solve in flight writes the outputs it clears, the early marginalisation
// the tags (k_reset_state clears them), and an all-gather's snapshot copy on the communication stream may still be reading v_b
dekf_status quiesce(dekf_handle h) {
    for (int i = 0; i < 2; ++i)
        if (h->solve_pending[i]) { HIPCHK(hipStreamWaitEvent(h->stream, h->ev_solve[i], 0)); h->solve_pending[i] = false; }
    if (h->early_pending) { HIPCHK(hipStreamWaitEvent(h->stream, h->ev_early_done, 0)); h->early_pending = false; }
    for (int i = 0; i < 2; ++i)
        if (h->vb_read_pending[i]) { HIPCHK(hipStreamWaitEvent(h->stream, h->ev_vb_read[i], 0)); h->vb_read_pending[i] = false; }
    return DEKF_OK;
}

struct Timed {  // brackets one launch with events when timing is on
    dekf_handle h;
    int cls;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st;
    Timed(dekf_handle h_, int cls_, hipStream_t st_ = nullptr) : h(h_), cls(cls_), st(st_ ? st_ : h_->stream) {
        if (!h->timing || (h->timing == 2 && cls != 2 && cls != 3)) return;  // (3: the all-gather, on the communication stream — off the step's critical path)
        if (!h->ev_pool.empty()) { a = h->ev_pool.back().first; b = h->ev_pool.back().second; h->ev_pool.pop_back(); }
        else if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
            if (a) (void)hipEventDestroy(a);
            a = b = nullptr;
            return;
        }
        (void)hipEventRecord(a, st);
    }
    ~Timed() {
        if (!a) return;
        (void)hipEventRecord(b, st);
        h->ev[cls].push_back({a, b});
    }
};

// where step T of an MHE handle runs (see the handle): the set of per-solve data, the copy of the input snapshot, the solve's stream
struct MheStep { int T, par, snap_set; DevState sp; hipStream_t ss; };
MheStep mhe_step(dekf_handle h, int T) {
    const int par = h->pipelined ? (T & 1) : 0, snap_set = h->pipelined ? T % DEKF_SNAP_SETS : 0;
    MheStep st = {T, par, snap_set, h->sp[par], h->pipelined ? h->solve_stream[par] : h->stream};
    // The assemble writes the solve's input snapshot.  With two copies it had to wait for the solve of step T - 2, and by
    // then step T - 1's 768 persistent workgroups hold every slot of the machine: the assemble crawled in (0.41 instead of
    // 0.07 ms) as they left, and the solve of step T started that much late — the pipeline ran on its dependencies, not on
    // the machine (profiles/r05_step_pipelining_timeline.txt).  With three copies it waits for step T - 3, which is long
    // over: the small kernels of a step run while the step before the previous one drains, and the solve of step T is
    // ready the moment a slot frees.  (Outputs and scratch slabs stay at two sets: solves on one stream are in order.)
    if (h->pipelined) st.sp.snap = h->s.snap + (size_t)st.snap_set * h->c.snap_len * h->c.B;
    return st;
}

// What a handle launches: one function per launch, which picks the twin of the handle's instance mode; the caller checks
// hipGetLastError.  Where the kernels are asymmetric the functions are: no *_act marginalise or solve kernel (the epoch and parameter
// twins do nothing for a paused instance), no *_pp innovation, latch or fold kernel (those read no noise constants).
// ... the launch that solve_launch describes, on stream ss
void launch_solve(dekf_handle h, const SolveLaunch& l, const DevState& sp, int T, int kstart, int K, hipStream_t ss) {
    if (l.admm) return (void)l.admm<<<l.grid, l.threads, l.lds, ss>>>(h->c, sp, kstart, K, h->gws_len);
    const DirectKernel& d = *h->direct;
    // the arguments of a variant, in the order of DEKF_DIRECT_PARAMS: the clock's head, cov, [win], [cross], the clock's tail
#define DEKF_DIRECT_HEADARG_WINDOW h->c, sp, kstart, K
#define DEKF_DIRECT_TAILARG_WINDOW
#define DEKF_DIRECT_HEADARG_EPOCH h->c, sp, T
#define DEKF_DIRECT_TAILARG_EPOCH , h->inst.t0
#define DEKF_DIRECT_HEADARG_PARAM sp, T
#define DEKF_DIRECT_TAILARG_PARAM , h->inst.t0, h->inst.pp_mhe
#define DEKF_DIRECT_LAUNCH_(SUFFIX, SMOOTH, CROSS, CLOCK, ...)                                                         \
    case dv##SUFFIX:                                                                                                   \
        d.fn##SUFFIX<<<l.grid, l.threads, l.lds, ss>>>(DEKF_DIRECT_HEADARG_##CLOCK, h->mhe_cov DEKF_DIRECT_IF_##SMOOTH(, h->win) \
                                                       DEKF_DIRECT_IF_##CROSS(, h->cross_st) DEKF_DIRECT_TAILARG_##CLOCK); \
        break;
    switch (l.variant) {
    DEKF_DIRECT_VARIANTS(DEKF_DIRECT_LAUNCH_)
    case dv_count: break;
    }
    if (l.gate) {  // (a gating handle: the statistics, then the gate on them, in one launch)
        if (direct_variants[l.variant].clock == Clock::WINDOW)
            l.gate->fn<<<l.grid, 64, l.lds_innov, ss>>>(h->c, sp, kstart, K, h->mhe_cov, h->innov_st, h->gate_st);
        else
            l.gate->fn_ep<<<l.grid, 64, l.lds_innov, ss>>>(h->c, sp, T, h->mhe_cov, h->innov_st, h->gate_st, h->inst.t0,
                                                           direct_variants[l.variant].clock == Clock::PARAM ? h->inst.pp_mhe : nullptr);
        return;
    }
    if (l.gate_smooth) {  // (a gating handle that smooths: the same launch, with the correction of the window the solve just left)
        if (direct_variants[l.variant].clock == Clock::WINDOW)
            l.gate_smooth->fn<<<l.grid, 64, l.lds_innov, ss>>>(h->c, sp, kstart, K, h->mhe_cov, h->innov_st, h->gate_st, h->win);
        else
            l.gate_smooth->fn_ep<<<l.grid, 64, l.lds_innov, ss>>>(h->c, sp, T, h->mhe_cov, h->innov_st, h->gate_st, h->inst.t0,
                                                                  direct_variants[l.variant].clock == Clock::PARAM ? h->inst.pp_mhe : nullptr, h->win);
        return;
    }
    if (!l.innov) return;
    // (an innovation handle: the statistics of the newest step from what the solve just left, in stream order behind it)
    if (direct_variants[l.variant].clock == Clock::WINDOW) l.innov->fn<<<l.grid, 64, l.lds_innov, ss>>>(h->c, sp, kstart, K, h->mhe_cov, h->innov_st);
    else l.innov->fn_ep<<<l.grid, 64, l.lds_innov, ss>>>(h->c, sp, T, h->mhe_cov, h->innov_st, h->inst.t0);
}
// ... the EKF tick (dekf_ekf_step)
void launch_tick(dekf_handle h) {
    const InstanceMode m = instance_mode(h);
    const int grid = (h->c.B + 63) / 64;
    if (m.clock == Clock::WINDOW) k_ekf_tick<<<grid, 64, 0, h->stream>>>(h->c, h->s, h->ekf_count);
    else if (m.clock == Clock::EPOCH && !m.paused) k_ekf_tick_ep<<<grid, 64, 0, h->stream>>>(h->c, h->s, h->ekf_count, h->inst.c0);
    else if (m.clock == Clock::EPOCH) k_ekf_tick_act<<<grid, 64, 0, h->stream>>>(h->c, h->s, h->ekf_count, h->inst.c0);
    else if (!m.paused) k_ekf_tick_pp<<<grid, 64, 0, h->stream>>>(h->c, h->s, h->ekf_count, h->inst.c0, h->inst.pp_ekf);
    else k_ekf_tick_act_pp<<<grid, 64, 0, h->stream>>>(h->c, h->s, h->ekf_count, h->inst.c0, h->inst.pp_ekf);
}
// ... the terms of step T into sp (dekf_initialize of a handle with a table: T = 0, pushes = 0, the initialise path on every instance's own prior)
void launch_assemble(dekf_handle h, const DevState& sp, int T, int pushes) {
    const InstanceMode m = instance_mode(h);
    if (m.clock == Clock::WINDOW) k_mhe_assemble<<<h->c.B, 64, h->lds_asm, h->stream>>>(h->c, sp, T, pushes);
    else if (m.clock == Clock::EPOCH && !m.paused) k_mhe_assemble_ep<<<h->c.B, 64, h->lds_asm, h->stream>>>(h->c, sp, T, pushes, h->inst.t0);
    else if (m.clock == Clock::EPOCH) k_mhe_assemble_act<<<h->c.B, 64, h->lds_asm, h->stream>>>(h->c, sp, T, pushes, h->inst.t0);
    else if (!m.paused) k_mhe_assemble_pp<<<h->c.B, 64, h->lds_asm, h->stream>>>(sp, T, pushes, h->inst.t0, h->inst.pp_mhe);
    else k_mhe_assemble_act_pp<<<h->c.B, 64, h->lds_asm, h->stream>>>(sp, T, pushes, h->inst.t0, h->inst.pp_mhe);
}
// ... the arrival cost of step T ahead of time, on the early stream (marginalize_next_early)
void launch_marginalize_early(dekf_handle h, int T) {
    switch (instance_mode(h).clock) {
    case Clock::WINDOW: k_mhe_marginalize_early<<<h->c.B, 64, h->lds_asm, h->early_stream>>>(h->c, h->s, T); break;
    case Clock::EPOCH: k_mhe_marginalize_early_ep<<<h->c.B, 64, h->lds_asm, h->early_stream>>>(h->c, h->s, T, h->inst.t0); break;
    case Clock::PARAM: k_mhe_marginalize_early_pp<<<h->c.B, 64, h->lds_asm, h->early_stream>>>(h->s, T, h->inst.t0, h->inst.pp_mhe); break;
    }
}
// ... the VO latch (dekf_push_vo; device pointers): a sample for a paused instance is dropped
void launch_latch_vo(dekf_handle h, const int* mask, const double* t_pre, const double* t_now, const double* dp, const double* t_pose,
                     const double* q_vo) {
    const int grid = (h->c.B + 255) / 256;
    if (instance_mode(h).paused) k_latch_vo_act<<<grid, 256, 0, h->stream>>>(h->c, h->s, mask, h->inst.t0, t_pre, t_now, dp, t_pose, q_vo);
    else k_latch_vo<<<grid, 256, 0, h->stream>>>(h->c, h->s, mask, t_pre, t_now, dp, t_pose, q_vo);
}
// ... the fold of the device's epochs with the host's EKF tick count (dekf_ekf_step): the sentinel of a paused instance stays
void launch_fold(dekf_handle h, int count_old, int count_new) {
    const int grid = (h->c.B + 255) / 256;
    if (instance_mode(h).paused) k_fold_epochs_act<<<grid, 256, 0, h->stream>>>(h->inst.c0, h->c.B, count_old, count_new, h->c.ekf_hist);
    else k_fold_epochs<<<grid, 256, 0, h->stream>>>(h->inst.c0, h->c.B, count_old, count_new, h->c.ekf_hist);
}
// ... the initial state of every instance of set sp (dekf_reset): with a table every instance's own, and the table survives
void launch_reset_state(dekf_handle h, const DevState& sp) {
    const int grid = (h->c.B + 255) / 256;
    if (instance_mode(h).clock == Clock::PARAM) k_reset_state_pp<<<grid, 256, 0, h->stream>>>(h->c, sp, h->inst.pp_ekf);
    else k_reset_state<<<grid, 256, 0, h->stream>>>(h->c, sp);
}
// ... the restart of the instances of a device mask: with a table every instance's own initial EKF state; the innovation stores' entries NaN, as cov
void launch_reset_instances(dekf_handle h, const int* dmask) {
    const int grid = (h->c.B + 255) / 256;
    if (instance_mode(h).clock == Clock::PARAM)
        k_reset_instances_pp<<<grid, 256, 0, h->stream>>>(h->c, h->s, dmask, h->mhe_cov, h->inst.t0, h->inst.c0, h->next_T, h->ekf_count, h->inst.pp_ekf);
    else k_reset_instances<<<grid, 256, 0, h->stream>>>(h->c, h->s, dmask, h->mhe_cov, h->inst.t0, h->inst.c0, h->next_T, h->ekf_count);
    if (h->innov_st.nu) k_innov_nan<<<grid, 256, 0, h->stream>>>(h->c, dmask, h->innov_st);
}

// *steps of the window getters on a handle with epochs, behind the update of step T: the largest window of the batch, which is that of
// the instance restarted (or loaded with the oldest record) longest ago, none at its local step 0, or of a paused one where it stands
int epoch_window_steps(const dekf_handle_s* h, int T) {
    const int Ta = T - h->inst.min_t0;
    const int Tl = Ta > h->inst.max_frozen ? Ta : h->inst.max_frozen;
    return Tl < 1 ? 0 : (Tl + 1 < h->c.N ? Tl + 1 : h->c.N);
}

// the terms of step T: waits for the snapshot copy to be free and for the arrival cost computed ahead, then the assemble
dekf_status assemble_step(dekf_handle h, const MheStep& st) {
    if (h->pipelined && h->snap_busy[st.snap_set]) HIPCHK(hipStreamWaitEvent(h->stream, h->ev_snap_free[st.snap_set], 0));
    if (h->early_pending) { HIPCHK(hipStreamWaitEvent(h->stream, h->ev_early_done, 0)); h->early_pending = false; }
    { Timed t(h, 1); launch_assemble(h, st.sp, st.T, h->pushes); }
    HIPCHK(hipGetLastError());
    if (h->early_stream) HIPCHK(hipEventRecord(h->ev_asm_done, h->stream));
    return DEKF_OK;
}

// the solve of step T behind its terms, and what the getters need to know about it
dekf_status solve_step(dekf_handle h, const MheStep& st) {
    const int T = st.T, par = st.par;
    const hipStream_t ss = st.ss;
    if (h->pipelined) {
        HIPCHK(hipEventRecord(h->ev_asm[par], h->stream));
        HIPCHK(hipStreamWaitEvent(ss, h->ev_asm[par], 0));
        // the all-gather of step T - 2 read THIS set's v_b until its snapshot copy was through (dekf_allgather_vb)
        if (h->vb_read_pending[par]) { HIPCHK(hipStreamWaitEvent(ss, h->ev_vb_read[par], 0)); h->vb_read_pending[par] = false; }
        // A recorded event between the stream-waits and the launch: measured, not understood.  Without it the solve of step
        // T + 1 does not start under the last round of step T's solve and the mode gains nothing (2.09 M steps/s, Go1 at 4096);
        // with it the two overlap (2.16 M).  Found because bench.py's timing events had the same effect; an event recorded only
        // AFTER the launch does not (profiles/r05_step_pipelining_queues.txt).
        HIPCHK(hipEventRecord(h->ev_mark[par], ss));
    }
    const int kstart = T - h->c.N + 1 > 0 ? T - h->c.N + 1 : 0;
    const int K = T - kstart + 1;
    {
        Timed t(h, 2, ss);
#ifdef DEKF_AB_KNOBS  // A/B builds only: a quiet gap (an empty kernel) between the term construction and the solve launch
        { static const int gap = getenv("DEKF_DEBUG_GAP_KERNEL") ? atoi(getenv("DEKF_DEBUG_GAP_KERNEL")) : 0;
          for (int i = 0; i < gap; ++i) k_gap<<<1, 64, 0, ss>>>(); }
#endif
        launch_solve(h, solve_launch(h, K), st.sp, T, kstart, K, ss);  // (with the innovation kernel of an innovation handle: one launch of class 2)
    }
    if (h->pipelined) {
        HIPCHK(hipEventRecord(h->ev_solve[par], ss));
        h->solve_pending[par] = true;
        HIPCHK(hipEventRecord(h->ev_snap_free[st.snap_set], ss));
        h->snap_busy[st.snap_set] = true;
    }
    h->last_par = par;
    h->mhe_cov_valid = h->solver == DEKF_SOLVER_DIRECT;
    h->innov_valid = h->innov;
    h->win_steps = h->smoother ? K : 0;
    if (instance_mode(h).restarted && h->smoother) h->win_steps = epoch_window_steps(h, T);
    return DEKF_OK;
}

// in-order mode: the arrival cost of step T + 1 on early_stream, behind the assemble of step T (the arrival cost and the records as it
// left them), beside its solve
dekf_status marginalize_next_early(dekf_handle h, int T) {
    HIPCHK(hipStreamWaitEvent(h->early_stream, h->ev_asm_done, 0));
    HIPCHK(hipEventRecord(h->ev_early_mark, h->early_stream));  // (as before a pipelined solve launch: see there)
    launch_marginalize_early(h, T + 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev_early_done, h->early_stream));
    h->early_pending = true;
    return DEKF_OK;
}

// The per-instance entry points' common ground: fn needs an in-order direct MHE handle, and with need_init an initialised one; fn's
// [B] mask (read_mask); [B] ints to the caller's host or device memory (deliver_ints)
dekf_status need_direct(dekf_handle h, const char* fn, bool need_init) {
    const std::string f(fn);
    if (h->c.est_type != 0) return fail(DEKF_ERR_INVALID, (f + " needs a direct MHE handle: this is a KF handle (est_type 1)").c_str());
    if (h->pipelined) return fail(DEKF_ERR_INVALID, (f + " cannot be combined with solve_pipeline = 1").c_str());
    if (h->solver != DEKF_SOLVER_DIRECT) return fail(DEKF_ERR_INVALID, (f + " needs a direct handle (dekf_set_solver(h, DEKF_SOLVER_DIRECT))").c_str());
    if (need_init && !h->initialized) return fail(DEKF_ERR_ORDER, (f + " before dekf_initialize").c_str());
    return DEKF_OK;
}
// (the host reads the mask: it refuses values other than 0 and 1 and keeps the books.  A device mask costs a copy and a wait here;
// restarts and pauses are rare, and the call between two ticks is not on the hot path)
dekf_status read_mask(dekf_handle h, const char* fn, const int* mask, dekf_mem where, std::vector<int>& m) {
    const size_t B = (size_t)h->c.B;
    m.resize(B);
    if (where == DEKF_HOST) std::memcpy(m.data(), mask, B * sizeof(int));
    else {
        HIPCHK(hipMemcpyAsync(m.data(), mask, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    for (size_t b = 0; b < B; ++b)
        if (m[b] != 0 && m[b] != 1) return fail(DEKF_ERR_INVALID, (std::string(fn) + ": mask entries must be 0 or 1").c_str());
    return DEKF_OK;
}
dekf_status deliver_ints(dekf_handle h, int* dst, const std::vector<int>& v, dekf_mem where) {
    if (where == DEKF_HOST) std::memcpy(dst, v.data(), v.size() * sizeof(int));
    else {
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipMemcpyAsync(dst, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));  // (v is the caller's local)
    }
    return DEKF_OK;
}

}  // namespace

// the epoch arrays of a direct handle (t0 | c0 in one block, all 0), allocated by the first call that needs them
dekf_status dekf_handle_s::Instances::ensure(dekf_handle h) {
    if (t0) return DEKF_OK;
    const size_t B = (size_t)h->c.B;
    TRY(dev_alloc(h, 2 * B * sizeof(int), &t0));
    c0 = t0 + B;
    pz_step.assign(B, 0);
    pz_count.assign(B, 0);
    return clear(h);
}

// what the window getters' steps take from the epochs: the smallest one of the active instances, the largest frozen local step
void dekf_handle_s::Instances::bounds() {
    min_t0 = DEKF_EPOCH_PAUSED;
    max_frozen = -1;
    for (size_t b = 0; b < t0_host.size(); ++b) {
        if (act_host[b]) { if (t0_host[b] < min_t0) min_t0 = t0_host[b]; }
        else if (pz_step[b] - 1 > max_frozen) max_frozen = pz_step[b] - 1;
    }
}

// every epoch 0 and nobody paused: the handle launches the kernels of a handle that never restarted an instance again
dekf_status dekf_handle_s::Instances::clear(dekf_handle h) {
    if (!t0) return DEKF_OK;
    const size_t B = (size_t)h->c.B;
    HIPCHK(hipMemsetAsync(t0, 0, 2 * B * sizeof(int), h->stream));
    t0_host.assign(B, 0);
    c0_host.assign(B, 0);
    act_host.assign(B, 1);
    min_t0 = 0;
    max_frozen = -1;
    restarted = paused = false;
    return DEKF_OK;
}

extern "C" {

void dekf_default_params(dekf_params* p) { default_params(p); }
int dekf_abi_version(void) { return DEKF_ABI_VERSION; }
int dekf_hip_runtime_version(void) {
    int v = 0;
    return hipRuntimeGetVersion(&v) == hipSuccess ? v : 0;
}
const char* dekf_last_error(void) { return g_err.c_str(); }

dekf_status dekf_create(const dekf_params* p, int batch, int device, void* stream, dekf_handle* out) {
    if (!p || !out) return fail(DEKF_ERR_INVALID, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(DEKF_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
    if (device < 0 || device >= ndev) return fail(DEKF_ERR_INVALID, "device ordinal out of range");
    DevCfg c;
    if (const char* msg = fill_cfg(*p, batch, c)) return fail(DEKF_ERR_INVALID, msg);
#ifdef DEKF_NO_POLISH_KERNELS
    if (c.polish && c.est_type == 0) return fail(DEKF_ERR_INVALID, "this diagnostic build (-DDEKF_NO_POLISH_KERNELS) carries no polishing kernels");
#endif
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_err = std::string("device is ") + prop.gcnArchName + ", this build targets gfx950 only";
        return DEKF_ERR_NO_DEVICE;
    }
    dekf_handle h = new dekf_handle_s();
    h->prm = *p;
    h->c = c;
    h->device = device;
    if (stream) h->stream = (hipStream_t)stream;
    else {
        if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
            h->stream = nullptr;
            dekf_destroy(h);
            return fail(DEKF_ERR_HIP, "hipStreamCreate failed");
        }
        h->own_stream = true;
    }
    SolveLayout lay;
    lay.init(c.N, c.L, c.ft);
    h->lds_solve = lay.lds_bytes();
    h->c.gws_wt = !c.ft && !lay.factor_in_lds();  // the factor streams from the slab: the outward legs read a transposed copy of W (Gws::WT)
#ifdef DEKF_PROFILE
    // diagnostic build only: DEKF_DEBUG_LDS_PAD=<bytes> inflates the request (e.g. to force one workgroup per CU)
    if (const char* pad = getenv("DEKF_DEBUG_LDS_PAD")) h->lds_solve += (size_t)atol(pad);
#endif
    // the placement of the factor (SolveLayout), or the foot-position states' own family (two rows per block in the solve)
    const SolveRole role = c.ft ? (lay.factor_in_lds() ? SolveRole::foot_lg : SolveRole::foot_gg)
                                : (lay.pa_in_lds() ? SolveRole::ll : (lay.factor_in_lds() ? SolveRole::lg : SolveRole::gg));
    h->solve_entry = solve_kernel(role, c.L, c.N);
#ifdef DEKF_PROFILE
    // diagnostic build only: DEKF_DEBUG_PLACEMENT=1|2 forces the _lg / _gg placement (2 also shrinks the LDS request)
    if (const char* pl = getenv("DEKF_DEBUG_PLACEMENT")) {
        int p = atoi(pl);
        if ((p == 1 || p == 2) && !c.ft) h->solve_entry = solve_kernel(p == 1 ? SolveRole::lg : SolveRole::gg, c.L, 0);
        // the _gg kernels carve D, E, bounds and R behind the iterates when SolveLayout::gg_consts_in_lds() says so
        if (p == 2) h->lds_solve = (size_t)(lay.vec + (lay.gg_consts_in_lds() ? lay.gg_consts() : 0)) * sizeof(double);
        if (p == 2) h->c.gws_wt = !c.ft;
    }
#endif
    h->lds_asm = (size_t)AsmScratch::len(c.L, c.ft) * sizeof(double);
    h->lds_kf = (size_t)KfScratch::len(c.L, c.ft) * sizeof(double);
    if (h->lds_solve > 160 * 1024) {
        dekf_destroy(h);
        return fail(DEKF_ERR_INVALID, "window too large: ADMM iterates exceed the 160 KiB LDS of one CU");
    }
    // (the rows of the window-fill kernels have no warm twin: this is the kernel a warm handle launches too)
    const SolveFn fill = solve_twin(h->solve_entry, c.polish != 0, false).fn;
    if (h->lds_solve > 64 * 1024) (void)hipFuncSetAttribute((const void*)fill, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_solve);
    int per_cu = 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)fill, DEKF_SOLVE_THREADS, h->lds_solve) != hipSuccess || per_cu < 1)
        per_cu = 1;
    const int cap = p->solve_workgroups_per_cu;  // 0: no cap
    if (cap > 0 && per_cu > cap) per_cu = cap;
    long slots = (long)per_cu * prop.multiProcessorCount;
    h->solve_grid = (int)(slots < batch ? slots : batch);
    // Full windows (K == N) of some shapes run kernels of their own with more workgroups per CU: the first family whose rule takes it.
    // Go1 / Cassie (N = 20): r3 for EVERY batch since round 6 (it used to be only where the batch fills more slots than the
    // two-workgroup kernel offers, "below that the row state would travel through the slab for no residency gained"): measured, the
    // rows-in-registers kernel solves a full window in 0.278 ms against 0.350 ms even ALONE on its CU — 21-22 % less solve time at
    // 64 ... 512 instances (profiles/r06_r3_at_small_batches.txt).  The two-workgroup kernels keep the window-fill ticks, and full
    // windows when the caller caps the residency at two; solve_workgroups_per_cu = 4 selects r4.
    // One-legged robots with long windows (PogoX: N = 100): the generic placement keeps 103 KB of iterates in LDS, one workgroup per
    // CU; rr keeps the row state in registers (mhe_admm_core.h: admm_chunk_rr) — 77 KB, two per CU — for every batch since round 6
    // (10-13 % less solve time than the generic kernel at 32 ... 256 instances too, profiles/r06_r3_at_small_batches.txt).
    const bool above_cap = cap == 0 || cap > per_cu;
    const FullWindowFamily families[] = {
        // four workgroups of three wavefronts per CU (round 6, admm_chunk_r4).  ADVICE (its own change): query the occupancy, LDS from prop
        {SolveRole::r4, cap == 4, DEKF_R4_THREADS, lay.r4_lds_bytes(), &SolveLayout::r4_fits, 4, false, "DEKF_DEBUG_R4_GRID", nullptr},
        {SolveRole::r3, above_cap, DEKF_SOLVE_THREADS, lay.r3_lds_bytes(), &SolveLayout::r3_fits, DEKF_R3_WAVES, true, nullptr, "DEKF_DEBUG_R3_ONLY_ABOVE_512"},
        {SolveRole::rr, above_cap, DEKF_SOLVE_THREADS, lay.rr_lds_bytes(), &SolveLayout::rr_fits, 2, true, nullptr, "DEKF_DEBUG_RR_ONLY_ABOVE_256"},
    };
    for (const FullWindowFamily& f : families)
        if (take_full_window(h, f, lay, per_cu, cap, prop.multiProcessorCount, batch)) break;
    const int solve_slots = h->solve_entry_full && h->solve_grid_full > h->solve_grid ? h->solve_grid_full : h->solve_grid;
    Gws g;
    g.init(c.N, c.L, c.ft, h->c.gws_wt);
    h->gws_len = g.total;
    h->pipelined = c.est_type == 0 && p->solve_pipeline == 1;
    bool ok = true;
    alloc_state(h->c, h->s, solve_slots, [&](size_t bytes) -> void* {
        void* q = nullptr;
        if (!ok) return nullptr;
        if (dev_alloc(h, bytes ? bytes : 8, &q) != DEKF_OK) { ok = false; return nullptr; }
        if (hipMemsetAsync(q, 0, bytes ? bytes : 8, h->stream) != hipSuccess) ok = false;
        return q;
    }, h->pipelined ? 2 : 1);
    if (!ok) {
        dekf_destroy(h);
        return fail(DEKF_ERR_HIP, "hipMalloc failed while allocating the estimator state");
    }
    h->sp[0] = h->s;
    h->sp[1] = h->pipelined ? second_set(h->c, h->s, solve_slots) : h->s;
    state_map(h->c, h->s, h->snap_map);
    int prio_least = 0, prio_greatest = 0;  // (of the streams the two modes create below)
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    // (N = 1: the record folded at step T gets its gains AT step T.  DEKF_DEBUG_NO_EARLY_MARGINALIZE in the environment: diagnostic switch,
    // everything on the handle's stream as before round 5 — same bits either way, tests/test_gpu_configs.py)
    if (!h->pipelined && c.est_type == 0 && c.N >= 2 && !getenv("DEKF_DEBUG_NO_EARLY_MARGINALIZE")) {
        // least priority: background work that is to take the slots the solve leaves, not to compete for them when both are ready
        // (and a priority class of its own: never on a hardware queue with the caller's streams — see the solve streams below)
        if (hipStreamCreateWithPriority(&h->early_stream, hipStreamNonBlocking, prio_least) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_asm_done, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_early_done, hipEventDisableTiming) != hipSuccess ||
            hipEventCreate(&h->ev_early_mark) != hipSuccess) {
            dekf_destroy(h);
            return fail(DEKF_ERR_HIP, "could not create the stream of the early marginalisation");
        }
    }
    if (h->pipelined) {
        // The two solve streams are created at the greatest stream priority: HIP maps streams round-robin onto a few hardware queues
        // PER PRIORITY CLASS (GPU_MAX_HW_QUEUES, default 4), and a stream-wait is a barrier packet that holds its whole queue — with
        // one more normal-priority stream alive in the process (another handle, idle) a solve stream shared a queue with the handle's
        // own stream and the mode ran at 1.34 M instead of 2.1 M steps/s (profiles/r05_step_pipelining_queues.txt).  In their own
        // class they share queues with nothing the caller creates by default.
        for (int i = 0; i < 2 && ok; ++i) {
            ok = hipStreamCreateWithPriority(&h->solve_stream[i], hipStreamNonBlocking, prio_greatest) == hipSuccess &&
                 hipEventCreateWithFlags(&h->ev_asm[i], hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&h->ev_solve[i], hipEventDisableTiming) == hipSuccess &&
                 hipEventCreate(&h->ev_mark[i]) == hipSuccess;
        }
        for (int i = 0; i < DEKF_SNAP_SETS && ok; ++i) ok = hipEventCreateWithFlags(&h->ev_snap_free[i], hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            dekf_destroy(h);
            return fail(DEKF_ERR_HIP, "could not create the solve streams");
        }
    }
    // the handle is published only once it is usable: a caller that checks the status alone leaks nothing
    const dekf_status st = dekf_reset(h);
    if (st != DEKF_OK) {
        const std::string keep = g_err;
        dekf_destroy(h);
        g_err = keep;
        return st;
    }
    *out = h;
    return DEKF_OK;
}

dekf_status dekf_destroy(dekf_handle h) {
    if (!h) return DEKF_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (int i = 0; i < 2; ++i) {
        if (h->solve_stream[i]) { (void)hipStreamSynchronize(h->solve_stream[i]); (void)hipStreamDestroy(h->solve_stream[i]); }
        if (h->ev_asm[i]) (void)hipEventDestroy(h->ev_asm[i]);
        if (h->ev_solve[i]) (void)hipEventDestroy(h->ev_solve[i]);
        if (h->ev_mark[i]) (void)hipEventDestroy(h->ev_mark[i]);
    }
    for (int i = 0; i < DEKF_SNAP_SETS; ++i) if (h->ev_snap_free[i]) (void)hipEventDestroy(h->ev_snap_free[i]);
    if (h->early_stream) { (void)hipStreamSynchronize(h->early_stream); (void)hipStreamDestroy(h->early_stream); }
    if (h->ev_asm_done) (void)hipEventDestroy(h->ev_asm_done);
    if (h->ev_early_done) (void)hipEventDestroy(h->ev_early_done);
    if (h->ev_early_mark) (void)hipEventDestroy(h->ev_early_mark);
    if (h->comm_stream) (void)hipStreamSynchronize(h->comm_stream);
    if (h->comm) rccl_destroy(h->comm);
    if (h->ev_vb_ready) (void)hipEventDestroy(h->ev_vb_ready);
    if (h->ev_ag_done) (void)hipEventDestroy(h->ev_ag_done);
    for (int i = 0; i < 2; ++i) if (h->ev_vb_read[i]) (void)hipEventDestroy(h->ev_vb_read[i]);
    if (h->comm_stream) (void)hipStreamDestroy(h->comm_stream);
    if (h->vb_snapshot) (void)hipFree(h->vb_snapshot);
    for (auto& v : h->ev) for (auto& pr : v) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto& pr : h->ev_pool) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (void* q : h->blocks) (void)hipFree(q);
    if (h->stage) (void)hipFree(h->stage);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return DEKF_OK;
}

dekf_status dekf_reset(dekf_handle h) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    HIPCHK(hipSetDevice(h->device));
    TRY(quiesce(h));
    for (int i = 0; i < DEKF_SNAP_SETS; ++i) h->snap_busy[i] = false;  // (every solve is behind the events just waited for)
    for (int i = 0; i < (h->pipelined ? 2 : 1); ++i) {
        launch_reset_state(h, h->sp[i]);
        HIPCHK(hipGetLastError());
    }
    h->last_par = h->ekf_count = h->pushes = h->next_T = 0;
    h->initialized = false;
    h->mhe_cov_valid = false;  // (the solver, smoother, cross and innovation settings survive)
    h->innov_valid = false;
    if (h->innov_st.nu)  // every entry NaN again (all bits set is one): an instance keeps it until its first solve
        HIPCHK(hipMemsetAsync(h->innov_st.nu, 0xff, (size_t)h->c.B * InnovStore::len(h->c.L) * sizeof(double), h->stream));
    if (h->gate_st.gated) HIPCHK(hipMemsetAsync(h->gate_st.gated, 0, (size_t)h->c.B * h->c.L * sizeof(int), h->stream));  // (the bound survives)
    h->win_steps = 0;
    TRY(h->inst.clear(h));
    return DEKF_OK;
}

dekf_status dekf_reset_instances(dekf_handle h, const int* mask, dekf_mem where) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (!mask) return fail(DEKF_ERR_INVALID, "null mask");
    TRY(need_direct(h, "dekf_reset_instances", true));
    HIPCHK(hipSetDevice(h->device));
    const size_t B = (size_t)h->c.B;
    dekf_handle_s::Instances& in = h->inst;
    std::vector<int> m;
    TRY(read_mask(h, "dekf_reset_instances", mask, where, m));
    bool any = false;
    for (size_t b = 0; b < B; ++b) any = any || m[b] == 1;
    if (!any) return DEKF_OK;  // nothing changes, the kernels the handle launches included
    TRY(quiesce(h));  // (what dekf_reset waits for)
    TRY(in.ensure(h));
    const int* dmask = where == DEKF_HOST ? m.data() : mask;
    if (where == DEKF_HOST) {
        TRY(ensure_stage(h, B * sizeof(int)));
        TRY(stage_in(h, 0, &dmask, B));
    }
    launch_reset_instances(h, dmask);
    HIPCHK(hipGetLastError());
    if (h->gate_st.gated)  // the restarted instances have gated nothing: their entries 0, one fill per run of them
        for (size_t b = 0; b < B;) {
            size_t e = b;
            while (e < B && m[e] == 1) ++e;
            if (e > b) HIPCHK(hipMemsetAsync(h->gate_st.gated + b * h->c.L, 0, (e - b) * h->c.L * sizeof(int), h->stream));
            b = e > b ? e : b + 1;
        }
    if (where == DEKF_HOST) HIPCHK(hipStreamSynchronize(h->stream));  // (m, a local, is the source of the copy)
    for (size_t b = 0; b < B; ++b)  // (a paused instance that is restarted is active: its new life starts here)
        if (m[b]) restart_instance((int)b, in.act_host.data(), in.t0_host.data(), in.c0_host.data(), h->next_T, h->ekf_count);
    in.bounds();
    in.restarted = true;
    return DEKF_OK;
}

dekf_status dekf_get_instance_ticks(dekf_handle h, int* ticks, dekf_mem where) {
    if (!h || !ticks) return fail(DEKF_ERR_INVALID, "null argument");
    if (!h->initialized) return fail(DEKF_ERR_ORDER, "dekf_get_instance_ticks before dekf_initialize");
    const dekf_handle_s::Instances& in = h->inst;
    const int T = h->next_T - 1;  // the step of the last update (0: dekf_initialize)
    std::vector<int> t((size_t)h->c.B, T);
    if (instance_mode(h).restarted)
        for (size_t b = 0; b < t.size(); ++b) t[b] = instance_tick((int)b, T, in.act_host.data(), in.pz_step.data(), in.t0_host.data());
    return deliver_ints(h, ticks, t, where);
}

dekf_status dekf_set_active(dekf_handle h, const int* active, dekf_mem where) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (!active) return fail(DEKF_ERR_INVALID, "null mask");
    TRY(need_direct(h, "dekf_set_active", true));
    HIPCHK(hipSetDevice(h->device));
    const size_t B = (size_t)h->c.B;
    dekf_handle_s::Instances& in = h->inst;
    std::vector<int> m;
    TRY(read_mask(h, "dekf_set_active", active, where, m));
    bool change = false;
    for (size_t b = 0; b < B; ++b) change = change || m[b] != (in.t0 ? in.act_host[b] : 1);
    if (!change) return DEKF_OK;  // the mask the handle has: nothing changes, the kernels it launches included
    TRY(quiesce(h));  // (what dekf_reset_instances waits for: the arrival cost computed ahead reads the epochs)
    TRY(in.ensure(h));
    for (size_t b = 0; b < B; ++b)
        set_active_instance((int)b, m[b], in.act_host.data(), in.pz_step.data(), in.pz_count.data(), in.t0_host.data(), in.c0_host.data(),
                            h->next_T, h->ekf_count, h->c.ekf_hist);
    HIPCHK(hipMemcpyAsync(in.t0, in.t0_host.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(in.c0, in.c0_host.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));  // (the host's copies change at the next call)
    in.bounds();
    in.restarted = in.paused = true;  // (a change on a handle that has paused nobody is a pause)
    return DEKF_OK;
}

dekf_status dekf_get_active(dekf_handle h, int* active, dekf_mem where) {
    if (!h || !active) return fail(DEKF_ERR_INVALID, "null argument");
    if (!h->initialized) return fail(DEKF_ERR_ORDER, "dekf_get_active before dekf_initialize");
    return deliver_ints(h, active, instance_mode(h).paused ? h->inst.act_host : std::vector<int>((size_t)h->c.B, 1), where);
}

dekf_status dekf_set_instance_params(dekf_handle h, const dekf_params* sets, int nsets, const int* set_of) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    TRY(need_direct(h, "dekf_set_instance_params", false));  // (allowed before dekf_initialize: that is when a fresh handle takes its table)
    if (nsets < 0) return fail(DEKF_ERR_INVALID, "dekf_set_instance_params: nsets must be >= 0");
    if (nsets == 0 ? (sets || set_of) : (!sets || !set_of))
        return fail(DEKF_ERR_INVALID, "dekf_set_instance_params: sets and set_of must both be given (nsets > 0) or both be NULL (nsets = 0)");
    const size_t B = (size_t)h->c.B;
    dekf_handle_s::Instances& in = h->inst;
    const bool fresh = !h->initialized && h->ekf_count == 0;  // before the first tick since dekf_create / dekf_reset
    if (nsets == 0) {  // drop the table: the handle's own constants for every instance, and its former kernels
        if (instance_mode(h).clock != Clock::PARAM) return DEKF_OK;
        if (!fresh) return fail(DEKF_ERR_ORDER, "dekf_set_instance_params: the table is dropped before the first tick or right after dekf_reset");
        HIPCHK(hipSetDevice(h->device));
        TRY(quiesce(h));
        in.table = false;
        in.inst_prm.clear();
        launch_reset_state(h, h->s);  // (no table any more: k_reset_state, the EKF state at the handle's initial values)
        HIPCHK(hipGetLastError());
        return DEKF_OK;
    }
    // everything is checked before anything is applied
    for (int k = 0; k < nsets; ++k) {
        if (!same_but_noise(sets[k], h->prm))
            return fail(DEKF_ERR_INVALID, "dekf_set_instance_params: a set differs from the handle's parameters in a field that is not a noise field");
        if (const char* msg = check_noise(sets[k])) return fail(DEKF_ERR_INVALID, msg);
    }
    const int T = h->next_T - 1;
    bool any = false;
    for (size_t b = 0; b < B; ++b) {
        if (set_of[b] < -1 || set_of[b] >= nsets) return fail(DEKF_ERR_INVALID, "dekf_set_instance_params: set_of entries must lie in -1 .. nsets - 1");
        any = any || set_of[b] >= 0;
    }
    if (!fresh)
        for (size_t b = 0; b < B; ++b) {
            if (set_of[b] < 0) continue;
            // only an instance that dekf_reset_instances has restarted and that has seen neither an update nor an EKF tick since:
            // its own local step is -1 and its own local EKF count 0, whatever the handle ticked before the restart (or ticks
            // while the instance is paused: mhe_pause_core.h)
            const bool restarted = h->initialized && instance_mode(h).restarted &&
                                   instance_tick((int)b, T, in.act_host.data(), in.pz_step.data(), in.t0_host.data()) == -1 &&
                                   instance_count((int)b, h->ekf_count, in.act_host.data(), in.pz_count.data(), in.c0_host.data()) == 0;
            if (!restarted)
                return fail(DEKF_ERR_ORDER, "dekf_set_instance_params: an instance takes a set before its first tick only (before the first "
                                            "dekf_ekf_step, right after dekf_reset, or right after dekf_reset_instances restarted it)");
        }
    HIPCHK(hipSetDevice(h->device));
    TRY(quiesce(h));  // (the arrival cost computed ahead reads the table)
    TRY(in.ensure(h));
    if (!in.pp_mhe) {
        TRY(dev_alloc(h, B * sizeof(DevCfg), &in.pp_mhe));
        TRY(dev_alloc(h, B * PpEkf::len * sizeof(double), &in.pp_ekf));
    }
    if (instance_mode(h).clock != Clock::PARAM) in.inst_prm.assign(B, h->prm);  // (a new table: every instance on the handle's own set)
    for (size_t b = 0; b < B; ++b)
        if (set_of[b] >= 0) in.inst_prm[b] = with_noise_of(h->prm, sets[set_of[b]]);
    // both tables are written whole from the host's copy (the entries of untouched instances with the values they hold): the handle's
    // DevCfg with the constants fill_cfg derives for a handle created with the instance's set
    std::vector<DevCfg> tm(B, h->c);
    std::vector<double> te(B * PpEkf::len);
    std::vector<int> mask(B);
    for (size_t b = 0; b < B; ++b) {
        fill_noise(in.inst_prm[b], tm[b]);
        pp_pack_ekf(tm[b], te.data(), B, b);
        mask[b] = set_of[b] >= 0;
    }
    HIPCHK(hipMemcpyAsync(in.pp_mhe, tm.data(), tm.size() * sizeof(DevCfg), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(in.pp_ekf, te.data(), te.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (any) {  // the EKF state of the instances that took a set: their set's initial quaternion and covariance
        const int* dmask = mask.data();
        TRY(ensure_stage(h, B * sizeof(int)));
        TRY(stage_in(h, 0, &dmask, B));
        k_ekf_init_pp<<<(h->c.B + 255) / 256, 256, 0, h->stream>>>(h->c, h->s, dmask, in.pp_ekf);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(h->stream));  // (the sources of the copies are locals)
    in.table = true;
    return DEKF_OK;
}

dekf_status dekf_get_instance_params(dekf_handle h, int b, dekf_params* out) {
    if (!h || !out) return fail(DEKF_ERR_INVALID, "null argument");
    if (b < 0 || b >= h->c.B) return fail(DEKF_ERR_INVALID, "dekf_get_instance_params: instance out of range");
    *out = instance_mode(h).clock == Clock::PARAM ? h->inst.inst_prm[(size_t)b] : h->prm;
    return DEKF_OK;
}

namespace {
// what dekf_save_instances and dekf_load_instances ask of their arguments alike; the header a blob of n instances of h carries
dekf_status snapshot_args(dekf_handle h, const char* fn, const int* idx, int n, const void* blob, size_t bytes) {
    const std::string f(fn);
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (!idx || !blob) return fail(DEKF_ERR_INVALID, (f + ": null idx or blob").c_str());
    TRY(need_direct(h, fn, true));
    if (n <= 0) return fail(DEKF_ERR_INVALID, (f + ": n must be positive").c_str());
    std::vector<unsigned char> seen((size_t)h->c.B, 0);
    if (!snapshot_indices_valid(idx, n, h->c.B, seen.data()))
        return fail(DEKF_ERR_INVALID, (f + ": every index must lie in 0 .. B - 1 and be named once").c_str());
    if (bytes < dekf_snapshot_bytes(h, n)) return fail(DEKF_ERR_INVALID, (f + ": the blob is smaller than dekf_snapshot_bytes(h, n)").c_str());
    return DEKF_OK;
}
SnapHeader snapshot_header_of(const dekf_handle_s* h, int n) {
    return snapshot_header(h->prm, h->snap_map, n, h->solver, h->smoother, h->cross, h->innov, h->gate_st.nis_leg_max);
}
const dekf_params* instance_params_of(const dekf_handle_s* h, int b) {
    return instance_mode(h).clock == Clock::PARAM ? &h->inst.inst_prm[(size_t)b] : &h->prm;
}
// workgroups per instance of the snapshot kernels: a few instances are spread over the machine by the arrays of the map
int snapshot_chunks(int n) { return n >= 512 ? 1 : (n >= 64 ? 4 : 16); }
// device memory for the length of one call: the image of a host blob
struct TempDev {
    unsigned char* p = nullptr;
    ~TempDev() { if (p) (void)hipFree(p); }
};
}  // namespace

size_t dekf_snapshot_bytes(dekf_handle h, int n) {
    if (!h || n <= 0 || h->c.est_type != 0 || h->pipelined || h->solver != DEKF_SOLVER_DIRECT) return 0;
    return snap_header_bytes() + (size_t)n * snap_record_bytes(h->snap_map);
}

dekf_status dekf_save_instances(dekf_handle h, const int* idx, int n, void* blob, size_t bytes, dekf_mem where) {
    TRY(snapshot_args(h, "dekf_save_instances", idx, n, blob, bytes));
    HIPCHK(hipSetDevice(h->device));
    TRY(quiesce(h));  // (what dekf_reset_instances waits for: the arrival cost computed ahead must have landed before it is copied)
    const dekf_handle_s::Instances& in = h->inst;
    const size_t hb = snap_header_bytes(), rb = snap_record_bytes(h->snap_map), N = (size_t)n;
    // header | books of the n records | idx: built here, staged in one copy; the kernel writes the books at the head of every record
    std::vector<unsigned char> host(hb + N * sizeof(SnapBooks) + N * sizeof(int), 0);
    const SnapHeader hd = snapshot_header_of(h, n);
    std::memcpy(host.data(), &hd, sizeof(hd));
    SnapBooks* bk = (SnapBooks*)(host.data() + hb);
    const bool epochs = in.t0 != nullptr;
    for (size_t i = 0; i < N; ++i) {
        snapshot_books(idx[i], epochs ? in.act_host.data() : nullptr, in.pz_step.data(), in.pz_count.data(), in.t0_host.data(),
                       in.c0_host.data(), h->next_T, h->ekf_count, h->c.ekf_hist, &bk[i].step, &bk[i].count);
        pack_noise(*instance_params_of(h, idx[i]), bk[i].noise);
    }
    std::memcpy(host.data() + hb + N * sizeof(SnapBooks), idx, N * sizeof(int));
    TRY(ensure_stage(h, host.size()));
    unsigned char* const stage = (unsigned char*)h->stage;
    HIPCHK(hipMemcpyAsync(stage, host.data(), host.size(), hipMemcpyHostToDevice, h->stream));
    TempDev tmp;
    unsigned char* dst = (unsigned char*)blob;
    if (where == DEKF_HOST) {
        HIPCHK(hipMalloc((void**)&tmp.p, hb + N * rb));
        dst = tmp.p;
    }
    HIPCHK(hipMemcpyAsync(dst, stage, hb, hipMemcpyDeviceToDevice, h->stream));
    k_save_instances<<<dim3((unsigned)n, (unsigned)snapshot_chunks(n)), 256, 0, h->stream>>>(
        h->snap_map, (const int*)(stage + hb + N * sizeof(SnapBooks)), (const SnapBooks*)(stage + hb), dst + hb, rb);
    HIPCHK(hipGetLastError());
    if (where == DEKF_HOST) HIPCHK(hipMemcpyAsync(blob, dst, hb + N * rb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));  // (a host blob is there when the call returns; `host`, a local, is the source of the staging copy)
    return DEKF_OK;
}

dekf_status dekf_load_instances(dekf_handle h, const int* idx, int n, const void* blob, size_t bytes, dekf_mem where) {
    TRY(snapshot_args(h, "dekf_load_instances", idx, n, blob, bytes));
    HIPCHK(hipSetDevice(h->device));
    dekf_handle_s::Instances& in = h->inst;
    const size_t hb = snap_header_bytes(), rb = snap_record_bytes(h->snap_map), N = (size_t)n;
    const unsigned char* const src = (const unsigned char*)blob;
    // everything is checked before anything is applied: the header, then the books of every record (a device blob's are copied to the
    // host and waited for, as a device mask is)
    SnapHeader got;
    std::vector<SnapBooks> bk(N);
    if (where == DEKF_HOST) std::memcpy(&got, src, sizeof(got));
    else {
        HIPCHK(hipMemcpyAsync(&got, src, sizeof(got), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    const SnapHeader want = snapshot_header_of(h, n);
    if (got.magic != DEKF_SNAP_MAGIC) return fail(DEKF_ERR_INVALID, "dekf_load_instances: not a snapshot blob (magic)");
    if (got.version != DEKF_SNAP_VERSION) return fail(DEKF_ERR_INVALID, "dekf_load_instances: the blob has another format version");
    if (got.n != n) return fail(DEKF_ERR_INVALID, "dekf_load_instances: n is not the blob's n");
    if (std::memcmp(&got, &want, sizeof(got)) != 0)
        return fail(DEKF_ERR_INVALID, "dekf_load_instances: the blob's fingerprint is not this handle's (parameters outside the noise fields, settings, stores)");
    if (where == DEKF_HOST)
        for (size_t i = 0; i < N; ++i) std::memcpy(&bk[i], src + hb + i * rb, sizeof(SnapBooks));
    else {
        HIPCHK(hipMemcpy2DAsync(bk.data(), sizeof(SnapBooks), src + hb, rb, sizeof(SnapBooks), N, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (h->next_T >= DEKF_EPOCH_PAUSED) return fail(DEKF_ERR_ORDER, "dekf_load_instances: the handle has run 2^31 - 2^16 steps: dekf_reset it");
    for (size_t i = 0; i < N; ++i) {
        if (!snapshot_books_valid(bk[i].step, bk[i].count, h->c.ekf_hist))
            return fail(DEKF_ERR_INVALID, "dekf_load_instances: a record's local step or EKF count is out of range");
        double noise[DEKF_SNAP_NOISE];
        pack_noise(*instance_params_of(h, idx[i]), noise);
        if (std::memcmp(noise, bk[i].noise, sizeof(noise)) != 0)
            return fail(DEKF_ERR_INVALID, "dekf_load_instances: a record's noise fields are not those of the instance it loads into "
                                          "(dekf_reset_instances, then dekf_set_instance_params gives the slot the set first)");
    }
    TRY(quiesce(h));
    TRY(in.ensure(h));
    TempDev tmp;
    const unsigned char* recs = src + hb;
    if (where == DEKF_HOST) {
        HIPCHK(hipMalloc((void**)&tmp.p, N * rb));
        HIPCHK(hipMemcpyAsync(tmp.p, src + hb, N * rb, hipMemcpyHostToDevice, h->stream));
        recs = tmp.p;
    }
    const int* didx = idx;
    TRY(ensure_stage(h, N * sizeof(int)));
    TRY(stage_in(h, 0, &didx, N));
    k_load_instances<<<dim3((unsigned)n, (unsigned)snapshot_chunks(n)), 256, 0, h->stream>>>(h->snap_map, didx, recs, rb);
    HIPCHK(hipGetLastError());
    // the books: every loaded instance is active on the epochs of a resume (mhe_snapshot_core.h: load_instance)
    const size_t B = (size_t)h->c.B;
    for (size_t i = 0; i < N; ++i)
        load_instance(idx[i], bk[i].step, bk[i].count, in.act_host.data(), in.t0_host.data(), in.c0_host.data(), h->next_T, h->ekf_count,
                      h->c.ekf_hist);
    HIPCHK(hipMemcpyAsync(in.t0, in.t0_host.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(in.c0, in.c0_host.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));  // (the caller's idx and a host blob are sources of the copies; the host's epochs change at the next call)
    in.bounds();
    in.restarted = true;  // (the epoch twins from here on, as after a restart)
    if (h->smoother && h->win_steps) h->win_steps = epoch_window_steps(h, h->next_T - 1);  // (the loaded windows count from now on)
    return DEKF_OK;
}

dekf_status dekf_sync(dekf_handle h) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < 2; ++i)
        if (h->solve_stream[i]) HIPCHK(hipStreamSynchronize(h->solve_stream[i]));
    if (h->comm_stream) HIPCHK(hipStreamSynchronize(h->comm_stream));
    // (the arrival cost of the next step may still be running beside the last solve: dekf.h promises that ALL work is complete here,
    // and an asynchronous failure of that kernel must surface here too)
    if (h->early_stream) HIPCHK(hipStreamSynchronize(h->early_stream));
    return DEKF_OK;
}
int dekf_batch(dekf_handle h) { return h ? h->c.B : 0; }
void* dekf_stream(dekf_handle h) { return h ? (void*)h->stream : nullptr; }

dekf_status dekf_push_imu(dekf_handle h, const double* imu_time, const double* accel_b, const double* gyro_b, dekf_mem where) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    size_t B = h->c.B;
    double* const dst[3] = {h->s.imu_t, h->s.accel, h->s.gyro};
    const double* const src[3] = {imu_time, accel_b, gyro_b};
    const size_t cnt[3] = {B, 3 * B, 3 * B};
    return put_many(h, 3, dst, src, cnt, where);
}

dekf_status dekf_push_leg(dekf_handle h, const double* p_imu_2_foot, const double* J_imu_2_foot, const double* joint_velocity,
                          const double* contact, dekf_mem where) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    size_t B = h->c.B, L = h->c.L, nj = h->c.nj;
    double* const dst[4] = {h->s.p_foot, h->s.J, h->s.qdot, h->s.contact};
    const double* const src[4] = {p_imu_2_foot, J_imu_2_foot, joint_velocity, contact};
    const size_t cnt[4] = {3 * L * B, 3 * L * nj * B, L * nj * B, L * B};
    return put_many(h, 4, dst, src, cnt, where);
}

dekf_status dekf_push_go1_joints(dekf_handle h, const double* joint_position, const double* joint_velocity,
                                 const double* foot_force, dekf_mem where) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (h->c.L != 4 || h->c.nj != 3) return fail(DEKF_ERR_INVALID, "dekf_push_go1_joints needs num_legs 4, joints_per_leg 3");
    size_t B = h->c.B;
    const double *jp = joint_position, *jv = joint_velocity, *ff = foot_force;
    if (!jp || !jv || !ff) return fail(DEKF_ERR_INVALID, "null input pointer");
    if (where == DEKF_HOST) {  // jp(12) jv(12) ff(4): 28 doubles per instance
        TRY(ensure_stage(h, 28 * B * 8));
        TRY(stage_in(h, 0, &jp, 12 * B));
        TRY(stage_in(h, 12 * B * 8, &jv, 12 * B));
        TRY(stage_in(h, 24 * B * 8, &ff, 4 * B));
    }
    k_go1_leg_odometry<<<(h->c.B + 63) / 64, 64, 0, h->stream>>>(h->c, h->s, jp, jv, ff, h->prm.contact_effort_threshold,
                                                               h->prm.p_ib[0], h->prm.p_ib[1], h->prm.p_ib[2]);
    HIPCHK(hipGetLastError());
    return DEKF_OK;
}

dekf_status dekf_push_vo(dekf_handle h, const int* mask, const double* t_pre, const double* t_now, const double* dp_body,
                         const double* t_pose, const double* q_vo, dekf_mem where) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (!mask || !t_pre || !t_now || !dp_body) return fail(DEKF_ERR_INVALID, "null input pointer");
    if ((q_vo == nullptr) != (t_pose == nullptr)) return fail(DEKF_ERR_INVALID, "t_pose and q_vo must be given together");
    size_t B = h->c.B;
    if (where == DEKF_HOST) {
        // t_pre t_now dp(3) t_pose q(4) mask(int): 10 doubles + 1 int per instance
        TRY(ensure_stage(h, (10 * 8 + 8) * B));
        TRY(stage_in(h, 10 * B * 8, &mask, B));
        TRY(stage_in(h, 0, &t_pre, B));
        TRY(stage_in(h, B * 8, &t_now, B));
        TRY(stage_in(h, 2 * B * 8, &dp_body, 3 * B));
        if (q_vo) {
            TRY(stage_in(h, 5 * B * 8, &t_pose, B));
            TRY(stage_in(h, 6 * B * 8, &q_vo, 4 * B));
        }
    }
    launch_latch_vo(h, mask, t_pre, t_now, dp_body, t_pose, q_vo);
    HIPCHK(hipGetLastError());
    return DEKF_OK;
}

dekf_status dekf_push_quaternion(dekf_handle h, const double* quat, dekf_mem where) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    return put(h, h->s.quat, quat, 4 * (size_t)h->c.B * 8, where);
}

dekf_status dekf_ekf_step(dekf_handle h) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    { Timed t(h, 0); launch_tick(h); }
    HIPCHK(hipGetLastError());
    h->ekf_count++;
    // the kernel uses the count only modulo the ring depth and to know whether the ring is full: folded long before
    // the int overflows (a 500 Hz node reaches 2^31 ticks after 49 days)
    if (h->ekf_count >= (1 << 30)) {
        const int folded = h->c.ekf_hist + h->ekf_count % h->c.ekf_hist;
        // A restarted instance's tick runs on its local count, ekf_count - c0[b]: every epoch is moved so that the local count keeps
        // its value modulo the ring depth and whether it has reached it (mhe_epoch_core.h: fold_epoch).  An epoch of 0 stays 0.
        // A paused instance's epoch is the sentinel and stays it; its stored local count needs no fold (mhe_pause_core.h).
        if (instance_mode(h).restarted) {
            launch_fold(h, h->ekf_count, folded);
            HIPCHK(hipGetLastError());
            for (int& c0 : h->inst.c0_host) c0 = fold_epoch_active(c0, h->ekf_count, folded, h->c.ekf_hist);  // (the host's copy moves alike)
        }
        h->ekf_count = folded;
    }
    return DEKF_OK;
}

dekf_status dekf_initialize(dekf_handle h) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (h->initialized) return fail(DEKF_ERR_ORDER, "dekf_initialize called twice without dekf_reset");
    if (h->c.est_type == 0) {
        if (instance_mode(h).clock == Clock::PARAM) launch_assemble(h, h->s, 0, 0);  // (nobody is restarted or paused before this call)
        else k_mhe_initialize<<<h->c.B, 64, h->lds_asm, h->stream>>>(h->c, h->s);
        h->pushes = 1;
    } else {
        k_kf_initialize<<<h->c.B, 64, h->lds_kf, h->stream>>>(h->c, h->s);
        h->pushes = 2;
    }
    HIPCHK(hipGetLastError());
    h->last_par = 0;
    h->initialized = true;
    h->next_T = 1;
    return DEKF_OK;
}

dekf_status dekf_update(dekf_handle h, int T) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (!h->initialized) return fail(DEKF_ERR_ORDER, "dekf_update before dekf_initialize");
    if (T != h->next_T) return fail(DEKF_ERR_ORDER, "update(T) must be called with T = 1, 2, 3, ... (EstSub.cpp:58-75)");
    if (instance_mode(h).paused && T >= DEKF_EPOCH_PAUSED) return fail(DEKF_ERR_ORDER, "a handle that has paused an instance runs 2^31 - 2^16 steps: dekf_reset it");
    if (h->c.est_type == 0) {
        // the terms, the solve behind them (pipelined: on its own stream), in-order: the next step's arrival cost beside the solve
        const MheStep st = mhe_step(h, T);
        TRY(assemble_step(h, st));
        TRY(solve_step(h, st));
        if (h->early_stream) TRY(marginalize_next_early(h, T));
    } else {
        Timed t(h, 1);
        k_kf_update<<<h->c.B, 64, h->lds_kf, h->stream>>>(h->c, h->s, h->pushes);
    }
    HIPCHK(hipGetLastError());
    h->pushes++;
    h->next_T++;
    return DEKF_OK;
}

dekf_status dekf_step(dekf_handle h, int T) {
    TRY(dekf_ekf_step(h));
    return T == 0 ? dekf_initialize(h) : dekf_update(h, T);
}

dekf_status dekf_get(dekf_handle h, double* x_mhe, double* v_b, double* quat, double* p_vo, int* status, dekf_mem where) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    size_t B = h->c.B;
    TRY(await_results(h));
    const DevState& s = h->sp[h->last_par];
    TRY(fetch(h, x_mhe, s.x_mhe, (size_t)h->c.ns * B * 8, where));
    TRY(fetch(h, v_b, s.v_b, 3 * B * 8, where));
    TRY(fetch(h, quat, s.quat, 4 * B * 8, where));
    TRY(fetch(h, p_vo, s.p_vo, 3 * B * 8, where));
    TRY(fetch(h, status, s.status, B * 4, where));
    return host_sync(h, where);
}

dekf_status dekf_get_ekf_cov(dekf_handle h, double* cov, dekf_mem where) {
    if (!h || !cov) return fail(DEKF_ERR_INVALID, "null argument");
    // device layout is [16][B] (field-major, one lane per instance in k_ekf_tick); hand out [B][4][4].  The transpose
    // is a kernel in stream order: with DEKF_DEVICE this call is as asynchronous as every other getter.
    const size_t B = h->c.B;
    double* dst = cov;
    if (where == DEKF_HOST) {
        TRY(ensure_stage(h, 16 * B * sizeof(double)));
        dst = (double*)h->stage;
    }
    k_ekf_cov_out<<<(int)((16 * B + 255) / 256), 256, 0, h->stream>>>(h->c, h->s, dst);
    HIPCHK(hipGetLastError());
    if (where == DEKF_HOST) TRY(fetch(h, cov, dst, 16 * B * sizeof(double), where));
    return host_sync(h, where);
}

dekf_status dekf_get_solver_info(dekf_handle h, int* iters, int* rho_updates, double* pri_res, double* dua_res, dekf_mem where) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    size_t B = h->c.B;
    TRY(await_results(h));
    const DevState& s = h->sp[h->last_par];
    TRY(fetch(h, iters, s.iters, B * 4, where));
    TRY(fetch(h, rho_updates, s.rho_updates, B * 4, where));
    TRY(fetch(h, pri_res, s.pri_res, B * 8, where));
    TRY(fetch(h, dua_res, s.dua_res, B * 8, where));
    return host_sync(h, where);
}

dekf_status dekf_get_polish_status(dekf_handle h, int* polish_status, dekf_mem where) {
    if (!h || !polish_status) return fail(DEKF_ERR_INVALID, "null argument");
    TRY(await_results(h));
    TRY(fetch(h, polish_status, h->sp[h->last_par].polish_status, (size_t)h->c.B * 4, where));
    return host_sync(h, where);
}

dekf_status dekf_set_warm_start(dekf_handle h, int on) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (on != 0 && on != 1) return fail(DEKF_ERR_INVALID, "dekf_set_warm_start: on must be 0 or 1");
    if (h->c.est_type != 0) return fail(DEKF_ERR_INVALID, "warm start is an MHE setting: this is a KF handle (est_type 1)");
    if (h->pipelined) return fail(DEKF_ERR_INVALID, "warm start cannot be combined with solve_pipeline = 1");
    if (h->initialized) return fail(DEKF_ERR_ORDER, "dekf_set_warm_start is allowed before dekf_initialize or right after dekf_reset");
    if (on && h->solver == DEKF_SOLVER_DIRECT) return fail(DEKF_ERR_INVALID, "warm start has no meaning for a direct solve (dekf_set_solver)");
    HIPCHK(hipSetDevice(h->device));
    if (on && !h->s.warm) {
        WarmLayout wl;
        wl.init(h->c.N, h->c.ns, h->c.nm);
        const size_t B = (size_t)h->c.B;
        double* w = nullptr;
        int* t = nullptr;
        TRY(dev_alloc(h, B * wl.len * sizeof(double), &w));
        TRY(dev_alloc(h, 2 * B * sizeof(int), &t));
        HIPCHK(hipMemsetAsync(t, 0xff, B * sizeof(int), h->stream));  // tags -1: no store is valid yet
        HIPCHK(hipMemsetAsync(t + B, 0, B * sizeof(int), h->stream));
        h->s.warm = w;
        h->s.warm_tag = t;
        h->s.warm_used = t + B;
        h->sp[0] = h->s;
        h->sp[1] = h->s;  // (not pipelined)
    }
    h->c.warm = on;  // (a full-window kernel whose register budget left the warm start's code out: solve_twin picks the twin that carries it)
    return DEKF_OK;
}

dekf_status dekf_get_warm_status(dekf_handle h, int* warm, dekf_mem where) {
    if (!h || !warm) return fail(DEKF_ERR_INVALID, "null argument");
    const size_t n = (size_t)h->c.B * sizeof(int);
    if (!h->s.warm_used) {  // never enabled: every solve started cold
        if (where == DEKF_HOST) std::memset(warm, 0, n);
        else HIPCHK(hipMemsetAsync(warm, 0, n, h->stream));
        return DEKF_OK;
    }
    TRY(fetch(h, warm, h->s.warm_used, n, where));
    return host_sync(h, where);
}

dekf_status dekf_set_solver(dekf_handle h, int solver) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (solver != DEKF_SOLVER_ADMM && solver != DEKF_SOLVER_DIRECT)
        return fail(DEKF_ERR_INVALID, "dekf_set_solver: solver must be DEKF_SOLVER_ADMM (0) or DEKF_SOLVER_DIRECT (1)");
    if (h->c.est_type != 0) return fail(DEKF_ERR_INVALID, "the solver is an MHE setting: this is a KF handle (est_type 1)");
    if (h->pipelined) return fail(DEKF_ERR_INVALID, "dekf_set_solver cannot be combined with solve_pipeline = 1");
    if (h->initialized) return fail(DEKF_ERR_ORDER, "dekf_set_solver is allowed before dekf_initialize or right after dekf_reset");
    if (solver == DEKF_SOLVER_ADMM && instance_mode(h).clock == Clock::PARAM)
        return fail(DEKF_ERR_INVALID, "the handle has a parameter table (dekf_set_instance_params): drop it first (nsets = 0)");
    if (solver == DEKF_SOLVER_DIRECT) {
        if (h->c.polish) return fail(DEKF_ERR_INVALID, "the direct solve cannot be combined with osqp.polish = 1");
        if (h->c.warm) return fail(DEKF_ERR_INVALID, "the direct solve cannot be combined with warm start (dekf_set_warm_start)");
        const DirectKernel* k = direct_kernel(h->c.L, h->c.ft, h->c.N);
        if (!k) return fail(DEKF_ERR_INVALID, "no direct solve kernel for this shape");
        HIPCHK(hipSetDevice(h->device));
        if (!h->mhe_cov) {
            TRY(dev_alloc(h, (size_t)h->c.B * h->c.ns * h->c.ns * sizeof(double), &h->mhe_cov));
            h->snap_map.add(h->mhe_cov, h->c.ns * h->c.ns, 8, SNAP_INSTANCE_MAJOR, SNAP_TAG_COV);
        }
        h->direct = k;
        h->lds_direct = (size_t)DirectScratch::len(h->c.ns) * sizeof(double);
    }
    h->solver = solver;
    h->mhe_cov_valid = false;
    if (solver == DEKF_SOLVER_ADMM) {  // the smoother, its cross-covariances, the innovation statistics and their gate are the direct solve's
        h->smoother = h->cross = h->innov = h->gate_smoother = false;
        h->gate_st.nis_leg_max = 0.0;
    }
    h->innov_valid = false;
    h->win_steps = 0;
    return DEKF_OK;
}

// the window smoother's stores and their entries of the state map, at the first call that needs them (dekf_set_smoother,
// dekf_set_gate_smoother)
static dekf_status smoother_stores(dekf_handle h) {
    if (h->win.x) return DEKF_OK;
    HIPCHK(hipSetDevice(h->device));
    const size_t B = (size_t)h->c.B, N = (size_t)h->c.N, ns = (size_t)h->c.ns;
    TRY(dev_alloc(h, B * (N * ns + (2 * N - 1) * ns * ns) * sizeof(double), &h->win.x));  // x | cov | t1 in one block
    h->win.cov = h->win.x + B * N * ns;
    h->win.t1 = h->win.cov + B * N * ns * ns;
    h->snap_map.add(h->win.x, h->c.N * h->c.ns, 8, SNAP_INSTANCE_MAJOR, SNAP_TAG_WIN_X);
    h->snap_map.add(h->win.cov, h->c.N * h->c.ns * h->c.ns, 8, SNAP_INSTANCE_MAJOR, SNAP_TAG_WIN_COV);
    h->snap_map.add(h->win.t1, (h->c.N - 1) * h->c.ns * h->c.ns, 8, SNAP_INSTANCE_MAJOR, SNAP_TAG_WIN_T1);
    return DEKF_OK;
}

dekf_status dekf_set_smoother(dekf_handle h, int on) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (on != 0 && on != 1) return fail(DEKF_ERR_INVALID, "dekf_set_smoother: on must be 0 or 1");
    if (on && h->gate_st.nis_leg_max > 0.0)
        return fail(DEKF_ERR_INVALID, "the window smoother cannot be combined with the innovation gate (dekf_set_innovation_gate)");
    if (on && h->solver != DEKF_SOLVER_DIRECT) return fail(DEKF_ERR_INVALID, "the window smoother needs a direct handle (dekf_set_solver(h, DEKF_SOLVER_DIRECT))");
    if (h->initialized) return fail(DEKF_ERR_ORDER, "dekf_set_smoother is allowed before dekf_initialize or right after dekf_reset");
    if (on) TRY(smoother_stores(h));
    h->smoother = on != 0;
    if (!on) h->cross = h->gate_smoother = false;  // the cross-covariances and the gate's window are the smoother's: switched off with it
    h->win_steps = 0;
    return DEKF_OK;
}

dekf_status dekf_set_gate_smoother(dekf_handle h, int on) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (on != 0 && on != 1) return fail(DEKF_ERR_INVALID, "dekf_set_gate_smoother: on must be 0 or 1");
    if (on && !(h->innov && h->gate_st.nis_leg_max > 0.0))
        return fail(DEKF_ERR_INVALID, "dekf_set_gate_smoother needs a gating handle (dekf_set_innovation_gate with a bound > 0)");
    if (on && h->smoother && !h->gate_smoother)
        return fail(DEKF_ERR_INVALID, "dekf_set_gate_smoother(h, 1) needs the smoother off: it switches it on itself");
    if (h->initialized) return fail(DEKF_ERR_ORDER, "dekf_set_gate_smoother is allowed before dekf_initialize or right after dekf_reset");
    if (on) TRY(smoother_stores(h));
    if (on || h->gate_smoother) {  // (off on a handle without the option leaves a smoothing handle as it is)
        h->smoother = h->gate_smoother = on != 0;
        h->win_steps = 0;
    }
    return DEKF_OK;
}

dekf_status dekf_set_window_cross(dekf_handle h, int on) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (on != 0 && on != 1) return fail(DEKF_ERR_INVALID, "dekf_set_window_cross: on must be 0 or 1");
    if (on && !h->smoother) return fail(DEKF_ERR_INVALID, "the window cross-covariances need a smoothing handle (dekf_set_smoother(h, 1))");
    if (on && h->gate_smoother)
        return fail(DEKF_ERR_INVALID, "the window cross-covariances cannot be combined with dekf_set_gate_smoother: their backward pass overwrites T1_k");
    if (h->initialized) return fail(DEKF_ERR_ORDER, "dekf_set_window_cross is allowed before dekf_initialize or right after dekf_reset");
    if (on && !h->cross_st.newest) {
        HIPCHK(hipSetDevice(h->device));
        const size_t B = (size_t)h->c.B, N = (size_t)h->c.N, ns = (size_t)h->c.ns;
        TRY(dev_alloc(h, B * N * ns * ns * sizeof(double), &h->cross_st.newest));  // (the lag-one blocks take the smoother's t1 store)
        h->snap_map.add(h->cross_st.newest, h->c.N * h->c.ns * h->c.ns, 8, SNAP_INSTANCE_MAJOR, SNAP_TAG_CROSS);
    }
    h->cross = on != 0;
    h->win_steps = 0;
    return DEKF_OK;
}

dekf_status dekf_get_window(dekf_handle h, int* steps, double* x_win, double* cov_win, dekf_mem where) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (!h->smoother) return fail(DEKF_ERR_INVALID, "dekf_get_window needs a smoothing handle (dekf_set_smoother(h, 1))");
    if (!h->win_steps) return fail(DEKF_ERR_ORDER, "dekf_get_window before the first update (since dekf_create or dekf_reset)");
    const size_t B = (size_t)h->c.B, N = (size_t)h->c.N, ns = (size_t)h->c.ns, K = (size_t)h->win_steps;
    if (steps) *steps = h->win_steps;
    // the K written entries of every instance: [B][N][...] with a pitch of N entries on both sides
    TRY(fetch_rows(h, x_win, h->win.x, N * ns * 8, K * ns * 8, B, where));
    TRY(fetch_rows(h, cov_win, h->win.cov, N * ns * ns * 8, K * ns * ns * 8, B, where));
    return x_win || cov_win ? host_sync(h, where) : DEKF_OK;
}

dekf_status dekf_get_window_cross(dekf_handle h, int* steps, double* cov_lag1, double* cov_newest, dekf_mem where) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (!h->cross) return fail(DEKF_ERR_INVALID, "dekf_get_window_cross needs a cross handle (dekf_set_window_cross(h, 1))");
    if (!h->win_steps) return fail(DEKF_ERR_ORDER, "dekf_get_window_cross before the first update (since dekf_create or dekf_reset)");
    const size_t B = (size_t)h->c.B, N = (size_t)h->c.N, n2 = (size_t)h->c.ns * h->c.ns, K = (size_t)h->win_steps;
    if (steps) *steps = h->win_steps;
    // the K - 1 and K written entries of every instance: [B][N - 1][ns^2] and [B][N][ns^2], the pitch the same on both sides
    TRY(fetch_rows(h, cov_lag1, h->win.t1, (N - 1) * n2 * 8, (K - 1) * n2 * 8, B, where));
    TRY(fetch_rows(h, cov_newest, h->cross_st.newest, N * n2 * 8, K * n2 * 8, B, where));
    return cov_lag1 || cov_newest ? host_sync(h, where) : DEKF_OK;
}

dekf_status dekf_set_innovation(dekf_handle h, int on) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (on != 0 && on != 1) return fail(DEKF_ERR_INVALID, "dekf_set_innovation: on must be 0 or 1");
    if (on && h->solver != DEKF_SOLVER_DIRECT) return fail(DEKF_ERR_INVALID, "the innovation statistics need a direct handle (dekf_set_solver(h, DEKF_SOLVER_DIRECT))");
    if (on && h->c.ft) return fail(DEKF_ERR_INVALID, "the innovation statistics are not available with foot-position states (leg_odom_type 1)");
    if (h->initialized) return fail(DEKF_ERR_ORDER, "dekf_set_innovation is allowed before dekf_initialize or right after dekf_reset");
    if (on && !h->innov_st.nu) {
        HIPCHK(hipSetDevice(h->device));
        const size_t B = (size_t)h->c.B, L = (size_t)h->c.L, nm = 3 * L;
        double* q = nullptr;
        TRY(dev_alloc(h, B * InnovStore::len(h->c.L) * sizeof(double), &q));  // nu | S | nis | nis_leg | loglik in one block
        HIPCHK(hipMemsetAsync(q, 0xff, B * InnovStore::len(h->c.L) * sizeof(double), h->stream));  // (NaN: an instance keeps it until its first solve)
        h->innov_st.nu = q;
        h->innov_st.S = q + B * nm;
        h->innov_st.nis = h->innov_st.S + B * nm * nm;
        h->innov_st.nis_leg = h->innov_st.nis + B;
        h->innov_st.loglik = h->innov_st.nis_leg + B * L;
        h->snap_map.add(h->innov_st.nu, (int)nm, 8, SNAP_INSTANCE_MAJOR, SNAP_TAG_INNOV_NU);
        h->snap_map.add(h->innov_st.S, (int)(nm * nm), 8, SNAP_INSTANCE_MAJOR, SNAP_TAG_INNOV_S);
        h->snap_map.add(h->innov_st.nis, 1, 8, SNAP_INSTANCE_MAJOR, SNAP_TAG_INNOV_NIS);
        h->snap_map.add(h->innov_st.nis_leg, (int)L, 8, SNAP_INSTANCE_MAJOR, SNAP_TAG_INNOV_NIS_LEG);
        h->snap_map.add(h->innov_st.loglik, 1, 8, SNAP_INSTANCE_MAJOR, SNAP_TAG_INNOV_LOGLIK);
    }
    h->innov = on != 0;
    h->innov_valid = false;
    if (!on) h->gate_st.nis_leg_max = 0.0;  // the gate is the statistics': switched off with them
    if (!on && h->gate_smoother) {          // ... and with the gate its window and the smoother that came with it
        h->smoother = h->gate_smoother = false;
        h->win_steps = 0;
    }
    return DEKF_OK;
}

dekf_status dekf_set_innovation_gate(dekf_handle h, double nis_leg_max) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (!(nis_leg_max >= 0.0) || !(nis_leg_max <= 1.7976931348623157e308))
        return fail(DEKF_ERR_INVALID, "dekf_set_innovation_gate: nis_leg_max must be finite and not negative (0 switches the gate off)");
    if (nis_leg_max > 0.0 && !h->innov) return fail(DEKF_ERR_INVALID, "the innovation gate needs an innovation handle (dekf_set_innovation(h, 1))");
    if (nis_leg_max > 0.0 && h->smoother && !h->gate_smoother) return fail(DEKF_ERR_INVALID, "the innovation gate cannot be combined with the window smoother (dekf_set_smoother)");
    if (h->initialized) return fail(DEKF_ERR_ORDER, "dekf_set_innovation_gate is allowed before dekf_initialize or right after dekf_reset");
    if (nis_leg_max > 0.0 && !h->gate_st.gated) {
        HIPCHK(hipSetDevice(h->device));
        const size_t n = (size_t)h->c.B * h->c.L * sizeof(int);
        TRY(dev_alloc(h, n, &h->gate_st.gated));
        HIPCHK(hipMemsetAsync(h->gate_st.gated, 0, n, h->stream));
        h->snap_map.add(h->gate_st.gated, h->c.L, 4, SNAP_INSTANCE_MAJOR, SNAP_TAG_GATED);
    }
    h->gate_st.nis_leg_max = nis_leg_max;
    if (!(nis_leg_max > 0.0) && h->gate_smoother) {  // the gate's window goes with the gate, and the smoother that came with it
        h->smoother = h->gate_smoother = false;
        h->win_steps = 0;
    }
    return DEKF_OK;
}

dekf_status dekf_get_innovation_gate(dekf_handle h, double* nis_leg_max, int* gated, dekf_mem where) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (nis_leg_max) *nis_leg_max = h->gate_st.nis_leg_max;
    if (!gated) return DEKF_OK;
    if (!(h->gate_st.nis_leg_max > 0.0)) return fail(DEKF_ERR_INVALID, "dekf_get_innovation_gate: gated needs a gating handle (dekf_set_innovation_gate)");
    TRY(fetch(h, gated, h->gate_st.gated, (size_t)h->c.B * h->c.L * sizeof(int), where));
    return host_sync(h, where);
}

dekf_status dekf_get_innovation(dekf_handle h, double* innov, double* innov_cov, double* nis, double* nis_leg, double* loglik, dekf_mem where) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (!h->innov) return fail(DEKF_ERR_INVALID, "dekf_get_innovation needs an innovation handle (dekf_set_innovation(h, 1))");
    if (!h->innov_valid) return fail(DEKF_ERR_ORDER, "dekf_get_innovation before the first update (since dekf_create or dekf_reset)");
    const size_t B = (size_t)h->c.B, L = (size_t)h->c.L, nm = 3 * L;
    TRY(fetch(h, innov, h->innov_st.nu, B * nm * 8, where));
    TRY(fetch(h, innov_cov, h->innov_st.S, B * nm * nm * 8, where));
    TRY(fetch(h, nis, h->innov_st.nis, B * 8, where));
    TRY(fetch(h, nis_leg, h->innov_st.nis_leg, B * L * 8, where));
    TRY(fetch(h, loglik, h->innov_st.loglik, B * 8, where));
    return innov || innov_cov || nis || nis_leg || loglik ? host_sync(h, where) : DEKF_OK;
}

dekf_status dekf_get_mhe_cov(dekf_handle h, double* cov, dekf_mem where) {
    if (!h || !cov) return fail(DEKF_ERR_INVALID, "null argument");
    if (h->solver != DEKF_SOLVER_DIRECT) return fail(DEKF_ERR_INVALID, "dekf_get_mhe_cov needs a direct handle (dekf_set_solver(h, DEKF_SOLVER_DIRECT))");
    if (!h->mhe_cov_valid) return fail(DEKF_ERR_ORDER, "dekf_get_mhe_cov before the first update (since dekf_create or dekf_reset)");
    TRY(fetch(h, cov, h->mhe_cov, (size_t)h->c.ns * h->c.ns * h->c.B * 8, where));
    return host_sync(h, where);
}

dekf_status dekf_get_kf_cov(dekf_handle h, double* cov, dekf_mem where) {
    if (!h || !cov) return fail(DEKF_ERR_INVALID, "null argument");
    TRY(fetch(h, cov, h->s.kf_C, (size_t)h->c.ns * h->c.ns * h->c.B * 8, where));
    return host_sync(h, where);
}

dekf_status dekf_timing_enable(dekf_handle h, int on) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    h->timing = on == 2 ? 2 : (on != 0 ? 1 : 0);
    // events are created here, not inside the timed region: enough pairs for a few hundred steps of three launches
    if (h->timing) {
        size_t have = h->ev_pool.size();
        for (int c = 0; c < DEKF_TIMING_CLASSES; ++c) have += h->ev[c].size();
        for (size_t i = have; i < 3 * 1024; ++i) {
            hipEvent_t a = nullptr, b = nullptr;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
                if (a) (void)hipEventDestroy(a);
                break;
            }
            h->ev_pool.push_back({a, b});
        }
    }
    return DEKF_OK;
}
dekf_status dekf_timing_read(dekf_handle h, double* ms_sum, int* launches) {
    if (!h || !ms_sum || !launches) return fail(DEKF_ERR_INVALID, "null argument");
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < 2; ++i)
        if (h->solve_stream[i]) HIPCHK(hipStreamSynchronize(h->solve_stream[i]));
    if (h->comm_stream && !h->ev[3].empty()) HIPCHK(hipStreamSynchronize(h->comm_stream));
    for (int c = 0; c < DEKF_TIMING_CLASSES; ++c) {
        double sum = 0.0;
        for (auto& pr : h->ev[c]) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, pr.first, pr.second));
            sum += ms;
            h->ev_pool.push_back(pr);
        }
        ms_sum[c] = sum;
        launches[c] = (int)h->ev[c].size();
        h->ev[c].clear();
    }
    return DEKF_OK;
}

dekf_status dekf_launch_info(dekf_handle h, int* solve_workgroups, int* compute_units, double* clock_hz) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, h->device));
    if (solve_workgroups) *solve_workgroups = solve_launch(h, h->c.N).grid;  // (the full-window kernel's where the handle has one)
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (clock_hz) *clock_hz = (double)prop.clockRate * 1e3;
    return DEKF_OK;
}

const char* dekf_solve_kernel_name(dekf_handle h, int full_window) {
    if (!h || h->c.est_type != 0) return nullptr;
    return solve_launch(h, full_window ? h->c.N : h->c.N - 1).name;
}

// not part of include/dekf.h: section cycles [B][DEKF_PROF_SLOTS] of the last solve; all zero unless this
// library was built with -DDEKF_PROFILE (libdekf_prof.so, tools/profile_sections.py)
dekf_status dekf_debug_sections(dekf_handle h, double* out_host) {
    if (!h || !out_host) return fail(DEKF_ERR_INVALID, "null argument");
    TRY(await_results(h));
    TRY(fetch(h, out_host, h->sp[h->last_par].prof, DEKF_PROF_SLOTS * (size_t)h->c.B * 8, DEKF_HOST));
    return host_sync(h, DEKF_HOST);
}

#ifdef DEKF_BOUNDS
extern "C" __global__ void k_bounds_selftest(double* a);
dekf_status dekf_debug_bounds_selftest(void) {
    double* a = nullptr;
    HIPCHK(hipMalloc(&a, 32 * sizeof(double)));
    k_bounds_selftest<<<1, 1>>>(a);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipFree(a));
    return DEKF_OK;
}
// not part of include/dekf.h: the bounds-checked diagnostic build (libdekf_bounds.so, wave.h: BPtr).  out[0] = out-of-range
// dereferences since the library was loaded, out[1] = offset of the first one in elements from the start of its array,
// out[2] = that array's extent, out[3] = unused.  Synchronises the device.
dekf_status dekf_debug_bounds_reset(void) {
    const unsigned long long z[4] = {0ull, 0ull, 0ull, 0ull};
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(dekf::dekf_bounds_hits), z, sizeof(z)));
    return DEKF_OK;
}
dekf_status dekf_debug_bounds(unsigned long long* out4) {
    if (!out4) return fail(DEKF_ERR_INVALID, "null argument");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out4, HIP_SYMBOL(dekf::dekf_bounds_hits), 4 * sizeof(unsigned long long)));
    return DEKF_OK;
}
#endif

// ---------------------------------------------------------------- RCCL all-gather
dekf_status dekf_comm_unique_id(void* id_out) {
    if (!id_out) return fail(DEKF_ERR_INVALID, "null argument");
    const char* e = rccl_unique_id(id_out);
    if (e) return fail(DEKF_ERR_COMM, e);
    return DEKF_OK;
}
dekf_status dekf_comm_init(dekf_handle h, int world, int rank, const void* id) {
    if (!h || !id || world < 1 || rank < 0 || rank >= world) return fail(DEKF_ERR_INVALID, "bad communicator arguments");
    if (h->comm) return fail(DEKF_ERR_ORDER, "dekf_comm_init was already called on this handle");
    HIPCHK(hipSetDevice(h->device));
    // Everything the all-gather needs besides the communicator comes first and the communicator is assigned LAST, so
    // a failure on the way leaves the handle exactly as it was (h->comm == nullptr: dekf_allgather_vb refuses, a retry
    // is accepted) instead of half-initialised.
    hipStream_t cs = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr, e3 = nullptr;
    double* snap = nullptr;
    auto rollback = [&] {
        if (snap) (void)hipFree(snap);
        if (e3) (void)hipEventDestroy(e3);
        if (e2) (void)hipEventDestroy(e2);
        if (e1) (void)hipEventDestroy(e1);
        if (e0) (void)hipEventDestroy(e0);
        if (cs) (void)hipStreamDestroy(cs);
    };
    hipError_t he = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&e0, hipEventDisableTiming);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&e1, hipEventDisableTiming);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&e2, hipEventDisableTiming);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&e3, hipEventDisableTiming);
    if (he == hipSuccess) he = hipMalloc((void**)&snap, 3 * (size_t)h->c.B * sizeof(double));
    if (he != hipSuccess) {
        rollback();
        g_err = std::string("dekf_comm_init: ") + hipGetErrorString(he);
        return DEKF_ERR_HIP;
    }
    void* comm = nullptr;
    const char* e = rccl_init_rank(&comm, world, rank, id);  // collective: every rank of `world` must be here
    if (e) {
        rollback();
        return fail(DEKF_ERR_COMM, e);
    }
    h->comm_stream = cs;
    h->ev_vb_ready = e0;
    h->ev_ag_done = e1;
    h->ev_vb_read[0] = e2;
    h->ev_vb_read[1] = e3;
    h->vb_read_pending[0] = h->vb_read_pending[1] = false;
    h->vb_snapshot = snap;
    h->world = world;
    h->rank = rank;
    h->ag_pending = false;
    h->comm = comm;
    return DEKF_OK;
}
dekf_status dekf_allgather_vb(dekf_handle h, double* v_b_all_dev) {
    if (!h || !v_b_all_dev) return fail(DEKF_ERR_INVALID, "null argument");
    if (!h->comm) return fail(DEKF_ERR_ORDER, "dekf_comm_init has not been called");
    HIPCHK(hipSetDevice(h->device));
    const size_t n = 3 * (size_t)h->c.B;
    if (h->pipelined) {
        // Everything on the communication stream, which is in order (the previous all-gather has read the snapshot): wait for the
        // solve that produced v_b, copy it, exchange.  The handle's stream is not involved, so the next step's pushes, EKF tick and
        // assemble are not held back; the solve that will overwrite this set's v_b (two steps on) waits for ev_vb_read (dekf_update).
        if (h->solve_pending[h->last_par]) HIPCHK(hipStreamWaitEvent(h->comm_stream, h->ev_solve[h->last_par], 0));
        else {  // (T = 0: no solve yet; v_b is what the reset / initialise kernels on the handle's stream left)
            HIPCHK(hipEventRecord(h->ev_vb_ready, h->stream));
            HIPCHK(hipStreamWaitEvent(h->comm_stream, h->ev_vb_ready, 0));
        }
        HIPCHK(hipMemcpyAsync(h->vb_snapshot, h->sp[h->last_par].v_b, n * sizeof(double), hipMemcpyDeviceToDevice, h->comm_stream));
        HIPCHK(hipEventRecord(h->ev_vb_read[h->last_par], h->comm_stream));
        h->vb_read_pending[h->last_par] = true;
    } else {
    // the previous all-gather must have read the snapshot before it is overwritten (it finished a step ago)
    if (h->ag_pending) HIPCHK(hipStreamWaitEvent(h->stream, h->ev_ag_done, 0));
    HIPCHK(hipMemcpyAsync(h->vb_snapshot, h->s.v_b, n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipEventRecord(h->ev_vb_ready, h->stream));
    HIPCHK(hipStreamWaitEvent(h->comm_stream, h->ev_vb_ready, 0));
    }
    {
        Timed t(h, 3, h->comm_stream);
        const char* e = rccl_allgather_f64(h->comm, h->vb_snapshot, v_b_all_dev, n, h->comm_stream);
        if (e) return fail(DEKF_ERR_COMM, e);
    }
    HIPCHK(hipEventRecord(h->ev_ag_done, h->comm_stream));
    h->ag_pending = true;
    return DEKF_OK;
}
dekf_status dekf_comm_info(dekf_handle h, int* comm_world, int* comm_rank) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (!h->comm) return fail(DEKF_ERR_ORDER, "dekf_comm_init has not been called");
    int cw = 0, cr = -1;
    const char* e = rccl_comm_info(h->comm, &cw, &cr);
    if (e) return fail(DEKF_ERR_COMM, e);
    if (comm_world) *comm_world = cw;
    if (comm_rank) *comm_rank = cr;
    return DEKF_OK;
}
dekf_status dekf_comm_ranks_seen(dekf_handle h, int* ranks_seen) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (!h->comm) return fail(DEKF_ERR_ORDER, "dekf_comm_init has not been called");
    HIPCHK(hipSetDevice(h->device));
    // one double per rank through the very communicator and stream the v_b exchange uses
    double* buf = nullptr;
    HIPCHK(hipMalloc((void**)&buf, (size_t)(h->world + 1) * sizeof(double)));
    const double mine = (double)h->rank;
    hipError_t he = hipMemcpyAsync(buf + h->world, &mine, sizeof(double), hipMemcpyHostToDevice, h->comm_stream);
    if (he == hipSuccess) he = hipStreamSynchronize(h->comm_stream);  // (`mine` is a stack variable)
    const char* e = he == hipSuccess ? rccl_allgather_f64(h->comm, buf + h->world, buf, 1, h->comm_stream) : nullptr;
    std::vector<double> got((size_t)h->world, -1.0);
    if (he == hipSuccess && !e) he = hipMemcpyAsync(got.data(), buf, (size_t)h->world * sizeof(double), hipMemcpyDeviceToHost, h->comm_stream);
    if (he == hipSuccess && !e) he = hipStreamSynchronize(h->comm_stream);
    (void)hipFree(buf);
    if (e) return fail(DEKF_ERR_COMM, e);
    if (he != hipSuccess) { g_err = std::string("dekf_comm_ranks_seen: ") + hipGetErrorString(he); return DEKF_ERR_HIP; }
    std::vector<char> seen((size_t)h->world, 0);
    int n = 0;
    for (int i = 0; i < h->world; ++i) {
        const int r = (int)got[(size_t)i];
        if (got[(size_t)i] == (double)r && r >= 0 && r < h->world && got[(size_t)i] == (double)i && !seen[(size_t)r]) { seen[(size_t)r] = 1; ++n; }  // slot i must hold rank i
    }
    if (ranks_seen) *ranks_seen = n;
    return DEKF_OK;
}
dekf_status dekf_allgather_wait(dekf_handle h) {
    if (!h) return fail(DEKF_ERR_INVALID, "null handle");
    if (h->ag_pending) HIPCHK(hipStreamWaitEvent(h->stream, h->ev_ag_done, 0));
    return DEKF_OK;
}

}  // extern "C"
