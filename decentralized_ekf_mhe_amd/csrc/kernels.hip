// kernels.hip — gfx950 kernel entry points of the estimator hot path.
//   k_ekf_tick        one lane per instance              (ekf_core.h)
//   k_mhe_initialize  one wavefront per instance         (mhe_assemble_core.h)
//   k_mhe_assemble    one wavefront per instance         (mhe_assemble_core.h)
//   k_mhe_solve_*     persistent four-wavefront workgroups, grid-stride over instances; each
//                     workgroup owns one scratch slab in HBM, so a slab is only ever touched
//                     from one XCD (its L2 is the only one that caches it)
//                     (mhe_solve_core.h, mhe_admm_core.h)
//   k_mhe_solve_direct_*  the direct solve (dekf_set_solver), one wavefront per instance: rows x variants of direct_kernels.def (mhe_direct_core.h)
//   k_mhe_innov_*     the innovation statistics behind the direct solve (dekf_set_innovation), one wavefront per instance (mhe_innov_core.h)
//   k_mhe_innov_gate_*  the innovation gate in place of the innovation kernel (dekf_set_innovation_gate, mhe_gate_core.h); _smooth: with
//                     the gate's correction carried down the smoothed window (dekf_set_gate_smoother, mhe_gate_window_core.h)
//   k_kf_*            KF alternative                      (kf_core.h)
//   k_latch_vo        masked VO latch (robotSub::vo_callback for a batch)
//   k_latch4          device-to-device sensor latch of one push (IMU or leg arrays) in one launch
//   k_reset_instances, k_*_ep   restarting single instances of a direct handle (dekf_reset_instances, mhe_epoch_core.h)
//   k_*_pp            the same with noise parameters per instance (dekf_set_instance_params, mhe_params_core.h)
//   k_*_act           the tick, assemble, VO latch and fold of a handle that has paused an instance (dekf_set_active, mhe_pause_core.h)
//   k_save_instances, k_load_instances   single instances to and from a snapshot blob (dekf_save_instances, mhe_snapshot_core.h)
#include <hip/hip_runtime.h>

#include "cfg.h"
#include "ekf_core.h"
#include "go1_kin.h"
#include "kf_core.h"
#include "mhe_assemble_core.h"
#include "mhe_direct_core.h"
#include "mhe_epoch_core.h"
#include "mhe_innov_core.h"
#include "mhe_gate_core.h"
#include "mhe_gate_window_core.h"
#include "mhe_params_core.h"
#include "mhe_pause_core.h"
#include "mhe_snapshot_core.h"
#include "mhe_solve_core.h"

using namespace dekf;

#ifdef DEKF_BOUNDS
namespace dekf {
__device__ unsigned long long dekf_bounds_hits[4] = {0ull, 0ull, 0ull, 0ull};  // wave.h: BPtr
}
// proves that the checker fires: one read and one write just past a 16-element array (both are counted and redirected)
extern "C" __global__ void k_bounds_selftest(double* a) {
    dekf::dptr p = DEKF_SPAN(a, 16);
    const double v = p[16];
    (p + 3)[13] = v + 1.0;
}
#endif

// The solve kernels' instance queue (round 6).  A persistent workgroup takes its next instance from a device-side counter instead of
// striding over the batch by the grid size: instances whose solves take different numbers of ADMM iterations (a fleet that is not in
// lock-step) balance themselves, and a workgroup that the hardware could not place next to the others (four per CU fit on 96-99 % of
// the CUs, tools/probes/r4_residency_probe.hip) finds the queue empty when it finally starts instead of holding the launch for a
// whole round of its own.  queue[0]: next instance; queue[1]: workgroups that have left — the last one resets both, so the counter
// needs nothing from the host and nothing between launches (every workgroup's final fetch has returned before it counts itself out).
__device__ __forceinline__ void solve_queue_leave(const dekf::DevState& s) {
#if DEKF_QUEUE_MODE == 0
    return;
#endif
    if (threadIdx.x == 0 && atomicAdd(s.queue + 1, 1) == (int)gridDim.x - 1) {
        s.queue[0] = 0;
        s.queue[1] = 0;
    }
}

// Two forms of the loop.  STATIC FIRST (every kernel whose grid is placed at once — all of them but the four-per-CU kernels): the first
// instance of a workgroup is its own index (no stampede of gridDim.x atomics on one address when a launch starts); the counter counts
// instances beyond the first gridDim.x.  DYNAMIC (the four-per-CU kernels, whose last workgroups the hardware places late on 2-9 % of
// the CUs, profiles/r06_go1_four_per_cu_3waves.txt): every instance comes from the counter, so a workgroup that starts late holds no
// instance hostage.  In both the fetch of the NEXT instance is issued from INSIDE the current solve (solve_window_t, in front of the
// first ADMM iterations: SolveInfo::next_fetch) — in lock-step every workgroup of a round fetches at the same moment, the atomics on
// one address serialise (about 4 us for 768 of them), and a wavefront's memory operations return in order: issued where the
// wavefront runs LDS-only iterations for the next 60 us, nobody waits for it.
// Measured (Go1, 4096): a lock-step fleet pays 0.2 % for the queue (1.8558 -> 1.860 ms per launch), a mixed fleet (cameras at 5-50 Hz,
// every tenth robot blind: 21 % of the solves stop at 50 iterations, 78 % at 75) gains 4.2 % (1.92 -> 1.84 ms)
// (profiles/r06_fleet_not_in_lock_step.txt).  -DDEKF_QUEUE_MODE=0 (cfg.h): the static grid-stride of rounds 1-5, for A/B builds.
#if DEKF_QUEUE_MODE == 0
#define DEKF_QUEUE_LOOP(...) \
        for (int b = blockIdx.x; b < c.B; b += gridDim.x) { (void)(__VA_ARGS__); DEKF_WG_TRACE_COUNT; }
#define DEKF_QUEUE_LOOP_DYNAMIC(...) DEKF_QUEUE_LOOP(__VA_ARGS__)
#else
#define DEKF_QUEUE_LOOP(...)                                                                         \
        for (int b = blockIdx.x; b < c.B;) {                                                         \
            const dekf::SolveInfo si_ = (__VA_ARGS__);                                               \
            DEKF_WG_TRACE_COUNT;                                                                     \
            if (threadIdx.x == 0) next_instance = si_.next_fetch + (int)gridDim.x;                   \
            __syncthreads();                                                                         \
            b = next_instance;                                                                       \
            __syncthreads();                                                                         \
        }
#define DEKF_QUEUE_LOOP_DYNAMIC(...)                                                                 \
        int nb_ = 0;                                                                                 \
        if (threadIdx.x == 0) nb_ = atomicAdd(s.queue, 1);                                           \
        for (;;) {                                                                                   \
            if (threadIdx.x == 0) next_instance = nb_;                                               \
            __syncthreads();                                                                         \
            const int b = next_instance;                                                             \
            if (b >= c.B) break;                                                                     \
            const dekf::SolveInfo si_ = (__VA_ARGS__);                                               \
            DEKF_WG_TRACE_COUNT;                                                                     \
            nb_ = si_.next_fetch;                                                                    \
        }
#endif

// A/B builds only (-DDEKF_AB_KNOBS, tools/probes/r4_wg_trace.py): when each persistent workgroup started and left (100 MHz wall clock),
// how many instances it solved and where it ran, into the section-stamp buffer (slots 0..3 of row blockIdx.x)
#ifdef DEKF_AB_KNOBS
#define DEKF_WG_TRACE_BEGIN const long long wg_t0_ = wall_clock64(); int wg_n_ = 0;
#define DEKF_WG_TRACE_COUNT ++wg_n_
#define DEKF_WG_TRACE_END                                                                                           \
    if (threadIdx.x == 0 && blockIdx.x < c.B) {                                                                     \
        double* o_ = s.prof + (size_t)blockIdx.x * dekf::DEKF_PROF_SLOTS;                                           \
        o_[0] = (double)wg_t0_; o_[1] = (double)wall_clock64(); o_[2] = (double)wg_n_;                              \
        o_[3] = (double)((__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 0xf) * 65536u + (__builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4) & 0xffffu)); \
    }
#else
#define DEKF_WG_TRACE_BEGIN
#define DEKF_WG_TRACE_COUNT (void)0
#define DEKF_WG_TRACE_END
#endif

extern "C" {

// -DDEKF_KSET_ONLY (the parallel product build, build.sh): this translation unit carries ONLY the kernels of its mask — no stubs
// for the others (another unit defines them) — and the kernels that are not solves only with bit 1024.
#if !defined(DEKF_KSET_ONLY) || (defined(DEKF_KSET) && (DEKF_KSET & 1024))
#define DEKF_MISC_KERNELS 1
#else
#define DEKF_MISC_KERNELS 0
#endif
// ... and the innovation kernels (dekf_set_innovation) only with bit 2048: a unit of their own in the product build, whose resource
// remarks go to a file of their own (build.sh), so that the compiler's account of the kernels of before stays the file it was
#if !defined(DEKF_KSET_ONLY) || (defined(DEKF_KSET) && (DEKF_KSET & 2048))
#define DEKF_INNOV_KERNELS 1
#else
#define DEKF_INNOV_KERNELS 0
#endif
// ... and the gate kernels (dekf_set_innovation_gate) only with bit 4096: one more unit, one more remarks file
#if !defined(DEKF_KSET_ONLY) || (defined(DEKF_KSET) && (DEKF_KSET & 4096))
#define DEKF_GATE_KERNELS 1
#else
#define DEKF_GATE_KERNELS 0
#endif
// ... and the snapshot kernels (dekf_save_instances, dekf_load_instances) only with bit 8192: the same again
#if !defined(DEKF_KSET_ONLY) || (defined(DEKF_KSET) && (DEKF_KSET & 8192))
#define DEKF_SNAPSHOT_KERNELS 1
#else
#define DEKF_SNAPSHOT_KERNELS 0
#endif
// ... and the gate kernels of a smoothing gate handle (dekf_set_gate_smoother) only with bit 16384: the same again
#if !defined(DEKF_KSET_ONLY) || (defined(DEKF_KSET) && (DEKF_KSET & 16384))
#define DEKF_GATE_SMOOTH_KERNELS 1
#else
#define DEKF_GATE_SMOOTH_KERNELS 0
#endif
#if DEKF_MISC_KERNELS
__global__ void __launch_bounds__(64) k_ekf_tick(DevCfg c, DevState s, int count) {
    int b = blockIdx.x * 64 + threadIdx.x;
    if (b < c.B) ekf_tick(c, s, b, count);
}

__global__ void __launch_bounds__(64) k_mhe_initialize(DevCfg c, DevState s) {
    extern __shared__ double lds[];
    assemble_initialize(c, s, blockIdx.x, lds);
    if (threadIdx.x == 0) { s.status[blockIdx.x] = DEKF_SOLVE_NONE; s.iters[blockIdx.x] = 0; }
}

// three wavefronts per SIMD (168 VGPRs, 10 spilled): 0.071 ms per step of 4096 instances against 0.076 ms with the 182 registers and two
// wavefronts the compiler takes unasked; four (128 VGPRs, 290 spilled): 0.074 ms
#ifndef DEKF_ASM_WAVES
#define DEKF_ASM_WAVES 3
#endif
__global__ void __launch_bounds__(64, DEKF_ASM_WAVES) k_mhe_assemble(DevCfg c, DevState s, int T, int pushes) {
    extern __shared__ double lds[];
    assemble_update(c, s, blockIdx.x, T, pushes, lds);
}
// the arrival cost of step T ahead of time (mhe_assemble_core.h: marginalize_early; launched on a second stream behind the assemble
// of step T - 1, so that it runs in the slots the solve of step T - 1 frees in its last round)
__global__ void __launch_bounds__(64, DEKF_ASM_WAVES) k_mhe_marginalize_early(DevCfg c, DevState s, int T) {
    extern __shared__ double lds[];
    marginalize_early(c, s, blockIdx.x, T, lds);
}

// A direct handle that has restarted an instance (dekf_reset_instances) launches these in place of k_ekf_tick, k_mhe_assemble and
// k_mhe_marginalize_early: the same cores on every instance's local step (mhe_epoch_core.h).  t0, c0: the epochs, [B] each.
__global__ void __launch_bounds__(64) k_ekf_tick_ep(DevCfg c, DevState s, int count, const int* c0) {
    int b = blockIdx.x * 64 + threadIdx.x;
    if (b < c.B) ekf_tick_epoch(c, s, b, count, c0);
}
__global__ void __launch_bounds__(64, DEKF_ASM_WAVES) k_mhe_assemble_ep(DevCfg c, DevState s, int T, int pushes, const int* t0) {
    extern __shared__ double lds[];
    assemble_epoch(c, s, blockIdx.x, T, pushes, t0, lds);
}
__global__ void __launch_bounds__(64, DEKF_ASM_WAVES) k_mhe_marginalize_early_ep(DevCfg c, DevState s, int T, const int* t0) {
    extern __shared__ double lds[];
    marginalize_early_epoch(c, s, blockIdx.x, T, t0, lds);
}

// A direct handle with a parameter table (dekf_set_instance_params) launches these in place of the three above, from its first tick
// on (every epoch 0 until an instance restarts): the same cores on every instance's own noise constants (mhe_params_core.h).
// pe: the EKF table [PpEkf::len][B], a lane per instance; pc: the MHE table, a DevCfg per instance, whose address is uniform in the
// workgroup: const __restrict__, so the cores read it through scalar loads as they read the kernel arguments.
__global__ void __launch_bounds__(64) k_ekf_tick_pp(DevCfg c, DevState s, int count, const int* c0, const double* __restrict__ pe) {
    int b = blockIdx.x * 64 + threadIdx.x;
    if (b < c.B) ekf_tick_pp(c, s, b, count, c0, pe);
}
__global__ void __launch_bounds__(64, DEKF_ASM_WAVES) k_mhe_assemble_pp(DevState s, int T, int pushes, const int* t0,
                                                                        const DevCfg* __restrict__ pc) {
    extern __shared__ double lds[];
    assemble_pp(pc, s, blockIdx.x, T, pushes, t0, lds);
}
__global__ void __launch_bounds__(64, DEKF_ASM_WAVES) k_mhe_marginalize_early_pp(DevState s, int T, const int* t0,
                                                                                 const DevCfg* __restrict__ pc) {
    extern __shared__ double lds[];
    marginalize_early_pp(pc, s, blockIdx.x, T, t0, lds);
}

// A direct handle that has paused an instance (dekf_set_active) launches these in place of k_ekf_tick_ep and k_mhe_assemble_ep, or of
// k_ekf_tick_pp and k_mhe_assemble_pp where it has a parameter table: the same cores, or nothing for an instance whose epoch is the
// sentinel (mhe_pause_core.h; in the assemble kernels one scalar load per workgroup).  The marginalise and solve kernels of such a
// handle are the epoch and parameter twins as they are: they do nothing below a local step of 2 and of 1.
__global__ void __launch_bounds__(64) k_ekf_tick_act(DevCfg c, DevState s, int count, const int* c0) {
    int b = blockIdx.x * 64 + threadIdx.x;
    if (b < c.B) ekf_tick_active(c, s, b, count, c0);
}
__global__ void __launch_bounds__(64) k_ekf_tick_act_pp(DevCfg c, DevState s, int count, const int* c0, const double* __restrict__ pe) {
    int b = blockIdx.x * 64 + threadIdx.x;
    if (b < c.B) ekf_tick_active_pp(c, s, b, count, c0, pe);
}
__global__ void __launch_bounds__(64, DEKF_ASM_WAVES) k_mhe_assemble_act(DevCfg c, DevState s, int T, int pushes, const int* t0) {
    extern __shared__ double lds[];
    assemble_active(c, s, blockIdx.x, T, pushes, t0, lds);
}
__global__ void __launch_bounds__(64, DEKF_ASM_WAVES) k_mhe_assemble_act_pp(DevState s, int T, int pushes, const int* t0,
                                                                            const DevCfg* __restrict__ pc) {
    extern __shared__ double lds[];
    assemble_active_pp(pc, s, blockIdx.x, T, pushes, t0, lds);
}
#endif  // DEKF_MISC_KERNELS

// The solve kernels (solve_kernels.def).  One workgroup of DEKF_SOLVE_THREADS lanes (4 wavefronts, one per SIMD of the CU) per
// instance; the leg count is a compile-time constant of each instantiation.  The second launch bound (2 waves per SIMD) caps
// VGPR+AGPR at 256 so that TWO workgroups stay resident per CU — LDS allows exactly two, and at 260 registers the kernel silently
// dropped to one (2x slower).
// DEKF_SOLVE_MIN_WAVES: wavefronts per SIMD the generic instantiations are compiled for (2 -> 256 VGPRs; the
// residency experiment in EXPERIMENTS.md II §4.4 builds them with 3 -> 168 VGPRs)
#ifndef DEKF_SOLVE_MIN_WAVES
#define DEKF_SOLVE_MIN_WAVES 2
#endif
// ON: false for an empty body (a warm twin the row's role does not have, solve_kernels.def: DEKF_WARM_TWIN_*)
#define DEKF_SOLVE_BODY_(NAME, THREADS, WAVES, LOOP, ON, POLISH, WARM, ...)                                                   \
    __global__ void __launch_bounds__(THREADS, WAVES) NAME(DevCfg c, DevState s, int kstart, int K, int gws_len) {            \
        if constexpr (ON) {                                                                                                  \
        extern __shared__ double lds[];                                                                                      \
        __shared__ int next_instance;                                                                                        \
        double* gws = s.gws + (size_t)blockIdx.x * gws_len;                                                                  \
        DEKF_WG_TRACE_BEGIN                                                                                                  \
        LOOP(SolveEntry<POLISH, WARM>::template run<__VA_ARGS__>(c, s, b, kstart, K, lds, gws))                              \
        solve_queue_leave(s);                                                                                                \
        DEKF_WG_TRACE_END                                                                                                    \
        }                                                                                                                    \
    }
#define DEKF_SOLVE_STUB_(NAME) __global__ void NAME(DevCfg, DevState, int, int, int) {}
// a kernel of the build's sets, its polishing twin (-DDEKF_NO_POLISH_KERNELS, A/B and diagnostic builds: an empty twin — half the
// compile time; osqp.polish true is then refused by dekf_create) and, for the roles with DEKF_WARM_TWIN_<role> 1, the warm twins
// NAME_warm / NAME_warm_pol: NAME is then compiled without the warm start's code (empty stubs for the other roles, whose kernels
// carry it behind a run-time branch)
#define DEKF_WARM_TWIN_(ROLE) DEKF_WARM_TWIN_##ROLE
#ifdef DEKF_NO_POLISH_KERNELS
#define DEKF_SOLVE_KERNEL(NAME, ROLE, THREADS, WAVES, LOOP, ...)                                                              \
    DEKF_SOLVE_BODY_(NAME, THREADS, WAVES, LOOP, true, false, !DEKF_WARM_TWIN_(ROLE), __VA_ARGS__)                            \
    DEKF_SOLVE_STUB_(NAME##_pol)                                                                                             \
    DEKF_SOLVE_BODY_(NAME##_warm, THREADS, WAVES, LOOP, DEKF_WARM_TWIN_(ROLE), false, true, __VA_ARGS__)                      \
    DEKF_SOLVE_STUB_(NAME##_warm_pol)
#else
#define DEKF_SOLVE_KERNEL(NAME, ROLE, THREADS, WAVES, LOOP, ...)                                                              \
    DEKF_SOLVE_BODY_(NAME, THREADS, WAVES, LOOP, true, false, !DEKF_WARM_TWIN_(ROLE), __VA_ARGS__)                            \
    DEKF_SOLVE_BODY_(NAME##_pol, THREADS, WAVES, LOOP, true, true, !DEKF_WARM_TWIN_(ROLE), __VA_ARGS__)                       \
    DEKF_SOLVE_BODY_(NAME##_warm, THREADS, WAVES, LOOP, DEKF_WARM_TWIN_(ROLE), false, true, __VA_ARGS__)                      \
    DEKF_SOLVE_BODY_(NAME##_warm_pol, THREADS, WAVES, LOOP, DEKF_WARM_TWIN_(ROLE), true, true, __VA_ARGS__)
#endif
// a kernel outside the sets: empty stubs, so a library built with a mask solves only the shapes of its kernels; none in the
// product build's per-set units (-DDEKF_KSET_ONLY: another unit defines it)
#ifdef DEKF_KSET_ONLY
#define DEKF_SOLVE_KERNEL_OFF(...)
#else
#define DEKF_SOLVE_KERNEL_OFF(NAME, ...) DEKF_SOLVE_STUB_(NAME) DEKF_SOLVE_STUB_(NAME##_pol) DEKF_SOLVE_STUB_(NAME##_warm) DEKF_SOLVE_STUB_(NAME##_warm_pol)
#endif
#include "solve_kernels.def"

// The direct solve kernels (direct_kernels.def): one wavefront per instance, a grid of B; every instance does the same work, so the
// instance queue of the ADMM kernels would gain nothing.  cov: Cov(x_T) per instance, [B][ns][ns].
// Every row of the catalogue is defined once per variant of its list, NAME##SUFFIX: direct_solve_t's <L, FT, SMOOTH, CROSS>
// instantiation (win: the window stores, DirectWindow; cross: the store of the to-newest cross-covariances, DirectCross) inside the
// body of the variant's clock.  EPOCH: one scalar load of the epoch per workgroup, then the instance's local window, or nothing at its
// local step 0 (mhe_epoch_core.h).  PARAM: the same on pc[blockIdx.x] (scalar loads from a workgroup-uniform address, mhe_params_core.h);
// of the noise constants the direct solve reads Q_bias_dt2 alone, the rest is in the window records the assemble step wrote.
#define DEKF_DIRECT_BODY_WINDOW(...) __VA_ARGS__;
#define DEKF_DIRECT_BODY_EPOCH(...) int kstart, K; if (direct_window_epoch(c, T, t0[blockIdx.x], kstart, K)) __VA_ARGS__;
#define DEKF_DIRECT_BODY_PARAM(...) const DevCfg& c = pc[blockIdx.x]; DEKF_DIRECT_BODY_EPOCH(__VA_ARGS__)
#define DEKF_DIRECT_DEFINE_(SUFFIX, SMOOTH, CROSS, CLOCK, NAME, L, FT)                                                        \
    __global__ void __launch_bounds__(64) NAME##SUFFIX(DEKF_DIRECT_PARAMS(SMOOTH, CROSS, CLOCK)) {                            \
        extern __shared__ double lds[];                                                                                      \
        DEKF_DIRECT_BODY_##CLOCK(direct_solve_t<L, FT, SMOOTH, CROSS>(c, s, blockIdx.x, kstart, K, lds, cov                   \
                                                                      DEKF_DIRECT_IF_##SMOOTH(, win) DEKF_DIRECT_IF_##CROSS(, cross))) \
    }
#define DEKF_DIRECT_STUB_(SUFFIX, SMOOTH, CROSS, CLOCK, NAME) __global__ void NAME##SUFFIX(DEKF_DIRECT_PARAMS(SMOOTH, CROSS, CLOCK)) {}
#define DEKF_DIRECT_KERNEL(NAME, L, FT, NFIX) DEKF_DIRECT_VARIANTS(DEKF_DIRECT_DEFINE_, NAME, L, FT)
#ifdef DEKF_KSET_ONLY
#define DEKF_DIRECT_KERNEL_OFF(...)
#else
#define DEKF_DIRECT_KERNEL_OFF(NAME, ...) DEKF_DIRECT_VARIANTS(DEKF_DIRECT_STUB_, NAME)
#endif
#include "direct_kernels.def"

#if DEKF_INNOV_KERNELS
// The innovation kernels (dekf_set_innovation, mhe_innov_core.h): launched behind the direct solve on its stream, one wavefront per
// instance, a grid of B; one per leg count (foot-state handles are outside the interface).  They read what the solve left (x_mhe, the
// status, cov) and the newest window record.  Kernels of their own, in a set of their own (bit 2048, below): the direct kernels are the
// code they were, and every build without -DDEKF_KSET_ONLY carries these, whatever its mask.
// The epoch twin k_mhe_innov_L_ep is what a handle launches that launches the direct kernels' epoch or parameter twins: it takes the
// handle's step T in place of (kstart, K) and finds its instance's newest record from the local step, or does nothing below a local
// step of 1 (a restarted instance at its step 0, a paused instance).  No parameter twin: the record carries the instance's own Q_m,
// and all the kernel reads of DevCfg is the structure, which is the handle's.
#define DEKF_INNOV_KERNEL(L)                                                                                                  \
    __global__ void __launch_bounds__(64) k_mhe_innov_##L(DevCfg c, DevState s, int kstart, int K, const double* cov, InnovStore out) { \
        extern __shared__ double lds[];                                                                                      \
        innovation_t<L>(c, s, blockIdx.x, (kstart + K - 1) % c.wcap, cov, out, lds);                                          \
    }                                                                                                                        \
    __global__ void __launch_bounds__(64) k_mhe_innov_##L##_ep(DevCfg c, DevState s, int T, const double* cov, InnovStore out, \
                                                               const int* t0) {                                              \
        extern __shared__ double lds[];                                                                                      \
        int kstart, K;                                                                                                       \
        if (direct_window_epoch(c, T, t0[blockIdx.x], kstart, K))                                                            \
            innovation_t<L>(c, s, blockIdx.x, (kstart + K - 1) % c.wcap, cov, out, lds);                                      \
    }
DEKF_INNOV_KERNEL(1)
DEKF_INNOV_KERNEL(2)
DEKF_INNOV_KERNEL(3)
DEKF_INNOV_KERNEL(4)
#undef DEKF_INNOV_KERNEL
// dekf_reset_instances of an innovation handle (dekf_set_innovation), behind the kernel above: the restarted instances' entries of the
// five arrays NaN until their first solve, as their block of cov.  A kernel of its own: k_reset_instances stays the code it was
__global__ void k_innov_nan(DevCfg c, const int* mask, InnovStore out) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= c.B || !mask[b]) return;
    const int nm = c.nm, L = c.L;
    for (int i = 0; i < nm; ++i) out.nu[(size_t)nm * b + i] = NAN;
    for (int i = 0; i < nm * nm; ++i) out.S[(size_t)nm * nm * b + i] = NAN;
    for (int i = 0; i < L; ++i) out.nis_leg[(size_t)L * b + i] = NAN;
    out.nis[b] = NAN;
    out.loglik[b] = NAN;
}
#endif  // DEKF_INNOV_KERNELS

#if DEKF_GATE_KERNELS
// The gate kernels (dekf_set_innovation_gate, mhe_gate_core.h): what a gating handle launches IN PLACE of the innovation kernel of its
// leg count, so there is no third launch.  The body of k_mhe_innov_L[_ep] with innovation_t called as it is there (the five arrays are
// that kernel's bits), then gate_t in the same wavefront: the decision from the per-leg NIS, the edit of the newest record's Q_m block
// and the rank-3 correction of x_mhe, v_b and cov[b].  A set of their own (bit 4096), carried by every build without -DDEKF_KSET_ONLY.
// The epoch twin takes the parameter table too (pc, null on a handle without one): the swing gain written into the record is the
// instance's own.
#define DEKF_GATE_KERNEL(L)                                                                                                   \
    __global__ void __launch_bounds__(64) k_mhe_innov_gate_##L(DevCfg c, DevState s, int kstart, int K, double* cov, InnovStore out, \
                                                               GateStore gs) {                                               \
        extern __shared__ double lds[];                                                                                      \
        const int slot = (kstart + K - 1) % c.wcap;                                                                          \
        const bool solved = innovation_t<L>(c, s, blockIdx.x, slot, cov, out, lds);                                          \
        gate_t<L>(c, c, s, blockIdx.x, slot, cov, out, gs, solved, lds);                                                     \
    }                                                                                                                        \
    __global__ void __launch_bounds__(64) k_mhe_innov_gate_##L##_ep(DevCfg c, DevState s, int T, double* cov, InnovStore out, \
                                                                    GateStore gs, const int* t0, const DevCfg* __restrict__ pc) { \
        extern __shared__ double lds[];                                                                                      \
        int kstart, K;                                                                                                       \
        if (direct_window_epoch(c, T, t0[blockIdx.x], kstart, K)) {                                                          \
            const int slot = (kstart + K - 1) % c.wcap;                                                                      \
            const bool solved = innovation_t<L>(c, s, blockIdx.x, slot, cov, out, lds);                                      \
            gate_t<L>(c, pc ? pc[blockIdx.x] : c, s, blockIdx.x, slot, cov, out, gs, solved, lds);                           \
        }                                                                                                                    \
    }
DEKF_GATE_KERNEL(1)
DEKF_GATE_KERNEL(2)
DEKF_GATE_KERNEL(3)
DEKF_GATE_KERNEL(4)
#undef DEKF_GATE_KERNEL
#endif  // DEKF_GATE_KERNELS

#if DEKF_GATE_SMOOTH_KERNELS
// The gate kernels of a smoothing gate handle (dekf_set_gate_smoother, mhe_gate_window_core.h): what such a handle launches IN PLACE
// of the gate kernel of its leg count, behind the direct kernel's _smooth twin.  The body of k_mhe_innov_gate_L[_ep] and, for an
// instance that gated a leg, gate_window_t in the same wavefront: the gate's correction carried down the window the smoothing kernel
// has just left (win).  An instance that gates nothing runs the gate kernel's instructions and no more.  The epoch twin takes K from
// direct_window_epoch.  A set of their own (bit 16384), carried by every build without -DDEKF_KSET_ONLY: the eight gate kernels stay
// the code they were.
#define DEKF_GATE_SMOOTH_KERNEL(L)                                                                                            \
    __global__ void __launch_bounds__(64) k_mhe_innov_gate_##L##_smooth(DevCfg c, DevState s, int kstart, int K, double* cov, \
                                                                        InnovStore out, GateStore gs, DirectWindow win) {    \
        extern __shared__ double lds[];                                                                                      \
        const int slot = (kstart + K - 1) % c.wcap;                                                                          \
        const bool solved = innovation_t<L>(c, s, blockIdx.x, slot, cov, out, lds);                                          \
        bool corrected = false;                                                                                              \
        if (gate_t<L>(c, c, s, blockIdx.x, slot, cov, out, gs, solved, lds, &corrected))                                     \
            gate_window_t<L>(c, blockIdx.x, K, corrected, win, lds);                                                         \
    }                                                                                                                        \
    __global__ void __launch_bounds__(64) k_mhe_innov_gate_##L##_smooth_ep(DevCfg c, DevState s, int T, double* cov, InnovStore out, \
                                                                           GateStore gs, const int* t0,                      \
                                                                           const DevCfg* __restrict__ pc, DirectWindow win) { \
        extern __shared__ double lds[];                                                                                      \
        int kstart, K;                                                                                                       \
        if (direct_window_epoch(c, T, t0[blockIdx.x], kstart, K)) {                                                          \
            const int slot = (kstart + K - 1) % c.wcap;                                                                      \
            const bool solved = innovation_t<L>(c, s, blockIdx.x, slot, cov, out, lds);                                      \
            bool corrected = false;                                                                                          \
            if (gate_t<L>(c, pc ? pc[blockIdx.x] : c, s, blockIdx.x, slot, cov, out, gs, solved, lds, &corrected))           \
                gate_window_t<L>(c, blockIdx.x, K, corrected, win, lds);                                                     \
        }                                                                                                                    \
    }
DEKF_GATE_SMOOTH_KERNEL(1)
DEKF_GATE_SMOOTH_KERNEL(2)
DEKF_GATE_SMOOTH_KERNEL(3)
DEKF_GATE_SMOOTH_KERNEL(4)
#undef DEKF_GATE_SMOOTH_KERNEL
#endif  // DEKF_GATE_SMOOTH_KERNELS

#if DEKF_SNAPSHOT_KERNELS
// The snapshot kernels (dekf_save_instances, dekf_load_instances; mhe_snapshot_core.h).  A grid of (n, chunks) workgroups of 256 lanes:
// workgroup (i, j) walks the state map m for instance idx[i] and moves every chunks-th array, from j on, between the handle's state
// and record i of the blob (recs: its first record; rec_bytes apart).  The record side of every copy is contiguous, consecutive lanes
// on consecutive elements; so is the state side of an instance-major array; an element-major one (the EKF state and its history, a
// lane per instance in k_ekf_tick) is strided by B there.  books: the host-side books of the n records, which the save writes at the
// head of each.  A set of their own (bit 8192), carried by every build without -DDEKF_KSET_ONLY.
__global__ void __launch_bounds__(256) k_save_instances(StateMap m, const int* __restrict__ idx, const SnapBooks* __restrict__ books,
                                                        unsigned char* recs, size_t rec_bytes) {
    const size_t i = blockIdx.x;
    snapshot_instance<true>(m, idx[i], recs + i * rec_bytes, books + i, (int)blockIdx.y, (int)gridDim.y);
}
__global__ void __launch_bounds__(256) k_load_instances(StateMap m, const int* __restrict__ idx, const unsigned char* recs, size_t rec_bytes) {
    const size_t i = blockIdx.x;
    snapshot_instance<false>(m, idx[i], const_cast<unsigned char*>(recs) + i * rec_bytes, nullptr, (int)blockIdx.y, (int)gridDim.y);
}
#endif  // DEKF_SNAPSHOT_KERNELS

#if DEKF_MISC_KERNELS
__global__ void k_gap() {}
__global__ void __launch_bounds__(64) k_kf_initialize(DevCfg c, DevState s) {
    extern __shared__ double lds[];
    kf_initialize(c, s, blockIdx.x, lds);
}

__global__ void __launch_bounds__(64) k_kf_update(DevCfg c, DevState s, int pushes) {
    extern __shared__ double lds[];
    kf_update(c, s, blockIdx.x, pushes, lds);
}

__global__ void k_latch_vo(DevCfg c, DevState s, const int* mask, const double* t_pre, const double* t_now,
                           const double* dp, const double* t_pose, const double* q_vo) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= c.B || !mask[b]) return;
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

// k_latch_vo of a handle that has paused an instance: a sample for a paused instance is dropped (mhe_pause_core.h).  t0: the epochs
__global__ void k_latch_vo_act(DevCfg c, DevState s, const int* mask, const int* t0, const double* t_pre, const double* t_now,
                               const double* dp, const double* t_pose, const double* q_vo) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= c.B || !mask[b]) return;
    latch_vo_active(s, b, t0, t_pre, t_now, dp, t_pose, q_vo);
}

// the device-pointer form of dekf_push_imu / dekf_push_leg: all arrays of one push in one grid-stride copy
__global__ void __launch_bounds__(256) k_latch4(LatchCopy4 a) {
    const size_t total = a.end[3], stride = (size_t)gridDim.x * blockDim.x;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int seg = e < a.end[0] ? 0 : (e < a.end[1] ? 1 : (e < a.end[2] ? 2 : 3));
        const size_t off = e - (seg == 0 ? 0 : a.end[seg - 1]);
        a.dst[seg][off] = a.src[seg][off];
    }
}

__global__ void __launch_bounds__(64) k_go1_leg_odometry(DevCfg c, DevState s, const double* jp, const double* jv,
                                                         const double* force, double thr, double pibx, double piby,
                                                         double pibz) {
    int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= c.B) return;
    const double p_ib[3] = {pibx, piby, pibz};
    go1_leg_odometry(s, b, jp, jv, force, thr, p_ib);
}

// Cov_q_ of every instance as [B][4][4] from the field-major EKF state [16][B]: consecutive lanes write consecutive
// doubles, the strided side is the read (16 streams of B doubles: each is contiguous across the lanes that share i)
__global__ void __launch_bounds__(256) k_ekf_cov_out(DevCfg c, DevState s, double* out) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x, B = (size_t)c.B;
    if (e >= 16 * B) return;
    const size_t b = e / 16, i = e - 16 * b;
    out[e] = s.ekf_P[i * B + b];
}

// dekf_reset_instances: reset_instance (mhe_epoch_core.h) for the instances of the mask; cov: the handle's Cov(x_T) store
__global__ void k_reset_instances(DevCfg c, DevState s, const int* mask, double* cov, int* t0, int* c0, int next_T, int ekf_count) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= c.B || !mask[b]) return;
    reset_instance(c, s, b, cov, t0, c0, next_T, ekf_count);
}
// the host has folded its EKF tick count from count_old to count_new (dekf_ekf_step): every epoch follows (fold_epoch)
__global__ void k_fold_epochs(int* c0, int B, int count_old, int count_new, int H) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) c0[b] = fold_epoch(c0[b], count_old, count_new, H);
}
// the same on a handle that has paused an instance: the sentinel of a paused one stays (fold_epoch_active)
__global__ void k_fold_epochs_act(int* c0, int B, int count_old, int count_new, int H) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) c0[b] = fold_epoch_active(c0[b], count_old, count_new, H);
}

// dekf_reset_instances and dekf_reset of a handle with a parameter table: every instance's own initial EKF state (mhe_params_core.h);
// and dekf_set_instance_params itself, for the instances of its mask (all of them at local tick 0 or -1)
__global__ void k_reset_instances_pp(DevCfg c, DevState s, const int* mask, double* cov, int* t0, int* c0, int next_T, int ekf_count,
                                     const double* __restrict__ pe) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= c.B || !mask[b]) return;
    reset_instance_pp(c, s, b, cov, t0, c0, next_T, ekf_count, pe);
}
__global__ void k_reset_state_pp(DevCfg c, DevState s, const double* __restrict__ pe) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < c.B) reset_state_pp(c, s, b, pe);  // (a direct handle has no warm store)
}
__global__ void k_ekf_init_pp(DevCfg c, DevState s, const int* mask, const double* __restrict__ pe) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < c.B && mask[b]) ekf_init_pp(c, s, b, pe);
}

__global__ void k_reset_state(DevCfg c, DevState s) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= c.B) return;
    reset_state_of(c, s, b);  // (mhe_epoch_core.h: what dekf_reset_instances does to one instance)
    if (s.warm_tag) {  // (dekf_reset: no solve starts warm from before it)
        s.warm_tag[b] = -1;
        s.warm_used[b] = 0;
    }
}

#endif  // DEKF_MISC_KERNELS

}  // extern "C"
