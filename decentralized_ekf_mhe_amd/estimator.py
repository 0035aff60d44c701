"""Host-side mirror of the reference's estimator interface for a batch of robots.

``BatchedEstimator`` keeps the method names of ``DecentralizedEstimation``
(initialize / update / reset, DecentralEst.hpp:96-103) and exposes what the reference keeps
in public members (x_MHE_, v_MHE_b_, p_vo_accmulate_, ...) as ``get()``.  All arithmetic
happens in csrc/libdekf.so on the GPU; arguments are numpy arrays (host) or torch CUDA
tensors (HBM, zero-copy)."""
import ctypes as C
import os
import sys

import numpy as np

from . import capi
from .params import DekfParams


def _ptr_where(a, dtype):
    """(void*, DEKF_HOST|DEKF_DEVICE) of a contiguous numpy array or torch tensor"""
    if a is None:
        return None, None
    if isinstance(a, np.ndarray):
        assert a.dtype == dtype and a.flags["C_CONTIGUOUS"], (a.dtype, dtype)
        return C.c_void_p(a.ctypes.data), capi.DEKF_HOST
    import torch
    assert isinstance(a, torch.Tensor) and a.is_contiguous()
    want = torch.float64 if dtype == np.float64 else torch.int32
    assert a.dtype == want, (a.dtype, want)
    return C.c_void_p(a.data_ptr()), (capi.DEKF_DEVICE if a.is_cuda else capi.DEKF_HOST)


def _torch_runtime_first():
    """PyTorch-ROCm ships its own copy of the HIP runtime (torch/lib/libamdhip64.so).  If libdekf.so has already brought up the
    system's copy when torch initialises its own, torch finds no device ("No HIP GPUs are available": seen on the GPU box when a tool
    created an estimator first and uploaded tensors afterwards).  Loaded the other way round, libdekf.so binds to the runtime that is
    already in the process.  So a process that HAS imported torch — i.e. one that may hand tensors to this class — gets torch's
    runtime initialised before libdekf.so touches a device.  A process that has not imported torch (numpy arguments, the C / C++
    callers) is left alone: no torch import, no second HIP runtime in the address space, no seconds of start-up.  A caller that
    imports torch only AFTER creating an estimator sets DEKF_TORCH_RUNTIME_FIRST=1 (or imports torch first)."""
    if "torch" not in sys.modules and os.environ.get("DEKF_TORCH_RUNTIME_FIRST", "0") != "1":
        return
    try:
        import torch
        torch.cuda.is_available()
    except Exception as e:  # noqa: BLE001
        print(f"decentralized_ekf_mhe_amd: torch is imported but its HIP runtime did not come up ({e}); continuing with the system runtime",
              file=sys.stderr)


def relative_cov(cov_win, cov_newest, k):
    """Cov(x_T - x_k) = P_T + P_k - Z_k - Z_k' of the window's newest state against its state k, from window()'s cov_win [..., K, ns, ns]
    and window_cross()'s newest [..., K, ns, ns] (Z_k = Cov(x_k, x_T))"""
    cov_win, cov_newest = np.asarray(cov_win), np.asarray(cov_newest)
    Z = cov_newest[..., k, :, :]
    return cov_win[..., -1, :, :] + cov_win[..., k, :, :] - Z - np.swapaxes(Z, -1, -2)


class BatchedEstimator:
    def __init__(self, params: DekfParams, batch: int, device: int = 0, stream=None, warm_start: bool = False, solver: str = "admm",
                 smoother: bool = False, cross: bool = False, innovation: bool = False, innovation_gate: float = 0.0,
                 gate_smoother: bool = False):
        """warm_start: full-window solves start from the previous tick's shifted solution (dekf_set_warm_start; off by default).
        solver: "admm" (default, the reference's OSQP-style ADMM) or "direct" (the exact optimum of the window QP and its covariance,
        dekf_set_solver; see mhe_cov)
        smoother: a direct handle also leaves every state of the window and its covariance (dekf_set_smoother; see window)
        cross: a smoothing handle also leaves the window's lag-one and to-newest cross-covariances (dekf_set_window_cross; see
        window_cross).  It implies nothing else: without smoother=True the library refuses it
        innovation: a direct handle also leaves the innovation of the newest leg measurement, its covariance, the NIS (whole and per
        leg) and the predictive log-likelihood of every tick (dekf_set_innovation; see innovation)
        innovation_gate: an innovation handle takes a stance leg whose per-leg NIS exceeds this bound out of the solve, as if it had been
        in swing at that tick (dekf_set_innovation_gate; see innovation_gate).  0.0: off.  Without innovation=True the library refuses it
        gate_smoother: a gating handle also smooths; the gate's correction is carried down the window (dekf_set_gate_smoother; see
        window).  Without innovation_gate > 0, or with smoother=True, the library refuses it"""
        if solver not in ("admm", "direct"):
            raise ValueError(f"solver must be 'admm' or 'direct', not {solver!r}")
        _torch_runtime_first()
        self.lib = capi.load()
        self.params = params.copy()
        self.batch = batch
        self.device = device
        h = C.c_void_p()
        capi.check(self.lib.dekf_create(C.byref(self.params), batch, device, C.c_void_p(stream or 0), C.byref(h)))
        self.h = h
        self.T = 0
        try:
            if solver == "direct":
                capi.check(self.lib.dekf_set_solver(self.h, capi.DEKF_SOLVER_DIRECT))
            if smoother:
                capi.check(self.lib.dekf_set_smoother(self.h, 1))
            if cross:
                capi.check(self.lib.dekf_set_window_cross(self.h, 1))
            if innovation:
                capi.check(self.lib.dekf_set_innovation(self.h, 1))
            if innovation_gate != 0.0:
                capi.check(self.lib.dekf_set_innovation_gate(self.h, float(innovation_gate)))
            if gate_smoother:
                capi.check(self.lib.dekf_set_gate_smoother(self.h, 1))
            if warm_start:
                capi.check(self.lib.dekf_set_warm_start(self.h, 1))
        except capi.DekfError:
            self.close()
            raise

    def close(self):
        if getattr(self, "h", None):
            self.lib.dekf_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    # ---- sensor latches --------------------------------------------------------------
    def _where(self, *arrays, dtypes=None):
        ptrs, wheres = [], set()
        for i, a in enumerate(arrays):
            p, w = _ptr_where(a, (dtypes[i] if dtypes else np.float64))
            ptrs.append(p)
            if w is not None:
                wheres.add(w)
        assert len(wheres) == 1, "all arguments of one call must live on the same side"
        return ptrs, wheres.pop()

    def push_imu(self, imu_t, accel, gyro):
        p, w = self._where(imu_t, accel, gyro)
        capi.check(self.lib.dekf_push_imu(self.h, *p, w))

    def push_leg(self, p_foot, J, qdot, contact):
        p, w = self._where(p_foot, J, qdot, contact)
        capi.check(self.lib.dekf_push_leg(self.h, *p, w))

    def push_go1_joints(self, joint_position, joint_velocity, foot_force):
        p, w = self._where(joint_position, joint_velocity, foot_force)
        capi.check(self.lib.dekf_push_go1_joints(self.h, *p, w))

    def push_vo(self, mask, t_pre, t_now, dp, t_pose=None, q_vo=None):
        p, w = self._where(mask, t_pre, t_now, dp, t_pose, q_vo,
                           dtypes=[np.int32] + [np.float64] * 5)
        capi.check(self.lib.dekf_push_vo(self.h, *p, w))

    def push_quaternion(self, quat):
        p, w = self._where(quat)
        capi.check(self.lib.dekf_push_quaternion(self.h, *p, w))

    def push_stream_step(self, s, k):
        """latch step k of a streams dict (numpy or torch-on-device, [K][B][...])"""
        self.push_imu(s["imu_t"][k], s["accel"][k], s["gyro"][k])
        self.push_leg(s["p_foot"][k], s["J"][k], s["qdot"][k], s["contact"][k])
        if s["vo_any"][k]:
            self.push_vo(s["vo_mask"][k], s["vo_t_pre"][k], s["vo_t_now"][k], s["vo_dp"][k],
                         s["vo_t_pose"][k], s["vo_q"][k])

    # ---- the hot path ----------------------------------------------------------------
    def ekf_step(self):
        capi.check(self.lib.dekf_ekf_step(self.h))

    def initialize(self):
        capi.check(self.lib.dekf_initialize(self.h))
        self.T = 1

    def update(self, T):
        capi.check(self.lib.dekf_update(self.h, int(T)))
        self.T = T + 1

    def step(self, T):
        capi.check(self.lib.dekf_step(self.h, int(T)))
        self.T = T + 1

    def reset(self):
        capi.check(self.lib.dekf_reset(self.h))
        self.T = 0

    def reset_instances(self, mask):
        """restart the instances whose mask entry is 1 (dekf_reset_instances; a direct handle, between update(T - 1) and the pushes of
        step T): they start over with the next samples while every other instance keeps running.  mask: int32 [B], numpy or a torch
        CUDA tensor (which must be complete on its stream)"""
        p, w = _ptr_where(mask, np.int32)
        capi.check(self.lib.dekf_reset_instances(self.h, p, w))

    def instance_ticks(self):
        """int32 [B]: the local step of every instance at the last update (dekf_get_instance_ticks): T, or T - T0 for an instance
        restarted before step T0; its window then holds min(ticks + 1, N) steps.  Frozen while an instance is paused (set_active)"""
        t = np.zeros(self.batch, np.int32)
        capi.check(self.lib.dekf_get_instance_ticks(self.h, C.c_void_p(t.ctypes.data), capi.DEKF_HOST))
        return t

    def set_active(self, mask):
        """pause the instances whose mask entry is 0 and resume those whose entry is 1 (dekf_set_active; a direct handle, between
        update(T - 1) and update(T)): a paused instance stands still, every getter keeps its bits, and it goes on where it stopped
        once it is resumed.  The call states the whole mask.  mask: int32 [B], numpy or a torch CUDA tensor (which must be complete on
        its stream)"""
        p, w = _ptr_where(mask, np.int32)
        capi.check(self.lib.dekf_set_active(self.h, p, w))

    def active(self):
        """int32 [B]: 1 for an instance that runs, 0 for a paused one (dekf_get_active)"""
        a = np.zeros(self.batch, np.int32)
        capi.check(self.lib.dekf_get_active(self.h, C.c_void_p(a.ctypes.data), capi.DEKF_HOST))
        return a

    def set_instance_params(self, sets, set_of):
        """noise parameters per instance of a direct handle (dekf_set_instance_params): sets, a sequence of DekfParams that differ from
        the handle's in noise fields only; set_of, B ints: instance b takes sets[set_of[b]], -1 leaves it as it is.  Before the first
        tick (or right after reset()) for any instance, later only for instances that reset_instances has just restarted.
        sets=None (or empty) with set_of=None drops the table"""
        if not sets and set_of is None:
            capi.check(self.lib.dekf_set_instance_params(self.h, None, 0, None))
            return
        arr = (DekfParams * len(sets))(*[s.copy() for s in sets])
        so = np.ascontiguousarray(set_of, np.int32)
        assert so.shape == (self.batch,), so.shape
        capi.check(self.lib.dekf_set_instance_params(self.h, C.cast(arr, C.c_void_p), len(sets), C.c_void_p(so.ctypes.data)))

    def instance_params(self, b):
        """the handle's parameters with instance b's noise fields (dekf_get_instance_params)"""
        out = DekfParams()
        capi.check(self.lib.dekf_get_instance_params(self.h, int(b), C.byref(out)))
        return out

    def snapshot_bytes(self, n):
        """bytes of a blob of n instances of this handle (dekf_snapshot_bytes); 0 on a handle that cannot save"""
        return int(self.lib.dekf_snapshot_bytes(self.h, int(n)))

    def save_instances(self, idx, device=False):
        """the instances `idx` (a sequence of distinct ints) as one opaque blob (dekf_save_instances; a direct handle, between
        update(T - 1) and update(T)): a uint8 numpy array, or with device=True a uint8 torch CUDA tensor written by the GPU alone.
        Saving changes nothing on the handle.  The blob loads into any slots of any handle with the same parameters outside the noise
        fields and the same settings (load_instances): a checkpoint, a migration to another batch, GPU or rank, or a fork"""
        ix = np.ascontiguousarray(idx, np.int32)
        nbytes = max(self.snapshot_bytes(len(ix)), 1)
        if device:
            import torch
            blob = torch.empty(nbytes, dtype=torch.uint8, device=f"cuda:{self.device}")
            torch.cuda.synchronize()
            ptr, where = C.c_void_p(blob.data_ptr()), capi.DEKF_DEVICE
        else:
            blob = np.zeros(nbytes, np.uint8)
            ptr, where = C.c_void_p(blob.ctypes.data), capi.DEKF_HOST
        capi.check(self.lib.dekf_save_instances(self.h, C.c_void_p(ix.ctypes.data), len(ix), ptr, nbytes, where))
        return blob

    def load_instances(self, idx, blob):
        """make instance idx[i] the i-th saved instance of `blob` (dekf_load_instances; uint8, numpy or a torch CUDA tensor that is
        complete on its stream): it is active and goes on, bit for bit, as its source would have.  Push IMU and leg samples before its
        next tick or update.  A blob of another configuration, or noise fields that are not the slot's, are refused and nothing is
        applied"""
        ix = np.ascontiguousarray(idx, np.int32)
        if isinstance(blob, np.ndarray):
            assert blob.dtype == np.uint8 and blob.flags["C_CONTIGUOUS"]
            ptr, where, nbytes = C.c_void_p(blob.ctypes.data), capi.DEKF_HOST, blob.nbytes
        else:
            import torch
            assert isinstance(blob, torch.Tensor) and blob.dtype == torch.uint8 and blob.is_contiguous()
            ptr, where, nbytes = C.c_void_p(blob.data_ptr()), (capi.DEKF_DEVICE if blob.is_cuda else capi.DEKF_HOST), blob.numel()
        capi.check(self.lib.dekf_load_instances(self.h, C.c_void_p(ix.ctypes.data), len(ix), ptr, nbytes, where))

    def sync(self):
        capi.check(self.lib.dekf_sync(self.h))

    # ---- results ---------------------------------------------------------------------
    def get(self):
        B = self.batch
        out = dict(x=np.zeros((B, self.params.dim_state)), v_b=np.zeros((B, 3)), quat=np.zeros((B, 4)), p_vo=np.zeros((B, 3)),
                   status=np.zeros(B, np.int32))
        capi.check(self.lib.dekf_get(self.h, *[C.c_void_p(out[k].ctypes.data) for k in ("x", "v_b", "quat", "p_vo", "status")],
                                     capi.DEKF_HOST))
        return out

    def get_into(self, x=None, v_b=None, quat=None, p_vo=None, status=None):
        """device-to-device copies into caller-owned torch CUDA tensors (asynchronous)"""
        ptrs = []
        for a, dt in ((x, np.float64), (v_b, np.float64), (quat, np.float64), (p_vo, np.float64), (status, np.int32)):
            p, w = _ptr_where(a, dt)
            assert a is None or w == capi.DEKF_DEVICE
            ptrs.append(p)
        capi.check(self.lib.dekf_get(self.h, *ptrs, capi.DEKF_DEVICE))

    def solver_info(self):
        B = self.batch
        out = dict(iters=np.zeros(B, np.int32), rho_updates=np.zeros(B, np.int32), pri_res=np.zeros(B), dua_res=np.zeros(B))
        capi.check(self.lib.dekf_get_solver_info(self.h, *[C.c_void_p(out[k].ctypes.data) for k in ("iters", "rho_updates", "pri_res", "dua_res")],
                                                 capi.DEKF_HOST))
        out["polish_status"] = np.zeros(B, np.int32)
        capi.check(self.lib.dekf_get_polish_status(self.h, C.c_void_p(out["polish_status"].ctypes.data), capi.DEKF_HOST))
        return out

    def warm_status(self):
        """per instance: 1 if the last update's solve started from the shifted previous solution, 0 if it started cold"""
        w = np.zeros(self.batch, np.int32)
        capi.check(self.lib.dekf_get_warm_status(self.h, C.c_void_p(w.ctypes.data), capi.DEKF_HOST))
        return w

    def ekf_cov(self):
        P = np.zeros((self.batch, 4, 4))
        capi.check(self.lib.dekf_get_ekf_cov(self.h, C.c_void_p(P.ctypes.data), capi.DEKF_HOST))
        return P

    def mhe_cov(self):
        """Cov(x_T) [B, ns, ns] of the last update of a direct handle (dekf_get_mhe_cov)"""
        ns = self.params.dim_state
        Cm = np.zeros((self.batch, ns, ns))
        capi.check(self.lib.dekf_get_mhe_cov(self.h, C.c_void_p(Cm.ctypes.data), capi.DEKF_HOST))
        return Cm

    def window(self):
        """(K, x_win [B, K, ns], cov_win [B, K, ns, ns]) of the last update of a smoothing handle (dekf_get_window): the K = min(T + 1, N)
        states of the window it solved, oldest first, and their covariances.  After reset_instances K is the largest window of the
        batch and instance b's first min(instance_ticks()[b] + 1, N) entries are its window"""
        ns, N = self.params.dim_state, self.params.N
        xw, cw = np.zeros((self.batch, N, ns)), np.zeros((self.batch, N, ns, ns))
        K = C.c_int(0)
        capi.check(self.lib.dekf_get_window(self.h, C.byref(K), C.c_void_p(xw.ctypes.data), C.c_void_p(cw.ctypes.data), capi.DEKF_HOST))
        return K.value, xw[:, :K.value].copy(), cw[:, :K.value].copy()

    def window_cross(self):
        """(K, lag1 [B, K - 1, ns, ns], newest [B, K, ns, ns]) of the last update of a cross handle (dekf_get_window_cross):
        lag1[b, k] = Cov(x_k, x_{k+1}) and newest[b, k] = Cov(x_k, x_T) of the window's K states, rows indexing x_k (see relative_cov)"""
        ns, N = self.params.dim_state, self.params.N
        l1, zn = np.zeros((self.batch, N - 1, ns, ns)), np.zeros((self.batch, N, ns, ns))
        K = C.c_int(0)
        capi.check(self.lib.dekf_get_window_cross(self.h, C.byref(K), C.c_void_p(l1.ctypes.data), C.c_void_p(zn.ctypes.data), capi.DEKF_HOST))
        return K.value, l1[:, :K.value - 1].copy(), zn[:, :K.value].copy()

    def innovation(self):
        """the innovation statistics of the last update of an innovation handle (dekf_get_innovation), a dict: innov [B, nm] = y - H x^-,
        innov_cov [B, nm, nm] = S, nis [B], nis_leg [B, L] and loglik [B] = log p(y_T | the rest of the window), nm = 3 num_legs.  NaN for
        an instance whose solve failed or that has not solved since its restart.  Summed over a log, loglik is the score of the
        instance's noise set; nis_leg is chi-square with 3 degrees of freedom on a consistent estimator"""
        B, L = self.batch, self.params.num_legs
        out = dict(innov=np.zeros((B, 3 * L)), innov_cov=np.zeros((B, 3 * L, 3 * L)), nis=np.zeros(B), nis_leg=np.zeros((B, L)), loglik=np.zeros(B))
        capi.check(self.lib.dekf_get_innovation(self.h, *[C.c_void_p(out[k].ctypes.data) for k in ("innov", "innov_cov", "nis", "nis_leg", "loglik")],
                                                capi.DEKF_HOST))
        return out

    def innovation_gate(self):
        """(nis_leg_max, gated [B, L]) of a gating handle (dekf_get_innovation_gate): the bound, and 1 for the legs the last update took
        out of the solve because their nis_leg exceeded it"""
        gated = np.zeros((self.batch, self.params.num_legs), dtype=np.int32)
        bound = C.c_double(0.0)
        capi.check(self.lib.dekf_get_innovation_gate(self.h, C.byref(bound), C.c_void_p(gated.ctypes.data), capi.DEKF_HOST))
        return bound.value, gated

    def set_gate_smoother(self, on):
        """switch the window of a gating handle on or off (dekf_set_gate_smoother; before initialize() or right after reset())"""
        capi.check(self.lib.dekf_set_gate_smoother(self.h, int(on)))

    def kf_cov(self):
        ns = self.params.dim_state
        Cm = np.zeros((self.batch, ns, ns))
        capi.check(self.lib.dekf_get_kf_cov(self.h, C.c_void_p(Cm.ctypes.data), capi.DEKF_HOST))
        return Cm

    # ---- measurement ------------------------------------------------------------------
    def timing_enable(self, on=True):
        """True / 1: HIP events around every kernel launch; 2: around the MHE solve launches only (an event pair costs the stream ~7 us)"""
        capi.check(self.lib.dekf_timing_enable(self.h, int(on)))

    def timing_read(self):
        """{'ekf'|'assemble'|'solve'|'allgather': (device ms summed, launches)} since the last read"""
        ms = (C.c_double * 4)()
        cnt = (C.c_int * 4)()
        capi.check(self.lib.dekf_timing_read(self.h, ms, cnt))
        return {k: (ms[i], cnt[i]) for i, k in enumerate(("ekf", "assemble", "solve", "allgather"))}

    def launch_info(self):
        """{'solve_workgroups', 'compute_units', 'clock_hz'} of the solve kernel's launch on this device"""
        wg, cu, hz = C.c_int(), C.c_int(), C.c_double()
        capi.check(self.lib.dekf_launch_info(self.h, C.byref(wg), C.byref(cu), C.byref(hz)))
        return dict(solve_workgroups=wg.value, compute_units=cu.value, clock_hz=hz.value)

    def solve_kernel_name(self, full_window=True):
        """symbol of the solve kernel this handle launches (full windows / window-fill ticks); None for a KF handle"""
        n = self.lib.dekf_solve_kernel_name(self.h, int(bool(full_window)))
        return n.decode() if n else None

    # ---- multi-GPU --------------------------------------------------------------------
    def comm_init(self, world, rank, unique_id: bytes):
        buf = C.create_string_buffer(unique_id, capi.DEKF_UNIQUE_ID_BYTES)
        capi.check(self.lib.dekf_comm_init(self.h, world, rank, buf))

    def comm_info(self):
        """(world, rank) as the RCCL communicator itself reports them (ncclCommCount / ncclCommUserRank)"""
        w, r = C.c_int(0), C.c_int(-1)
        capi.check(self.lib.dekf_comm_info(self.h, C.byref(w), C.byref(r)))
        return w.value, r.value

    def comm_ranks_seen(self):
        """collective: all-gathers every rank's number through the handle's communicator and stream; distinct rank numbers that arrived"""
        n = C.c_int(0)
        capi.check(self.lib.dekf_comm_ranks_seen(self.h, C.byref(n)))
        return n.value

    def allgather_vb(self, out_tensor):
        """asynchronous (own stream, overlaps the next step); complete after sync() or allgather_wait()"""
        capi.check(self.lib.dekf_allgather_vb(self.h, C.c_void_p(out_tensor.data_ptr())))

    def allgather_wait(self):
        """the estimator's stream waits for the last all-gather (no host block)"""
        capi.check(self.lib.dekf_allgather_wait(self.h))


def new_unique_id() -> bytes:
    _torch_runtime_first()
    buf = C.create_string_buffer(capi.DEKF_UNIQUE_ID_BYTES)
    capi.check(capi.load().dekf_comm_unique_id(buf))
    return buf.raw


def streams_to_device(s, device="cuda"):
    """upload a streams dict once so the timed loop only hands device pointers over"""
    import torch
    out = {}
    for k, v in s.items():
        if isinstance(v, np.ndarray) and not k.startswith("gt_"):
            out[k] = torch.from_numpy(v).to(device)
    out["vo_any"] = [bool(m.any()) for m in s["vo_mask"]]
    return out


def streams_host(s):
    out = dict(s)
    out["vo_any"] = [bool(m.any()) for m in s["vo_mask"]]
    return out
