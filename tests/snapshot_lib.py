"""What the instance-snapshot tests share (test_instance_snapshot.py, test_gpu_instance_snapshot.py): the lane-sequential harness with
snapshots (tests/hostsim/snapshot_hostsim.cpp), the streams of a destination that carries migrated instances, and the comparisons.

A move is (source instance, destination slot).  The source handle runs a log; before its tick T0 some instances are saved; a
destination handle that stands before its own tick D0 loads them into the slots of the moves and is fed, at its tick D0 + j, the
source's samples of tick T0 + j in those slots.  Slot of the destination at tick D0 + j must then equal the source instance of an
uninterrupted run at tick T0 + j, on every getter key, to the bit.
TEST INFRASTRUCTURE ONLY.  Importing this module does not touch the GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

import direct_lib as DL
import epoch_lib as EL
import hostsim_lib as HL
import pause_lib as PL

LIB = os.path.join(DL.HOSTSIM, "libsnapshot_hostsim.so")
_libs = {}


class Stores(C.Structure):
    _fields_ = [("cov", HL._dp), ("xw", HL._dp), ("cw", HL._dp), ("l1", HL._dp), ("zn", HL._dp), ("smoother", C.c_int), ("cross", C.c_int)]


def snapshot_hostsim():
    """tests/hostsim/snapshot_hostsim.cpp as libsnapshot_hostsim.so, rebuilt when a source is newer, and bound"""
    if "lib" not in _libs:
        srcs = [os.path.join(DL.HOSTSIM, f) for f in os.listdir(DL.HOSTSIM) if f.endswith(".cpp")] + \
            [os.path.join(DL.CSRC, f) for f in os.listdir(DL.CSRC) if f.endswith(".h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in srcs):
            subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-DDEKF_HOSTSIM", "-w", "-O2", "-o", LIB,
                                   os.path.join(DL.HOSTSIM, "snapshot_hostsim.cpp")])
        L = HL._bind(C.CDLL(LIB))
        vp, dp, ip = C.c_void_p, HL._dp, HL._ip
        # (the pause harness underneath, as pause_lib binds it)
        L.hs_epochs_create.restype = vp
        L.hs_epochs_create.argtypes = [C.c_int]
        L.hs_epochs_destroy.argtypes = [vp]
        L.hs_epochs_copy.argtypes = [vp, ip, ip]
        L.hs_pauses_create.restype = vp
        L.hs_pauses_create.argtypes = [C.c_int]
        L.hs_pauses_destroy.argtypes = [vp]
        L.hs_set_active.restype = C.c_int
        L.hs_set_active.argtypes = [vp, vp, vp, ip]
        L.hs_get_active.argtypes = [vp, ip]
        L.hs_reset_instances_pause.argtypes = [vp, vp, vp, ip, dp]
        L.hs_push_vo_pause.argtypes = [vp, vp, ip, dp, dp, dp, dp, dp]
        L.hs_ekf_step_pause.argtypes = [vp, vp]
        L.hs_instance_ticks_pause.argtypes = [vp, vp, C.c_int, ip]
        L.hs_update_direct_pause.argtypes = [vp, vp, C.c_int, dp]
        L.hs_update_direct_smooth_pause.argtypes = [vp, vp, C.c_int, dp, dp, dp]
        L.hs_update_direct_cross_pause.argtypes = [vp, vp, C.c_int, dp, dp, dp, dp, dp]
        ll = C.c_longlong
        pp, sp, bp = C.POINTER(DL.DekfParams), C.POINTER(Stores), C.POINTER(C.c_ubyte)
        L.hs_snapshot_map_bytes.argtypes = [pp, C.c_int, C.POINTER(ll)]
        L.hs_snapshot_header_bytes.restype = ll
        L.hs_snapshot_books_bytes.restype = ll
        L.hs_snapshot_record_bytes.restype = ll
        L.hs_snapshot_record_bytes.argtypes = [vp, sp]
        L.hs_save_instances.restype = C.c_int
        L.hs_save_instances.argtypes = [vp, vp, vp, pp, sp, ip, C.c_int, bp, ll]
        L.hs_load_instances.restype = C.c_int
        L.hs_load_instances.argtypes = [vp, vp, vp, pp, sp, ip, C.c_int, bp, ll]
        L.hs_snapshot_arith.argtypes = [C.c_int] * 7 + [ip]
        _libs["lib"] = L
    return _libs["lib"]


def map_bytes(p, B):
    """(covered per instance, allocated by alloc_state, left out by name, entries) of the state map of a handle of B instances"""
    out = (C.c_longlong * 4)()
    snapshot_hostsim().hs_snapshot_map_bytes(C.byref(p), B, out)
    return tuple(int(v) for v in out)


def arith(t0, c0, next_T, count, H, next_T2, count2):
    """(step, count of the books, t0, c0 after the load, books valid) of the host's arithmetic alone"""
    out = np.zeros(5, np.int32)
    snapshot_hostsim().hs_snapshot_arith(t0, c0, next_T, count, H, next_T2, count2, HL._p(out))
    return tuple(int(v) for v in out)


class SnapSim(PL.PauseSim):
    """pause_lib.PauseSim on the snapshot harness, with save() and load().  The window stores exist from the start (a handle allocates
    them with the setting), so a sim that has not updated yet can take a record"""

    def __init__(self, params, batch, variant="plain"):
        assert variant in DL.VARIANTS
        self.p, self.B, self.L, self.variant = params, batch, snapshot_hostsim(), variant
        self.h = self.L.hs_create(C.byref(params), batch)
        assert self.h, "hs_create rejected the parameters"
        self.e = self.L.hs_epochs_create(batch)
        self.z = self.L.hs_pauses_create(batch)
        self.cov = np.full((batch, params.dim_state, params.dim_state), np.nan)
        self.win = {}
        ns, N, B = params.dim_state, params.N, batch
        if variant != "plain":
            self.win = dict(xw=np.full((B, N, ns), DL.FILL), cw=np.full((B, N, ns, ns), DL.FILL))
        if variant == "cross":
            self.win.update(l1=np.full((B, N - 1, ns, ns), DL.FILL), zn=np.full((B, N, ns, ns), DL.FILL))

    def stores(self):
        w = self.win
        return Stores(HL._p(self.cov), HL._p(w.get("xw")), HL._p(w.get("cw")), HL._p(w.get("l1")), HL._p(w.get("zn")),
                      int(self.variant != "plain"), int(self.variant == "cross"))

    def header_bytes(self):
        return int(self.L.hs_snapshot_header_bytes())

    def record_bytes(self):
        return int(self.L.hs_snapshot_record_bytes(self.h, C.byref(self.stores())))

    def snapshot_bytes(self, n):
        return self.header_bytes() + n * self.record_bytes()

    def save(self, idx, nbytes=None):
        """(status, blob)"""
        ix = np.ascontiguousarray(idx, np.int32)
        blob = np.zeros(self.snapshot_bytes(len(ix)) if nbytes is None else nbytes, np.uint8)
        st = self.L.hs_save_instances(self.h, self.e, self.z, C.byref(self.p), C.byref(self.stores()), HL._p(ix), len(ix),
                                      blob.ctypes.data_as(C.POINTER(C.c_ubyte)), blob.nbytes)
        return st, blob

    def load(self, idx, blob):
        ix = np.ascontiguousarray(idx, np.int32)
        return self.L.hs_load_instances(self.h, self.e, self.z, C.byref(self.p), C.byref(self.stores()), HL._p(ix), len(ix),
                                        blob.ctypes.data_as(C.POINTER(C.c_ubyte)), blob.nbytes)


def books_of(blob, header_bytes, record_bytes, n):
    """[(step, count)] of the n records of a host blob"""
    return [tuple(int(v) for v in blob[header_bytes + i * record_bytes:header_bytes + i * record_bytes + 8].view(np.int32)) for i in range(n)]


def sim_record(sim, k):
    t0, c0 = sim.epochs()
    return dict(EL._record(sim, sim.cov), ticks=sim.ticks(k), active=sim.active(), t0=t0, c0=c0)


# ------------------------------------------------------------------ streams of a destination
def _per_tick(s):
    K, B = s["imu_t"].shape
    return [k for k, v in s.items() if isinstance(v, np.ndarray) and v.shape[:2] == (K, B)]


def migrated_streams(s_dst, D0, s_src, T0, moves, ticks):
    """the destination's own log up to its tick D0, then `ticks` more in which slot d of every move (b, d) carries instance b of the
    source's log from its tick T0 on; every other slot goes on with the destination's own log"""
    out = {}
    for key in _per_tick(s_dst):
        a = np.ascontiguousarray(s_dst[key][:D0 + ticks]).copy()
        for b, d in moves:
            a[D0:D0 + ticks, d] = s_src[key][T0:T0 + ticks, b]
        out[key] = a
    for key, v in s_dst.items():
        out.setdefault(key, v)
    out["vo_any"] = out["vo_mask"].any(axis=1)
    return out


def assert_moved_equal(got, D0, ref, T0, moves, ticks, N, keys, what, first=0):
    """slot d of `got` at its tick D0 + j against instance b of `ref` at tick T0 + j for every move (b, d) and j in first .. ticks - 1:
    array_equal on `keys`, the local tick, and the first K_b entries of the window arrays"""
    for j in range(first, ticks):
        g, f = got[D0 + j], ref[T0 + j]
        for b, d in moves:
            for key in keys:
                if key not in f or key not in g:
                    assert key == "cov" and T0 + j == 0, (what, key)
                    continue
                assert np.array_equal(g[key][d], f[key][b], equal_nan=True), (what, b, d, j, key)
            assert g["ticks"][d] == f["ticks"][b], (what, b, d, j, g["ticks"], f["ticks"])
            Kb = EL.local_K(int(f["ticks"][b]), N)
            for key in EL.WINDOW_KEYS:
                if key in f and Kb:
                    n = EL.window_lengths(key, Kb)
                    assert np.array_equal(g[key][d, :n], f[key][b, :n]), (what, b, d, j, key)


def assert_slots_equal(got, ref, slots, ticks, N, keys, what):
    """the slots `slots` of two runs of one handle shape at the ticks `ticks`: array_equal on keys and window entries"""
    for k in ticks:
        g, f = got[k], ref[k]
        for b in slots:
            for key in keys:
                if key in f or key in g:
                    assert np.array_equal(g[key][b], f[key][b], equal_nan=True), (what, b, k, key)
            Kb = EL.local_K(int(f["ticks"][b]), N)
            for key in EL.WINDOW_KEYS:
                if key in f and Kb:
                    n = EL.window_lengths(key, Kb)
                    assert np.array_equal(g[key][b, :n], f[key][b, :n]), (what, b, k, key)


# ------------------------------------------------------------------ the GPU runners
def gpu_ticks(est, sh, ticks, variant, out, hooks=None):
    """the ticks `ticks` of a streams dict on a direct handle, pause_lib.gpu_record appended to `out` after each; hooks[k](est) runs
    before the pushes of tick k"""
    for k in ticks:
        if hooks and k in hooks:
            hooks[k](est)
        est.push_stream_step(sh, k)
        est.step(k)
        out.append(PL.gpu_record(est, k, variant))
    return out


def gpu_names(est):
    return (est.solve_kernel_name(True), est.solve_kernel_name(False))


def blob_bytes(blob):
    """a host or device blob as a numpy uint8 array"""
    return blob if isinstance(blob, np.ndarray) else blob.cpu().numpy()
