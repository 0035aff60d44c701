"""Snapshots of single instances of a direct handle on the GPU (dekf_snapshot_bytes, dekf_save_instances, dekf_load_instances;
BatchedEstimator.save_instances / load_instances): a saved instance loaded into another slot of another handle, at another step, goes
on as its source does on an uninterrupted handle, on every getter, to the bit; instances not named and the source itself keep every
bit.  Migration through a host blob, a fork through a device blob, sources in every state, other shapes, the innovation and gate
stores, a parameter table, what is refused."""
import ctypes as C

import numpy as np
import pytest

import direct_lib as DL
import epoch_lib as EL
import gate_lib as GL
import innov_lib as IL
import instance_params_lib as PL
import pause_lib as PZ
import snapshot_lib as SL
import tworate_lib as TL
from decentralized_ekf_mhe_amd import capi, go1_params
from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host

pytestmark = pytest.mark.gpu

D0 = 3            # a destination stands before its own tick 3
KEYS = PZ.GPU_KEYS


def migrate(name, variant, T0, after, moves, B_dst, blob_device=False):
    """the shape's source handle runs its log to tick T0 + after and saves the sources of `moves` before tick T0; a destination of B_dst
    instances loads them before its tick D0.  Checks everything test 1 of the issue lists; returns the destination's records"""
    mk, B, K, kernel = EL.GPU_SHAPES[name]
    p, s = EL.gpu_streams(name)
    assert T0 + after <= K
    sibling, twin = kernel + EL.SIBLING_SUFFIX[variant], kernel + EL.TWIN_SUFFIX[variant]
    ref = PZ.gpu_fresh(name, variant, tuple(range(K)))          # a fresh uninterrupted run of the whole log
    src = BatchedEstimator(p, B, solver="direct", **DL.VARIANTS[variant])
    blobs = []
    got_src = SL.gpu_ticks(src, streams_host(s), range(T0 + after), variant, [],
                           {T0: lambda est: blobs.append(est.save_instances([b for b, _ in moves], device=blob_device))})
    assert SL.gpu_names(src) == (sibling, sibling)
    src.close()
    for b in range(B):                                          # the source after the save is the source without it
        PZ.assert_cut_life_equal(got_src, ref, b, tuple(range(T0 + after)), p.N, KEYS, ("source", name, variant))
    s_own = DL.rough_streams(p, B_dst, D0 + after, seed_shift=11)
    plain = EL.run_gpu(p, s_own, B_dst, D0 + after, variant)[0]
    dst = BatchedEstimator(p, B_dst, solver="direct", **DL.VARIANTS[variant])
    sh = streams_host(SL.migrated_streams(s_own, D0, s, T0, moves, after))
    got = SL.gpu_ticks(dst, sh, range(D0), variant, [])
    assert SL.gpu_names(dst) == (sibling, sibling)
    dst.load_instances([d for _, d in moves], blobs[0])
    assert SL.gpu_names(dst) == (twin, twin)
    at_load = PZ.gpu_record(dst, D0 - 1, variant)               # right after the load: the source's getters of its tick T0 - 1
    SL.assert_moved_equal({D0 - 1: at_load}, D0 - 1, ref, T0 - 1, moves, 1, p.N, KEYS, ("at the load", name, variant))
    SL.gpu_ticks(dst, sh, range(D0, D0 + after), variant, got)
    assert SL.gpu_names(dst) == (twin, twin)
    dst.close()
    SL.assert_moved_equal(got, D0, ref, T0, moves, after, p.N, KEYS, ("after the load", name, variant))
    others = [d for d in range(B_dst) if d not in [m[1] for m in moves]]
    for d in others:
        PZ.assert_cut_life_equal(got, plain, d, tuple(range(D0 + after)), p.N, KEYS, ("slots not named", name, variant))
    return got


# ------------------------------------------------------------------ 1. migration
@pytest.mark.parametrize("variant", list(DL.VARIANTS))
def test_migration_through_a_host_blob(variant):
    """Go1, B = 6 to tick 45 (full windows with VO rows), instances {1, 3} into slots {2, 0} of a handle of 4 at its step 3, 40 ticks"""
    got = migrate("go1", variant, 45, 40, [(1, 2), (3, 0)], 4)
    assert got[-1]["ticks"].tolist() == [84, D0 + 39, 84, D0 + 39]


# ------------------------------------------------------------------ 2. a fork on one handle, through a device blob
def test_fork_on_one_handle_through_a_device_blob():
    name, variant, T0, after = "go1", "cross", 25, 40
    mk, B, K, kernel = EL.GPU_SHAPES[name]
    p, s = EL.gpu_streams(name)
    ref = PZ.gpu_fresh(name, variant, tuple(range(K)))
    est = BatchedEstimator(p, B, solver="direct", **DL.VARIANTS[variant])
    sh = streams_host(SL.migrated_streams(s, T0, s, T0, [(1, 4)], after))   # from tick 25 on instance 4 is fed instance 1's samples

    def fork(e):
        blob = e.save_instances([1], device=True)
        assert blob.is_cuda and blob.numel() == e.snapshot_bytes(1)
        e.load_instances([4], blob)

    got = SL.gpu_ticks(est, sh, range(T0 + after), variant, [], {T0: fork})
    est.close()
    SL.assert_moved_equal(got, T0, ref, T0, [(1, 4)], after, p.N, KEYS, "the fork")
    for b in (0, 1, 2, 3, 5):
        PZ.assert_cut_life_equal(got, ref, b, tuple(range(T0 + after)), p.N, KEYS, "beside the fork")


# ------------------------------------------------------------------ 3. sources in every state, on a two-rate handle
def test_sources_in_every_state_from_a_two_rate_handle():
    """EKF 500 Hz, MHE 200 Hz on tworate_lib's grid.  Before ms 127, between the EKF ticks of ms 126 and 128 in the gap of the updates
    of ms 125 and 130, one handle saves: instance 0, restarted before ms 101 and inside its window fill (its next local step is 5);
    instance 1, paused since ms 63; instance 2, restarted in this very gap (local tick -1: its first update after the load is its
    dekf_initialize); instance 3, which just runs.  A handle of four that stands before its ms 17 loads them and is driven over the
    source's grid from ms 127 on.  Each then equals a fresh handle driven over the grid cut down to the ms the instance lived"""
    name, H, B, variant, G = "go1", 256, 6, "cross", 127
    p, s, n_grid = TL.streams(name, H, B)
    made = []

    def dev(batch):
        made.append(TL.GpuDev(BatchedEstimator(p, batch, solver="direct", **DL.VARIANTS[variant]), variant))
        return made[-1]

    def one(b):
        m = np.zeros(B, np.int32)
        m[b] = 1
        return m

    blobs = []
    moves = [(0, 3), (1, 0), (2, 1), (3, 2)]
    try:
        pokes = {63: lambda d: d.est.set_active(1 - one(1)), 101: lambda d: d.restart([0]),
                 G: lambda d: (d.restart([2]), blobs.append(d.est.save_instances([b for b, _ in moves])))}
        PZ.drive_ms(dev(B), s, range(G + 1), pokes)
        hb = made[0].est.snapshot_bytes(1) - (made[0].est.snapshot_bytes(2) - made[0].est.snapshot_bytes(1))
        rb = made[0].est.snapshot_bytes(2) - made[0].est.snapshot_bytes(1)
        # local step | local EKF count: ms 101 .. 126 hold 5 updates and 13 ticks; ms 0 .. 62 hold 13 and 32; ms 0 .. 126 hold 26 and 64
        assert SL.books_of(blobs[0], hb, rb, 4) == [(5, 13), (13, 32), (0, 0), (26, 64)]
        # the destination: its own first 17 ms (4 updates, 9 ticks), then the source's grid in the slots of the moves
        s_own = TL.streams(name, H, 4)[1]
        dst = dev(4)
        got = PZ.drive_ms(dst, s_own, range(17))
        dst.est.load_instances([d for _, d in moves], blobs[0])
        assert dst.est.instance_ticks().tolist() == [12, -1, 25, 4] and dst.est.active().tolist() == [1, 1, 1, 1]
        s_run = SL.migrated_streams(s_own, 0, s, 0, moves, n_grid)   # (slot d carries instance b at every ms)
        for i in range(G, n_grid):
            if s_run["vo_mask"][i].any():
                dst.vo(s_run, i)
            if i % 2 == 0:
                dst.sensors(s_run, i)
                dst.ekf_step()
            if i % 5 == 0:
                dst.timer(len(got))
                got.append(dst.record(len(got)))
        lived = {0: range(101, n_grid), 1: [i for i in range(n_grid) if not 63 <= i < G], 2: range(G, n_grid), 3: range(n_grid)}
        for b, d in moves:
            fresh = TL.gpu_fresh(name, H, B, variant) if b == 3 else PZ.drive_ms(dev(B), s, lived[b])
            before = len([i for i in lived[b] if i < G and i % 5 == 0])   # the life's updates before the save
            SL.assert_moved_equal(got, 4, fresh, before, [(b, d)], len(got) - 4, p.N, KEYS, ("two rates", b), first=0)
    finally:
        for d in made:
            d.est.close()


# ------------------------------------------------------------------ 4. other shapes
@pytest.mark.parametrize("name,B_dst,moves", [("tripod", 3, [(1, 2), (4, 0)]), ("go1_foot", 3, [(1, 2), (3, 0)])])
def test_other_shapes(name, B_dst, moves):
    """the generic run-time-K kernel (tripod, N = 12) and ns = 21 (Go1 with foot states, B = 4), 60 ticks, variant cross"""
    migrate(name, "cross", 25, 35, moves, B_dst)


# ------------------------------------------------------------------ 5. the innovation and gate stores
def test_innovation_and_gate_stores_travel_behind_a_gated_update():
    """gate_lib's Go1 log at its high gate: the slips of (tick 26, instance 1, legs 0 and 3) fire; instances {1, 0} are saved behind
    that update and go on in another gating handle, through the slips of ticks 33, 44 and 46"""
    p, B, K, _, s = GL.case_streams("go1", gpu=True)
    gate, T0, moves = GL.CASES["go1"][1], 27, [(1, 2), (0, 0)]
    blobs = []
    ref, names, _ = GL.run_gpu(p, s, B, K, gate, after=lambda k, est: blobs.append(est.save_instances([1, 0])) if k == T0 - 1 else None)
    assert ref[T0 - 2]["gated"][1].tolist() == [1, 0, 0, 1] and len(blobs) == 1
    s_own = DL.rough_streams(p, 3, D0 + K - T0, seed_shift=11)
    sh = streams_host(SL.migrated_streams(s_own, D0, s, T0, moves, K - T0))
    dst = BatchedEstimator(p, 3, solver="direct", innovation=True, innovation_gate=gate)

    def record():
        r = IL.gpu_record(dst)
        r.update(dst.innovation())
        r["gated"], r["ticks"] = dst.innovation_gate()[1], dst.instance_ticks()
        return r

    for k in range(D0):
        dst.push_stream_step(sh, k)
        dst.step(k)
    dst.load_instances([d for _, d in moves], blobs[0])
    got = [record()]
    for k in range(D0, D0 + K - T0):
        dst.push_stream_step(sh, k)
        dst.step(k)
        got.append(record())
    dst.close()
    fired = 0
    for j, g in enumerate(got):                       # got[j]: the source's tick T0 - 1 + j, which is ref[T0 - 2 + j]
        f = ref[T0 - 2 + j]
        for b, d in moves:
            for key in ("x", "v_b", "status", "iters", "cov", "gated") + IL.KEYS:
                assert np.array_equal(g[key][d], f[key][b], equal_nan=True), (j, b, key)
            assert g["ticks"][d] == T0 - 1 + j
            fired += int(j > 0 and f["gated"][b].any())
    assert got[0]["gated"][2].tolist() == [1, 0, 0, 1] and fired >= 3


# ------------------------------------------------------------------ 6. a parameter table
def test_parameter_table_a_record_loads_into_a_slot_on_its_set_only():
    mk, B, set_of, kernel = PL.GPU_SHAPES["go1"]     # set_of = [0, 1, 2, 2, 0, 1]
    p, s = PL.gpu_streams("go1")
    variant, T0, after, b = "cross", 25, PL.K_LOG - 25, 1
    sets = PL.param_sets(p)
    src = BatchedEstimator(p, B, solver="direct", **DL.VARIANTS[variant])
    src.set_instance_params(sets, set_of)
    SL.gpu_ticks(src, streams_host(s), range(T0), variant, [])
    blob = src.save_instances([b])
    src.close()
    # the destination: a handle with a table in which every slot is on set 0; slot 2 is given set 1 by the restart route
    s_own = DL.rough_streams(p, 4, D0 + after, seed_shift=11)
    sh = streams_host(SL.migrated_streams(s_own, D0, s, T0, [(b, 2)], after))
    dst = BatchedEstimator(p, 4, solver="direct", **DL.VARIANTS[variant])
    dst.set_instance_params(sets, [0, 0, 0, 0])
    got = SL.gpu_ticks(dst, sh, range(D0), variant, [])
    lib = capi.load()
    ix = np.array([2], np.int32)
    refused = lib.dekf_load_instances(dst.h, C.c_void_p(ix.ctypes.data), 1, C.c_void_p(blob.ctypes.data), blob.nbytes, capi.DEKF_HOST)
    assert refused == capi.DEKF_ERR_INVALID and dst.instance_ticks().tolist() == [D0 - 1] * 4     # slot 2 is on set 0
    dst.reset_instances(np.array([0, 0, 1, 0], np.int32))
    dst.set_instance_params(sets, [-1, -1, 1, -1])
    dst.load_instances([2], blob)
    assert SL.gpu_names(dst) == (kernel + PL.TWIN_SUFFIX[variant],) * 2
    SL.gpu_ticks(dst, sh, range(D0, D0 + after), variant, got)
    dst.close()
    SL.assert_moved_equal(got, D0, PL.gpu_uniform("go1", variant, 1), T0, [(b, 2)], after, p.N, KEYS, "set 1")
    # the refused load applied nothing: the other slots are a uniform set-0 handle on their own log
    plain = EL.run_gpu(p, s_own, 4, D0 + after, variant)[0]
    for d in (0, 1, 3):
        PZ.assert_cut_life_equal(got, plain, d, tuple(range(D0 + after)), p.N, KEYS, "beside")


# ------------------------------------------------------------------ 7. what is refused, 8. host and device blobs
def test_errors_and_host_and_device_blobs_hold_the_same_bytes():
    import torch
    lib = capi.load()
    p = DL._params(go1_params)
    B, K = 4, 8
    s = DL.rough_streams(p, B, K)
    sh = streams_host(s)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    ix = np.array([2, 0], np.int32)
    scratch = np.zeros(1 << 20, np.uint8)

    def started(est, ticks=range(3)):
        for k in ticks:
            est.push_stream_step(sh, k)
            est.step(k)
        return est

    def save(est, idx, n, blob, nbytes):
        return lib.dekf_save_instances(est.h, None if idx is None else ptr(idx), n, None if blob is None else ptr(blob), nbytes, capi.DEKF_HOST)

    def load(est, idx, n, blob, nbytes):
        return lib.dekf_load_instances(est.h, None if idx is None else ptr(idx), n, None if blob is None else ptr(blob), nbytes, capi.DEKF_HOST)

    # ADMM, KF and pipelined handles cannot save: no bytes, both calls refused
    for est in (BatchedEstimator(p, B), BatchedEstimator(DL._params(go1_params, est_type=1), B),
                BatchedEstimator(DL._params(go1_params, solve_pipeline=1), B)):
        started(est)
        assert lib.dekf_snapshot_bytes(est.h, 2) == 0
        assert save(est, ix, 2, scratch, scratch.nbytes) == capi.DEKF_ERR_INVALID
        assert load(est, ix, 2, scratch, scratch.nbytes) == capi.DEKF_ERR_INVALID
        est.close()
    assert lib.dekf_snapshot_bytes(None, 2) == 0
    assert lib.dekf_save_instances(None, ptr(ix), 2, ptr(scratch), scratch.nbytes, capi.DEKF_HOST) == capi.DEKF_ERR_INVALID
    assert lib.dekf_load_instances(None, ptr(ix), 2, ptr(scratch), scratch.nbytes, capi.DEKF_HOST) == capi.DEKF_ERR_INVALID
    est = BatchedEstimator(p, B, solver="direct")
    n2 = est.snapshot_bytes(2)
    assert 0 < n2 <= scratch.nbytes and est.snapshot_bytes(0) == 0 and est.snapshot_bytes(3) - n2 == n2 - est.snapshot_bytes(1) > 0
    assert save(est, ix, 2, scratch, n2) == capi.DEKF_ERR_ORDER and load(est, ix, 2, scratch, n2) == capi.DEKF_ERR_ORDER   # before dekf_initialize
    started(est)
    blob = est.save_instances(ix)
    assert blob.nbytes == n2
    # 8. the device blob of the same call holds the same bytes
    assert np.array_equal(SL.blob_bytes(est.save_instances(ix, device=True)), blob)
    plain = EL.run_gpu(p, s, B, K, "plain")[0]

    def refused(call, *a):
        assert call(est, *a) == capi.DEKF_ERR_INVALID, a[:2]

    canary = np.full(n2, 0xA5, np.uint8)
    for idx, n, b, nb in ((None, 2, canary, n2), (ix, 2, None, n2), (ix, 0, canary, n2), (ix, -1, canary, n2),
                          (np.array([2, B], np.int32), 2, canary, n2), (np.array([-1, 2], np.int32), 2, canary, n2),
                          (np.array([1, 1], np.int32), 2, canary, n2), (ix, 2, canary, n2 - 1)):
        refused(save, idx, n, b, nb)
        assert (canary == 0xA5).all()                                    # nothing written
        refused(load, idx, n, None if b is None else blob, nb)
    # blobs of other handles: another N, a smoothing handle; a corrupted magic, version, n
    for other in (BatchedEstimator(DL._params(go1_params, N=12), B, solver="direct"), BatchedEstimator(p, B, solver="direct", smoother=True)):
        foreign = started(other).save_instances(ix)
        other.close()
        refused(load, ix, 2, foreign, foreign.nbytes)
        refused(load, ix, 2, np.concatenate([foreign, scratch[:n2]]), foreign.nbytes + n2)
    for at in (0, 8, 12):
        bad = blob.copy()
        bad[at] ^= 1
        refused(load, ix, 2, bad, n2)
    dev_bad = torch.from_numpy(bad).cuda()
    torch.cuda.synchronize()
    assert lib.dekf_load_instances(est.h, ptr(ix), 2, C.c_void_p(dev_bad.data_ptr()), n2, capi.DEKF_DEVICE) == capi.DEKF_ERR_INVALID
    assert est.solve_kernel_name() == "k_mhe_solve_direct_4_n20"          # no refused load changed what the handle launches
    # after every refused call the following steps give the bits of the run without the calls
    got = SL.gpu_ticks(est, sh, range(3, K), "plain", [None] * 3)
    est.close()
    SL.assert_slots_equal(got, plain, range(B), range(3, K), p.N, KEYS + ("ticks",), "after the refused calls")
