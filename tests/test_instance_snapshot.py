"""dekf_save_instances / dekf_load_instances on the CPU: the state map, the copy loops and the host's books of
csrc/mhe_snapshot_core.h in the lane-sequential build (tests/hostsim/snapshot_hostsim.cpp).  Every comparison is array_equal."""
import functools

import numpy as np
import pytest

import direct_lib as DL
import pause_lib as PL
import snapshot_lib as SL
from decentralized_ekf_mhe_amd import go1_params, pogox_params

T0, D0, AFTER = 30, 3, 40          # the source is saved before its tick 30, the destination stands before its tick 3, 40 ticks follow
K_SRC = T0 + AFTER
B_SRC, B_DST = 6, 4


# ------------------------------------------------------------------ 1. the map is complete
@pytest.mark.parametrize("name,make", [("go1", lambda: DL._params(go1_params)), ("tripod", DL.tripod_params),
                                       ("go1_foot", lambda: DL._params(go1_params, leg_odom_type=1)),
                                       ("pogox", lambda: DL._params(pogox_params)), ("go1_kf", lambda: DL._params(go1_params, est_type=1))])
def test_the_state_map_covers_every_array_of_alloc_state_but_the_three_left_out_by_name(name, make):
    """bytes per instance of the map's entries, times B, plus gws, queue and prof, are what alloc_state allocates: a DevState array
    added later without a line in state_map fails here"""
    p = make()
    for B in (1, 3, 64):
        covered, allocated, excluded, entries = SL.map_bytes(p, B)
        assert entries == 44 and covered > 0
        assert B * covered + excluded == allocated, (name, B, covered, excluded, allocated)


# ------------------------------------------------------------------ 2. the round trip
@functools.lru_cache(maxsize=None)
def source(variant):
    """(p, streams, the uninterrupted run, the run with the saves, blob of every instance, blobs of the two moves)"""
    p = DL._params(go1_params)
    s = DL.rough_streams(p, B_SRC, K_SRC)
    ref = PL.run_pause_sim(p, s, B_SRC, K_SRC, variant, {})
    sim = SL.SnapSim(p, B_SRC, variant)
    got, blobs = [], None
    for k in range(K_SRC):
        if k == T0:
            blobs = [sim.save(ix) for ix in (range(B_SRC), [5, 0, 3, 2], [1, 4])]
        sim.feed(s, k)
        sim.step(k)
        got.append(SL.sim_record(sim, k))
    assert all(st == 0 for st, _ in blobs)
    return p, s, ref, got, [b for _, b in blobs], (sim.header_bytes(), sim.record_bytes())


def destination(p, variant, s_run, K):
    sim = SL.SnapSim(p, B_DST, variant)
    return sim, lambda k: (sim.feed(s_run, k), sim.step(k), SL.sim_record(sim, k))[2]


@pytest.mark.parametrize("variant", ["plain", "cross"])
def test_round_trip_into_a_smaller_younger_sim_in_permuted_slots(variant):
    p, s, ref, got_src, (blob_all, blob_a, blob_b), (hb, rb) = source(variant)
    keys = PL.SIM_KEYS
    # saving changed nothing on the source
    SL.assert_slots_equal(got_src, ref, range(B_SRC), range(K_SRC), p.N, keys, "the source after its saves")
    # a record does not depend on the blob it sits in
    for blob, ix in ((blob_a, [5, 0, 3, 2]), (blob_b, [1, 4])):
        for i, b in enumerate(ix):
            assert np.array_equal(blob[hb + i * rb:hb + (i + 1) * rb], blob_all[hb + b * rb:hb + (b + 1) * rb]), (ix, b)
    assert SL.books_of(blob_all, hb, rb, B_SRC) == [(T0, T0)] * B_SRC
    s_own = DL.rough_streams(p, B_DST, D0 + AFTER, seed_shift=11)
    plain_dst = PL.run_pause_sim(p, s_own, B_DST, D0 + AFTER, variant, {})
    for blob, moves in ((blob_a, [(5, 2), (0, 0), (3, 3), (2, 1)]), (blob_b, [(1, 3), (4, 0)])):
        s_run = SL.migrated_streams(s_own, D0, s, T0, moves, AFTER)
        sim, tick = destination(p, variant, s_run, D0 + AFTER)
        got = [tick(k) for k in range(D0)]
        assert sim.load([d for _, d in moves], blob) == 0
        # right after the load the slots are the saved instances: the source's outputs of its tick T0 - 1, and its local tick
        at_load = SL.sim_record(sim, D0 - 1)
        SL.assert_moved_equal({D0 - 1: at_load}, D0 - 1, ref, T0 - 1, moves, 1, p.N, keys, ("at the load", variant))
        t0, c0 = sim.epochs()
        for _, d in moves:
            assert (t0[d], c0[d]) == (D0 - T0, D0 - T0) and at_load["active"][d] == 1
        got += [tick(k) for k in range(D0, D0 + AFTER)]
        SL.assert_moved_equal(got, D0, ref, T0, moves, AFTER, p.N, keys, ("after the load", variant))
        others = [d for d in range(B_DST) if d not in [m[1] for m in moves]]
        SL.assert_slots_equal(got, plain_dst, others, range(D0 + AFTER), p.N, keys, ("slots not named", variant))


# ------------------------------------------------------------------ 3. the host's books
def test_books_of_an_active_a_paused_and_a_restarted_instance_and_the_epochs_of_their_load():
    p, s = PL.cpu_streams("go1")
    B = PL.CPU_SHAPES["go1"][1]
    sim = SL.SnapSim(p, B)
    for k in range(15):
        if k == 10:
            sim.set_active([1, 0, 1])          # instance 1 stands at its next local step 10
        sim.feed(s, k)
        sim.step(k)
    sim.reset([2])                             # instance 2: restarted, not yet initialised (local tick -1)
    st, blob = sim.save([0, 1, 2])
    assert st == 0
    hb, rb = sim.header_bytes(), sim.record_bytes()
    assert SL.books_of(blob, hb, rb, 3) == [(15, 15), (10, 10), (0, 0)]
    assert list(sim.ticks(14)) == [14, 9, -1] and list(sim.active()) == [1, 0, 1]   # saving changed no book
    # an old robot into a young handle: t0 is negative; the restarted one loads as a restart at the destination's step
    dst = SL.SnapSim(p, B)
    for k in range(D0):
        dst.feed(s, k)
        dst.step(k)
    assert dst.load([2, 0, 1], blob) == 0
    t0, c0 = dst.epochs()
    assert list(t0) == [D0 - 10, D0 - 0, D0 - 15] and list(c0) == [D0 - 10, D0 - 0, D0 - 15]
    assert list(dst.ticks(D0 - 1)) == [9, -1, 14] and list(dst.active()) == [1, 1, 1]
    # the host's arithmetic alone: a count of H or more is stored reduced, and the epochs give the stored step and count back
    H = 256
    for t0_, c0_, T, cnt, T2, cnt2 in ((0, 0, 4000, 10000, 3, 7), (17, -100, 5000, 2 ** 30 + 5, 1, 1), (9, 9, 9, 9, 123456, 2 ** 30)):
        step, count, nt0, nc0, ok = SL.arith(t0_, c0_, T, cnt, H, T2, cnt2)
        local = cnt - c0_
        assert ok and step == T - t0_ and count == (local if local < H else H + local % H)
        assert T2 - nt0 == step and cnt2 - nc0 == count and nc0 > cnt2 - 2 * H


def test_what_is_refused_is_refused_whole():
    p, s = PL.cpu_streams("go1")
    B = PL.CPU_SHAPES["go1"][1]
    sims = {v: SL.SnapSim(p, B, v) for v in ("plain", "smooth")}
    for k in range(6):
        for sim in sims.values():
            sim.feed(s, k)
            sim.step(k)
    sim = sims["plain"]
    before = SL.sim_record(sim, 5)
    st, blob = sim.save([0, 2])
    assert st == 0
    for ix in ([0, 3], [-1, 0], [1, 1]):
        assert sim.save(ix)[0] == 1 and sim.load(ix, blob) == 1
    assert sim.save([0, 2], nbytes=sim.snapshot_bytes(2) - 1)[0] == 1
    assert sim.load([0, 2], blob[:-1].copy()) == 1
    assert sim.load([1], blob) == 1                              # n is not the blob's
    assert sim.load([1, 0], sims["smooth"].save([0, 2])[1]) == 1  # a blob of a smoothing handle
    bad = blob.copy()
    bad[0] ^= 1
    assert sim.load([1, 0], bad) == 1                            # the magic
    bad = blob.copy()
    bad[sim.header_bytes() + sim.record_bytes() + 8] ^= 1       # the second record's noise fields: checked before the first is applied
    assert sim.load([1, 0], bad) == 1
    after = SL.sim_record(sim, 5)
    for key in before:
        assert np.array_equal(before[key], after[key], equal_nan=True), key
    assert sim.load([1, 0], blob) == 0
